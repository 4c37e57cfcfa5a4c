"""GPU: the baselines (csrc/baselines.hip, footprints_amd/baselines/) against the host restatement (tests/baselines_restatement.py) and
the reference's recorded run (fixture g20_baselines).  tests/test_baselines_cpu.py pins the restatement; nothing here reads the reference.

The hull is integer arithmetic and is compared byte for byte.  The plane's inlier counts are integers that the fixture's generator has
shown to be decided by the arithmetic (no point within 1e-9 of the threshold), so they are compared exactly; the plane and its depth are
compared within 16 x dev_ref, dev_ref being the reference's own deviation from an extended-precision evaluation (recorded in the
fixture) and 16 the margin for the different summation order of the back-projection."""
import os
import shutil

import numpy as np
import pytest
import torch

from tests import baselines_restatement as BR
from tests.golden import baselines_inputs as BI

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HULL_CASES = BI.hull_cases()
_hull_refs = {}


@pytest.fixture(scope="module")
def ops():
    from footprints_amd import ops
    return ops


@pytest.fixture(scope="module")
def g20():
    g = np.load(os.path.join(ROOT, "tests", "golden", "g20_baselines.npz"))
    return [{key.split(".", 1)[1]: g[key] for key in g.files if key.startswith("f%d." % k)} for k in range(len(BI.SHAPES))]


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def hull_ref(i):
    if i not in _hull_refs:
        _hull_refs[i] = np.stack([BR.hull(m) for m in HULL_CASES[i][1]]).astype(np.uint8)
    return _hull_refs[i]


# ---- convex hull -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["uint8", "float16"])
@pytest.mark.parametrize("i", range(len(HULL_CASES)), ids=[name for name, _ in HULL_CASES])
def test_hull_is_byte_equal_to_the_restatement(ops, i, dtype):
    mask = HULL_CASES[i][1]
    if dtype == "uint8":
        out = ops.convex_hull_mask(dev(mask * np.uint8(255 if i % 2 else 1)))
    else:
        rng = np.random.RandomState(i)
        x = np.where(mask != 0, 0.5 + 2.0 ** -11 + 0.4 * rng.rand(*mask.shape), 0.5 * rng.rand(*mask.shape))
        x[(mask == 0) & (rng.rand(*mask.shape) < 0.2)] = 0.5                      # the threshold itself is not set
        x = x.astype(np.float16)
        assert np.array_equal(x > 0.5, mask != 0)
        out = ops.convex_hull_mask(dev(x), 0.5)
    assert out.dtype == torch.uint8
    out = out.cpu().numpy()
    ref = hull_ref(i)
    assert np.array_equal(out, ref), "%d of %d pixels differ" % ((out != ref).sum(), ref.size)


def test_hull_threshold_is_compared_in_the_mask_s_dtype(ops):
    """0.3 is not a float16: numpy compares a float16 array with float16(0.3); float32(0.3) differs from both"""
    values = np.array([0.29980469, 0.30004883, 0.3, 0.30029297], np.float64)
    for dt in (np.float16, np.float32):
        x = np.zeros((1, 3, 8), dt)
        x[0, 1, 1:5] = values.astype(dt)
        want = np.stack([BR.hull(x[0] > 0.3)]).astype(np.uint8)
        assert np.array_equal(ops.convex_hull_mask(dev(x), 0.3).cpu().numpy(), want), dt


def test_hull_remove_keep_epilogue_is_bounding_box_frame_predict(ops):
    b = BI.batch(3, 33, 70, seed=31)
    vis, box = b["visible_ground"], b["bounding_box"]
    want = np.stack([BR.bounding_box_mask(v, bb) for v, bb in zip(vis, box)]).astype(np.uint8)
    plain = np.stack([BR.hull(v > 0.5) for v in vis]).astype(np.uint8)
    assert (want != plain).any()
    x = dev(vis)
    assert np.array_equal(ops.convex_hull_mask(x, 0.5, remove=dev(box), keep=x).cpu().numpy(), want)
    assert np.array_equal(ops.convex_hull_mask(x, 0.5, remove=dev(box.astype(np.float32)), keep=dev((vis > 0.5).astype(np.uint8))).cpu().numpy(), want)
    assert np.array_equal(ops.convex_hull_mask(x, 0.5).cpu().numpy(), plain)


# ---- RANSAC plane ------------------------------------------------------------------------------------------------------------------
def _padded_batch(g20):
    """the fixture's two frames as one batch: the smaller one padded to the right and below with unmasked pixels, which changes neither
    a pixel's coordinates nor the raster order of the masked ones"""
    H, W = BI.SHAPES[-1]
    depth, vis = np.ones((2, H, W), np.float32), np.zeros((2, H, W), np.float32)
    for k, f in enumerate(g20):
        h, w = f["depth"].shape
        depth[k, :h, :w], vis[k, :h, :w] = f["depth"], f["visible_ground"]
    return depth, np.stack([f["inv_K"] for f in g20]), vis, np.stack([f["samples"] for f in g20])


def test_plane_fit_and_depth_equal_the_reference(ops, g20):
    depth, inv_K, vis, samples = _padded_batch(g20)
    counts = ops.baseline_mask_counts(dev(vis), 0.5).cpu().numpy()
    assert counts.dtype == np.int32 and counts.tolist() == [int(f["n"]) for f in g20]
    fit = ops.baseline_plane_fit(dev(depth), dev(inv_K), dev(vis), dev(samples), threshold=0.5)
    floor = ops.baseline_plane_depth(dev(depth), dev(inv_K), fit["best_plane"]).cpu().numpy()
    fit = {k: v.cpu().numpy() for k, v in fit.items()}
    assert floor.dtype == np.float64 and fit["planes"].shape == (2, 100, 4) and fit["counts"].shape == (2, 100)
    for k, f in enumerate(g20):
        real = ~f["degenerate"]
        h, w = f["depth"].shape
        tol = 16 * float(f["dev_ref"])
        plane_dev = BR.same_up_to_sign(fit["best_plane"][k], f["model"])
        depth_dev = float((np.abs(floor[k, :h, :w] - f["plane_depth"]) / np.abs(f["plane_depth"])).max())
        print("frame %d: best_plane deviation %.3e, plane_depth relative deviation %.3e, bound %.3e" % (k, plane_dev, depth_dev, tol))
        assert np.array_equal(fit["counts"][k][real], f["counts"][real])
        assert (fit["counts"][k][~real] == 0).all() and not fit["planes"][k][~real].any()
        assert fit["best"][k].tolist() == [int(f["best_index"]), int(f["best_ic"])]
        assert np.array_equal(fit["best_plane"][k], fit["planes"][k][int(f["best_index"])])
        assert np.abs(np.linalg.norm(fit["planes"][k][real], axis=1) - 1).max() < 1e-14
        assert plane_dev <= tol and depth_dev <= tol
        # the ranks' pixels: the masked pixels in raster order
        pix = np.flatnonzero((vis[k] > 0.5).ravel())
        assert np.array_equal(fit["sample_pix"][k], pix[f["samples"]])
        # the sign of the plane is free
        flipped = ops.baseline_plane_depth(dev(depth[k:k + 1]), dev(inv_K[k:k + 1]), dev(-fit["best_plane"][k:k + 1])).cpu().numpy()
        assert (np.abs(flipped[0, :h, :w] - f["plane_depth"]) / np.abs(f["plane_depth"])).max() <= tol


def test_plane_fit_degenerate_samples_score_zero(ops, g20):
    f = g20[0]
    n, win = int(f["n"]), f["samples"][int(f["best_index"])]
    samples = np.array([[[5, 5, 9], [0, 1, n], win, [-1, 2, 3], [7, 3, 7]]], np.int32)
    fit = ops.baseline_plane_fit(dev(f["depth"][None]), dev(f["inv_K"][None]), dev(f["visible_ground"][None]), dev(samples), threshold=0.5)
    fit = {k: v.cpu().numpy()[0] for k, v in fit.items()}
    assert fit["counts"].tolist() == [0, 0, int(f["best_ic"]), 0, 0] and fit["best"].tolist() == [2, int(f["best_ic"])]
    assert not fit["planes"][[0, 1, 3, 4]].any() and fit["planes"][2].any()
    assert fit["sample_pix"][1, 2] == -1 and fit["sample_pix"][3, 0] == -1 and (fit["sample_pix"][[0, 2, 4]] >= 0).all()
    # nothing but degenerate samples: no winner
    none = ops.baseline_plane_fit(dev(f["depth"][None]), dev(f["inv_K"][None]), dev(f["visible_ground"][None]), dev(samples[:, :2]), threshold=0.5)
    assert none["best"].cpu().numpy().tolist() == [[-1, 0]] and not none["best_plane"].cpu().numpy().any()


def test_frame_with_19_masked_pixels_passes_its_depth_through(ops, g20):
    from footprints_amd.baselines.footprint_baseline import RansacPlane
    f = g20[0]
    vis = np.zeros_like(f["visible_ground"])
    vis.ravel()[np.flatnonzero(f["visible_ground"].ravel() > 0.5)[:19]] = 0.9
    both = np.stack([vis, f["visible_ground"]])
    assert ops.baseline_mask_counts(dev(both), 0.5).cpu().numpy().tolist() == [19, int(f["n"])]
    depth, inv_K = np.stack([f["depth"]] * 2), np.stack([f["inv_K"]] * 2)
    plane = np.stack([f["model"]] * 2)
    out = ops.baseline_plane_depth(dev(depth), dev(inv_K), dev(plane), passthrough=dev(np.array([1, 0], np.uint8))).cpu().numpy()
    assert np.array_equal(out[0], f["depth"].astype(np.float64)) and not np.array_equal(out[1], out[0])
    predictor = RansacPlane("matterport", random_seed=3, predictions="unused")
    mask, floor = predictor.frame_predict({"depth": f["depth"], "inv_K": f["inv_K"], "visible_ground": vis})
    assert mask is f["depth"] and floor is f["depth"]
    vis20 = vis.copy()
    vis20.ravel()[np.flatnonzero(f["visible_ground"].ravel() > 0.5)[19]] = 0.9
    mask, floor = predictor.frame_predict({"depth": f["depth"], "inv_K": f["inv_K"], "visible_ground": vis20})
    assert floor.dtype == np.float64 and floor is mask


def test_plane_scoring_over_more_than_one_workgroup(ops):
    """a workgroup of the scoring kernel takes 1024 pixels: 25 x 41 = 1025 is the smallest frame with a second one"""
    H, W = 25, 41
    found = None
    for seed in range(40, 60):                                      # the first scene whose counts the arithmetic decides (margin 1e-9)
        fr = BI.frame(H, W, seed)
        mask = fr["visible_ground"] > 0.5
        samples = BR.draw_samples(int(mask.sum()), seed)
        planes, counts, best = BR.plane_fit(fr["depth"], fr["inv_K"], mask, samples)
        data = BR.backproject(fr["depth"], fr["inv_K"])[0][mask.ravel()]
        margin = min(np.abs(np.abs(BR.plane_distance(p, data)) - BR.INLIER_THRESHOLD).min() for p in planes if p.any())
        if margin >= 1e-9:
            found = (fr, mask, samples, planes, counts, best)
            break
    assert found is not None
    fr, mask, samples, planes, counts, best = found
    assert mask.ravel()[1024:].any(), "the second workgroup has no masked pixel"
    fit = ops.baseline_plane_fit(dev(fr["depth"][None]), dev(fr["inv_K"][None]), dev(fr["visible_ground"][None]), dev(samples[None]), threshold=0.5)
    fit = {k: v.cpu().numpy()[0] for k, v in fit.items()}
    assert np.array_equal(fit["counts"], counts) and fit["best"].tolist() == list(best)
    # the winner explains most of the floor, so its triple is spread out: two float64 evaluations of its minors agree far below 1e-10
    assert BR.same_up_to_sign(fit["best_plane"], planes[best[0]]) < 1e-10


# ---- the classes -------------------------------------------------------------------------------------------------------------------
def _png(path):
    from PIL import Image
    im = Image.open(path)
    assert im.mode == "L"
    return np.asarray(im)


@pytest.fixture(scope="module")
def kitti_tree(tmp_path_factory):
    from PIL import Image
    root = tmp_path_factory.mktemp("kitti")
    (root / "kitti_predictions").mkdir()
    (root / "boxes").mkdir()
    frames = []
    for n in range(4):
        fr = BI.frame(192, 640, 70 + n)
        pred = np.zeros((4, 192, 640), np.float16)
        pred[0] = fr["visible_ground"]
        np.save(root / "kitti_predictions" / ("%03d.npy" % n), pred)
        Image.fromarray(np.stack([fr["bounding_box"]] * 3, -1)).save(root / "boxes" / ("%03d_colorfootprint.png" % n))
        vis = pred[0]
        frames.append({"visible_ground": vis, "bounding_box": fr["bounding_box"], "hull": BR.hull(vis > 0.5)})
    return root, frames


def _kitti_paths(root):
    return {"predictions": str(root / "kitti_predictions"), "bounding_boxes": str(root / "boxes")}


@pytest.mark.parametrize("name", ["VisibleGround", "ConvexHull", "BoundingBox"])
def test_mask_baselines_write_the_reference_s_files(kitti_tree, name):
    from footprints_amd.baselines import footprint_baseline as FB
    root, frames = kitti_tree
    args = ("kitti", "3d_boundingbox") if name == "BoundingBox" else ("kitti",)
    predictor = getattr(FB, name)(*args, **_kitti_paths(root))
    predictor.filenames = list(range(4))
    predictor.run_all(batch_size=3)
    folder = root / "predictions_rerun" / predictor.get_baseline_type()
    assert sorted(os.listdir(folder)) == ["%d_ground_mask.png" % n for n in range(4)]
    for n, fr in enumerate(frames):
        if name == "VisibleGround":
            want = fr["visible_ground"] > 0.1
        elif name == "ConvexHull":
            want = fr["hull"]
        else:
            want = fr["hull"].copy()
            want[fr["bounding_box"] < 0.5] = 0
            want[(fr["visible_ground"] > 0.5) == 1] = 1
        assert np.array_equal(_png(folder / ("%d_ground_mask.png" % n)), (want * 255).astype(np.uint8)), n
        mask, depth = predictor.frame_predict(predictor.loader(n))                 # the batch of one, bit for bit
        assert depth is None and mask.dtype == bool and np.array_equal(mask, want)
    shutil.rmtree(folder)


@pytest.fixture(scope="module")
def matterport_tree(tmp_path_factory):
    root = tmp_path_factory.mktemp("matterport")
    gt_dir = root / "gt" / "matterport_ground_truth" / "matterport_ground_truth"
    gt_dir.mkdir(parents=True)
    lines, frames = [], []
    for n in range(4):
        scan, frame_data = "scan%d" % (n % 2), ("scan%d" % (n % 2), "frame%d" % n, "1", str(n))
        lines.append(" ".join(frame_data))
        (root / "matterport_predictions" / scan).mkdir(parents=True, exist_ok=True)
        cam = root / "data" / scan / scan / "matterport_camera_intrinsics"
        cam.mkdir(parents=True, exist_ok=True)
        (cam / ("%s_intrinsics_%s.txt" % frame_data[1:3])).write_text(" ".join(str(v) for v in BI.CALIBRATION) + "\n")
        fr = BI.frame(512, 640, 80 + n)
        pred = np.zeros((4, 512, 640), np.float16)
        pred[0] = fr["visible_ground"]
        if n == 2:                                                                  # fewer than 20 visible-ground pixels
            pred[0] = 0.1
            pred[0, 400, 100:110] = 0.9
        pred[2] = (1.0 / fr["depth"].astype(np.float64) - 0.01) / (10.0 - 0.01)     # sigmoid_to_depth's inverse
        np.save(root / "matterport_predictions" / scan / ("%s_%s_%s.npy" % frame_data[1:]), pred)
        gt = fr["visible_ground"] > 0.7
        np.save(gt_dir / ("%s_%s_%s_%s_groundtruth.npy" % frame_data), gt)
        frames.append({"pred": pred, "gt": gt})
    return root, lines, frames


@pytest.mark.parametrize("name", ["RansacPlane", "RansacPlaneOracle"])
def test_ransac_baselines_write_the_reference_s_files(matterport_tree, g20, name):
    from footprints_amd.baselines import footprint_baseline as FB
    from footprints_amd.utils import sigmoid_to_depth
    root, lines, frames = matterport_tree
    seed = 5
    predictor = getattr(FB, name)("matterport", random_seed=seed, predictions=str(root / "matterport_predictions"), ground_truth_dir=str(root / "gt"),
                                  dataset=str(root / "data"))
    predictor.filenames = lines
    predictor.run_all(batch_size=3)
    folder = root / "predictions_rerun" / predictor.get_baseline_type()
    names = [line.replace(" ", "_") for line in lines]
    assert sorted(os.listdir(folder)) == sorted([n + "_ground_mask.png" for n in names] + [n + "_ground_depth.npy" for n in names])
    tol = 16 * max(float(f["dev_ref"]) for f in g20)
    _, inv_K = BI.intrinsics(512, 640)
    passed_through = 0
    for n, fr in enumerate(frames):
        depth = np.asarray(sigmoid_to_depth(fr["pred"][2]), np.float32)
        vis = fr["pred"][0] if name == "RansacPlane" else fr["gt"]
        mask = vis > 0.5
        saved = np.load(folder / (names[n] + "_ground_depth.npy"))
        if mask.sum() < BR.MIN_POINTS:
            passed_through += 1
            assert saved.dtype == np.float32 and np.array_equal(saved, depth), n
        else:
            planes, _, (best, _) = BR.plane_fit(depth, inv_K, mask, BR.draw_samples(int(mask.sum()), seed))
            want = BR.plane_depth(depth, inv_K, planes[best])
            # plane_depth = depth - dist / dot.  The difference passes through zero, and dot = rhat . m[:3] does so on the rays that run
            # parallel to the plane (a whole image row here): its three products leave an absolute error of a few ulp of sum |m_i|,
            # which is a relative error of that over |dot| in the quotient.  So the error is measured against the terms the value is
            # formed from, |depth| + |dist / dot| (1 + sum |m_i| / |dot|), with the fixture's bound for the relative part.
            _, rays = BR.backproject(depth, inv_K)
            dot = ((rays / np.sqrt((rays ** 2).sum(1, keepdims=True))) @ planes[best][:3]).reshape(depth.shape)
            d64 = depth.astype(np.float64)
            scale = np.abs(d64) + np.abs(d64 - want) * (1 + np.abs(planes[best][:3]).sum() / np.abs(dot))
            worst = float((np.abs(saved - want) / scale).max())
            print("%s frame %d: plane depth deviation %.3e of its terms, bound %.3e" % (name, n, worst, tol))
            assert saved.dtype == np.float64 and worst <= tol, n
        # the "mask" of these classes is the reference's expression over the floor depth, evaluated by numpy on the host
        with np.errstate(invalid="ignore"):
            assert np.array_equal(_png(folder / (names[n] + "_ground_mask.png")), (saved * 255).astype(np.uint8)), n
        one_mask, one_depth = predictor.frame_predict(predictor.loader(lines[n]))  # the batch of one, bit for bit
        assert one_mask is one_depth and np.array_equal(one_depth, saved)
    assert passed_through == (1 if name == "RansacPlane" else 0)


def test_evaluate_reads_a_baseline_s_ground_masks(tmp_path):
    from PIL import Image
    from footprints_amd.evaluation.evaluate_model import evaluate, evaluate_arrays
    gt_dir = tmp_path / "gt" / "kitti_ground_truth" / "kitti_ground_truth"
    pred_dir = tmp_path / "convex_hull"
    gt_dir.mkdir(parents=True)
    pred_dir.mkdir()
    rng = np.random.RandomState(3)
    distinct = 5
    combined, ground, pred = rng.rand(distinct, 12, 20) < 0.6, rng.rand(distinct, 12, 20) < 0.4, rng.rand(distinct, 12, 20) < 0.5
    combined[4] = False                                                            # no ground truth: nan, left out of the means
    for k in range(distinct):
        Image.fromarray((combined[k] * 255).astype(np.uint8)).save(gt_dir / ("%05d_combined.png" % k))
        Image.fromarray((ground[k] * 255).astype(np.uint8)).save(gt_dir / ("%05d_ground.png" % k))
        Image.fromarray((pred[k] * 255).astype(np.uint8)).save(pred_dir / ("%d_ground_mask.png" % k))
    for n in range(distinct, 697):                                                 # evaluate() walks the whole KITTI test set
        k = n % distinct
        shutil.copy(gt_dir / ("%05d_combined.png" % k), gt_dir / ("%05d_combined.png" % n))
        shutil.copy(gt_dir / ("%05d_ground.png" % k), gt_dir / ("%05d_ground.png" % n))
        shutil.copy(pred_dir / ("%d_ground_mask.png" % k), pred_dir / ("%d_ground_mask.png" % n))
    got = evaluate(str(pred_dir), "kitti", "iou", str(tmp_path / "gt"), batch=128)
    order = [n % distinct for n in range(697)]
    _, want = evaluate_arrays(pred[order].astype(np.float32), combined[order], ground[order], "iou", batch=128)
    assert got == want and 0 < got["footprint_iou"] < 1
    # a folder that holds the arrays is read as before
    np.save(pred_dir / "000.npy", np.stack([pred[1]] * 4).astype(np.float16))
    assert evaluate(str(pred_dir), "kitti", "iou", str(tmp_path / "gt"), batch=128) != got
