"""CPU: the host side of the baselines (footprints_amd/baselines/, csrc/baselines.hip) -- the restatement the GPU tests compare
against is itself checked here: the hull against an exact brute force, the RANSAC path against the reference's recorded run
(tests/golden/g20_baselines.npz), the host's sample draw against the recorded ranks; then the loaders against a temporary tree and the
C ABI's three descriptions of the new entry points against each other.  No kernel is launched."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import baselines_restatement as BR
from tests.golden import baselines_inputs as BI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G20 = os.path.join(ROOT, "tests", "golden", "g20_baselines.npz")
NEW_SYMBOLS = ("fp_baseline_hull", "fp_baseline_mask_counts", "fp_baseline_plane_fit", "fp_baseline_plane_depth")


# ---- the hull ----------------------------------------------------------------------------------------------------------------------
def _cross(o, a, b):
    return (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])


def brute_force_hull(mask):
    """exact: doubled integer coordinates (Python integers), Andrew's monotone chain, inclusive cross test for every pixel centre"""
    mask = np.asarray(mask) != 0
    out = np.zeros(mask.shape, bool)
    pts = set()
    for r, c in np.argwhere(mask):
        r, c = int(r), int(c)
        pts |= {(2 * r + 1, 2 * c), (2 * r - 1, 2 * c), (2 * r, 2 * c + 1), (2 * r, 2 * c - 1)}
    if not pts:
        return out
    pts = sorted(pts)
    lower, upper = [], []
    for p in pts:
        while len(lower) >= 2 and _cross(lower[-2], lower[-1], p) <= 0:
            lower.pop()
        lower.append(p)
    for p in reversed(pts):
        while len(upper) >= 2 and _cross(upper[-2], upper[-1], p) <= 0:
            upper.pop()
        upper.append(p)
    ring = lower[:-1] + upper[:-1]                                             # counter-clockwise
    for r in range(mask.shape[0]):
        for c in range(mask.shape[1]):
            q = (2 * r, 2 * c)
            out[r, c] = all(_cross(ring[i], ring[(i + 1) % len(ring)], q) >= 0 for i in range(len(ring)))
    return out


def _hull_cpu_cases():
    rng = np.random.RandomState(11)
    cases = []
    for k in range(24):
        H, W = int(rng.randint(1, 25)), int(rng.randint(1, 41))
        cases.append(("random %d: %dx%d" % (k, H, W), rng.rand(H, W) < rng.choice([0.02, 0.1, 0.5])))
    cases.append(("24x40 blob", BI.blob(24, 40, 2) != 0))
    for H, W in ((1, 1), (3, 3), (1, 9), (9, 1)):
        for r, c in ((0, 0), (H - 1, W - 1), (H // 2, W // 2)):
            m = np.zeros((H, W), bool)
            m[r, c] = True
            cases.append(("single pixel %dx%d at %d,%d" % (H, W, r, c), m))
    row = np.zeros((7, 12), bool)
    row[3, 2:9] = True
    col = np.zeros((12, 7), bool)
    col[1:11, 4] = True
    far = np.zeros((24, 40), bool)
    far[0, 39] = far[23, 0] = True
    return cases + [("single row", row), ("single column", col), ("two far-apart pixels", far), ("empty", np.zeros((5, 6), bool))]


def test_restated_hull_equals_the_exact_brute_force():
    bad = [name for name, m in _hull_cpu_cases() if not np.array_equal(BR.hull(m), brute_force_hull(m))]
    assert not bad, bad


def test_hull_contains_its_mask_and_grows_with_it():
    """(not idempotent: the half-pixel offsets can admit further centres on the second application)"""
    m = BI.blob(24, 40, 4) != 0
    h = BR.hull(m)
    assert h[m].all() and h.sum() > m.sum() and BR.hull(h)[h].all()


# ---- RANSAC against the reference's recorded run -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def g20():
    return np.load(G20)


@pytest.mark.parametrize("k", range(len(BI.SHAPES)))
def test_restated_ransac_equals_the_reference(g20, k):
    f = lambda name: g20["f%d.%s" % (k, name)]
    depth, inv_K, samples = f("depth"), f("inv_K"), f("samples")
    assert depth.shape == BI.SHAPES[k] and depth.dtype == np.float32 and inv_K.dtype == np.float64
    mask = f("visible_ground") > 0.5
    planes, counts, (best, best_count) = BR.plane_fit(depth, inv_K, mask, samples)
    real = ~f("degenerate")
    assert np.array_equal(counts[real], f("counts")[real])
    assert (counts[~real] == 0).all()
    assert best == int(f("best_index")) and best_count == int(f("best_ic"))
    tol = 16 * float(f("dev_ref"))
    assert BR.same_up_to_sign(planes[best], f("model")) <= tol
    ref = f("plane_depth")
    assert (np.abs(BR.plane_depth(depth, inv_K, planes[best]) - ref) / np.abs(ref)).max() <= tol
    assert (np.abs(BR.plane_depth(depth, inv_K, -planes[best]) - ref) / np.abs(ref)).max() <= tol            # the sign is free


@pytest.mark.parametrize("k", range(len(BI.SHAPES)))
def test_fixture_inputs_are_the_input_module_s(g20, k):
    fr = BI.frame(*BI.SHAPES[k], 20 + k)
    for name in ("depth", "inv_K", "visible_ground"):
        assert np.array_equal(fr[name], g20["f%d.%s" % (k, name)]), name


@pytest.mark.parametrize("k", range(len(BI.SHAPES)))
def test_host_sample_draw_equals_the_recorded_ranks(g20, k):
    from footprints_amd.baselines.footprint_baseline import draw_sample_ranks
    n, seed = int(g20["f%d.n" % k]), int(g20["f%d.seed" % k])
    state = np.random.get_state()
    try:
        drawn = draw_sample_ranks(n, seed)
    finally:
        np.random.set_state(state)
    assert drawn.dtype == np.int32 and np.array_equal(drawn, g20["f%d.samples" % k])


# ---- loaders -----------------------------------------------------------------------------------------------------------------------
def test_kitti_loader_and_save_path(tmp_path):
    from PIL import Image
    from footprints_amd.baselines.prepare_test_data import KittiTestLoader
    pred_dir, box_dir = tmp_path / "kitti_predictions", tmp_path / "boxes"
    pred_dir.mkdir()
    box_dir.mkdir()
    rng = np.random.RandomState(0)
    pred = rng.rand(4, 192, 640).astype(np.float16)
    np.save(pred_dir / "007.npy", pred)                                       # this package's own inference name
    np.save(pred_dir / "008_color.npy", pred[::-1].copy())                    # the reference's name
    box = np.zeros((192, 640, 3), np.uint8)
    box[50:60, 100:200, 0] = 255
    Image.fromarray(box).save(box_dir / "007_colorfootprint.png")
    loader = KittiTestLoader(True, "pred", "bounding_box", predictions=str(pred_dir), bounding_boxes=str(box_dir))
    inputs = loader(7)
    assert sorted(inputs) == ["bounding_box_mask", "visible_ground"]
    assert inputs["visible_ground"].dtype == np.float16 and np.array_equal(inputs["visible_ground"], pred[0])
    assert np.array_equal(inputs["bounding_box_mask"], box[:, :, 0])
    assert np.array_equal(KittiTestLoader(False, "pred", "convex_hull", predictions=str(pred_dir))(8)["visible_ground"], pred[3])
    with pytest.raises(FileNotFoundError):
        loader(9)
    path = loader.get_save_path("bounding_box_3d_boundingbox", 7)
    assert os.path.normpath(path) == str(tmp_path / "predictions_rerun" / "bounding_box_3d_boundingbox" / "7")
    assert os.path.isdir(os.path.dirname(path))
    other = KittiTestLoader(False, "pred", "convex_hull", predictions=str(pred_dir), save_root=str(tmp_path / "out"))
    assert other.get_save_path("convex_hull", 12) == str(tmp_path / "out" / "predictions_rerun" / "convex_hull" / "12")
    # another size goes through the stated stand-in (Pillow mode "F", bilinear)
    np.save(pred_dir / "010.npy", pred[:, ::2, ::2].copy())
    small = loader.__class__(False, "pred", "convex_hull", predictions=str(pred_dir))(10)["visible_ground"]
    ref = np.asarray(Image.fromarray(pred[0, ::2, ::2].astype(np.float32)).resize((640, 192), Image.BILINEAR))
    assert small.shape == (192, 640) and np.array_equal(small, ref)


def test_matterport_loader_and_save_path(tmp_path):
    from footprints_amd.baselines.prepare_test_data import MatterportTestLoader
    from footprints_amd.utils import sigmoid_to_depth
    line = "scan0 abc123 2 5"
    pred_dir = tmp_path / "matterport_predictions"
    (pred_dir / "scan0").mkdir(parents=True)
    gt_dir = tmp_path / "gt" / "matterport_ground_truth" / "matterport_ground_truth"
    gt_dir.mkdir(parents=True)
    cam_dir = tmp_path / "data" / "scan0" / "scan0" / "matterport_camera_intrinsics"
    cam_dir.mkdir(parents=True)
    rng = np.random.RandomState(1)
    pred = rng.rand(4, 512, 640).astype(np.float16)
    np.save(pred_dir / "scan0" / "abc123_2_5.npy", pred)
    gt = rng.rand(512, 640) < 0.3
    np.save(gt_dir / "scan0_abc123_2_5_groundtruth.npy", gt)
    (cam_dir / "abc123_intrinsics_2.txt").write_text(" ".join(str(v) for v in BI.CALIBRATION) + "\n")
    paths = {"predictions": str(pred_dir), "ground_truth_dir": str(tmp_path / "gt"), "dataset": str(tmp_path / "data")}
    inputs = MatterportTestLoader(False, "ground_truth", "ransac_plane_oracle", **paths)(line)
    assert sorted(inputs) == ["K", "depth", "inv_K", "visible_ground"]
    assert inputs["depth"].dtype == np.float32 and np.array_equal(inputs["depth"], np.asarray(sigmoid_to_depth(pred[2]), np.float32))
    K, inv_K = BI.intrinsics(512, 640)
    assert np.array_equal(inputs["K"], K) and np.array_equal(inputs["inv_K"], inv_K) and inv_K.dtype == np.float64
    assert np.array_equal(inputs["visible_ground"], gt)
    hull_inputs = MatterportTestLoader(False, "pred", "convex_hull", **paths)(line)
    assert sorted(hull_inputs) == ["visible_ground"] and np.array_equal(hull_inputs["visible_ground"], pred[0])
    loader = MatterportTestLoader(False, "pred", "ransac_plane", **paths)
    path = loader.get_save_path("ransac_plane", line)
    assert os.path.normpath(path) == str(tmp_path / "predictions_rerun" / "ransac_plane" / "scan0_abc123_2_5")
    with pytest.raises(ValueError, match="dataset"):
        MatterportTestLoader(False, "pred", "ransac_plane", predictions=str(pred_dir))(line)


def test_baseline_classes_keep_the_reference_surface():
    from footprints_amd.baselines import footprint_baseline as FB
    want = {"VisibleGround": ("visible_ground", "pred"), "ConvexHull": ("convex_hull", "pred"), "BoundingBox": ("bounding_box", "pred"),
            "RansacPlane": ("ransac_plane", "pred"), "RansacPlaneOracle": ("ransac_plane_oracle", "ground_truth")}
    for name, (baseline_type, visible) in want.items():
        cls = getattr(FB, name)
        assert (cls.baseline_type, cls.load_visible_ground) == (baseline_type, visible)
        assert cls.load_bounding_box_predictions == (name == "BoundingBox")
        for method in ("frame_predict", "run_all", "get_baseline_type"):
            assert callable(getattr(cls, method))
    box = FB.BoundingBox("kitti", "3d_boundingbox", predictions="p", bounding_boxes="b")
    assert box.get_baseline_type() == "bounding_box_3d_boundingbox" and box.loader.load_bounding_box_predictions is True
    assert FB.RansacPlane("matterport", predictions="p").random_seed is None


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree_on_the_new_symbols():
    import ctypes as C
    from footprints_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "footprints_hip.h")).read()
    decls = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    ctype_of = {"int32_t": C.c_int32, "double": C.c_double, "fp_stream_t": C.c_void_p}
    for name in NEW_SYMBOLS:
        m = re.search(r"\bint %s\((.*?)\);" % name, decls, flags=re.S)
        assert m, name
        params = [" ".join(p.split()) for p in m.group(1).split(",")]
        assert params[-1] == "fp_stream_t stream", (name, params[-1])                 # the stream goes last
        assert not any("fp_aux" in p for p in params)
        want = [C.c_void_p if "*" in p else ctype_of[p.rsplit(" ", 1)[0]] for p in params]
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and args == want, (name, args, want)
        assert re.search(r"\bT %s$" % name, exported, flags=re.M), name
    lib = _lib.load()
    # argument checks run before any launch: they work without a device
    assert lib.fp_baseline_hull(1, 0, 0.0, None, 0, None, 0, 0.0, 1, 4096, 8, 1, 1, None) == -1 and b"H <= 2040" in lib.fp_last_error_string()
    assert lib.fp_baseline_plane_fit(1, 1, 1, 0, 0.5, 1, 101, 1, 8, 8, 1, 1, 1, 1, 1, None) == -1 and b"candidates" in lib.fp_last_error_string()
    assert lib.fp_baseline_mask_counts(1, 3, 0.5, 1, 8, 8, 1, None) == -1 and b"dtype" in lib.fp_last_error_string()
    assert lib.fp_baseline_plane_depth(None, 1, 1, None, 1, 8, 8, 1, None) == -1 and b"null" in lib.fp_last_error_string()
