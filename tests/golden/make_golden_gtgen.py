"""Writes tests/golden/g13_gtgen*.npz: what the REFERENCE's own geometry.py / ground_truth_generator.py compute on the inputs of
tests/golden/gtgen_inputs.py, plus the reference's own fp32-vs-float64 deviations, which set the tolerances of the GPU tests.

Needs the reference checkout (oracle/ref_import.py); run as `python -m tests.golden.make_golden_gtgen` from the repository root.
The reference runs on the CPU here: its `.cuda()` calls are made the identity, cv2 is the stand-in of oracle/ref_import.py, and torch
runs one thread so that the scatter of extract_depth_from_projections is serial (last assignment wins).
"""
import importlib
import os
import types

import numpy as np
import torch

from oracle import ref_import
from tests import gtgen_restatement as GR
from tests.golden import digest, gtgen_inputs as GI

NAME = "g13_gtgen"
PART_LIMIT = 760 * 1024


def load_reference_gtgen():
    if ref_import.load_reference() is None:
        raise SystemExit("the reference checkout is not available")
    torch.Tensor.cuda = lambda self, *a, **k: self
    keep = {k: os.environ.get(k) for k in ("MKL_NUM_THREADS", "NUMEXPR_NUM_THREADS", "OMP_NUM_THREADS")}
    geometry = importlib.import_module("footprints.preprocessing.ground_truth_generation.geometry")
    generator = importlib.import_module("footprints.preprocessing.ground_truth_generation.ground_truth_generator")
    for k, v in keep.items():               # the module pins the thread counts to 1 at import; undo
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    return geometry, generator


def save_parts(name, arrays, limit=PART_LIMIT):
    keys = list(arrays)
    for n in range(1, len(keys) + 1):
        groups, sizes = [[] for _ in range(n)], [0] * n
        for key in sorted(keys, key=lambda name_: -np.asarray(arrays[name_]).nbytes):         # largest first into the emptiest part
            i = sizes.index(min(sizes))
            groups[i].append(key)
            sizes[i] += np.asarray(arrays[key]).nbytes
        paths = [digest._part_path(name, k + 1) for k in range(n)]
        for path, group in zip(paths, groups):
            np.savez_compressed(path, **{key: arrays[key] for key in group})
        if all(os.path.getsize(p) < limit for p in paths):
            break
    k = n + 1
    while os.path.exists(digest._part_path(name, k)):
        os.remove(digest._part_path(name, k))
        k += 1
    return paths


def both_valid_deviation(cp32, cp64, H, W):
    """max |du|, |dv| (pixels) and max relative |dz| over the points valid in both runs"""
    ok = (GR.decide(cp32, H, W) >= 0) & (GR.decide(cp64, H, W) >= 0)
    du = np.abs(cp32[:, 0].astype(np.float64) - cp64[:, 0])[ok].max()
    dv = np.abs(cp32[:, 1].astype(np.float64) - cp64[:, 1])[ok].max()
    dz = (np.abs(cp32[:, 2].astype(np.float64) - cp64[:, 2]) / np.abs(cp64[:, 2]))[ok].max()
    return np.array([du, dv, dz])


def main():
    torch.set_num_threads(1)
    geometry, generator = load_reference_gtgen()
    H, W = GI.H, GI.W
    out = {}

    gen = object.__new__(generator.GroundTruthGenerator)
    gen.projector = geometry.BatchProjector(H, W)
    gen.footprint_threshold = GI.FOOTPRINT_THRESHOLD

    # ---- hidden depth: per-frame projections, medians ------------------------------------------------------------------------------
    data = GI.hidden_depth_inputs()
    tdata = {k: torch.from_numpy(v) for k, v in data.items()}
    world = gen.projector.project_to_world(tdata["depths"], tdata["inv_intrinsics"])
    cam_pix = gen.projector.project_to_camera(world, tdata["poses"], tdata["intrinsics"])
    projections = gen.projector.extract_depth_from_projections(cam_pix).numpy()
    cp32 = cam_pix.numpy()
    out["hd.projections"] = projections
    out["hd.median_robust"] = np.asarray(gen.process_data(dict(tdata), robust_aggregation=True), np.float32)
    out["hd.median_plain"] = np.asarray(gen.process_data(dict(tdata), robust_aggregation=False), np.float32)
    pix32 = GR.decide(cp32, H, W)
    out["hd.ref_pix"] = pix32.astype(np.int32)
    out["hd.ref_z_frames"] = np.array([0, 5, 9])
    out["hd.ref_z"] = cp32[out["hd.ref_z_frames"], 2]
    cp64 = GR.warp(data["depths"], data["inv_intrinsics"], data["poses"], data["intrinsics"])
    pix64 = GR.decide(cp64, H, W)
    out["hd.deviation_uvz"] = both_valid_deviation(cp32, cp64, H, W)
    reach, diff = GR.differing_reach(pix32, pix64, H, W)
    out["hd.differing_share"] = np.float64(diff.sum() / max((pix64 >= 0).sum(), 1))
    out["hd.ref_excluded"] = np.packbits(reach.any(0))
    share = reach.any(0).mean()
    assert share <= 0.005, "the reference's own fp32-vs-float64 differences exclude %.3f %% of the pixels" % (100 * share)
    multi = np.mean([(np.bincount(p[p >= 0], minlength=H * W) > 1).sum() / max((np.bincount(p[p >= 0], minlength=H * W) > 0).sum(), 1)
                     for p in pix32])
    n_pos = (projections > 0).sum(0)
    print("hidden depth: deviation (du, dv, rel dz) %s, differing share %.2e, excluded pixels %.3f %%, hit pixels with collisions %.1f %%, "
          "pixels with n > 2: %.1f %%, even n: %.1f %%" % (out["hd.deviation_uvz"], out["hd.differing_share"], 100 * share, 100 * multi,
                                                           100 * (n_pos > 2).mean(), 100 * ((n_pos > 0) & (n_pos % 2 == 0)).mean()))
    assert (n_pos > 2).mean() > 0.1 and ((n_pos > 0) & (n_pos % 2 == 0)).mean() > 0.02

    # ---- moving-object mask --------------------------------------------------------------------------------------------------------
    mv = GI.moving_inputs()
    K, invK = GI.intrinsics()
    det = object.__new__(generator.KITTIMovingObjectDetector)
    det.projector = gen.projector
    det.K, det.invK = torch.from_numpy(K)[None], torch.from_numpy(invK)[None]
    det.loader = types.SimpleNamespace(stereo_baseline=GI.STEREO_BASELINE)
    mask = det.process_data({"base_data": {"pose": mv["base_pose"], "disparity": mv["disparity"], "flow": mv["flow"]},
                             "lookup_data": {"pose": mv["lookup_pose"]}})
    out["mv.mask"] = np.packbits(mask)
    fb = float(det.K[0, 0, 0]) * GI.STEREO_BASELINE
    n64 = GR.moving_norm(mv["disparity"], mv["flow"], invK[None], mv["T"][None], K[None], fb)
    n32 = GR.moving_norm(mv["disparity"], mv["flow"], invK[None], mv["T"][None], K[None], fb, np.float32)
    # the reference's own norm, recomputed from its cam_pix
    depth = torch.from_numpy(np.float32(fb) / mv["disparity"])[None]
    cpm = gen.projector.project_to_camera(gen.projector.project_to_world(depth, det.invK), torch.from_numpy(mv["T"])[None], det.K)
    cpm = cpm[0, :2].reshape(2, H, W).numpy()
    x, y = np.meshgrid(np.arange(W), np.arange(H))
    cpm[0] -= x
    cpm[1] -= y
    dref = cpm - mv["flow"]
    nref = np.sqrt(dref[0] * dref[0] + dref[1] * dref[1])
    assert np.array_equal(nref > 3, mask)
    fin = np.isfinite(nref) & np.isfinite(n64)
    assert np.array_equal(np.isfinite(nref), np.isfinite(n64))
    out["mv.norm_deviation"] = np.float64(np.abs(nref - n64)[fin].max())
    band = 4 * out["mv.norm_deviation"]
    excluded = fin & (np.abs(n64 - 3) <= band)
    assert excluded.mean() <= 0.01 and np.array_equal((n64 > 3)[~excluded], mask[~excluded])
    assert 0.01 <= mask.mean() <= 0.5, mask.mean()
    print("moving mask: share %.1f %%, norm deviation %.2e (numpy fp32 restatement: %.2e), excluded %.3f %%" % (
        100 * mask.mean(), out["mv.norm_deviation"], np.abs(n32 - n64)[fin].max(), 100 * excluded.mean()))

    # ---- depth mask ----------------------------------------------------------------------------------------------------------------
    dm = GI.depth_mask_inputs()
    ground = (dm["ground_seg"] > GI.FOOTPRINT_THRESHOLD).reshape(-1)
    samples = GI.draw_samples(int(ground.sum()))
    np.random.seed(GI.SAMPLE_SEED)
    tdepth = torch.from_numpy(dm["depth"])[None]
    ref_mask = gen.compute_depth_mask(tdepth, dm["ground_seg"], det.K, det.invK)
    world_xyz = gen.projector.project_to_world(tdepth, det.invK).numpy()[0, :3].T
    np.random.seed(GI.SAMPLE_SEED)
    ref_plane, ref_count, _ = geometry.fit_plane(world_xyz[ground])
    planes, counts, best = GR.plane_scores(world_xyz, ground, samples)
    assert all(pl[:3].any() for pl in planes), "a drawn sample is degenerate"
    order = np.sort(counts)
    near = 0
    for pl in planes:
        near = max(near, int((np.abs(np.abs(GR.plane_distance(pl, world_xyz[ground])) - GR.INLIER_THRESHOLD) < 1e-6).sum()))
    assert order[-1] - order[-2] > near, (order[-3:], near)
    assert counts[best] == ref_count, (counts[best], ref_count)
    unit = lambda p: p / np.linalg.norm(p[:3])
    cosine = float(np.dot(unit(planes[best])[:3], unit(ref_plane)[:3]))
    assert abs(abs(cosine) - 1) < 1e-9 and np.allclose(unit(planes[best]) * np.sign(cosine), unit(ref_plane), atol=1e-9), (planes[best], ref_plane)
    out["dm.samples"], out["dm.best"], out["dm.best_count"] = samples, np.int64(best), np.int64(ref_count)
    out["dm.plane"] = np.asarray(ref_plane, np.float64)
    out["dm.mask"] = np.packbits(ref_mask)
    assert 0.01 <= ref_mask.mean() <= 0.5, "depth mask true share %.3f" % ref_mask.mean()
    # the reference's fp32 projection of the copies against float64, with ITS plane: what its rounding can decide
    cp32 = GR.flatten_copies(world_xyz, ground, ref_plane, K)
    proj32 = GR.splat(cp32, H, W)[0]
    assert np.array_equal(GR.depth_mask_filter(proj32, dm["depth"], dm["ground_seg"]), ref_mask), "restatement != reference depth mask"
    cp64 = GR.flatten_copies(world_xyz, ground, ref_plane, K, np.float64)
    out["dm.deviation_uvz"] = both_valid_deviation(cp32, cp64, H, W)
    reach, diff = GR.differing_reach(GR.decide(cp32, H, W), GR.decide(cp64, H, W), H, W)
    out["dm.ref_excluded"] = np.packbits(reach[0])
    proj64 = GR.scatter(GR.decide(cp64, H, W), cp64[:, 2], H, W)[0]
    excluded = reach[0].reshape(H, W) | GR.filter_band(proj64, dm["depth"], 4 * out["dm.deviation_uvz"][2])
    assert excluded.mean() <= 0.02, excluded.mean()
    print("depth mask: true share %.1f %%, best / second count %d / %d (%d near the threshold), excluded %.3f %%, copies deviation %s" % (
        100 * ref_mask.mean(), order[-1], order[-2], near, 100 * excluded.mean(), out["dm.deviation_uvz"]))

    for p in save_parts(NAME, out):
        print(p, os.path.getsize(p))


if __name__ == "__main__":
    main()
