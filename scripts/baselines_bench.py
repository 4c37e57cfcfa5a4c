"""GPU box: time of the baselines' device steps (csrc/baselines.hip) for a Matterport batch (12 x 512 x 640) and a KITTI batch
(12 x 192 x 640) of the synthetic scenes of tests/golden/baselines_inputs.py: the convex hull, the masked counts, the plane fit
(100 candidates) and the plane depth -- kernels alone, then with the host-to-device and device-to-host copies a batch of run_all()
makes -- next to the host restatement (tests/baselines_restatement.py: Qhull and a facet test per pixel; numpy float64 RANSAC, one
pass over the points per candidate, as the reference does it) on one core.

    python scripts/baselines_bench.py [--seconds 1.0] [--host_frames 2]

HIP events after a warm-up; every timed loop runs for about `--seconds`.  Prints one JSON line.  KITTI has no depth in the
reference's baselines, so only the hull is timed there."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from footprints_amd import ops
from tests import baselines_restatement as BR
from tests.golden import baselines_inputs as BI


def timed(fn, seconds):
    """mean milliseconds of fn by device events: a warm-up, a probe to size the loop, then about `seconds` of back-to-back calls"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(3):
        fn()
    a.record()
    fn()
    b.record()
    b.synchronize()
    iters = int(max(5, min(2000, seconds * 1000.0 / max(a.elapsed_time(b), 1e-3))))
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def host_ms(fn, frames):
    t = time.perf_counter()
    for f in range(frames):
        fn(f)
    return (time.perf_counter() - t) * 1000.0 / frames


def case(name, B, H, W, with_plane, seconds, host_frames):
    torch.set_num_threads(1)
    b = BI.batch(B, H, W)
    vis16 = b["visible_ground"].astype(np.float16)                      # the inference pass's file format
    pin = lambda a: torch.from_numpy(np.ascontiguousarray(a)).pin_memory()
    h_vis, h_depth, h_invK = pin(vis16), pin(b["depth"]), pin(b["inv_K"])
    vis, depth, inv_K = h_vis.cuda(), h_depth.cuda(), h_invK.cuda()
    out = {"shape": [B, H, W]}

    out["hull_kernels_ms"] = timed(lambda: ops.convex_hull_mask(vis, 0.5), seconds)
    out["hull_with_copies_ms"] = timed(lambda: ops.convex_hull_mask(h_vis.cuda(non_blocking=True), 0.5).cpu(), seconds)
    out["host_hull_ms_per_frame"] = host_ms(lambda f: BR.hull(vis16[f] > 0.5), host_frames)
    if with_plane:
        counts = ops.baseline_mask_counts(vis, 0.5).cpu().numpy()
        samples_h = pin(np.stack([BR.draw_samples(int(n), 1) for n in counts]))
        samples = samples_h.cuda()
        fit = ops.baseline_plane_fit(depth, inv_K, vis, samples, 0.5)
        out["masked_points_per_frame"] = float(counts.mean())
        out["counts_kernel_ms"] = timed(lambda: ops.baseline_mask_counts(vis, 0.5), seconds)
        out["fit_kernels_ms"] = timed(lambda: ops.baseline_plane_fit(depth, inv_K, vis, samples, 0.5), seconds)
        out["depth_kernel_ms"] = timed(lambda: ops.baseline_plane_depth(depth, inv_K, fit["best_plane"]), seconds)

        def whole():
            d, k, v = h_depth.cuda(non_blocking=True), h_invK.cuda(non_blocking=True), h_vis.cuda(non_blocking=True)
            ops.baseline_mask_counts(v, 0.5).cpu()
            f = ops.baseline_plane_fit(d, k, v, samples_h.cuda(non_blocking=True), 0.5)
            return ops.baseline_plane_depth(d, k, f["best_plane"]).cpu()
        out["ransac_with_copies_ms"] = timed(whole, seconds)
        s_np = samples_h.numpy()
        out["host_ransac_ms_per_frame"] = host_ms(lambda f: BR.ransac_plane(b["depth"][f], b["inv_K"][f], b["visible_ground"][f], s_np[f]), host_frames)
    return name, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--host_frames", type=int, default=2)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "baselines_bench.py needs the GPU"
    res = dict([case("matterport", 12, 512, 640, True, args.seconds, args.host_frames),
                case("kitti", 12, 192, 640, False, args.seconds, args.host_frames)])
    print(json.dumps({"baselines_bench": res}))


if __name__ == "__main__":
    main()
