"""GPU box: time of the label generation for one KITTI target (76 x 192 x 640, robust) and one Matterport-sized target (40 x 480 x 640):
the fused HIP path per kernel and in total, next to the same pipeline written with stock PyTorch device ops (batched matmul, per-frame
masked index_put_, sort-based masked median) -- the reference's own formulation, which is what a user would otherwise run on a GPU.

    python scripts/gtgen_bench.py [--seconds 2.0] [--rounds 5]

HIP events after a warm-up; both sides in one process, alternating round by round; every timed loop runs for about `--seconds` in total.
Prints one JSON line.  Algorithmic bytes: the depths read once, the key plane written (cleared), updated and read once, one output plane."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from footprints_amd import ops
from tests.golden import gtgen_inputs as GI

HBM_PEAK = 8.0e12          # bytes / s, MI355X specification


def timed(fn, iters):
    """mean milliseconds of fn over `iters` back-to-back calls, by device events"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def torch_pipeline(d, H, W, robust, grid):
    """the reference's process_data with device ops only"""
    B = d["depths"].shape[0]
    world = torch.matmul(d["inv_intrinsics"][:, :3, :3], grid) * d["depths"].reshape(B, 1, -1)
    world = torch.cat([world, (d["depths"].reshape(B, 1, -1) > 0).float()], 1)
    cam = torch.matmul(d["intrinsics"], torch.matmul(d["poses"], world))
    cam[:, :2] /= (cam[:, 2].unsqueeze(1) + 1e-7)
    proj = torch.zeros((B, H, W), device=cam.device)
    for i in range(B):
        c = cam[i]
        c = c[:, (c[0] > 0) * (c[0] < W) * (c[1] > 0) * (c[1] < H) * (c[2] > 0) * (c[3] > 0)]
        proj[i].index_put_((c[1].long(), c[0].long()), c[2])
    flat = proj.reshape(B, -1)
    pos = flat > 0
    n = pos.sum(0)
    s = torch.where(pos, flat, torch.full_like(flat, float("inf"))).sort(0).values
    lo = s.gather(0, ((n - 1).clamp(min=0) // 2)[None])[0]
    hi = s.gather(0, (n // 2).clamp(max=B - 1)[None])[0]
    med = (lo + hi) * 0.5
    return torch.where(n > (2 if robust else 0), med, torch.zeros_like(med)).reshape(H, W)


def case(name, B, H, W, robust, seconds, rounds):
    d = {k: torch.from_numpy(v).cuda() for k, v in GI.hidden_depth_inputs(B, H, W).items()}
    x, y = np.meshgrid(np.arange(W), np.arange(H))
    grid = torch.from_numpy(np.stack([x, y, np.ones([H, W])]).reshape(1, 3, -1)).float().cuda()
    keys = ops.gt_keys(B, H, W, d["depths"].device)
    cam_pix = ops.gt_project(d["depths"], d["inv_intrinsics"], d["poses"], d["intrinsics"])
    legs = {
        "fused_total": lambda: ops.gt_aggregate(ops.gt_warp_splat(d["depths"], d["inv_intrinsics"], d["poses"], d["intrinsics"], keys), H, W, robust),
        "warp_splat": lambda: ops.gt_warp_splat(d["depths"], d["inv_intrinsics"], d["poses"], d["intrinsics"], keys),
        "aggregate": lambda: ops.gt_aggregate(keys, H, W, robust),
        "clear_keys": lambda: ops.zero_u32(keys.view(torch.int32)),
        "staged_project": lambda: ops.gt_project(d["depths"], d["inv_intrinsics"], d["poses"], d["intrinsics"]),
        "staged_splat": lambda: ops.gt_splat(cam_pix, H, W, keys),
        "torch_total": lambda: torch_pipeline(d, H, W, robust, grid),
    }
    # warm-up, and how many calls of each leg fill seconds / rounds
    iters = {}
    for leg, fn in legs.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        once = max(timed(fn, 3), 1e-3)
        iters[leg] = max(3, int(seconds * 1e3 / rounds / once))
    samples = {leg: [] for leg in legs}
    for _ in range(rounds):                                        # alternating: every round times every leg once
        for leg, fn in legs.items():
            samples[leg].append(timed(fn, iters[leg]))
    ms = {leg: float(np.median(v)) for leg, v in samples.items()}
    spread = {leg: float((max(v) - min(v)) / np.median(v)) for leg, v in samples.items()}
    ours = legs["fused_total"]().cpu().numpy()
    theirs = legs["torch_total"]().cpu().numpy()
    valid = int((ops.gt_aggregate(keys, H, W, False, want_projections=True)[1] > 0).sum().item())
    hw = H * W
    bytes_alg = B * hw * 4 + 2 * B * hw * 8 + hw * 4
    return {"case": name, "frames": B, "height": H, "width": W, "robust": robust, "ms": ms, "spread": spread, "calls_per_round": iters,
            "rounds": rounds, "algorithmic_bytes": bytes_alg, "hbm_fraction_fused": bytes_alg / (ms["fused_total"] * 1e-3) / HBM_PEAK,
            "speedup_vs_torch": ms["torch_total"] / ms["fused_total"], "points_splatted_nonempty_pixels": valid,
            "pixels_equal_to_torch_composition": float((ours == theirs).mean()), "pixels_nonzero": float((ours > 0).mean())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=2.0, help="total time of every timed loop, over all rounds")
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gtgen_bench.py needs a GPU: a time measured anywhere else says nothing about it")
    out = {"device": torch.cuda.get_device_name(0), "hbm_peak_bytes_per_s": HBM_PEAK,
           "cases": [case("kitti", 76, 192, 640, True, a.seconds, a.rounds), case("matterport", 40, 480, 640, False, a.seconds, a.rounds)]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
