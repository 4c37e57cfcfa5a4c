"""GPU box: time of the reader work for one KITTI batch of 12 -- mixed native frame sizes -> 192 x 640 through Pillow's LANCZOS, and the
depth-mask filter on 192 x 640 masks at ~10 % density -- on the device (csrc/resample_u8.hip, csrc/reader.hip) next to the host path it replaces, measured on
the same machine: PIL.Image.resize and scipy.ndimage.label + the reference's loop (footprint_dataset.py:96-105), each on one core.

    python scripts/reader_bench.py [--seconds 2.0] [--rounds 5]

HIP events after a warm-up, alternating round by round; every timed loop runs for about `--seconds` in total.  Prints one JSON line.
Algorithmic bytes of the resize: every source byte read once, the uint8 intermediate written and read once, the output written once."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from footprints_amd import ops
from tests.golden import reader_inputs as RI

HBM_PEAK = 8.0e12          # bytes / s, MI355X specification
HBM_ACHIEVABLE = 6.3e12    # what a float4 copy reaches on this chip
KITTI_SIZES = [(375, 1242), (370, 1224), (374, 1238), (376, 1241)]
B, H, W = 12, 192, 640


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def host_ms(fn, seconds):
    fn()
    n, t0 = 0, time.perf_counter()
    while n < 3 or time.perf_counter() - t0 < seconds:
        fn()
        n += 1
    return (time.perf_counter() - t0) * 1e3 / n, n


def host_filter(mask, label):
    processed = np.zeros_like(mask)
    connected = label(mask)
    for index in range(1, connected.max() + 1):
        size = (connected == index).sum()
        if size < W * H / 100:
            processed[connected == index] = 1
    return processed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=2.0, help="total time of every timed loop, over all rounds")
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("reader_bench.py needs a GPU: a time measured anywhere else says nothing about it")
    frames = [RI.image(*KITTI_SIZES[i % len(KITTI_SIZES)], 3, i) for i in range(B)]
    masks = np.stack([RI.random_mask(H, W, 10, i) for i in range(B)])
    tables = ops.resize_table_set("cuda")
    packed, records, total, C, max_h, max_w = ops.resize_pack(frames, H, W, tables)
    h_src = torch.from_numpy(packed).pin_memory()
    d_src, d_rec = h_src.cuda(), torch.from_numpy(records).cuda()
    d_out = torch.empty((B, H, W, 3), dtype=torch.uint8, device="cuda")
    d_masks = {"f32": torch.from_numpy(masks.astype(np.float32)).cuda(), "f64": torch.from_numpy(masks).cuda()}
    d_mout = {k: torch.empty_like(v) for k, v in d_masks.items()}
    legs = {
        "resize": lambda: ops.resize_u8_packed(d_src, total, d_rec, B, H, W, 3, max_h, max_w, tables, out=d_out),
        "resize_with_upload": lambda: (d_src.copy_(h_src, non_blocking=True),
                                       ops.resize_u8_packed(d_src, total, d_rec, B, H, W, 3, max_h, max_w, tables, out=d_out)),
        "resize_to_tensor": lambda: ops.to_tensor_u8(ops.resize_u8_packed(d_src, total, d_rec, B, H, W, 3, max_h, max_w, tables, out=d_out)),
        "filter_f32": lambda: ops.filter_depth_mask(d_masks["f32"], out=d_mout["f32"]),
        "filter_f64": lambda: ops.filter_depth_mask(d_masks["f64"], out=d_mout["f64"]),
    }
    iters = {}
    for leg, fn in legs.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        iters[leg] = max(3, int(a.seconds * 1e3 / a.rounds / max(timed(fn, 3), 1e-3)))
    samples = {leg: [] for leg in legs}
    for _ in range(a.rounds):
        for leg, fn in legs.items():
            samples[leg].append(timed(fn, iters[leg]))
    ms = {leg: float(np.median(v)) for leg, v in samples.items()}
    spread = {leg: float((max(v) - min(v)) / np.median(v)) for leg, v in samples.items()}

    out = {"device": torch.cuda.get_device_name(0), "hbm_peak_bytes_per_s": HBM_PEAK, "hbm_achievable_bytes_per_s": HBM_ACHIEVABLE, "batch": B, "height": H, "width": W,
           "source_sizes": KITTI_SIZES, "mask_density": float(masks.mean()), "ms": ms, "spread": spread, "calls_per_round": iters, "rounds": a.rounds}
    inter = sum(f.shape[0] * W * 3 for f in frames)
    bytes_alg = total + 2 * inter + B * H * W * 3
    out["resize_bytes"] = {"source": total, "intermediate_written_and_read": 2 * inter, "output": B * H * W * 3, "total": bytes_alg}
    out["resize_fraction_of_achievable_hbm"] = bytes_alg / (ms["resize"] * 1e-3) / HBM_ACHIEVABLE

    # the host path on ONE core of this machine
    torch.set_num_threads(1)
    host = {}
    try:
        from PIL import Image
        pil = [Image.fromarray(f) for f in frames]
        host["pillow_resize_ms"], host["pillow_resize_calls"] = host_ms(lambda: [p.resize((W, H), Image.LANCZOS) for p in pil], a.seconds)
        ref = np.stack([np.asarray(p.resize((W, H), Image.LANCZOS)) for p in pil])
        legs["resize"]()
        out["resize_bytes_equal_to_pillow"] = bool(np.array_equal(d_out.cpu().numpy(), ref))
        import PIL
        host["pillow_version"] = PIL.__version__
    except ImportError:
        host["pillow_resize_ms"] = None
    try:
        import scipy.ndimage
        label = lambda m: scipy.ndimage.label(m, structure=np.ones((3, 3)))[0]
        host["filter"] = "scipy.ndimage.label + the reference's loop"
    except ImportError:
        from tests import reader_restatement as RR
        label = RR.components
        host["filter"] = "flood fill in Python + the reference's loop"
    host["filter_ms"], host["filter_calls"] = host_ms(lambda: [host_filter(m, label) for m in masks], a.seconds)
    legs["filter_f64"]()
    out["filter_equal_to_host"] = bool(np.array_equal(d_mout["f64"].cpu().numpy(), np.stack([host_filter(m, label) for m in masks])))
    out["host_one_core"] = host
    if host.get("pillow_resize_ms"):
        out["resize_speedup_vs_pillow_one_core"] = host["pillow_resize_ms"] / ms["resize_with_upload"]
    out["filter_speedup_vs_host_one_core"] = host["filter_ms"] / ms["filter_f64"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
