"""GPU box: time of predict_simple's overlay on the device (csrc/visualise.hip) next to the host path it restates
(`InferenceManager.visualise`: Pillow's mode-"F" BILINEAR, matplotlib's colour map, a float64 blend -- on one core of the same machine), for

* one KITTI batch of 12: photos of 375 x 1242 over predictions of 192 x 640, and
* one Matterport frame: 1024 x 1280 over 512 x 640;

then the wall time per image of folder prediction -- decode, forward, .npy, overlay, JPEG -- with
`--device_resize --device_vis --batch_size 12` against the default path (per-image forward, host resize, host overlay: the code every
earlier commit runs) on the same folder in the same process, each after a warm-up pass over the folder, in alternating passes (the median is reported).

    python scripts/vis_bench.py [--seconds 2.0] [--rounds 5] [--files 24] [--folder_rounds 3]

HIP events after a warm-up, alternating round by round; every timed loop runs for about `--seconds` in total.  Prints one JSON line.
Algorithmic bytes of the overlay per output pixel: both float maps of the intermediate written and read at the photo's width, the resized
depth and the mask written and read, the photo read and the overlay written."""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from footprints_amd import ops
from tests import vis_restatement as VR

HBM_ACHIEVABLE = 6.3e12    # bytes / s: what a float4 copy reaches on this chip
WORKLOADS = {"kitti_batch_of_12": (12, (192, 640), (375, 1242)), "matterport_one_frame": (1, (512, 640), (1024, 1280))}


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


def overlay_workload(name, a):
    from PIL import Image
    from footprints_amd.predict_simple import InferenceManager
    B, (H, W), (h, w) = WORKLOADS[name]
    preds = np.stack([VR.prediction(H, W, 200 + i) for i in range(B)])
    photos = [VR.original(h, w, 300 + i) for i in range(B)]
    tables = ops.vis_table_set("cuda")
    records, total, max_h, max_w = ops.vis_records([(h, w)] * B, H, W, tables)
    d_pred = torch.from_numpy(preds).cuda()
    d_src = torch.from_numpy(np.concatenate([p.reshape(-1) for p in photos])).cuda()
    d_rec = torch.from_numpy(records).cuda()
    d_out = torch.empty(total, dtype=torch.uint8, device="cuda")
    h_out = torch.empty(total, dtype=torch.uint8).pin_memory()
    legs = {
        "kernels": lambda: ops.vis_overlay_packed(d_pred, d_src, total, d_rec, max_h, max_w, tables, out=d_out),
        "kernels_and_d2h": lambda: h_out.copy_(ops.vis_overlay_packed(d_pred, d_src, total, d_rec, max_h, max_w, tables, out=d_out), non_blocking=True),
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
    pil = [Image.fromarray(p) for p in photos]
    host, calls = host_ms(lambda: [InferenceManager.visualise(preds[i], pil[i]) for i in range(B)], a.seconds)
    legs["kernels_and_d2h"]()
    torch.cuda.synchronize()
    ref = np.concatenate([InferenceManager.visualise(preds[i], pil[i]).reshape(-1) for i in range(B)])
    px = B * h * w
    bytes_alg = B * H * w * 2 * 4 * 2 + px * (4 + 1) * 2 + px * 3 * 2 + B * H * W * 2 * 4
    return {"batch": B, "prediction": [H, W], "photo": [h, w], "ms": ms, "spread": spread, "calls_per_round": iters,
            "host_visualise_one_core_ms": host, "host_calls": calls, "bytes_equal_to_host": bool(np.array_equal(h_out.numpy(), ref)),
            "mask_fraction": float((ref.reshape(-1, 3) != np.concatenate([p.reshape(-1, 3) for p in photos])).any(axis=1).mean()),
            "algorithmic_bytes": bytes_alg, "bytes_per_output_pixel": bytes_alg / px,
            "fraction_of_achievable_hbm": bytes_alg / (ms["kernels"] * 1e-3) / HBM_ACHIEVABLE,
            "speedup_vs_host_one_core": host / ms["kernels_and_d2h"]}


def folder_prediction(a):
    from PIL import Image
    from footprints_amd.model_manager import ModelManager
    from footprints_amd.predict_simple import InferenceManager
    torch.manual_seed(5)
    mm = ModelManager(is_inference=True)
    out = {"files": a.files, "photo": [375, 1242], "model": "kitti, random weights"}
    with tempfile.TemporaryDirectory() as tmp:
        folder = os.path.join(tmp, "photos")
        os.makedirs(folder)
        for i in range(a.files):
            Image.fromarray(VR.original(375, 1242, 400 + i)).save(os.path.join(folder, "%03d.png" % i))
        configs = {"default_path": {}, "device_resize_vis_batch_12": dict(device_resize=True, device_vis=True, batch_size=12),
                   "device_resize_vis_batch_1": dict(device_resize=True, device_vis=True)}
        with open(os.devnull, "w") as devnull:
            stdout, sys.stdout = sys.stdout, devnull
            try:
                ims = {tag: InferenceManager("kitti", os.path.join(tmp, tag), model_manager=mm, **kw) for tag, kw in configs.items()}
                for im in ims.values():
                    im.predict(folder)                              # warm-up: plans, tables, workspaces
                samples = {tag: [] for tag in ims}
                for _ in range(a.folder_rounds):                    # alternating, so a busy host weighs on every configuration
                    for tag, im in ims.items():
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        im.predict(folder)
                        torch.cuda.synchronize()
                        samples[tag].append((time.perf_counter() - t0) * 1e3 / a.files)
            finally:
                sys.stdout = stdout
        for tag, v in samples.items():
            out[tag + "_ms_per_image"] = float(np.median(v))
            out[tag + "_ms_per_image_rounds"] = v
        # where the time of one image goes on the host side of either path
        pil = Image.open(os.path.join(folder, "000.png"))
        out["decode_png_ms"] = host_ms(lambda: Image.open(os.path.join(folder, "000.png")).convert("RGB"), 0.5)[0]
        vis = np.asarray(pil.convert("RGB"))
        out["encode_jpeg_ms"] = host_ms(lambda: Image.fromarray(vis).save(os.path.join(tmp, "x.jpg"), quality=95), 0.5)[0]
        pred = np.zeros((4, 192, 640), np.float32)
        out["save_npy_ms"] = host_ms(lambda: np.save(os.path.join(tmp, "x.npy"), pred), 0.5)[0]
    out["batched_device_path_is_faster"] = out["device_resize_vis_batch_12_ms_per_image"] < out["default_path_ms_per_image"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=2.0, help="total time of every timed loop, over all rounds")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--files", type=int, default=24, help="photos in the folder of the folder-prediction comparison")
    ap.add_argument("--folder_rounds", type=int, default=3, help="timed passes over the folder per configuration, alternating")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("vis_bench.py needs a GPU: a time measured anywhere else says nothing about it")
    torch.set_num_threads(1)
    out = {"device": torch.cuda.get_device_name(0), "hbm_achievable_bytes_per_s": HBM_ACHIEVABLE}
    for name in WORKLOADS:
        out[name] = overlay_workload(name, a)
    out["folder_prediction"] = folder_prediction(a)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
