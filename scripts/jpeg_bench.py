"""GPU box: the device JPEG encoder (csrc/jpeg.hip) against Pillow's on one core, on the two kinds of picture the package writes, and the
three routes that write them with and without --device_jpeg.

    python scripts/jpeg_bench.py [--frames 240] [--photos 24] [--rounds 5] [--iters 50]

Two workloads, both drawn on the device from synthetic, picture-like frames (smooth shading, a few shapes, mild noise; pure noise
compresses ten times worse and is not what these routes write):
  seg_pictures   12 pictures of 192 x 1280 out of fp_seg_pack (the network's input beside the plasma map of its prediction)
  overlays       12 overlays of 375 x 1242 out of fp_vis_overlay
For each, in the same run: `launches_us` the encoder's six launches between two device events (median over --rounds of --iters calls),
`call_ms` one call with its copies (length table to the host, wait, the bytes in use, headers), `pillow_ms` Image.save(quality=95) of
the same 12 pictures on one core, `bytes` what the files weigh.  Kernel durations are NOT in here: they need a trace of their own.
Then the routes, alternated inside every round, median over the rounds with smallest and largest:
  tester          Tester.test() at 192 x 640, batch 12: no pictures / pictures encoded by the writer thread / pictures with --device_jpeg
  predict_simple  a folder of --photos files with --device_resize --device_vis --batch_size 12, without and with --device_jpeg
Prints one JSON line."""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from footprints_amd import ops
from footprints_amd.preprocessing.segmentation.datasets.inference import KITTIInferenceDataset
from footprints_amd.preprocessing.segmentation.inference import Tester
from footprints_amd.preprocessing.segmentation.network import Segmentor
from footprints_amd.preprocessing.segmentation.options import SegmentationOptions

B, H, W = 12, 192, 640
NATIVE = [(375, 1242), (370, 1226), (376, 1241)]


def photo(h, w, seed):
    """a picture-like frame: sky-to-ground shading, a few flat shapes, mild sensor noise"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    img = np.stack([90 + 100 * yy / h + 20 * np.sin(xx / 97), 110 + 60 * yy / h + 25 * np.cos(xx / 61), 160 - 70 * yy / h + 15 * np.sin((xx + yy) / 45)], -1)
    for _ in range(12):
        cy, cx, r = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(10, 90)
        inside = (yy - cy) ** 2 + ((xx - cx) / 2) ** 2 < r * r
        img[inside] = img[inside] * 0.4 + rng.uniform(0, 255, 3) * 0.6
    return np.clip(img + rng.normal(0, 2.5, img.shape), 0, 255).astype(np.uint8)


class MemoryKITTI(KITTIInferenceDataset):
    def __init__(self, pool, n):
        super().__init__("", ["seq/drive_%04d %d l" % (i // 1000, i) for i in range(n)], H, W)
        self.pool = pool

    def _load_image(self, index):
        return self.pool[index % len(self.pool)]


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def spread(values, digits=2):
    return {"median": round(statistics.median(values), digits), "min": round(min(values), digits), "max": round(max(values), digits)}


def encoder_alone(buffer, total, shapes, iters, rounds):
    """the encoder on pictures lying in a device buffer: launches between events, the whole call, Pillow on one core"""
    from PIL import Image
    n = len(shapes)
    records, _, max_h, max_w = ops.jpeg_records(shapes)
    rec = torch.from_numpy(records).cuda()
    out = torch.empty(ops.jpeg_max_scan_bytes(n, max_h, max_w), dtype=torch.uint8, device="cuda")
    table = torch.empty((n + 1, 2), dtype=torch.int64, device="cuda")
    launch = lambda: ops.jpeg_encode_packed(buffer, total, rec, n, 95, out=out, max_h=max_h, max_w=max_w, table=table)

    def call():
        launch()
        t = table.cpu().numpy()
        return ops.jpeg_files(out[:int(t[n][0])].cpu().numpy(), t, shapes, 95)
    files = call()
    pictures = ops.split_pictures(buffer[:total].cpu().numpy(), shapes)

    def pillow():
        made = []
        for p in pictures:
            buf = io.BytesIO()
            Image.fromarray(p).save(buf, format="JPEG", quality=95)
            made.append(buf.getvalue())
        return made
    equal = pillow() == files
    launches = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            launch()
        b.record()
        b.synchronize()
        launches.append(a.elapsed_time(b) * 1e3 / iters)
    calls = [wall(call) * 1e3 for _ in range(rounds)]
    pil = [wall(pillow) * 1e3 for _ in range(rounds)]
    return {"pictures": n, "bytes": sum(len(f) for f in files), "raw_bytes": int(total), "equal_to_pillow": bool(equal),
            "launches_us": spread(launches, 1), "call_ms": spread(calls), "pillow_ms": spread(pil)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=240)
    ap.add_argument("--photos", type=int, default=24)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("jpeg_bench needs a MI355X: a timing taken elsewhere says nothing")
    from PIL import features
    pool = [photo(*NATIVE[i % 3], 50 + i) for i in range(2 * B)]
    result = {"bench": "jpeg", "B": B, "frames": args.frames, "photos": args.photos, "rounds": args.rounds, "iters": args.iters,
              "libjpeg_turbo": bool(features.check_feature("libjpeg_turbo"))}

    # ---- the segmentation route's pictures, and its pipeline
    torch.manual_seed(1)
    model = Segmentor(pretrained=False, use_PSP=True).cuda()
    base = ["--mode", "inference", "--height", str(H), "--width", str(W), "--batch_size", str(B), "--num_workers", "4"]
    extras = {"no_pictures": [], "pictures": ["--save_test_visualisations"], "pictures_device_jpeg": ["--save_test_visualisations", "--device_jpeg"]}
    with tempfile.TemporaryDirectory() as tmp:
        testers = {k: Tester(SegmentationOptions().parse(base + e), model=model, dataset=MemoryKITTI(pool, args.frames), save_path=os.path.join(tmp, k))
                   for k, e in extras.items()}
        with contextlib.redirect_stdout(io.StringIO()):
            for t in testers.values():                          # warm-up: every shape of the timed windows, the short last batch included
                t.dataset = MemoryKITTI(pool, 2 * B + 5)
                t.test()
                t.dataset = MemoryKITTI(pool, args.frames)
            t = testers["pictures"]
            t.test_batch(pool[:B])
            result["seg_pictures"] = encoder_alone(t.ring.slots[0]["d_pic"].view(-1), B * H * 2 * W * 3, [(H, 2 * W)] * B, args.iters, args.rounds)
            fps = {k: [] for k in testers}
            for _ in range(args.rounds):
                for k, t in testers.items():
                    fps[k].append(args.frames / wall(t.test))
        result["tester_fps"] = {k: spread(v, 1) for k, v in fps.items()}
    del testers, model

    # ---- the overlays, and folder prediction
    from PIL import Image
    from footprints_amd.model_manager import ModelManager
    from footprints_amd.predict_simple import InferenceManager
    torch.manual_seed(5)
    mm = ModelManager(is_inference=True)
    with tempfile.TemporaryDirectory() as tmp:
        folder = os.path.join(tmp, "photos")
        os.makedirs(folder)
        for i in range(args.photos):
            Image.fromarray(pool[i % len(pool)]).save(os.path.join(folder, "%04d.jpg" % i), quality=95)
        managers = {k: InferenceManager("kitti", os.path.join(tmp, k), model_manager=mm, device_resize=True, device_vis=True, batch_size=B,
                                        device_jpeg=(k == "device_jpeg")) for k in ("host_jpeg", "device_jpeg")}
        with contextlib.redirect_stdout(io.StringIO()):
            for m in managers.values():
                m.predict(folder)
            big = [photo(375, 1242, 80 + i) for i in range(B)]
            with torch.no_grad():
                pred = mm.model(ops.load_images_u8(big, 192, 640))["1/1"].contiguous()
            buffer, total, shapes = ops.vis_overlay_device(pred, originals=big)
            torch.cuda.synchronize()
            result["overlays"] = encoder_alone(buffer, total, shapes, args.iters, args.rounds)
            ms = {k: [] for k in managers}
            for _ in range(args.rounds):
                for k, m in managers.items():
                    ms[k].append(wall(lambda: m.predict(folder)) * 1e3 / args.photos)
        result["predict_simple_ms_per_image"] = {k: spread(v, 3) for k, v in ms.items()}
        result["predict_simple_files_equal"] = all(
            open(os.path.join(tmp, "host_jpeg", "visualisations", f), "rb").read() == open(os.path.join(tmp, "device_jpeg", "visualisations", f), "rb").read()
            for f in sorted(os.listdir(os.path.join(tmp, "host_jpeg", "visualisations"))))
    print(json.dumps(result))


if __name__ == "__main__":
    main()
