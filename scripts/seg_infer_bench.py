"""GPU box: frames per second of the segmentation network's inference mode (preprocessing/segmentation/inference.Tester) at 192 x 640,
batch 12, on synthetic frames held in memory at KITTI's native sizes (375 x 1242, 370 x 1226, 376 x 1241, mixed in one batch).

    python scripts/seg_infer_bench.py [--frames 240] [--rounds 5] [--pack-iters 200]

With and without the pyramid-pooling module, three routes, alternated inside every round, medians over the rounds:
  pipeline      Tester.test(): reader threads, device half, results through the pinned ring, np.save of every frame to a temporary folder
  device_half   the device half alone: upload, resize, ToTensor, network (full-resolution head only), fp_seg_pack, copy back
  parent        what the package offered before: Image.resize(LANCZOS) on one host core -> InferenceManager.test_batch (all four heads,
                float32 to the host, torch's sigmoid) -> astype(float16); no file is written on this route
`pipeline_pictures` is the first route with --save_test_visualisations (the writer thread also encodes one JPEG per frame).
fp_seg_pack alone (HIP events) is set against its algorithmic bytes -- 4 B read + 2 B written per pixel, 12 B + 6 B more with the
picture -- over buffer sets rotated through more memory than the last-level cache holds.  Prints one JSON line."""
import argparse
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
from footprints_amd.datasets.ring import full_resolution_heads
from footprints_amd.preprocessing.segmentation.datasets.inference import KITTIInferenceDataset
from footprints_amd.preprocessing.segmentation.inference import InferenceManager, Tester
from footprints_amd.preprocessing.segmentation.network import Segmentor
from footprints_amd.preprocessing.segmentation.options import SegmentationOptions

B, H, W = 12, 192, 640
NATIVE = [(375, 1242), (370, 1226), (376, 1241)]


class MemoryKITTI(KITTIInferenceDataset):
    """`n` frames cycling over a small pool of decoded frames"""

    def __init__(self, pool, n):
        super().__init__("", ["seq/drive_%04d %d l" % (i // 1000, i) for i in range(n)], H, W)
        self.pool = pool

    def _load_image(self, index):
        return self.pool[index % len(self.pool)]


def parent_route(manager, frames):
    from PIL import Image
    for k in range(0, len(frames), B):
        batch = np.stack([np.asarray(Image.fromarray(f).resize((W, H), Image.LANCZOS)) for f in frames[k:k + B]])
        image = torch.from_numpy(batch).permute(0, 3, 1, 2).contiguous().float().div(255)
        manager.test_batch({"image": image}).astype(np.float16)


def device_half_route(tester, frames):
    ring = tester.ring
    with full_resolution_heads(tester.model):
        for k in range(0, len(frames), B):
            si = (k // B) % len(ring.slots)
            ring.slots[si]["ready"].synchronize()              # as in test(): a slot's pinned buffers are refilled only after its copies have landed
            ring.ahead(si, [{"image": f} for f in frames[k:k + B]])
            ring.rest(si)
    torch.cuda.synchronize()


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def pack_alone(picture, iters, rounds):
    """median microseconds of one fp_seg_pack on the engine's layout, and the GB/s its algorithmic bytes make of that"""
    per_call = B * H * W * (6 + (18 if picture else 0))
    footprint = B * H * W * (8 + 2 + (36 + 6 if picture else 0))          # what a set occupies: both channels of the head buffer
    nsets = max(2, -(-(768 << 20) // footprint))
    sets = []
    for _ in range(nsets):
        head = torch.randn((B, 2, H, W), device="cuda") * 4
        image = torch.rand((B, 3, H, W), device="cuda") if picture else None
        out = (torch.empty((B, 1, H, W), dtype=torch.float16, device="cuda"), None,
               torch.empty((B, H, 2 * W, 3), dtype=torch.uint8, device="cuda") if picture else None)
        sets.append((head[:, 0:1], image, out))
    run = lambda s: ops.seg_pack(s[0], s[1], want_picture=picture, out=s[2])
    for s in sets:
        run(s)
    torch.cuda.synchronize()
    times = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for i in range(iters):
            run(sets[i % nsets])
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3 / iters)
    us = statistics.median(times)
    return {"us": round(us, 2), "us_min": round(min(times), 2), "us_max": round(max(times), 2), "algorithmic_bytes": per_call,
            "GBps": round(per_call / us / 1e3, 1), "buffer_sets": nsets}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=240)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--pack-iters", type=int, default=200)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("seg_infer_bench needs a MI355X: a timing taken elsewhere says nothing")
    rng = np.random.default_rng(3)
    pool = [rng.integers(0, 256, NATIVE[i % 3] + (3,), dtype=np.uint8) for i in range(2 * B)]
    frames = [pool[i % len(pool)] for i in range(args.frames)]
    result = {"bench": "seg_infer", "B": B, "H": H, "W": W, "frames": args.frames, "rounds": args.rounds}
    for psp in (True, False):
        torch.manual_seed(1)
        model = Segmentor(pretrained=False, use_PSP=psp).cuda()
        base = ["--mode", "inference", "--height", str(H), "--width", str(W), "--batch_size", str(B), "--num_workers", "4"]
        fps = {"pipeline": [], "pipeline_pictures": [], "device_half": [], "parent": []}
        with tempfile.TemporaryDirectory() as tmp:
            testers = {}
            for key, extra in (("pipeline", []), ("pipeline_pictures", ["--save_test_visualisations"])):
                testers[key] = Tester(SegmentationOptions().parse(base + extra), model=model, dataset=MemoryKITTI(pool, args.frames),
                                      save_path=os.path.join(tmp, key))
            manager = InferenceManager(model=model)
            routes = {"pipeline": lambda: testers["pipeline"].test(), "pipeline_pictures": lambda: testers["pipeline_pictures"].test(),
                      "device_half": lambda: device_half_route(testers["pipeline"], frames), "parent": lambda: parent_route(manager, frames)}
            for key in ("pipeline", "pipeline_pictures"):            # warm-up: every shape of the timed windows, the short last batch included
                testers[key].dataset = MemoryKITTI(pool, 2 * B + 5)
                testers[key].test()
                testers[key].dataset = MemoryKITTI(pool, args.frames)
            device_half_route(testers["pipeline"], frames[:2 * B])
            parent_route(manager, frames[:2 * B])
            for _ in range(args.rounds):
                for key, fn in routes.items():
                    fps[key].append(args.frames / wall(fn))
        result["psp" if psp else "no_psp"] = {k: {"fps": round(statistics.median(v), 1), "fps_min": round(min(v), 1), "fps_max": round(max(v), 1)}
                                              for k, v in fps.items()}
        del model, testers, manager
    result["seg_pack"] = {"plain": pack_alone(False, args.pack_iters, args.rounds), "picture": pack_alone(True, args.pack_iters, args.rounds)}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
