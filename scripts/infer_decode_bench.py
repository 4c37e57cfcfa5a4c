"""GPU box: frames per second of the two inference pipelines with and without --device_decode (DESIGN.md section 0, N12;
profiles/infer_decode_notes.md), on a folder of picture-like 375 x 1242 frames (scripts/jpeg_decode_bench.py's `photo`) written by
Pillow at quality 95, 4:2:0, at 192 x 640 and batch 12.

    python scripts/infer_decode_bench.py [--frames 240] [--rounds 5] [--pool 12] [--pack-iters 200] [--workers 1 4 16]

Routes, alternated inside every round; median, smallest and largest round:
  seg/<w>/<host|device>[/pictures]    preprocessing/segmentation/inference.Tester.test() at --num_workers w, files decoded on the reader
                                      threads or on the device; `pictures` = --save_test_visualisations --device_jpeg
  main/<w>/<host|device>[/pictures]   evaluation/inference.InferenceManager.run_dataset the same way
  main/blocking                       what the package offered before: InferenceManager.run(loader) over the same files -- Pillow's
                                      decode and LANCZOS resize on one core, a blocking step and a .cpu() per batch
`condition` repeats the issue's: at 4 workers a pipeline with device decoding is not slower than without by more than the run's own
round-to-round spread.  fp_infer_pack alone (HIP events) is set against fp_pack_pred_fp16 + fp_vis_side_by_side over buffer sets
rotated through more memory than the last-level cache holds.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from footprints_amd import ops
from footprints_amd.datasets.inference import KITTIInferenceDataset
from footprints_amd.evaluation.inference import InferenceManager
from footprints_amd.model_manager import ModelManager
from footprints_amd.preprocessing.segmentation.datasets.inference import KITTIInferenceDataset as SegKITTI
from footprints_amd.preprocessing.segmentation.inference import Tester
from footprints_amd.preprocessing.segmentation.network import Segmentor
from footprints_amd.preprocessing.segmentation.options import SegmentationOptions
from scripts.jpeg_decode_bench import photo, wall

B, H, W = 12, 192, 640


def cycling(cls, folder, pool, n):
    """a dataset of n frames that cycles over the folder's `pool` files"""
    class Cycling(cls):
        def image_path(self, index):
            return os.path.join(folder, "%04d.jpg" % (index % pool))
    return Cycling(folder, ["seq/drive_%04d %d l" % (i // 1000, i) for i in range(n)], H, W)


def spread(values):
    return {"fps": round(statistics.median(values), 1), "fps_min": round(min(values), 1), "fps_max": round(max(values), 1)}


def blocking_loader(dataset):
    """the reference reader's batches, made on the calling thread: decode, Image.resize(LANCZOS), ToTensor"""
    from PIL import Image
    for k in range(0, len(dataset), B):
        frames = []
        for i in range(k, min(k + B, len(dataset))):
            with Image.open(dataset.image_path(i)) as im:
                frames.append(np.asarray(im.convert("RGB").resize((W, H), Image.LANCZOS)))
        image = torch.from_numpy(np.stack(frames)).permute(0, 3, 1, 2).contiguous().float().div(255)
        yield {"image": image, "idx": ["%03d" % i for i in range(k, k + len(frames))]}


def pack_alone(picture, iters, rounds):
    """median microseconds of fp_infer_pack and of the two launches it replaces"""
    footprint = B * H * W * (16 + 8 + (12 + 6 if picture else 0))
    nsets = max(2, -(-(768 << 20) // footprint))
    sets = []
    for _ in range(nsets):
        pred = torch.randn((B, 4, H, W), device="cuda") * 4
        image = torch.rand((B, 3, H, W), device="cuda") if picture else None
        sets.append((pred, image, torch.empty((B, 4, H, W), dtype=torch.float16, device="cuda"),
                     torch.empty((B, H, 2 * W, 3), dtype=torch.uint8, device="cuda") if picture else None))

    def one(s):
        ops.infer_pack(s[0], s[1], want_picture=picture, out=(s[2], s[3]))

    def two(s):
        ops.pack_pred_fp16(s[0], out=s[2])
        if picture:
            ops.vis_side_by_side(s[1], s[0], out=s[3])

    out = {"algorithmic_bytes": B * H * W * (16 + 8 + (12 + 6 if picture else 0)), "buffer_sets": nsets}
    times = {"infer_pack": [], "two_launches": []}
    for s in sets:
        one(s)
        two(s)
    torch.cuda.synchronize()
    for _ in range(rounds):
        for key, run in (("infer_pack", one), ("two_launches", two)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for i in range(iters):
                run(sets[i % nsets])
            b.record()
            b.synchronize()
            times[key].append(a.elapsed_time(b) * 1e3 / iters)
    for key, v in times.items():
        out[key] = {"us": round(statistics.median(v), 2), "us_min": round(min(v), 2), "us_max": round(max(v), 2)}
    out["infer_pack"]["GBps"] = round(out["algorithmic_bytes"] / out["infer_pack"]["us"] / 1e3, 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=240)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--pool", type=int, default=12)
    ap.add_argument("--pack-iters", type=int, default=200)
    ap.add_argument("--workers", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    ap.add_argument("--pack-only", action="store_true", help="time fp_infer_pack next to the two launches and nothing else")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("infer_decode_bench needs a MI355X: a timing taken elsewhere says nothing")
    result = {"bench": "infer_decode", "B": B, "H": H, "W": W, "frames": args.frames, "rounds": args.rounds, "pool": args.pool}
    if not args.pack_only:
        pipelines(args, result)
    result["infer_pack"] = {"plain": pack_alone(False, args.pack_iters, args.rounds), "picture": pack_alone(True, args.pack_iters, args.rounds)}
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


def pipelines(args, result):
    from PIL import Image
    with tempfile.TemporaryDirectory() as tmp:
        folder = os.path.join(tmp, "frames")
        os.makedirs(folder)
        for i in range(args.pool):
            Image.fromarray(photo(375, 1242, 80 + i)).save(os.path.join(folder, "%04d.jpg" % i), quality=95, subsampling=2)
        result["file_bytes_mean"] = int(np.mean([os.path.getsize(os.path.join(folder, f)) for f in os.listdir(folder)]))
        torch.manual_seed(1)
        seg_model = Segmentor(pretrained=False, use_PSP=True).cuda()
        mm = ModelManager(is_inference=True)
        routes, counters = {}, {}
        warm = 2 * B + 5                                # warm-up: every shape of the timed windows, the short last batch included
        for w in args.workers:
            for pictures in (False, True):
                for dd in (False, True):
                    tail = "%d/%s%s" % (w, "device" if dd else "host", "/pictures" if pictures else "")
                    opt = SegmentationOptions().parse(["--mode", "inference", "--height", str(H), "--width", str(W), "--batch_size", str(B),
                                                       "--num_workers", str(w)] + (["--save_test_visualisations", "--device_jpeg"] if pictures else [])
                                                      + (["--device_decode"] if dd else []))
                    tester = Tester(opt, model=seg_model, dataset=cycling(SegKITTI, folder, args.pool, warm), save_path=os.path.join(tmp, "seg", tail))
                    tester.test()
                    tester.dataset = cycling(SegKITTI, folder, args.pool, args.frames)
                    routes["seg/" + tail] = tester.test
                    im = InferenceManager(model_manager=mm, save_path=os.path.join(tmp, "main", tail), save_test_visualisations=pictures,
                                          device_jpeg=pictures)
                    im.run_dataset(cycling(KITTIInferenceDataset, folder, args.pool, warm), B, num_workers=w, device_decode=dd)
                    dataset = cycling(KITTIInferenceDataset, folder, args.pool, args.frames)

                    def run(im=im, dataset=dataset, w=w, dd=dd, key="main/" + tail):
                        counters[key] = im.run_dataset(dataset, B, num_workers=w, device_decode=dd)
                    routes["main/" + tail] = run
        blocking = InferenceManager(model_manager=mm, save_path=os.path.join(tmp, "main", "blocking"))
        dataset = cycling(KITTIInferenceDataset, folder, args.pool, args.frames)
        blocking.run(blocking_loader(cycling(KITTIInferenceDataset, folder, args.pool, warm)))
        routes["main/blocking"] = lambda: blocking.run(blocking_loader(dataset))
        fps = {key: [] for key in routes}
        devnull = open(os.devnull, "w")
        for r in range(args.rounds):
            print("round %d of %d" % (r + 1, args.rounds), file=sys.stderr, flush=True)
            for key, fn in routes.items():
                stdout, sys.stdout = sys.stdout, devnull            # the pipelines print their progress lines
                try:
                    seconds = wall(fn)
                finally:
                    sys.stdout = stdout
                fps[key].append(args.frames / seconds)
        result["routes"] = {key: spread(v) for key, v in fps.items()}
        result["counters"] = {key: c for key, c in counters.items() if "/device" in key}
        cond = {}
        for pipe in ("seg", "main"):
            for tail in ("", "/pictures"):
                if 4 not in args.workers:
                    continue
                host, dev = fps["%s/4/host%s" % (pipe, tail)], fps["%s/4/device%s" % (pipe, tail)]
                width = max(max(host) - min(host), max(dev) - min(dev))
                cond["%s%s" % (pipe, tail)] = {"host": round(statistics.median(host), 1), "device": round(statistics.median(dev), 1),
                                               "spread": round(width, 1), "holds": statistics.median(dev) >= statistics.median(host) - width}
        result["condition"] = cond


if __name__ == "__main__":
    main()
