"""GPU box: the ground-segmentation trainer fed from FILES -- what --num_workers and --device_decode change -- for batches of 12 at
192 x 640 over a synthetic on-disk tree this script writes with Pillow and numpy: Matterport-like 1024 x 1280 JPEGs with .npy masks, an
ADE20K-like mix of JPEGs with _seg.png label images, and Cityscapes-like 1024 x 2048 PNGs.

    python scripts/seg_train_reader_bench.py [--root DIR] [--legs a,b,c,d,e] [--files 24] [--repeat 15] [--rounds 5] [--seconds 2.0]

Legs (ms per step of 12 by a host clock around a loop that ends in a device synchronise, the loader's first two batches left out):
  a  Segmentor train step alone, batch resident
  b  the trainer's loaders (Trainer.create_dataloaders) over the files, --num_workers 0: one batch's files read and decoded one after the
     other on the staging thread.  Legs a and b use nothing newer than the loaders themselves, so `--legs a,b` also runs from a checkout
     of an older commit (copy this file into its scripts/): that run is the baseline
  c  as b with --num_workers 4 and 16
  d  as c with --device_decode; its epoch-end counters are reported
  c and d also time their loader with nobody training (ms per batch): a loop slower than leg a although its loader alone is faster than
  the step waits for the device, not for the files
  e  kernels by HIP events, alternating rounds, median and spread: fp_jpeg_decode_window for the rectangles a Matterport batch stages, and
     fp_jpeg_decode of the same files as whole frames, each followed by the same windowed resizes (the whole-frame leg reads its
     rectangles out of the decoded frames)
Prints one JSON line."""
import argparse
import gc
import json
import os
import random
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

B, H, W = 12, 192, 640
ADE_SIZES = [(256, 341), (512, 683), (683, 512), (1536, 2048), (375, 500), (768, 1024)]
GROUND = {"ADE20K": 976, "cityscapes": 7}


def picture(h, w, seed):
    """a picture-like frame: smooth shading, flat shapes, mild sensor noise"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    img = np.stack([90 + 100 * yy / h + 20 * np.sin(xx / 37), 110 + 60 * yy / h + 25 * np.cos(xx / 21), 160 - 70 * yy / h + 15 * np.sin((xx + yy) / 15)], -1)
    for _ in range(12):
        cy, cx, r = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(20, 200)
        inside = (yy - cy) ** 2 + ((xx - cx) / 2) ** 2 < r * r
        img[inside] = img[inside] * 0.4 + rng.uniform(0, 255, 3).astype(np.float32) * 0.6
    return np.clip(img + rng.normal(0, 2.5, img.shape).astype(np.float32), 0, 255).astype(np.uint8)


def label_ids(h, w, seed, ground):
    rng = np.random.default_rng(seed)
    blocks = rng.integers(0, 3, ((h + 31) // 32, (w + 31) // 32))     # 32 x 32 patches: unlabelled, ground, something else
    ids = np.where(blocks == 0, 0, np.where(blocks == 1, ground, ground + 1))
    return np.kron(ids, np.ones((32, 32), np.int64))[:h, :w]


def write_tree(root, files, repeat):
    """the three datasets under `root` with splits/<dataset>/{train,val}.txt (every file listed `repeat` times) and paths.yaml"""
    from PIL import Image
    ade, city, mp = (os.path.join(root, d) for d in ("ade", "city", "mp"))
    lines = {"ADE20K": [], "cityscapes": [], "matterport": []}
    for i in range(files):
        h, w = ADE_SIZES[i % len(ADE_SIZES)]
        os.makedirs(os.path.join(ade, "images"), exist_ok=True)
        Image.fromarray(picture(h, w, i)).save(os.path.join(ade, "images", "f%d.jpg" % i), quality=(90, 75, 95)[i % 3], subsampling=(2, 2, 0)[i % 3])
        ids = label_ids(h, w, i, GROUND["ADE20K"])
        Image.fromarray(np.stack([ids // 256 * 10, ids % 256, ids % 7], -1).astype(np.uint8)).save(os.path.join(ade, "images", "f%d_seg.png" % i))
        lines["ADE20K"].append("images/f%d.jpg" % i)
        for sub in ("leftImg8bit", "gtFine"):
            os.makedirs(os.path.join(city, sub, "train", "aachen"), exist_ok=True)
        Image.fromarray(picture(1024, 2048, 100 + i)).save(os.path.join(city, "leftImg8bit", "train", "aachen", "f%d_leftImg8bit.png" % i), compress_level=3)
        ids = label_ids(1024, 2048, 100 + i, GROUND["cityscapes"]).astype(np.uint8)
        Image.fromarray(ids).save(os.path.join(city, "gtFine", "train", "aachen", "f%d_gtFine_labelIds.png" % i))
        lines["cityscapes"].append("train aachen f%d" % i)
        scans = os.path.join(mp, "sample_dataset/v1/scans", "scanA")
        os.makedirs(os.path.join(scans, "scanA", "matterport_color_images"), exist_ok=True)
        os.makedirs(os.path.join(scans, "nia_ground_masks"), exist_ok=True)
        Image.fromarray(picture(1024, 1280, 200 + i)).save(os.path.join(scans, "scanA", "matterport_color_images", "p%d_i1_2.jpg" % i), quality=90)
        np.save(os.path.join(scans, "nia_ground_masks", "out_p%d_1_2_visibleground.npy" % i), (label_ids(1024, 1280, 200 + i, 1) == 1).astype(np.float32))
        lines["matterport"].append("scanA p%d 1 2" % i)
    for dataset, ls in lines.items():
        os.makedirs(os.path.join(root, "splits", dataset), exist_ok=True)
        for split in ("train", "val"):
            with open(os.path.join(root, "splits", dataset, split + ".txt"), "w") as fh:
                fh.write("\n".join(ls * repeat) + "\n")
    with open(os.path.join(root, "paths.yaml"), "w") as fh:
        fh.write("ADE20K:\n  dataset: %s\ncityscapes:\n  dataset: %s\nmatterport:\n  dataset: %s\n" % (ade, city, mp))
    return lines


def train_loader(root, dataset, num_workers, device_decode):
    """the trainer's own train loader for one dataset (the validation loader it also builds is dropped)"""
    from footprints_amd.preprocessing.segmentation.train import Trainer
    trainer = Trainer.__new__(Trainer)
    trainer.opt = argparse.Namespace(config_path=os.path.join(root, "paths.yaml"), training_datasets=[dataset], batch_size=B, height=H, width=W,
                                     num_workers=num_workers, device_decode=device_decode)
    cwd = os.getcwd()
    os.chdir(root)
    try:
        return trainer.create_dataloaders()[0]
    finally:
        os.chdir(cwd)


def loop_ms(loader, step, skip=2):
    random.seed(13)
    n, t0 = 0, None
    for batch in loader:
        if n == skip:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        step(batch)
        n += 1
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / (n - skip), n - skip


def timed(fn, iters, stream):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    for _ in range(iters):
        fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b) / iters


def kernel_legs(root, lines, rounds, seconds):
    """leg e: one Matterport batch; everything uploaded beforehand, the two legs are device work alone"""
    from footprints_amd import _lib, ops
    from footprints_amd.preprocessing.segmentation.datasets import READERS, plan as P
    reader = READERS["matterport"](os.path.join(root, "mp"), lines["matterport"][:B], device_decode=True)
    samples = [reader[i] for i in range(B)]
    files, infos = [s[1]["bytes"] for s in samples], [s[1]["info"] for s in samples]
    rng = random.Random(7)
    plans = [P.draw_seg_plan("matterport", (i["h"], i["w"]), (H, W), True, rng) for i in infos]
    geo = [P.image_stages(p, ops.resize_window_axis) for p in plans]
    rects = [tuple(int(v) for v in g[1]) for g in geo]
    lib, dev = _lib.load(), torch.device("cuda", torch.cuda.current_device())
    stream = torch.cuda.current_stream()

    def chain(offsets, staged):
        """the assembler's one or two resize calls reading sample b's `staged[b]` rectangle at offsets[b] -> a function that queues them"""
        calls, mid_off, out_bytes = [ops.WindowBatch(3), ops.WindowBatch(3)], B * H * W * 3, B * H * W * 3
        for b, (stages, _) in enumerate(geo):
            offset, rect = offsets[b], staged[b]
            for k, st in enumerate(stages):
                last = k == len(stages) - 1
                calls[k].add(offset, rect, calls[k].table(st["in_hw"][1], st["out_hw"][1], st["table_h"]),
                             calls[k].table(st["in_hw"][0], st["out_hw"][0], st["table_v"]), st["window"], b * H * W * 3 if last else mid_off)
                if not last:
                    offset, rect = mid_off, st["window"]
                    mid_off += st["window"][2] * st["window"][3] * 3
        buf = torch.empty(mid_off, dtype=torch.uint8, device=dev)
        args = []
        for k, call in enumerate(calls):
            if call.samples:
                rec, tab, coef = call.arrays()
                args.append((k, torch.from_numpy(rec.copy()).to(dev), len(call.samples), torch.from_numpy(tab.copy()).to(dev), len(call.tables),
                             torch.from_numpy(coef).to(dev), coef.size, call.max_src_h, call.max_src_w, call.max_win_h, call.max_win_w))

        def run(src, src_bytes):
            for k, rec, n, tab, n_tab, coef, n_coef, msh, msw, mwh, mww in args:
                s, sb = (src, src_bytes) if k == 0 else (buf, buf.numel())
                ops.resize_window_u8(s, sb, rec, n, tab, n_tab, coef, n_coef, buf, 3, msh, msw, mwh, mww)
        return run, buf

    legs, keep = {}, []
    for name, with_rects in (("window", True), ("whole_frames", False)):
        pack = ops.jpeg_decode_pack(files, infos, rects=rects if with_rects else None)
        offsets, at = [], 0
        for (h, w), (_, _, rh, rw) in zip(pack["shapes"], rects):
            offsets.append(at)
            at += (rh * rw if with_rects else h * w) * 3
        out = torch.empty(pack["out_bytes"], dtype=torch.uint8, device=dev)
        d_scans, d_rec = torch.from_numpy(pack["scans"]).to(dev), torch.from_numpy(pack["records"]).to(dev)
        d_tab = torch.from_numpy(pack["tables"].view("int32")).to(dev)
        status = torch.empty(B + 1, dtype=torch.int32, device=dev)
        need = lib.fp_jpeg_decode_workspace_bytes(B, pack["max_h"], pack["max_w"], pack["max_scan"], ops.JPEG_DECODE_SUBSEQ_BITS)
        ws = ops.workspace(need, dev, "jpeg_decode")
        # the whole-frame leg's resizes read each sample's rectangle out of its decoded frame: the frame is what is staged
        resize, buf = chain(offsets, rects if with_rects else [(0, 0, h, w) for h, w in pack["shapes"]])
        head = (d_scans.data_ptr(), int(pack["scan_bytes"]), d_rec.data_ptr(), d_tab.data_ptr(), pack["n_sets"], out.data_ptr(), out.numel(),
                status.data_ptr(), B, pack["max_h"], pack["max_w"])
        tail = (pack["max_scan"], ops.JPEG_DECODE_SUBSEQ_BITS, ops.JPEG_DECODE_MAX_ROUNDS, ws.data_ptr(), ws.numel())

        def decode(with_rects=with_rects, head=head, tail=tail, pack=pack):
            if with_rects:
                _lib.check(lib.fp_jpeg_decode_window(*head, pack["max_win_h"], pack["max_win_w"], *tail, ops.stream()), "fp_jpeg_decode_window")
            else:
                _lib.check(lib.fp_jpeg_decode(*head, *tail, ops.stream()), "fp_jpeg_decode")

        def both(decode=decode, resize=resize, out=out):
            decode()
            resize(out, out.numel())
        legs[name + "_decode"], legs[name + "_decode_and_resize"] = decode, both
        keep.append((d_scans, d_rec, d_tab, status, ws, out, buf))
        both()
        torch.cuda.synchronize()
        assert status.cpu().tolist() == [0] * (B + 1), (name, status.cpu().tolist())
        legs[name + "_bytes"] = int(out.numel())
    outs = [k[6][:B * H * W * 3].clone() for k in keep]
    assert torch.equal(outs[0], outs[1]), "the two legs resized different pixels"
    fns = {k: v for k, v in legs.items() if callable(v)}
    iters, ms = {}, {k: [] for k in fns}
    for k, fn in fns.items():
        iters[k] = max(3, int(seconds * 1e3 / rounds / max(timed(fn, 3, stream), 1e-3)))
    for _ in range(rounds):
        for k, fn in fns.items():
            ms[k].append(timed(fn, iters[k], stream))
    return {"ms": {k: float(np.median(v)) for k, v in ms.items()}, "spread": {k: float((max(v) - min(v)) / np.median(v)) for k, v in ms.items()},
            "decoded_bytes": {"window": legs["window_bytes"], "whole_frames": legs["whole_frames_bytes"]},
            "two_stage_samples": sum(len(g[0]) == 2 for g in geo)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=None, help="where the tree is written (default: a temporary directory)")
    ap.add_argument("--legs", default="a,b,c,d,e")
    ap.add_argument("--files", type=int, default=24, help="distinct files per dataset")
    ap.add_argument("--repeat", type=int, default=15, help="how often the split files list each of them")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=2.0, help="total time of every timed kernel loop, over all rounds")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("seg_train_reader_bench.py needs a GPU: a time measured anywhere else says nothing about it")
    legs = set(a.legs.split(","))
    from footprints_amd.optim import FusedAdam
    from footprints_amd.preprocessing.segmentation.evaluation import Evaluator
    from footprints_amd.preprocessing.segmentation.network import Segmentor
    import PIL
    with tempfile.TemporaryDirectory() as tmp:
        root = a.root or tmp
        t0 = time.perf_counter()
        lines = write_tree(root, a.files, a.repeat)
        out = {"device": torch.cuda.get_device_name(0), "batch": B, "height": H, "width": W, "files": a.files, "repeat": a.repeat,
               "pillow": PIL.__version__, "cpus": len(os.sched_getaffinity(0)), "tree_seconds": time.perf_counter() - t0, "ms_per_step": {}}
        model = Segmentor(pretrained=False, use_PSP=True).cuda()
        model.train()
        optimiser, evaluator = FusedAdam(model, lr=1e-4), Evaluator()

        def step(batch):
            loss = evaluator.compute_losses(model(batch["image"]), batch["ground_mask"], batch["labelled_pix"])
            model.zero_grad()
            loss.backward()
            optimiser.step()

        configs = [("b_workers0", "b", 0, False), ("c_workers4", "c", 4, False), ("c_workers16", "c", 16, False),
                   ("d_workers4_device", "d", 4, True), ("d_workers16_device", "d", 16, True)]
        for dataset in ("matterport", "ADE20K", "cityscapes"):
            res = out["ms_per_step"][dataset] = {}
            for name, leg, workers, device_decode in configs:
                if leg not in legs:
                    continue
                loader = train_loader(root, dataset, workers, device_decode)
                if leg == "b" and "a" in legs:              # leg a on this dataset's first batch
                    batch = {k: v.clone() for k, v in next(iter(loader)).items()}
                    for _ in range(5):
                        step(batch)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(30):
                        step(batch)
                    torch.cuda.synchronize()
                    res["a_step_alone"] = (time.perf_counter() - t0) * 1e3 / 30
                res[name], res[name + "_steps"] = loop_ms(loader, step)
                if leg != "b":                              # the same loader with nobody training: where a gap to leg a comes from
                    res[name + "_loader_alone"] = loop_ms(loader, lambda batch: None)[0]
                print("%s %s: %.2f ms per step" % (dataset, name, res[name]), file=sys.stderr, flush=True)
                if device_decode:
                    res[name + "_counters"] = loader.counters
                del loader
                gc.collect()
        if "e" in legs:
            out["kernels"] = kernel_legs(root, lines, a.rounds, a.seconds)
        print(json.dumps(out))


if __name__ == "__main__":
    main()
