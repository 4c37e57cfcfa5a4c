"""GPU box: what the label maps of a KITTI training batch cost on the device path (csrc/label_resize.hip, DeviceBatchAssembler(raw_maps=True))
next to the host chain it replaces, and what the file loader costs the training step: batches of 12 at 192 x 640, 5 maps per sample from
375 x 1242.

    python scripts/train_reader_bench.py [--seconds 2.0] [--rounds 5] [--steps 40] [--frames 48] [--workers 8] [--map_dtype float32]
                                         [--loader_stream own|dwg0]
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/train_reader_bench.py --only_resize      # the kernel's own time, in a run of its own

Legs: the fp_label_resize CALL alone on an uploaded batch (HIP events around a loop of calls: the status word's 4-byte memset, the launch
and the gaps between launches are in it -- an upper bound of the kernel's own time, not a kernel trace); the same with the H2D copies of
the packed maps and records; the host pack
(one thread, into pinned memory); the numpy restatement of cv2.resize on one core (tests/label_resize_restatement.py -- a STAND-IN for cv2,
which is not installed: the same arithmetic, vectorised by numpy instead of OpenCV's loops); per-stage host times of the file path (JPEG
decode, np.load, fill) on one thread; the training step alone on a resident batch; the loader alone; and the training step with the file
loader in the loop, on a synthetic on-disk tree this script writes (random frames and maps: JPEG entropy and .npy sizes are not KITTI's).
The last two legs run a second time with --device_decode (the readers hand over file bytes, the assembler decodes them on the device),
alternating with the Pillow legs inside each round, with the reader's, fill's and the decode stage's host times per batch and the
decode counters next to them.  Prints one JSON line."""
import argparse
import json
import os
import random
import shutil
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from footprints_amd import ops
from footprints_amd.datasets.device_path import MAP_KEYS, MAP_METHODS

B, H, W = 12, 192, 640
NATIVE = [(375, 1242), (370, 1226), (374, 1238), (376, 1241)]          # KITTI's raw frame sizes
FOLDERS = {"visible_ground": "ground_seg", "ground_depth": "hidden_depths", "depth_mask": "depth_masks", "disparity": "stereo_matching_disps",
           "moving_objects": "moving_objects"}
DTYPES = {"visible_ground": np.float32, "ground_depth": np.float32, "depth_mask": np.uint8, "disparity": np.float32, "moving_objects": np.uint8}


def timed(fn, iters, stream):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    for _ in range(iters):
        fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b) / iters


def host_ms(fn, seconds):
    fn()
    n, t0 = 0, time.perf_counter()
    while n < 3 or time.perf_counter() - t0 < seconds:
        fn()
        n += 1
    return (time.perf_counter() - t0) * 1e3 / n


def make_maps(rng, h, w, dtypes):
    m = {"visible_ground": rng.random((h, w)), "ground_depth": rng.random((h, w)) * 30 * (rng.random((h, w)) < 0.5),
         "depth_mask": rng.random((h, w)) < 0.02, "disparity": rng.random((h, w)) * 60, "moving_objects": rng.random((h, w)) < 0.05}
    return {k: v.astype(dtypes[k]) for k, v in m.items()}


def write_tree(root, frames, dtypes, seed=1):
    """a KITTI-shaped tree of random frames and maps -> split lines"""
    from PIL import Image
    rng = np.random.default_rng(seed)
    lines = []
    for j in range(frames):
        seq, name = "2011_09_26/2011_09_26_drive_%04d_sync" % (j % 3), str(j).zfill(10)
        h, w = NATIVE[j % len(NATIVE)]
        os.makedirs(os.path.join(root, "raw", seq, "image_02", "data"), exist_ok=True)
        # smooth content + noise: a random-noise JPEG would decode far slower than a photograph
        base = np.kron(rng.integers(0, 256, ((h + 15) // 16, (w + 15) // 16, 3)), np.ones((16, 16, 1)))[:h, :w]
        img = np.clip(base + rng.normal(0, 6, (h, w, 3)), 0, 255).astype(np.uint8)
        Image.fromarray(img).save(os.path.join(root, "raw", seq, "image_02", "data", name + ".jpg"), quality=92)
        for key, arr in make_maps(rng, h, w, dtypes).items():
            sub = os.path.join(root, "training_data", FOLDERS[key], seq, "image_02")
            sub = sub if key == "disparity" else os.path.join(sub, "data")
            os.makedirs(sub, exist_ok=True)
            np.save(os.path.join(sub, name + ".npy"), arr)
        lines.append("%s %d l" % (seq, j))
    os.makedirs(os.path.join(root, "splits", "kitti"), exist_ok=True)
    for split in ("train", "val"):
        with open(os.path.join(root, "splits", "kitti", split + ".txt"), "w") as fh:
            fh.write("\n".join(lines) + "\n")
    with open(os.path.join(root, "paths.yaml"), "w") as fh:
        fh.write("kitti:\n  dataset: %s\n  training_data: %s\n" % (os.path.join(root, "raw"), os.path.join(root, "training_data")))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=2.0, help="total time of every timed loop, over all rounds")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=40, help="train steps per timed loop")
    ap.add_argument("--frames", type=int, default=48, help="frames of the on-disk tree (cycled)")
    ap.add_argument("--workers", type=int, default=8, help="--num_workers of the file loader")
    ap.add_argument("--map_dtype", default="float32", choices=["float16", "float32", "float64"], help="stored dtype of the real-valued maps")
    ap.add_argument("--only_resize", action="store_true", help="the label-resize legs alone (for a kernel-trace run)")
    ap.add_argument("--loader_stream", default="own", choices=["own", "dwg0"],
                    help="the loaders' copy / assembly stream: one of their own (what main.py gives them) or the engine's decoder "
                         "weight-gradient stream (what bench.py gives its assembler)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("train_reader_bench.py needs a GPU: a time measured anywhere else says nothing about it")
    from tests import label_resize_restatement as LR
    dtypes = {k: (np.dtype(a.map_dtype).type if v == np.float32 else v) for k, v in DTYPES.items()}
    out = {"device": torch.cuda.get_device_name(0), "batch": B, "height": H, "width": W, "rounds": a.rounds, "map_dtype": a.map_dtype}
    rng = np.random.default_rng(2)
    keys = MAP_KEYS["kitti"]
    samples = [make_maps(rng, 375, 1242, dtypes) for _ in range(B)]
    maps = [s[k] for k in keys for s in samples]
    methods = [MAP_METHODS[k] for k in keys for _ in samples]
    flips = [b % 2 == 1 for _ in keys for b in range(B)]
    mults = [W / 1242 if k == "disparity" else 1.0 for k in keys for _ in samples]
    tables = ops.label_table_set("cuda")
    n = len(maps)
    cap = sum((m.nbytes + 7) // 8 * 8 for m in maps)
    h_src = torch.empty(cap, dtype=torch.uint8).pin_memory()
    h_rec = torch.empty(n * ops._lib.load().fp_label_sample_bytes(), dtype=torch.uint8).pin_memory()
    pack = lambda: ops.label_resize_pack(maps, H, W, methods, flips, mults, tables=tables, packed=h_src.numpy(), records=h_rec.numpy())
    total = pack()[2]
    d_src, d_rec = torch.empty_like(h_src, device="cuda"), torch.empty_like(h_rec, device="cuda")
    d_out = torch.empty((n, H, W), dtype=torch.float64, device="cuda")
    stream = torch.cuda.current_stream()

    def kernel():
        ops.label_resize_packed(d_src, total, d_rec, n, H, W, tables, out=d_out)

    def kernel_and_copies():
        d_src[:total].copy_(h_src[:total], non_blocking=True)
        d_rec.copy_(h_rec, non_blocking=True)
        kernel()
    kernel_and_copies()
    torch.cuda.synchronize()
    ref = LR.label_resize(maps[0], H, W, methods[0], flips[0], mults[0])
    assert np.array_equal(d_out[0].cpu().numpy(), ref[:, ::-1] if flips[0] else ref)          # what is timed computes what is tested
    legs = {"call": kernel, "call_and_copies": kernel_and_copies}
    iters, ms = {}, {leg: [] for leg in legs}
    for leg, fn in legs.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        iters[leg] = max(3, int(a.seconds * 1e3 / a.rounds / max(timed(fn, 3, stream), 1e-3)))
    for _ in range(a.rounds):                                           # the legs alternate inside every round
        for leg, fn in legs.items():
            ms[leg].append(timed(fn, iters[leg], stream))
    torch.cuda.synchronize()
    res = {"label_maps": n, "packed_bytes": int(total), "out_bytes": int(d_out.numel() * 8)}
    res["ms"] = {leg: float(np.median(v)) for leg, v in ms.items()}
    res["spread"] = {leg: float((max(v) - min(v)) / np.median(v)) for leg, v in ms.items()}
    res["call_gb_per_s_read_plus_written"] = (total + d_out.numel() * 8) / res["ms"]["call"] / 1e6
    res["ms"]["host_pack_one_thread"] = host_ms(pack, a.seconds / 2)
    torch.set_num_threads(1)
    res["ms"]["host_numpy_restatement_one_core"] = host_ms(
        lambda: [LR.label_resize(m, H, W, me, f, mu) for m, me, f, mu in zip(maps, methods, flips, mults)], a.seconds)
    out["label_resize"] = res
    if a.only_resize:
        print(json.dumps(out))
        return

    # ---- the file loader in the training loop ----
    from footprints_amd.datasets.training import KITTIReader, create_dataloaders, load_npy
    from footprints_amd.model_manager import ModelManager
    from footprints_amd.options import Options
    from footprints_amd.preprocessing.segmentation.datasets.base import pil_loader
    from footprints_amd.training.train import TrainStep
    root = tempfile.mkdtemp(prefix="train_reader_bench_")
    cwd = os.getcwd()
    try:
        lines = write_tree(root, a.frames, dtypes)
        os.chdir(root)
        opt = Options().parse(["--mode", "train", "--config_path", os.path.join(root, "paths.yaml"), "--num_workers", str(a.workers)])
        reader = KITTIReader(os.path.join(root, "raw"), os.path.join(root, "training_data"), lines, H, W)
        p = reader.paths(0)
        files = {"jpeg_decode_per_frame": lambda: pil_loader(p["image"]),
                 "np_load_5_maps_per_frame": lambda: [load_npy(p[k]) for k in keys]}
        stage = {k: host_ms(fn, a.seconds / 4) for k, fn in files.items()}
        mm = ModelManager(use_cuda=True)
        ts = TrainStep(mm.model, mm.optimiser)
        loader_stream = ts.eng.dwg[0] if a.loader_stream == "dwg0" else None
        train, _ = create_dataloaders(opt, stream=loader_stream)
        train_dd, _ = create_dataloaders(opt, stream=loader_stream, device_decode=True)
        for ld in (train, train_dd):
            ld.source.index = (ld.source.index * -(-(a.steps + 5) * B // a.frames))[:(a.steps + 5) * B]        # cycle the tree: steps + 5 batches per pass
        batch_samples = [reader[i] for i in range(B)]
        from footprints_amd.datasets import draw_augmentation
        prm = [draw_augmentation(True, random.Random(3)) for _ in range(B)]
        stage["fill_per_batch_one_thread"] = host_ms(lambda: train.asm.fill(batch_samples, prm), a.seconds / 4)
        # the same three under --device_decode: a reader thread's work per frame (file bytes + header), fill, and inside fill the decode
        # stage's host half (layout, records, scans and table blocks into the slot's pinned buffers)
        reader_dd = KITTIReader(os.path.join(root, "raw"), os.path.join(root, "training_data"), lines, H, W, device_decode=True)
        samples_dd = [reader_dd[i] for i in range(B)]
        stage["device_decode_read_and_parse_per_frame"] = host_ms(lambda: reader_dd.image(p["image"]), a.seconds / 4)
        stage["device_decode_fill_per_batch_one_thread"] = host_ms(lambda: train_dd.asm.fill(samples_dd, prm), a.seconds / 4)
        frames_dd = [smp for smp, _ in samples_dd]
        stage["device_decode_host_half_per_batch"] = host_ms(lambda: train_dd.asm.stage.prepare(train_dd.asm.slots[0], frames_dd), a.seconds / 4)
        train_dd.asm.slots[0]["batch"] = None
        finish, waited = train_dd.asm.stage.finish, []

        def timed_finish(s):                                            # the launching thread's time inside the status check of a batch
            t0 = time.perf_counter()
            try:
                return finish(s)
            finally:
                waited.append((time.perf_counter() - t0) * 1e3)
        train_dd.asm.stage.finish = timed_finish
        resident = {k: v.clone() for k, v in train.asm.collect(train.asm.submit(batch_samples, prm)).items()}
        for _ in range(5):
            ts(resident)
        torch.cuda.synchronize()
        alone, looped, loader_only, looped_dd, loader_only_dd = [], [], [], [], []
        for _ in range(max(a.rounds // 2, 2)):                         # the five loops alternate
            t0 = time.perf_counter()
            for _ in range(a.steps):
                ts(resident)
            torch.cuda.synchronize()
            alone.append((time.perf_counter() - t0) * 1e3 / a.steps)
            for sink, use, loader in ((looped, ts, train), (looped_dd, ts, train_dd), (loader_only, lambda bt: None, train),
                                      (loader_only_dd, lambda bt: None, train_dd)):
                k, t0 = 0, None
                for bt in loader:
                    if k == 5:                                          # the loader's first batches fill the pipeline
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                    use(bt)
                    k += 1
                torch.cuda.synchronize()
                sink.append((time.perf_counter() - t0) * 1e3 / (k - 5))
        loops = dict(train_step_alone=alone, train_step_with_file_loader=looped, file_loader_alone=loader_only,
                     train_step_with_file_loader_device_decode=looped_dd, file_loader_alone_device_decode=loader_only_dd)
        stage.update({k: float(np.median(v)) for k, v in loops.items()})
        stage["device_decode_status_check_per_batch_mean"] = float(np.mean(waited))
        stage["device_decode_status_check_per_batch_max"] = float(np.max(waited))
        out["file_loader"] = {"frames_on_disk": a.frames, "loader_stream": a.loader_stream, "workers": train.source.num_workers, "ms": stage,
                              "img_per_s": {k: B / stage[k] * 1e3 for k in loops},
                              "spread": {k: float((max(v) - min(v)) / np.median(v)) for k, v in loops.items()},
                              "loader_cost_fraction": stage["train_step_with_file_loader"] / stage["train_step_alone"] - 1.0,
                              # the condition of profiles/jpeg_decode_notes.md: with the flag not slower than without it by more than the run's spread
                              "device_decode_over_pillow": stage["train_step_with_file_loader_device_decode"] / stage["train_step_with_file_loader"],
                              "device_decode_gap_to_step_alone": stage["train_step_with_file_loader_device_decode"] / stage["train_step_alone"] - 1.0,
                              "device_decode_counters": train_dd.counters}
    finally:
        os.chdir(cwd)
        shutil.rmtree(root, ignore_errors=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
