"""GPU box: what the label generators' loader costs per KITTI target frame with the device-resident frame cache (data_loader.py,
csrc/gt_frames.hip) next to the host route it replaces, on a synthetic on-disk tree this script writes (random maps at 375 x 1242: the
.npy sizes are KITTI's, the values are not).

    python scripts/gt_loader_bench.py [--frames 90] [--targets 12] [--host_targets 1] [--iters 20]

Legs, all for hidden depths at 192 x 640 with the reference's window (up to 76 source frames):
* device: `KITTIGroundTruthGenerator.from_options` over the tree -- the first target frame (cold: every frame of the window is read, uploaded
  and resized) and the following target frames of the same parity (warm: two new frames each), `load_data` alone and with `process_data`;
  host clock around work that ends in a device synchronise;
* host: the same generator over the restated reference loader (tests/gt_frames_restatement.py: the numpy restatement of cv2.resize on one
  core -- a STAND-IN for cv2, which is not installed --, np.stack on the host, the generator's uploads), same targets;
* the fp_gt_frame_resize CALL alone on uploaded maps (HIP events around a loop of calls: launch gaps are in it -- an upper bound of the
  kernel's own time, not a kernel trace) and with the H2D copy of the packed maps, for a cold window (76 frames = 152 maps) and warm ones
  (2 and 4 frames), and fp_gt_gather_frames for 76 frames.
Prints one JSON line."""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from footprints_amd import ops
from footprints_amd.preprocessing.ground_truth_generation import KITTIGroundTruthGenerator, get_options

H, W = 192, 640
NATIVE = (375, 1242)
SEQ = "2011_09_26/2011_09_26_drive_0001_sync"


def write_tree(root, frames, rng):
    t = os.path.join(root, "training")
    pool = [((rng.random(NATIVE) * 80 + 1).astype(np.float32), rng.random((1,) + NATIVE).astype(np.float16)) for _ in range(4)]
    for f in range(frames):
        name = "{}.npy".format(str(f).zfill(10))
        pose = np.eye(4)[:3].copy()
        pose[2, 3] = 0.8 * f
        os.makedirs(os.path.join(t, "poses", SEQ, "orbslam_poses"), exist_ok=True)
        np.save(os.path.join(t, "poses", SEQ, "orbslam_poses", name), pose.reshape(-1))
        for j, side in enumerate(("image_02", "image_03")):
            disp, seg = pool[(2 * f + j) % 4]
            for folder, arr in ((os.path.join("stereo_matching_disps", SEQ, side), disp), (os.path.join("ground_seg", SEQ, side, "data"), seg)):
                os.makedirs(os.path.join(t, folder), exist_ok=True)
                np.save(os.path.join(t, folder, name), arr)
    with open(os.path.join(root, "paths.yaml"), "w") as fh:
        fh.write("kitti:\n  dataset: %s\n  training_data: %s\n" % (os.path.join(root, "raw"), t))
    return t


def per_target(gen, lines):
    """(load_data ms, load_data + process_data ms) per line, each ending in a device synchronise"""
    out = []
    for i, line in enumerate(lines):
        t0 = time.perf_counter()
        data = gen.load_data(i, line)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        gen.process_data(data, robust_aggregation=gen.robust_aggregation)
        torch.cuda.synchronize()
        out.append(((t1 - t0) * 1e3, (time.perf_counter() - t0) * 1e3))
    return out


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def resize_legs(n_frames, iters, rng):
    """ms of the resize call alone and with its H2D copy for n_frames frames (disparity float32 + segmentation float16 each)"""
    tables = ops.linear_table_set("cuda")
    maps, pre, thr = [], [], []
    for _ in range(n_frames):
        maps += [(rng.random(NATIVE) * 80 + 1).astype(np.float32), rng.random(NATIVE).astype(np.float16)]
        pre += [W / NATIVE[1], 1.0]
        thr += [None, 0.75]
    cache = torch.empty((2 * n_frames, H, W), dtype=torch.float32, device="cuda")
    pinned = torch.empty(ops.gt_frame_pack_bytes(maps), dtype=torch.uint8).pin_memory()
    t0 = time.perf_counter()
    pack = ops.gt_frame_pack(maps, H, W, [j * H * W for j in range(len(maps))], cache.numel(), "linear", pre, 1.0, thr, tables, packed=pinned.numpy())
    pack_ms = (time.perf_counter() - t0) * 1e3
    d_packed = torch.empty(pack.total, dtype=torch.uint8, device="cuda")
    d_packed.copy_(pinned[:pack.total])                                  # the call-alone leg reads the uploaded maps AND records

    def with_copy():
        d_packed.copy_(pinned[:pack.total], non_blocking=True)
        ops.gt_frame_resize(pack, d_packed, cache)
    return {"frames": n_frames, "packed_mb": round(pack.total / 1e6, 2), "host_pack_ms": round(pack_ms, 3),
            "resize_call_ms": round(timed(lambda: ops.gt_frame_resize(pack, d_packed, cache), iters), 4),
            "resize_with_copy_ms": round(timed(with_copy, iters), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=90)
    ap.add_argument("--targets", type=int, default=12)
    ap.add_argument("--host_targets", type=int, default=1)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "gt_loader_bench needs a GPU"
    rng = np.random.default_rng(0)
    root = tempfile.mkdtemp(prefix="gt_loader_bench_")
    try:
        t = write_tree(root, args.frames, rng)
        lines = ["%s %d l" % (SEQ, 26 + 2 * k) for k in range(args.targets)]
        with open(os.path.join(root, "files.txt"), "w") as fh:
            fh.write("\n".join(lines) + "\n")
        opts = get_options(["--config_path", os.path.join(root, "paths.yaml"), "--textfile", os.path.join(root, "files.txt")])
        gen = KITTIGroundTruthGenerator.from_options(opts)
        gen.load_data(0, lines[0])                                       # code objects, allocator, page cache of the files
        torch.cuda.synchronize()
        gen.loader.purge_buffer()
        gen.loader.frame_cache.uploads.clear()
        dev = per_target(gen, gen.filenames)
        uploads = list(gen.loader.frame_cache.uploads)
        res = {"tree": {"frames": args.frames, "native": NATIVE, "target": (H, W)}, "window_frames": int(gen.load_data(0, gen.filenames[0])["depths"].shape[0]),
               "device": {"cold_load_ms": round(dev[0][0], 2), "cold_total_ms": round(dev[0][1], 2),
                          "warm_load_ms": round(float(np.mean([d[0] for d in dev[1:]])), 2),
                          "warm_total_ms": round(float(np.mean([d[1] for d in dev[1:]])), 2),
                          "uploads_maps_bytes": uploads[:3] + uploads[-1:]}}
        if args.host_targets:
            from tests.gt_frames_restatement import HostKITTILoader
            host = KITTIGroundTruthGenerator(opts, HostKITTILoader(os.path.join(root, "raw"), t, H, W), training_datapath=t)
            hst = per_target(host, host.filenames[:1 + args.host_targets])
            res["host"] = {"cold_load_ms": round(hst[0][0], 1), "cold_total_ms": round(hst[0][1], 1),
                           "warm_load_ms": round(float(np.mean([d[0] for d in hst[1:]])), 1),
                           "warm_total_ms": round(float(np.mean([d[1] for d in hst[1:]])), 1)}
        res["resize"] = [resize_legs(n, args.iters, rng) for n in (76, 4, 2)]
        cache = torch.rand((152, H, W), device="cuda") + 0.5
        idx = list(range(0, 152, 2)), list(range(1, 152, 2))
        res["gather_76_frames_ms"] = round(timed(lambda: ops.gt_gather_frames(cache, idx[0], idx[1], 200.0), args.iters), 4)
    finally:
        shutil.rmtree(root, ignore_errors=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
