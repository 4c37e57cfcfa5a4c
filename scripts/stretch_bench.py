"""GPU box: what the stretched-map pictures cost (csrc/stretch_map.hip): the segmentation trainer's log event at 12 x 192 x 640 and one
label picture at 1 x 192 x 640.

    python scripts/stretch_bench.py [--reps 50] [--steps 300] [--targets 10] [--skip_training] [--skip_generator] [--out FILE]

Legs:
* the two launches of ops.seg_log_panels / ops.stretch_colour (HIP events around the call: launch gaps are in it -- an upper bound of the
  kernels' own time, not a kernel trace), and the launches with the copies an event needs (the pictures to pinned memory; for the label
  picture also the map's upload, which the generator does NOT do -- its result is on the device already);
* the host route on one core: the numpy / matplotlib restatements of tests/seg_log_restatement.py and tests/stretch_restatement.py,
  including the .cpu() copies the reference makes;
* the time the training thread spends inside `log()`, and the writer thread's encode + write time per event;
* the segmentation trainer's rate over `--steps` steps of synthetic device-assembled batches, validation on, log_freq 250, with summaries
  and without;
* the KITTI hidden-depth generator's time per target frame (load, process, save) on the synthetic tree of scripts/gt_loader_bench.py without
  pictures, with --save_visualisations, and with --device_jpeg as well.
Prints one JSON document; `--out FILE` also writes it."""
import argparse
import json
import os
import random
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

B, H, W = 12, 192, 640


def _event_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        t.append(a.elapsed_time(b))
    t.sort()
    return {"median_ms": round(t[len(t) // 2], 4), "min_ms": round(t[0], 4), "max_ms": round(t[-1], 4)}


def _host_ms(fn, reps):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    t.sort()
    return {"median_ms": round(t[len(t) // 2], 3), "min_ms": round(t[0], 3), "max_ms": round(t[-1], 3)}


def pieces(reps):
    from footprints_amd import ops
    from footprints_amd.preprocessing.segmentation.logger import SegPanelLogger
    from footprints_amd.training.summary import SummaryWriter
    from tests import seg_log_restatement as SR
    from tests import stretch_restatement as ST
    torch.set_num_threads(1)
    inputs, logits = SR.make_inputs(B, H, W, seed=1)
    dev_in = {k: torch.from_numpy(v).cuda() for k, v in inputs.items()}
    head = torch.zeros(B, 2, H, W, device="cuda")
    head[:, 0:1] = torch.from_numpy(logits).cuda()
    out, _ = ops.seg_log_panels(dev_in, head[:, 0:1])
    pinned = torch.empty(out.numel(), dtype=torch.uint8).pin_memory()
    res = {"log": {"picture_bytes": out.numel(), "launches": _event_ms(lambda: ops.seg_log_panels(dev_in, head[:, 0:1], out=out), reps)}}

    def log_with_copy():
        ops.seg_log_panels(dev_in, head[:, 0:1], out=out)
        pinned.copy_(out.view(-1), non_blocking=True)
    res["log"]["launches_with_copy"] = _event_ms(log_with_copy, reps)

    def log_host():
        host = {k: v.cpu().numpy() for k, v in dev_in.items()}
        SR.to_bytes(SR.float_parts(host, head[:, 0:1].cpu().numpy()))
    res["log"]["host_route_one_core"] = _host_ms(log_host, max(3, reps // 10))
    with tempfile.TemporaryDirectory() as tmp:
        writer, logger = SummaryWriter(tmp), SegPanelLogger()
        losses = {k: torch.tensor(0.5, device="cuda") for k in ("ground_loss_0", "ground_loss_1", "ground_loss_2", "ground_loss_3", "loss")}
        in_log = []
        for step in range(6):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            logger.log(writer, dev_in, head[:, 0:1], losses, 1e-4, step)
            in_log.append((time.perf_counter() - t0) * 1e3)
            logger.drain()
        logger.close()
        writer.close()
        res["log"]["file_bytes_per_event"] = os.path.getsize(writer.path) // 6
    res["log"]["log_call_ms"] = {"first": round(in_log[0], 3), "median_of_rest": round(sorted(in_log[1:])[len(in_log[1:]) // 2], 3)}
    ws = sorted(logger.writer_seconds)
    res["log"]["writer_thread_ms_per_event"] = {"median": round(ws[len(ws) // 2] * 1e3, 2), "max": round(ws[-1] * 1e3, 2)}

    rng = np.random.default_rng(2)
    x = ((rng.random((H, W)) * 40.0) * (rng.random((H, W)) < 0.6)).astype(np.float32)
    d_x = torch.from_numpy(x).cuda()
    pic = ops.stretch_colour(d_x)
    h_x, h_pic = torch.from_numpy(x).pin_memory(), torch.empty(pic.numel(), dtype=torch.uint8).pin_memory()
    res["label"] = {"picture_bytes": pic.numel(), "launches": _event_ms(lambda: ops.stretch_colour(d_x, out=pic), reps)}

    def label_with_copies():
        d_x.copy_(h_x, non_blocking=True)
        ops.stretch_colour(d_x, out=pic)
        h_pic.copy_(pic.view(-1), non_blocking=True)
    res["label"]["launches_with_copies"] = _event_ms(label_with_copies, reps)
    res["label"]["host_route_one_core"] = _host_ms(lambda: ST.rgb(d_x.cpu().numpy()), reps)
    res["label"]["pillow_encode_one_core"] = _host_ms(lambda: ST.pillow_file(pic.cpu().numpy()), reps)
    res["label"]["device_jpeg_files"] = _host_ms(lambda: ops.jpeg_encode(pic.unsqueeze(0), quality=75, dpi=(100, 100)), reps)
    return res


def training(steps, summaries):
    from footprints_amd.datasets.device_path import SegBatchAssembler, SyntheticSegSource
    from footprints_amd.preprocessing.segmentation.network import Segmentor
    from footprints_amd.preprocessing.segmentation.options import SegmentationOptions
    from footprints_amd.preprocessing.segmentation.train import Trainer
    frames = [("cityscapes", (1024, 2048)), ("ADE20K", (480, 640)), ("ADE20K", (375, 500))]
    with tempfile.TemporaryDirectory() as tmp:
        opts = SegmentationOptions().parse(["--log_freq", "250", "--epochs", "1", "--log_path", tmp, "--model_name", "bench"])
        torch.manual_seed(0)
        model = Segmentor(pretrained=False, use_PSP=True).cuda()

        def loader(n, seed, is_train):
            ld = SegBatchAssembler(B, H, W, max_src_hw=(1280, 2048)).loader(SyntheticSegSource(B, n, frames, seed=seed), is_train, random.Random(seed))
            ld.dataset = ld.source.dataset
            return ld
        trainer = Trainer(opts, model=model, train_loader=loader(steps, 1, True), val_loader=loader(10, 2, False), summaries=summaries)
        trainer.save_model = lambda: None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        trainer.train()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        files = sum(len(f) for _, _, f in os.walk(tmp))
    return {"steps": steps, "seconds": round(dt, 2), "steps_per_second": round(steps / dt, 3), "event_files": files,
            "log_events": len(trainer.history)}


def generator(targets):
    from gt_loader_bench import SEQ, write_tree
    from footprints_amd.preprocessing.ground_truth_generation import KITTIGroundTruthGenerator, get_options
    root = tempfile.mkdtemp(prefix="stretch_bench_")
    try:
        write_tree(root, 26 + 2 * targets + 44, np.random.default_rng(0))
        lines = ["%s %d l" % (SEQ, 26 + 2 * k) for k in range(targets + 1)]
        with open(os.path.join(root, "files.txt"), "w") as fh:
            fh.write("\n".join(lines) + "\n")
        res = {}
        for name, extra in (("no_pictures", []), ("pictures_pillow", ["--save_visualisations"]),
                            ("pictures_device_jpeg", ["--save_visualisations", "--device_jpeg"])):
            opts = get_options(["--config_path", os.path.join(root, "paths.yaml"), "--textfile", os.path.join(root, "files.txt"),
                                "--save_folder_name", "out_" + name] + extra)
            gen = KITTIGroundTruthGenerator.from_options(opts)
            per = []
            for i, line in enumerate(gen.filenames):
                t0 = time.perf_counter()
                data = gen.load_data(i, line)
                result = gen.process_data(data, robust_aggregation=gen.robust_aggregation)
                gen.save_result(result, line, save_viz=opts.save_visualisations)
                torch.cuda.synchronize()
                per.append((time.perf_counter() - t0) * 1e3)
            warm = sorted(per[1:])                         # the first target reads the whole window
            res[name] = {"first_ms": round(per[0], 2), "warm_median_ms": round(warm[len(warm) // 2], 2), "warm_mean_ms": round(float(np.mean(warm)), 2)}
        return res
    finally:
        shutil.rmtree(root, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--targets", type=int, default=10)
    ap.add_argument("--skip_training", action="store_true")
    ap.add_argument("--skip_generator", action="store_true")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "stretch_bench needs a GPU"
    res = {"shape": {"log": (B, H, W), "label": (1, H, W)}, "pieces": pieces(args.reps)}
    if not args.skip_generator:
        res["generator_per_frame"] = generator(args.targets)
    if not args.skip_training:
        # the run without summaries first and last: the first run of a process also pays for code objects and the allocator
        res["training"] = {"warm_up_no_summaries": training(args.steps, False), "summaries": training(args.steps, True),
                           "no_summaries": training(args.steps, False)}
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
