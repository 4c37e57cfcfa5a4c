"""What the trainer's TensorBoard logging costs (training/logger.py, csrc/log_panels.hip), for KITTI 12 x 192 x 640 and Matterport
4 x 512 x 640: the two launches of ops.log_panels, the copy of the panels into pinned memory, the writer thread's encode + write time per
event, the time the training thread spends inside `log()`, and the training rate of TrainManager's loop (synthetic loader, validation
on, log_freq 250) with and without summaries.  Prints one JSON document; `--out FILE` also writes it.

    python scripts/log_bench.py [--workload kitti|matterport|both] [--steps 600] [--reps 50] [--out FILE]

The reference's loop logs where `step % 100 == 0 and step % log_freq == 0`: with log_freq 250 that is steps 0, 500, 1000, ..."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

WORKLOADS = {"kitti": (12, 192, 640), "matterport": (4, 512, 640)}
DEPTH_RANGE = (0.1, 100.0)


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
    return {"median_ms": t[len(t) // 2], "min_ms": t[0], "max_ms": t[-1]}


def pieces(B, H, W, reps):
    from footprints_amd import ops
    from footprints_amd.training.logger import PanelLogger
    from footprints_amd.training.summary import SummaryWriter
    from footprints_amd.training.train import synthetic_batch
    batch = synthetic_batch(B, H, W, "cuda")
    pred = torch.rand(B, 4, H, W, device="cuda") * 6 - 3
    pred[:, 2:] = torch.sigmoid(pred[:, 2:])
    out, tags = ops.log_panels(batch, pred, DEPTH_RANGE)
    res = {"panels_bytes": out.numel(), "launches": _event_ms(lambda: ops.log_panels(batch, pred, DEPTH_RANGE, out=out), reps)}
    host = torch.empty(out.numel(), dtype=torch.uint8).pin_memory()
    res["copy"] = _event_ms(lambda: host.copy_(out.view(-1), non_blocking=True), reps)
    with tempfile.TemporaryDirectory() as tmp:
        writer, logger = SummaryWriter(tmp), PanelLogger(DEPTH_RANGE)
        in_log = []
        for step in range(6):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            logger.log(writer, batch, pred, {"loss": 1.0}, 1e-4, step)
            in_log.append((time.perf_counter() - t0) * 1e3)
            logger.drain()                                   # one event at a time: the time in log() without waiting for a slot
        logger.close()
        writer.close()
        res["file_bytes_per_event"] = os.path.getsize(writer.path) // 6
    res["log_call_ms"] = {"first": in_log[0], "median_of_rest": sorted(in_log[1:])[len(in_log[1:]) // 2]}
    ws = sorted(logger.writer_seconds)
    res["writer_thread_ms_per_event"] = {"median": ws[len(ws) // 2] * 1e3, "max": ws[-1] * 1e3}
    return res


def loop(B, H, W, steps, summaries):
    from footprints_amd.training.train import SyntheticLoader, TrainManager
    with tempfile.TemporaryDirectory() as tmp:
        tm = TrainManager(SyntheticLoader(B, H, W, steps), val_loader=SyntheticLoader(B, H, W, 10, seed=11), epochs=1, log_freq=250, val_batches=10,
                          log_path=tmp, model_name="bench", summaries=summaries, log=lambda *a: None)
        tm.model_manager.save_folder = None
        tm.epoch = 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tm.run_epoch()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        tm.close_summaries()
        t2 = time.perf_counter()
        return {"steps": steps, "seconds": t1 - t0, "img_per_s": steps * B / (t1 - t0), "close_seconds": t2 - t1, "log_time_seconds": tm.log_time,
                "val_seconds": tm.val_time, "log_events": len(tm.history["train"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="both", choices=["kitti", "matterport", "both"])
    ap.add_argument("--steps", type=int, default=600)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    doc = {}
    for name in (("kitti", "matterport") if a.workload == "both" else (a.workload,)):
        B, H, W = WORKLOADS[name]
        doc[name] = {"shape": [B, H, W], **pieces(B, H, W, a.reps)}
        if a.steps > 0:
            doc[name]["loop_without_summaries"] = loop(B, H, W, a.steps, False)
            doc[name]["loop_with_summaries"] = loop(B, H, W, a.steps, True)
            doc[name]["loop_without_summaries_again"] = loop(B, H, W, a.steps, False)
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
