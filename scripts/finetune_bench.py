"""Step time of the fine-tuning recipes against the full training step: TrainStep at 12 x 192 x 640, default operand format, for

    full            everything trains, batch statistics (the step bench.py measures)
    frozen_stats    everything trains, the encoder's BatchNorms on their running statistics (model.freeze_bn_stats())
    freeze_encoder  the decoders train (--freeze encoder), batch statistics still move
    freeze_encoder+frozen_stats   both: the forward is the BN-folded inference encoder, the backward stops at the features

One process, ONE model and engine (a second engine's side streams would share hardware queues with the first one's): every
configuration has its own optimiser and TrainStep, and a switch sets the parameters' requires_grad flags and the BatchNorm mode, which
drops the recorded plans -- so every window starts with a warm-up past plan recording (two eager steps, the recording step, replays).
Timing: device events around a window of replayed steps of at least `--window` seconds; the four configurations alternate and the whole
sequence runs `--repeats` times, so the spread of one configuration is visible next to the differences between them.  Launches per step =
the node count of the recorded plan (kernel launches + stream-ordering edges).

    python scripts/finetune_bench.py [--batch 12 --height 192 --width 640 --window 2.0 --repeats 3]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CONFIGS = [("full", (), False), ("frozen_stats", (), True), ("freeze_encoder", ("encoder",), False),
           ("freeze_encoder+frozen_stats", ("encoder",), True)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=12)
    ap.add_argument("--height", type=int, default=192)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--window", type=float, default=2.0, help="seconds of replayed steps per timed window (at least)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=8, help="steps before a window: 2 eager, 1 recording, the rest replays")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("finetune_bench: needs a GPU (there is no CPU path to time)")
    from footprints_amd._format import operand_format
    from footprints_amd.model_manager import ModelManager
    from footprints_amd.optim import FusedAdam
    from footprints_amd.training.train import SEED, TrainStep, synthetic_batch
    torch.manual_seed(SEED)
    mm = ModelManager(use_cuda=True)
    model = mm.model
    batch = synthetic_batch(a.batch, a.height, a.width, "cuda")
    runs = {}
    for name, prefixes, stats in CONFIGS:
        opt = FusedAdam(model, lr=1e-4)
        runs[name] = (opt, TrainStep(model, opt), prefixes, stats)

    def select(name):
        _, _, prefixes, stats = runs[name]
        for n, p in model.named_parameters():
            p.requires_grad_(not n.startswith(prefixes) if prefixes else True)
        model.freeze_bn_stats(stats)
        model.train()

    def window(name, steps):
        _, ts, _, _ = runs[name]
        select(name)
        for _ in range(a.warmup):
            ts(batch)
        assert len(ts._plans) == 1, "%s: the step did not reach its recorded plan (%d plans)" % (name, len(ts._plans))
        nodes = next(iter(ts._plans.values()))[3]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(steps):
            ts(batch)
        e1.record()
        torch.cuda.synchronize()
        assert len(ts._plans) == 1
        return e0.elapsed_time(e1) / steps, nodes, float(ts.losses[20])

    ms, nodes, steps = {n: [] for n, *_ in CONFIGS}, {}, {}
    for name, *_ in CONFIGS:                      # calibration: how many steps fill the window
        t, _, _ = window(name, 20)
        steps[name] = max(20, int(a.window * 1.05 * 1000.0 / t) + 1)      # (5 % over: a window a little faster than the calibration still lasts)
    for rep in range(a.repeats):
        for name, *_ in CONFIGS:
            t, n, loss = window(name, steps[name])
            ms[name].append(t)
            nodes[name] = n
            print("rep %d %-28s %8.3f ms/step over %d steps (%.2f s)  plan nodes %d  loss %.4f" % (rep, name, t, steps[name], t * steps[name] / 1000.0, n, loss),
                  flush=True)
    base = sorted(ms["full"])[len(ms["full"]) // 2]
    print("\n| configuration | ms / step (each repeat) | median | spread (max - min) | vs full | plan nodes / step |\n|---|---|---|---|---|---|")
    for name, *_ in CONFIGS:
        v = ms[name]
        med = sorted(v)[len(v) // 2]
        print("| %s | %s | %.3f | %.3f | %.3f x | %d |" % (name, " / ".join("%.3f" % x for x in v), med, max(v) - min(v), med / base, nodes[name]))
    print(json.dumps({"bench": "finetune", "shape": [a.batch, a.height, a.width], "operand_format": operand_format(), "window_s": a.window,
                      "ms_per_step": ms, "plan_nodes": nodes, "steps_per_window": steps}))


if __name__ == "__main__":
    main()
