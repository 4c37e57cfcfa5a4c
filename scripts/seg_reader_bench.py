"""GPU box: what a training batch of the ground-segmentation trainer costs on the device path (csrc/resample_u8.hip, csrc/seg_reader.hip,
datasets/device_path.SegBatchAssembler) next to the host chain it replaces and to the step it feeds, for three kinds of batches of 12 at
192 x 640: Cityscapes frames (1024 x 2048), Matterport frames (1024 rows x 1280 columns) and an ADE20K-like mix of small and large frames.

    python scripts/seg_reader_bench.py [--seconds 2.0] [--rounds 5] [--steps 40]

Per case: the kernels alone (windowed resizes + flip / jitter / ToTensor + labels; HIP events), the kernels with the H2D copies of the
staged rectangles and tables, the host half (`draw` + `fill`: plans, tables, rectangle copies into pinned memory; one thread), the
reference's per-sample Pillow chain on one core (decode and ColorJitter not included), the Segmentor train step alone on a resident
batch, and the train step with the loader in the loop on the synthetic source.  Prints one JSON line."""
import argparse
import json
import os
import random
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from footprints_amd import ops
from footprints_amd.datasets.device_path import SegBatchAssembler, SyntheticSegSource
from footprints_amd.preprocessing.segmentation.datasets import plan as P

B, H, W = 12, 192, 640
CASES = {
    "cityscapes": dict(frames=[("cityscapes", (1024, 2048))], max_src_hw=(544, 1664)),
    "matterport": dict(frames=[("matterport", (1024, 1280))], max_src_hw=(544, 1664)),
    "ade20k_mix": dict(frames=[("ADE20K", hw) for hw in [(256, 341), (512, 683), (683, 512), (1536, 2048), (375, 500), (768, 1024)]],
                       max_src_hw=(544, 1664)),
}


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


def pillow_chain(samples, plans):
    """the reference's per-sample chain with the plans' sizes: crop rows, LANCZOS + NEAREST resizes of the WHOLE frame, crop_all, in1d"""
    from PIL import Image
    for (name, image, labels), plan in zip(samples, plans):
        img, lab = Image.fromarray(image[:plan.rows]), Image.fromarray(labels[:plan.rows])
        for th, tw in P.plan_sizes(plan)[1:]:
            img, lab = img.resize((tw, th), Image.LANCZOS), lab.resize((tw, th), Image.NEAREST)
        top, left, h, w = plan.window
        img, lab = img.crop((left, top, left + w, top + h)), lab.crop((left, top, left + w, top + h))
        ids = np.array(lab)
        ids = ids[..., 0].astype(np.int64) // 10 * 256 + ids[..., 1] if name == "ADE20K" else (ids[..., 0] if ids.ndim == 3 else ids)
        np.isin(ids, P.GROUND_IDS[name]).astype(float)                  # np.in1d(...).reshape(...) of _generate_mask
        np.asarray(img)


def step_fn(model, optimiser, evaluator):
    def step(batch):
        loss = evaluator.compute_losses(model(batch["image"]), batch["ground_mask"], batch["labelled_pix"])
        model.zero_grad()
        loss.backward()
        optimiser.step()
        return loss
    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=2.0, help="total time of every timed loop, over all rounds")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=40, help="train steps per timed loop")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("seg_reader_bench.py needs a GPU: a time measured anywhere else says nothing about it")
    from footprints_amd.optim import FusedAdam
    from footprints_amd.preprocessing.segmentation.evaluation import Evaluator
    from footprints_amd.preprocessing.segmentation.network import Segmentor
    model = Segmentor(pretrained=False, use_PSP=True).cuda()
    model.train()
    step = step_fn(model, FusedAdam(model, lr=1e-4), Evaluator())
    out = {"device": torch.cuda.get_device_name(0), "batch": B, "height": H, "width": W, "rounds": a.rounds, "cases": {}}
    for case, cfg in CASES.items():
        source = SyntheticSegSource(B, a.steps + 5, cfg["frames"], seed=3)
        asm = SegBatchAssembler(B, H, W, max_src_hw=cfg["max_src_hw"])
        samples = next(iter(source))
        plans = asm.draw(samples, True, random.Random(7))
        slot = asm.submit(samples, plans)
        batch = {k: v.clone() for k, v in asm.collect(slot).items()}
        s = asm.slots[slot]
        used = dict(s["used"])
        res = {"staged_image_bytes": used["src"], "staged_label_bytes": used["lab"], "frame_bytes": sum(x[1].size for x in samples),
               "h2d_bytes": int(sum(n * s["h_" + k].element_size() for k, n in used.items())), "two_stage_samples": sum(p.stage1 is not None and p.stage2 is not None for p in plans)}

        def launch(with_copies):
            with ops.on_stream(asm.stream):
                asm._launch(s, copies=with_copies)
        legs = {"kernels": lambda: launch(False), "kernels_and_copies": lambda: launch(True)}
        iters, samples_ms = {}, {leg: [] for leg in legs}
        for leg, fn in legs.items():
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            iters[leg] = max(3, int(a.seconds * 1e3 / a.rounds / max(timed(fn, 3, asm.stream), 1e-3)))
        for _ in range(a.rounds):
            for leg, fn in legs.items():
                samples_ms[leg].append(timed(fn, iters[leg], asm.stream))
        torch.cuda.synchronize()
        res["ms"] = {leg: float(np.median(v)) for leg, v in samples_ms.items()}
        res["spread"] = {leg: float((max(v) - min(v)) / np.median(v)) for leg, v in samples_ms.items()}
        rng = random.Random(11)
        res["ms"]["host_draw_and_fill"] = host_ms(lambda: asm.fill(samples, asm.draw(samples, True, rng)), a.seconds / 2)
        torch.set_num_threads(1)
        try:
            import PIL
            res["ms"]["host_pillow_chain_one_core"] = host_ms(lambda: pillow_chain(samples, plans), a.seconds / 2)
            res["pillow_version"] = PIL.__version__
        except ImportError:
            res["ms"]["host_pillow_chain_one_core"] = None
        # the train step alone on the resident batch, then with the loader in the loop
        for _ in range(5):
            step(batch)
        torch.cuda.synchronize()
        alone, looped = [], []
        for _ in range(max(a.rounds // 2, 2)):
            t0 = time.perf_counter()
            for _ in range(a.steps):
                step(batch)
            torch.cuda.synchronize()
            alone.append((time.perf_counter() - t0) * 1e3 / a.steps)
            n, t0 = 0, None
            for bt in asm.loader(source, True, random.Random(13)):
                if n == 5:                      # the loader's first batches fill the pipeline
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                step(bt)
                n += 1
            torch.cuda.synchronize()
            looped.append((time.perf_counter() - t0) * 1e3 / (n - 5))
        res["ms"]["train_step_alone"] = float(np.median(alone))
        res["ms"]["train_step_with_loader"] = float(np.median(looped))
        res["img_per_s"] = {"train_step_alone": B / res["ms"]["train_step_alone"] * 1e3, "train_step_with_loader": B / res["ms"]["train_step_with_loader"] * 1e3}
        res["loader_cost_fraction"] = res["ms"]["train_step_with_loader"] / res["ms"]["train_step_alone"] - 1.0
        out["cases"][case] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
