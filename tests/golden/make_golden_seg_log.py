"""Writes tests/golden/g_seg_log.npz and tests/golden/g_stretch.npz.

g_seg_log.npz: what the REFERENCE's own `preprocessing/segmentation/logger.py::log` hands to its SummaryWriter on the inputs of
tests/seg_log_restatement.py.  Run where the reference is at hand (oracle/ref_import.py), as `python -m tests.golden.make_golden_seg_log`
from the repository root.  The reference's file is loaded by its path and run as it is (it imports numpy and matplotlib alone; matplotlib
is the installed one: the plasma colours in the fixture are its own); the writer is the recorder below.  As in the reference's trainer
(train.py:119, 132) `prediction` is {'ground': sigmoid(logits)}, here torch's float32 sigmoid on the CPU, and `losses` the Evaluator's
five keys in its order.  Per case the file holds the inputs, the tags of every add_image / add_scalar call in order, the scalar values,
and every picture turned to bytes by tensorboardX's rule of the reference's time, `(x.astype(float32) * 255).astype(uint8)`, as [H, 3 W, 3].

g_stretch.npz: the maps of tests/stretch_restatement.py::cases and the RGB bytes `plt.imsave(..., format="jpg")` encodes for them:
matplotlib's own `ScalarMappable.to_rgba(bytes=True)`, which imsave hands to Pillow (checked here: imsave's file is Pillow's file of them)."""
import importlib.util
import io
import os

import numpy as np
import torch

from oracle import ref_import
from tests import seg_log_restatement as SR
from tests import stretch_restatement as ST

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = (("b2", dict(B=2, H=8, W=12, seed=3101)), ("b12", dict(B=12, H=8, W=12, seed=3102)), ("constant", dict(B=1, H=8, W=12, seed=3103, constant=True)))
LOSS_KEYS = ("ground_loss_0", "ground_loss_1", "ground_loss_2", "ground_loss_3", "loss")


class Recorder:
    def __init__(self):
        self.images, self.scalars = [], []

    def add_scalar(self, tag, value, step):
        self.scalars.append((tag, float(value), int(step)))

    def add_image(self, tag, img, step):
        self.images.append((tag, np.asarray(img).copy(), int(step)))


def seg_log():
    assert ref_import.available(), "needs the reference"
    import matplotlib
    matplotlib.use("Agg")
    spec = importlib.util.spec_from_file_location(
        "reference_segmentation_logger", os.path.join(ref_import.REFERENCE_ROOT, "footprints", "preprocessing", "segmentation", "logger.py"))
    ref_logger = importlib.util.module_from_spec(spec)
    import sys
    sys.dont_write_bytecode = True
    spec.loader.exec_module(ref_logger)
    out = {"matplotlib_version": np.array(matplotlib.__version__)}
    for name, kw in CASES:
        inputs, logits = SR.make_inputs(**kw)
        t_inputs = {k: torch.from_numpy(v) for k, v in inputs.items()}
        prediction = {"ground": torch.sigmoid(torch.from_numpy(logits)[:, 0])}
        losses = {k: torch.tensor(0.25 * (i + 1)) for i, k in enumerate(LOSS_KEYS)}
        rec = Recorder()
        ref_logger.log(rec, t_inputs, prediction, losses, 1e-4, step=7, num_outputs=10)
        assert all(s == 7 for _, _, s in rec.images + rec.scalars)
        for k, v in inputs.items():
            out["%s.in.%s" % (name, k)] = v
        out["%s.in.logits" % name] = logits
        out["%s.tags" % name] = np.array([t for t, _, _ in rec.images])
        out["%s.scalar_tags" % name] = np.array([t for t, _, _ in rec.scalars])
        out["%s.scalars" % name] = np.array([v for _, v, _ in rec.scalars], np.float64)
        pics = [(a.astype(np.float32) * 255).astype(np.uint8).transpose(1, 2, 0) for _, a, _ in rec.images]
        out["%s.pictures" % name] = np.stack(pics)
    path = os.path.join(HERE, "g_seg_log.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))


def stretch():
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    from matplotlib import cm
    out = {"matplotlib_version": np.array(matplotlib.__version__)}
    for name, x in ST.cases().items():
        out[name + ".in"] = x
        sm = cm.ScalarMappable(cmap=plt.get_cmap("viridis"))
        out[name + ".rgb"] = sm.to_rgba(x, bytes=True)[:, :, :3].copy()
        buf = io.BytesIO()
        plt.imsave(buf, x, format="jpg")
        assert buf.getvalue() == ST.pillow_file(out[name + ".rgb"]), name        # the RGB kept here IS what imsave encoded
    path = os.path.join(HERE, "g_stretch.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    seg_log()
    stretch()
