"""Writes tests/golden/g21_log.npz: what the REFERENCE's own `training/logger.py::log` hands to its SummaryWriter, with the prediction
tensors its own `LossManager` builds, on the inputs of tests/log_panels_restatement.py.

Run where the reference is at hand (oracle/ref_import.py), as `python -m tests.golden.make_golden_log` from the repository root.  The
reference's imports that are not installed get stand-ins, as in make_golden.py: `cv2` and `torchvision` through oracle.ref_import, `loguru`
(a module with a `logger` whose `info` prints) and `tensorboardX` (never imported by logger.py; the writer is the recorder below).
matplotlib is installed and is the real one: the plasma colours in the fixture are its own.

Per case the file holds the inputs, the tags of every add_image / add_scalar call in order, and every array as float (the reference passes
float32 tensors, and a float64 array for the colour-mapped disparity)."""
import os
import sys
import types

import numpy as np
import torch

from oracle import ref_import
from tests import log_panels_restatement as LR

NAME = "g21_log"
DEPTH_RANGE = (0.1, 100)
CASES = (("plain", dict(B=4, H=8, W=16, seed=2101)), ("constant", dict(B=4, H=8, W=16, seed=2102, constant=True)))


class Recorder:
    def __init__(self):
        self.images, self.scalars = [], []

    def add_scalar(self, tag, value, step):
        self.scalars.append((tag, float(value), int(step)))

    def add_image(self, tag, img, step):
        a = img.detach().cpu().numpy() if torch.is_tensor(img) else np.asarray(img)
        self.images.append((tag, a.copy(), int(step)))


def main():
    mods = ref_import.load_reference()
    assert mods is not None, "needs the reference"
    _, loss_mod = mods
    if "loguru" not in sys.modules:
        lg = types.ModuleType("loguru")
        lg.logger = types.SimpleNamespace(info=print)
        sys.modules["loguru"] = lg
    import importlib
    import matplotlib
    matplotlib.use("Agg")
    ref_logger = importlib.import_module("footprints.training.logger")
    out = {"matplotlib_version": np.array(matplotlib.__version__)}
    for name, kw in CASES:
        inputs, pred = LR.make_inputs(**kw)
        # the four scales of `predictions`: the logger reads 1/1 alone; the others only feed the loss
        predictions = {k: pred.clone() for k in ("1/8", "1/4", "1/2", "1/1")}
        with torch.no_grad():
            losses = loss_mod.LossManager(DEPTH_RANGE, 0.25)(predictions, inputs)
        rec = Recorder()
        ref_logger.log(rec, inputs, predictions, losses, 1e-4, 7)
        for k, v in inputs.items():
            out["%s.in.%s" % (name, k)] = v.numpy()
        out["%s.in.pred" % name] = pred.numpy()
        out["%s.tags" % name] = np.array([t for t, _, _ in rec.images])
        out["%s.scalar_tags" % name] = np.array([t for t, _, _ in rec.scalars])
        out["%s.scalars" % name] = np.array([v for _, v, _ in rec.scalars], np.float64)
        assert all(s == 7 for _, _, s in rec.images + rec.scalars)
        for i, (_, a, _) in enumerate(rec.images):
            out["%s.img.%03d" % (name, i)] = a
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), NAME + ".npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
