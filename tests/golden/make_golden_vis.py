"""Writes tests/golden/g15_vis.npz: what the installed Pillow (mode-"F" BILINEAR resize), matplotlib (the plasma map) and
footprints_amd.predict_simple.InferenceManager.visualise -- the host path built on both -- give on the inputs of tests/vis_restatement.py.

Needs Pillow and matplotlib; run as `python -m tests.golden.make_golden_vis` from the repository root.  Outputs above 1024 elements are
stored as digests (tests/golden/digest.py).  The side-by-side picture is the reference's formula (evaluation/inference.py:114-118 and
matplotlib's float-to-byte rule `(x * 255).astype(uint8)`) on a float32 image.
"""
import os

import numpy as np
import torch
from PIL import Image

from tests import vis_restatement as VR
from tests.golden import digest

NAME = "g15_vis"
LIMIT = 1 << 10


def main():
    import matplotlib
    import PIL
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    from footprints_amd.predict_simple import InferenceManager
    cmap = plt.get_cmap("plasma", 256)
    out = {"pillow_version": np.array(PIL.__version__), "matplotlib_version": np.array(matplotlib.__version__)}
    out["lut"] = (cmap(np.arange(256))[:, :3] * 255).astype(np.uint8)
    put = lambda name, a: out.update(digest.digest(name, torch.from_numpy(np.array(a)), full_limit=LIMIT))
    for name, _, (h, w) in VR.SIZE_CASES:
        pred, orig = VR.size_case_inputs(name)
        # the float map as its bytes: a digest's sums are exact integers then, whatever order they are added in
        put("rf.%s" % name, np.asarray(Image.fromarray(pred[1], "F").resize((w, h), Image.BILINEAR)).view(np.uint8))
        put("vis.%s" % name, InferenceManager.visualise(pred, Image.fromarray(orig)))
    for name, pred in VR.value_cases().items():
        for h, w in VR.VALUE_SIZES:
            put("vis.%s.%dx%d" % (name, h, w), InferenceManager.visualise(pred, Image.fromarray(VR.original(h, w, 60))))
    image, pred = VR.side_by_side_inputs()
    sig = 1.0 / (1.0 + np.exp(-pred[:, 1].astype(np.float64)))          # nothing in (0, 1e-6): float64 and fp32 sigmoids agree about 0.5
    right = cmap((sig > 0.5).astype(float))[..., :3]
    left = (image * np.float32(255.0)).astype(np.uint8).transpose(0, 2, 3, 1)
    put("sbs", np.concatenate([left, (right * 255).astype(np.uint8)], axis=2))
    for p in digest.save(NAME, out):
        print(p, os.path.getsize(p))


if __name__ == "__main__":
    main()
