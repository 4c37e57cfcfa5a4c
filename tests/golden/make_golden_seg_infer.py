"""Writes tests/golden/g17_seg_infer.npz: what the REFERENCE's segmentation `Tester.test_batch`, `KITTIInferenceDataset.save_result` and the
installed matplotlib give on recorded logit maps.

Needs the reference checkout (oracle/ref_import.py), matplotlib and Pillow; run as `python -m tests.golden.make_golden_seg_infer` from the
repository root.  What runs from the reference: `Tester.test_batch` (on a Tester made without `__init__`, with
`opt.save_test_visualisations = True` and a `model` that returns the recorded logit maps) and `KITTIInferenceDataset.save_result` into a
temporary folder.  Every visualisation also goes through `plt.imsave(format="png")` and is read back with Pillow: those are the bytes
matplotlib writes before any JPEG coding.  Absent third-party modules are stood in HERE: tensorboardX (imported by train.py, never
called), torchvision.transforms.{Resize, ToTensor} (constructed by the dataset, never called), cv2 (never called) and Pillow's removed
alias Image.ANTIALIAS (= LANCZOS).
Stored: the logits, the images, the float32 predictions, the float16 files' contents and relative paths, the picture bytes."""
import argparse
import importlib
import io
import os
import sys
import tempfile
import types

import numpy as np
import torch
from PIL import Image

from oracle import ref_import
from tests.golden import digest

NAME = "g17_seg_infer"
B, H, W = 2, 8, 24
FILENAMES = ["2011_09_26/2011_09_26_drive_0001_sync 5 l", "2011_09_28/2011_09_28_drive_0002_sync 17 r"]
PLANTED = [100.0, -100.0, 17.3, -17.3, 17.4, -17.4, 9.7, -9.7, 0.0]


def inputs():
    rng = np.random.default_rng(17)
    logits = np.empty((B, 1, H, W), np.float32)
    logits[0, 0] = np.linspace(-20.0, 20.0, H * W, dtype=np.float64).astype(np.float32).reshape(H, W)
    rnd = (rng.standard_normal(H * W) * 6.0).astype(np.float32)
    rnd[rng.permutation(H * W)[:len(PLANTED)]] = np.array(PLANTED, np.float32)
    logits[1, 0] = rnd.reshape(H, W)
    # the network's input is ToTensor's k / 255; image 1 also holds the float32 neighbours of those values on both sides and plain floats
    n = 3 * H * W
    k = np.arange(256, dtype=np.float32) / np.float32(255)
    im0 = np.concatenate([k, rng.integers(0, 256, n - 256).astype(np.float32) / np.float32(255)])
    up, down = np.nextafter(k[:-1], np.float32(2)), np.nextafter(k[1:], np.float32(-1))
    im1 = np.concatenate([up, down, rng.random(n - 510, dtype=np.float32)])
    images = np.stack([rng.permutation(im0), rng.permutation(im1)]).astype(np.float32).reshape(B, 3, H, W)
    assert images.min() >= 0 and images.max() <= 1
    return logits, images


def _standins():
    ref_import.load_reference()
    if "tensorboardX" not in sys.modules:
        tbx = types.ModuleType("tensorboardX")
        tbx.SummaryWriter = object
        sys.modules["tensorboardX"] = tbx
    tvt = sys.modules["torchvision.transforms"]

    class Resize:
        def __init__(self, size, interpolation=None):
            self.size, self.interpolation = size, interpolation

    class ToTensor:
        pass

    fn = types.ModuleType("torchvision.transforms.functional")
    for name, obj in (("Resize", Resize), ("ToTensor", ToTensor), ("ColorJitter", Resize), ("functional", fn)):
        if not hasattr(tvt, name):
            setattr(tvt, name, obj)
    sys.modules.setdefault("torchvision.transforms.functional", fn)
    sys.modules["torchvision"].transforms = tvt
    if not hasattr(Image, "ANTIALIAS"):
        Image.ANTIALIAS = Image.LANCZOS


def main():
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    import PIL
    _standins()
    inference = importlib.import_module("footprints.preprocessing.segmentation.inference")
    logits, images = inputs()
    tester = object.__new__(inference.Tester)
    tester.opt = argparse.Namespace(save_test_visualisations=True)
    tester.sigmoid = torch.nn.Sigmoid()
    tester.model = lambda image: [None, None, None, torch.from_numpy(logits)]
    with torch.no_grad():
        preds, visualisations = tester.test_batch({"image": torch.from_numpy(images)})
    assert preds.dtype == np.float32 and preds.shape == (B, 1, H, W) and len(visualisations) == B
    dataset = inference.KITTIInferenceDataset("", FILENAMES, H, W)
    out = {"matplotlib_version": np.array(matplotlib.__version__), "pillow_version": np.array(PIL.__version__),
           "filenames": np.array(FILENAMES), "logits": logits, "images": images, "preds": preds}
    pictures = []
    with tempfile.TemporaryDirectory() as tmp:
        for i in range(B):
            dataset.save_result(i, preds[i], tmp, visualisations[i])
            buf = io.BytesIO()
            plt.imsave(buf, visualisations[i], format="png")
            buf.seek(0)
            pictures.append(np.asarray(Image.open(buf).convert("RGB")).copy())
        npy, jpg = [], []
        for root, _, files in sorted(os.walk(tmp)):
            for f in sorted(files):
                rel = os.path.relpath(os.path.join(root, f), tmp)
                (npy if f.endswith(".npy") else jpg).append(rel)
        out["npy_paths"], out["jpg_paths"] = np.array(npy), np.array(jpg)
        for i, rel in enumerate(npy):
            out["npy.%d" % i] = np.load(os.path.join(tmp, rel))
        out["jpg_sizes"] = np.array([Image.open(os.path.join(tmp, rel)).size[::-1] for rel in jpg], np.int64)
    out["pictures"] = np.stack(pictures)
    for k, v in out.items():
        print(k, v.dtype, v.shape)
    for p in digest.save(NAME, out):
        print(p, os.path.getsize(p))


if __name__ == "__main__":
    main()
