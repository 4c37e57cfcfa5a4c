"""Writes tests/golden/g16_seg_reader.npz: what the REFERENCE's own segmentation dataset code and the installed Pillow give on the inputs of
tests/golden/seg_reader_inputs.py.

Needs Pillow and the reference checkout (oracle/ref_import.py); run as `python -m tests.golden.make_golden_seg_reader` from the repository
root.  What runs from the reference:
* `CityscapesDataset.__getitem__` whole, on synthetic PNGs in a temporary directory;
* for ADE20K and Matterport `_preprocess`, `prepare_size`, `_augment_data` and `_generate_mask`; only the two lines of the reference that
  do not run are restated here: ade20k_dataset.py:51 (uint8 overflow under numpy 2: the id in integer arithmetic) and
  matterport_dataset.py:59 (`self.generate_mask` does not exist: `_generate_mask`).
Absent third-party modules are stood in HERE: torchvision.transforms.{Resize, ColorJitter, ToTensor} and transforms.functional.hflip
(torchvision 0.4.2's behaviour on top of the real Pillow; ColorJitter's byte arithmetic is oracle/data_path.jitter_pil), cv2 (never
called) and matplotlib (imported by a sibling module only).  `torch.rand(2)` of `_augment_data` is fed from Python's `random`, so that
ONE seeded stream makes every decision: the package's plan takes all draws from one rng (datasets/plan.py).  The uniform draws made are
recorded and stored, as are the sizes of every LANCZOS resize and the crop box, taken from Pillow's own calls.
The 1024 x 2048 batch is stored as a digest only (tests/golden/digest.py).
"""
import hashlib
import importlib
import os
import random
import sys
import tempfile
import types

import numpy as np
import torch
from PIL import Image

from oracle import data_path as D
from oracle import ref_import
from tests.golden import digest, seg_reader_inputs as SI

NAME = "g16_seg_reader"


def _standins():
    ref_import.load_reference()
    if "matplotlib" not in sys.modules:
        try:
            import matplotlib.pyplot  # noqa: F401
        except ImportError:
            mpl = types.ModuleType("matplotlib")
            mpl.pyplot = types.ModuleType("matplotlib.pyplot")
            sys.modules["matplotlib"], sys.modules["matplotlib.pyplot"] = mpl, mpl.pyplot
    tvt = sys.modules["torchvision.transforms"]

    class Resize:
        def __init__(self, size, interpolation=Image.BILINEAR):
            self.size, self.interpolation = size, interpolation

        def __call__(self, img):                       # functional.resize with a (h, w) size: img.resize(size[::-1], interpolation)
            return img.resize(self.size[::-1], self.interpolation)

    class ColorJitter:
        def __init__(self, brightness, contrast, saturation, hue):          # _check_input: [max(0, 1 - v), 1 + v]; hue [-v, v]
            self.ranges = tuple((max(0, 1 - v), 1 + v) for v in (brightness, contrast, saturation)) + ((-hue, hue),)

        def __call__(self, img):                       # get_params: four uniforms, then the shuffle of the transforms
            factors = [random.uniform(lo, hi) for lo, hi in self.ranges]
            order = [D.BRIGHTNESS, D.CONTRAST, D.SATURATION, D.HUE]
            random.shuffle(order)
            return D.jitter_pil(img, order, factors)

    class ToTensor:
        def __call__(self, pic):
            return torch.from_numpy(np.asarray(pic).copy()).permute(2, 0, 1).contiguous().float().div(255)

    fn = types.ModuleType("torchvision.transforms.functional")
    fn.hflip = lambda img: img.transpose(Image.FLIP_LEFT_RIGHT)
    tvt.Resize, tvt.ColorJitter, tvt.ToTensor, tvt.functional = Resize, ColorJitter, ToTensor, fn
    sys.modules["torchvision.transforms.functional"] = fn
    sys.modules["torchvision"].transforms = tvt


class _Torch:
    """`torch` as base_dataset.py sees it: rand(n) draws from Python's `random`, in float64 so that `> 0.5` decides on the draw itself"""

    def __getattr__(self, name):
        return getattr(torch, name)

    @staticmethod
    def rand(n):
        return torch.tensor([random.random() for _ in range(n)], dtype=torch.float64)


class _Recorder:
    """records the uniform draws of `random.random`, the LANCZOS resizes and the crops Pillow is asked for while it is active"""

    def __enter__(self):
        self.draws, self.resizes, self.crops = [], [], []
        self._random, self._resize, self._crop = random.random, Image.Image.resize, Image.Image.crop
        rec = self

        def rnd():
            v = rec._random()
            rec.draws.append(v)
            return v

        def resize(im, size, resample=None, *a, **k):
            if resample == Image.LANCZOS:
                rec.resizes.append((size[1], size[0]))
            return rec._resize(im, size, resample, *a, **k)

        def crop(im, box=None):
            if im.mode == "RGB":
                rec.crops.append(tuple(box))
            return rec._crop(im, box)
        random.random, Image.Image.resize, Image.Image.crop = rnd, resize, crop
        return self

    def __exit__(self, *exc):
        random.random, Image.Image.resize, Image.Image.crop = self._random, self._resize, self._crop


def run_sample(mods, case, feed, tmp):
    """one sample through the reference -> dict of arrays"""
    name, dataset, (h, w), is_train, seed = case
    _, image, labels = SI.sample_inputs(case)
    H, W = feed
    random.seed(seed)
    with _Recorder() as rec:
        if dataset == "cityscapes":
            for sub, arr, suffix in (("leftImg8bit", image, "_leftImg8bit.png"), ("gtFine", labels, "_gtFine_labelIds.png")):
                os.makedirs(os.path.join(tmp, sub, "train", name), exist_ok=True)
                Image.fromarray(arr, "RGB").save(os.path.join(tmp, sub, "train", name, "frame" + suffix))
            ds = mods["cityscapes"].CityscapesDataset(tmp, ["train %s frame" % name], H, W, is_train=is_train)
            rec.draws.clear()
            out = ds[0]
            img, ground, labelled = out["image"], out["ground_mask"], out["labelled_pix"]
        else:
            cls = mods["ADE20K"].ADE20KDataset if dataset == "ADE20K" else mods["matterport"].MatterportDataset
            ds = cls("", [], H, W, is_train=is_train)
            pil, lab = Image.fromarray(image, "RGB"), Image.fromarray(labels, "RGB" if dataset == "ADE20K" else "L")
            pil, lab = ds._preprocess(pil, lab)
            pil, lab = mods["utils"].prepare_size(pil, lab, H, W, keep_aspect_ratio=True)
            if is_train:
                pil, lab = ds._augment_data(pil, lab)
            img = ds.to_tensor(pil).float()
            lab = np.array(lab)
            if dataset == "ADE20K":                    # ade20k_dataset.py:51 in integers (uint8 overflows under numpy 2)
                lab = lab[..., 0].astype(np.int64) // 10 * 256 + lab[..., 1].astype(np.int64)
            ground = torch.from_numpy(ds._generate_mask(lab)).float()          # matterport_dataset.py:59 means _generate_mask
            labelled = torch.ones_like(ground).float()
    # crop_all's box, asked of the image and of an RGB label image alike (Cityscapes' row crop has another size)
    crops = sorted(set(c for c in rec.crops if (c[2] - c[0], c[3] - c[1]) == (W, H)))
    assert len(crops) <= 1 and img.shape == (3, H, W) and ground.shape == (H, W)
    box = crops[0] if crops else (0, 0, W, H)
    return {"image": img.numpy(), "ground_mask": ground.numpy(), "labelled_pix": labelled.numpy(), "draws": np.array(rec.draws, np.float64),
            "resizes": np.array(rec.resizes, np.int64).reshape(-1, 2), "window": np.array([box[1], box[0], H, W], np.int64)}


def main():
    import PIL
    _standins()
    pkg = "footprints.preprocessing.segmentation.datasets."
    mods = {"cityscapes": importlib.import_module(pkg + "cityscapes_dataset"), "ADE20K": importlib.import_module(pkg + "ade20k_dataset"),
            "matterport": importlib.import_module(pkg + "matterport_dataset"), "utils": importlib.import_module(pkg + "dataset_utils")}
    importlib.import_module(pkg + "base_dataset").torch = _Torch()
    out = {"pillow_version": np.array(PIL.__version__)}
    with tempfile.TemporaryDirectory() as tmp:
        for case in SI.SAMPLES:
            for k, v in run_sample(mods, case, SI.FEED, tmp).items():
                out["%s.%s" % (case[0], k)] = v
            print(case[0], out[case[0] + ".resizes"].tolist(), out[case[0] + ".window"].tolist(), out[case[0] + ".draws"].tolist())
        big = [run_sample(mods, case, SI.BIG_FEED, tmp) for case in SI.BIG]
    for case, r in zip(SI.BIG, big):
        for k in ("draws", "resizes", "window"):
            out["%s.%s" % (case[0], k)] = r[k]
        print(case[0], r["resizes"].tolist(), r["window"].tolist(), r["draws"].tolist())
    for k in ("image", "ground_mask", "labelled_pix"):
        a = np.ascontiguousarray(np.stack([r[k] for r in big]))
        out.update(digest.digest("big." + k, torch.from_numpy(a), full_limit=1 << 10))
        out["big.%s#sha256" % k] = np.frombuffer(hashlib.sha256(a.tobytes()).digest(), np.uint8)       # every byte, not a sample
    for p in digest.save(NAME, out):
        print(p, os.path.getsize(p))


if __name__ == "__main__":
    main()
