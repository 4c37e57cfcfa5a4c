"""Writes tests/golden/g14_reader.npz: what the installed Pillow's Image.resize and the REFERENCE's own FootprintsDataset.filter_depth_mask
give on the inputs of tests/golden/reader_inputs.py and tests/reader_restatement.mask_cases.

Needs Pillow, scipy and the reference checkout (oracle/ref_import.py); run as `python -m tests.golden.make_golden_reader` from the
repository root.  skimage.measure.label is stood in by scipy.ndimage.label with 8-connectivity, as in make_golden.py's g10_data_path.
The KITTI-size batch is stored as a digest only (tests/golden/digest.py).
"""
import importlib
import os

import numpy as np
import torch
from PIL import Image

from tests import reader_restatement as RR
from tests.golden import digest, reader_inputs as RI
from tests.golden.make_golden import _data_standins

NAME = "g14_reader"


def pil_resize(img, H, W, filt):
    out = np.asarray(Image.fromarray(img if img.ndim == 2 or img.shape[2] == 3 else img[:, :, 0]).resize((W, H), filt))
    return out.reshape(H, W, -1).copy()


def main():
    import PIL
    out = {"pillow_version": np.array(PIL.__version__)}
    for seed, (name, (h, w), (H, W), c) in enumerate(RI.SMALL_CASES):
        img = RI.image(h, w, c, seed)
        out["rs.%s.in" % name] = img
        out["rs.%s.out" % name] = pil_resize(img, H, W, Image.LANCZOS)
    name, (h, w), (H, W), c = RI.SMALL_CASES[0]
    for fname, filt in RR.FILTERS.items():
        out["rs.%s.%s.out" % (name, fname)] = pil_resize(RI.image(h, w, c, 0), H, W, filt)
    name, (h, w), (H, W), c = RI.HALF_CASE
    out["rs.%s.out" % name] = pil_resize(RR.half_image(h, w, c), H, W, Image.LANCZOS)
    for seed, (name, (h, w), (H, W), c) in enumerate(RI.SKIP_CASES):
        out.update(digest.digest("rs.%s.out" % name, torch.from_numpy(pil_resize(RI.image(h, w, c, 20 + seed), H, W, Image.LANCZOS)), full_limit=1 << 10))
    H, W = RI.KITTI_TARGET
    batch = np.stack([pil_resize(RI.image(h, w, 3, 30 + i), H, W, Image.LANCZOS) for i, (h, w) in enumerate(RI.KITTI_SIZES)])
    out.update(digest.digest("rs.kitti.out", torch.from_numpy(batch), full_limit=1 << 10))

    _data_standins()
    fd = importlib.import_module("footprints.datasets.footprint_dataset")
    ds = object.__new__(fd.FootprintsDataset)
    for H, W in RI.MASK_SIZES:
        ds.height, ds.width = H, W
        cases = dict(RR.mask_cases(H, W))
        for d in (10, 30, 55):
            cases["random%d" % d] = RI.random_mask(H, W, d, d)
        for name, m in cases.items():
            ref = ds.filter_depth_mask(m)
            assert ref.dtype == m.dtype and set(np.unique(ref)) <= {0.0, 1.0}
            out["dm.%dx%d.%s" % (H, W, name)] = np.packbits(ref.astype(bool))
    H, W = RI.KITTI_TARGET
    ds.height, ds.width = H, W
    for name, m in RI.kitti_masks().items():
        out["dm.%dx%d.%s" % (H, W, name)] = np.packbits(ds.filter_depth_mask(m).astype(bool))
    for p in digest.save(NAME, out):
        print(p, os.path.getsize(p))


if __name__ == "__main__":
    main()
