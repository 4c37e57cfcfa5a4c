"""NumPy restatement of fp_infer_pack (footprints_amd/csrc/infer_pack.hip), put together from the pieces of the existing restatements so
that it cannot drift from them: the float16 rounding and the float64 sigmoid of seg_infer_restatement.py, the picture of
vis_restatement.py::side_by_side.  Not a test; shared by test_infer_pipeline_cpu.py and test_gpu_infer_pipeline.py.

The kernel's sigmoid is a float32 one (accurate expf, correctly rounded division) and may differ from the float64 sigmoid rounded once by
its own error, so `halves` takes the float32 sigmoid to round as an argument where bytes are compared; the GPU test compares the kernel
with fp_pack_pred_fp16 bit for bit and uses this module for what both must satisfy."""
import numpy as np

from tests import seg_infer_restatement as SR
from tests import vis_restatement as VR


def halves(pred, p32=None):
    """pred float32 [B, 4, H, W] -> float16 [B, 4, H, W]: sigmoid on channels 0 and 1 (p32: the float32 sigmoid of those two channels,
    default the float64 one rounded once), channels 2 and 3 as they are, everything rounded to nearest even"""
    pred = np.asarray(pred, dtype=np.float32)
    if p32 is None:
        p32 = SR.sigmoid64(pred[:, :2]).astype(np.float32)
    return SR.to_half(np.concatenate([np.asarray(p32, np.float32), pred[:, 2:]], axis=1))


def pack(pred, image, colour0, colour1, p32=None):
    """-> (float16 [B, 4, H, W], uint8 [B, H, 2 W, 3] or None without an image)"""
    return halves(pred, p32), (VR.side_by_side(image, pred, colour0, colour1) if image is not None else None)


# logits the tests plant: signed zeros; +-1e-8 (positive or negative, but the sigmoid rounds to exactly 0.5: the picture follows the sign);
# saturation in float16 (+-20), near expf's overflow (+-88) and beyond it (+-104); sigmoids that are float16 subnormals (-17.3 .. -9.7)
PLANTED = np.array([0.0, -0.0, 1e-8, -1e-8, 20.0, -20.0, 88.0, -88.0, 104.0, -104.0, -17.3, -17.0, -16.0, -14.5, -12.0, -10.5, -9.8],
                   dtype=np.float32)


def inputs(B, H, W, seed):
    """(pred float32 [B, 4, H, W], image float32 [B, 3, H, W]): logits in [-30, 30] with PLANTED written into channels 0 and 1 as far as
    they fit; channels 2 and 3 in [0, 1] with exact float16 ties among them (a float16 plus half its spacing: round to even decides)"""
    rng = np.random.default_rng(seed)
    pred = np.empty((B, 4, H, W), np.float32)
    pred[:, :2] = rng.uniform(-30.0, 30.0, (B, 2, H, W)).astype(np.float32)
    depth = rng.random((B, 2, H, W), dtype=np.float32)
    h16 = depth.astype(np.float16)
    ties = (h16.astype(np.float32) + np.spacing(h16).astype(np.float32) / np.float32(2)).astype(np.float32)
    use = rng.random((B, 2, H, W)) < 0.25
    pred[:, 2:] = np.clip(np.where(use, ties, depth), 0.0, 1.0)
    for c in (0, 1):
        flat = pred[:, c].reshape(-1)                       # a copy when B > 1: written back below
        pos = rng.permutation(flat.size)[:PLANTED.size]
        flat[pos] = PLANTED[:pos.size]
        pred[:, c] = flat.reshape(B, H, W)
    k = np.arange(256, dtype=np.float32) / np.float32(255)
    pool = np.concatenate([k, np.nextafter(k[:-1], np.float32(2)), np.nextafter(k[1:], np.float32(-1)), rng.random(256, dtype=np.float32)])
    image = rng.choice(pool, size=(B, 3, H, W)).astype(np.float32)
    return pred, image
