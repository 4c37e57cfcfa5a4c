"""NumPy restatement of fp_seg_pack (footprints_amd/csrc/seg_infer.hip): what the reference's segmentation Tester.test_batch,
`save_result` and matplotlib's imsave do to a logit map and the network's input.  Not a test; shared by test_seg_infer_cpu.py (against
fixture G17, recorded from the reference and matplotlib) and test_gpu_seg_infer.py (against the kernel).

The two picture rules are plain truncations (both hold byte for byte against matplotlib 3.10's imsave, fixture G17):
  colour index  min(int(p * 256), 255) with the product in FLOAT32: Colormap.__call__ scales a float32 array in its own type, truncates,
                and maps p == 1 to the last entry
  image bytes   uint8(float64(image) * 255): the visualisation is a float64 array (the colour map's output promotes the concatenation),
                and the float image path multiplies by 255 and truncates"""
import numpy as np


def sigmoid64(logits):
    """the sigmoid in float64: the reference value of prob_f32"""
    x = np.asarray(logits, dtype=np.float64)
    return 1.0 / (1.0 + np.exp(-x))


def to_half(p32):
    """save_result's cast: round to nearest even, float16 subnormals included"""
    return np.asarray(p32, dtype=np.float32).astype(np.float16)


def colour_index(p32):
    p32 = np.asarray(p32, dtype=np.float32)
    return np.minimum((p32 * np.float32(256.0)).astype(np.int64), 255)


def picture(p32, image, lut):
    """p32 float32 [B, 1, H, W], image float32 [B, 3, H, W] in [0, 1], lut uint8 [256, 3] -> uint8 [B, H, 2 W, 3]"""
    left = (np.asarray(image, dtype=np.float32).astype(np.float64).transpose(0, 2, 3, 1) * 255.0).astype(np.uint8)
    right = np.asarray(lut, dtype=np.uint8)[colour_index(p32)[:, 0]]
    return np.concatenate([left, right], axis=2)


def pack(logits, image, lut, p32=None):
    """-> dict(p64 = float64 sigmoid, p32, half, picture); p32: the float32 sigmoid to round and draw (default: the float64 one rounded
    once -- a float32 implementation may differ from that by its own error, so a comparison of bytes feeds its p32 in)"""
    p64 = sigmoid64(logits)
    if p32 is None:
        p32 = p64.astype(np.float32)
    p32 = np.asarray(p32, dtype=np.float32)
    return {"p64": p64, "p32": p32, "half": to_half(p32), "picture": picture(p32, image, lut) if image is not None else None}
