"""matplotlib's `plt.imsave` of a 2-D array (Normalize by the array's own minimum and maximum, then the colour map with bytes=True),
restated in numpy: held against matplotlib itself and against tests/golden/g_stretch.npz by tests/test_stretch_map_cpu.py; the device
kernel (csrc/stretch_map.hip, fp_stretch_colour) is held byte for byte against this (tests/test_gpu_stretch_map.py).

    n     = float32( double(float32(x - min)) / (double(max) - double(min)) )      0 everywhere when max == min
    index = min((int)(n * 256.0f), 255)                                            in float32

Integer and boolean arrays become float32 first (matplotlib's Normalize.process_value).  dtype=float64 follows the same formulas in
float64 throughout (the band of the float32 form, not what matplotlib computes)."""
import io

import numpy as np

DPI = (100, 100)        # what imsave hands to Pillow


def byte_table(cmap="viridis"):
    import matplotlib
    return (matplotlib.colormaps[cmap].resampled(256)(np.arange(256))[:, :3] * 255).astype(np.uint8)


def normalise(x, dtype=np.float32):
    x = np.asarray(x)
    x = x.astype(dtype)
    lo, hi = x.min(), x.max()
    if lo == hi:
        return np.zeros_like(x)
    return ((x - lo).astype(np.float64) / (np.float64(hi) - np.float64(lo))).astype(dtype)


def indices(x, dtype=np.float32):
    n = normalise(x, dtype)
    return np.minimum((n * n.dtype.type(256)).astype(np.int64), 255)


def rgb(x, table=None, dtype=np.float32):
    """[H, W] -> uint8 [H, W, 3]"""
    table = byte_table() if table is None else table
    return table[indices(x, dtype)]


def pillow_file(picture):
    """the file imsave writes for these RGB bytes: Pillow's default quality (75) with imsave's dpi"""
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(picture)).save(buf, format="JPEG", dpi=DPI)
    return buf.getvalue()


def cases(H=8, W=12):
    """name -> map: the value patterns the label generators save (medians filled with 0, boolean masks) and the edges of the arithmetic"""
    rng = np.random.default_rng(4242)
    with_zeros = (rng.random((H, W)) * 40.0).astype(np.float32) * (rng.random((H, W)) < 0.6)
    odd_range = (rng.random((H, W)) * 1000.0).astype(np.float32)
    odd_range.flat[0], odd_range.flat[1] = np.float32(-1e-3), np.float32(1000.5)     # max - min needs more than 24 bits
    mask = rng.random((H, W)) < 0.3
    out = {"float_with_zeros": with_zeros.astype(np.float32), "range_not_float32": odd_range, "constant": np.full((H, W), 2.5, np.float32),
           "all_zero": np.zeros((H, W), np.float32), "bool_mask": mask, "all_false": np.zeros((H, W), bool), "all_true": np.ones((H, W), bool)}
    assert np.float64(np.float32(np.float64(odd_range.max()) - np.float64(odd_range.min()))) != np.float64(odd_range.max()) - np.float64(odd_range.min())
    return out
