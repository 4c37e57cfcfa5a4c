"""NumPy restatement of the two reader operations that csrc/resample_u8.hip and csrc/reader.hip run on the device (no Pillow, scipy or skimage needed):

* Pillow's 8-bit `Image.resize` (libImaging/Resample.c: precompute_coeffs, normalize_coeffs_8bpc, ImagingResampleHorizontal_8bpc /
  Vertical_8bpc): per axis a table of window bounds and 22-bit fixed-point taps built in double, then int32 accumulation, an arithmetic
  shift and a clip; horizontal pass into a uint8 intermediate first, a pass whose sizes agree skipped.
* the reference's `filter_depth_mask` (footprints/datasets/footprint_dataset.py:96-105): 8-connected components of the ones, those
  with fewer than W * H / 100 pixels kept -- as a plain flood fill.

tests/test_reader_cpu.py pins both to the installed Pillow and to scipy.ndimage.label + the reference's loop.
"""
import math

import numpy as np

LANCZOS, BILINEAR, BICUBIC, BOX = 1, 2, 3, 4                  # Pillow's Image.Resampling numbers
FILTERS = {"lanczos": LANCZOS, "bilinear": BILINEAR, "bicubic": BICUBIC, "box": BOX}
PRECISION_BITS = 32 - 8 - 2


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x               # math.sin is the C library's sin, which is what Pillow calls


def _lanczos(x):
    return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0


def _bilinear(x):
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


def _bicubic(x):
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _box(x):
    return 1.0 if -0.5 < x <= 0.5 else 0.0


_FILTER = {LANCZOS: (_lanczos, 3.0), BILINEAR: (_bilinear, 1.0), BICUBIC: (_bicubic, 2.0), BOX: (_box, 0.5)}


def ksize(in_size, out_size, filt=LANCZOS):
    return 2 * int(math.ceil(_FILTER[filt][1] * max(in_size / out_size, 1.0))) + 1


def coeffs(in_size, out_size, filt=LANCZOS):
    """-> bounds int32 [out, 2] (first source index, tap count), kk int32 [out, ksize]"""
    fn, support = _FILTER[filt]
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = support * fs
    ks = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    bounds, kk = np.zeros((out_size, 2), np.int32), np.zeros((out_size, ks), np.int32)
    for xx in range(out_size):
        center = 0.0 + (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)                  # int(): truncation, like the C cast
        xmax = min(int(center + support + 0.5), in_size) - xmin
        k = [fn((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for w in k:                                                 # the running sum, in the order Pillow adds
            ww += w
        for x in range(xmax):
            v = k[x] / ww if ww != 0.0 else k[x]
            kk[xx, x] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
        bounds[xx] = (xmin, xmax)
    return bounds, kk


def apply_axis_raw(a, bounds, kk):
    """the pass along axis 0 of uint8 `a` before the shift and the clip -> int64 [out, ...] (int32 suffices; int64 shows it)"""
    out = np.empty((bounds.shape[0],) + a.shape[1:], np.int64)
    src = a.astype(np.int64)
    for xx, (xmin, n) in enumerate(bounds):
        out[xx] = (1 << (PRECISION_BITS - 1)) + np.tensordot(kk[xx, :n].astype(np.int64), src[xmin:xmin + n], axes=(0, 0))
    assert np.abs(out).max() < 2 ** 31
    return out


def apply_axis(a, bounds, kk):
    return np.clip(apply_axis_raw(a, bounds, kk) >> PRECISION_BITS, 0, 255).astype(np.uint8)


def resize(img, H, W, filt=LANCZOS):
    """PIL.Image.fromarray(img).resize((W, H), filt) for uint8 [h, w] or [h, w, C]"""
    img = np.ascontiguousarray(img)
    assert img.dtype == np.uint8
    h, w = img.shape[:2]
    if w != W:
        img = np.swapaxes(apply_axis(np.swapaxes(img, 0, 1), *coeffs(w, W, filt)), 0, 1)
    if h != H:
        img = apply_axis(img, *coeffs(h, H, filt))
    return np.ascontiguousarray(img)


def pre_clip_range(img, H, W, filt=LANCZOS):
    """(min, max) over both passes of the shifted values before the clip to [0, 255]"""
    h, w = img.shape[:2]
    lo, hi = 0, 255
    if w != W:
        raw = apply_axis_raw(np.swapaxes(img, 0, 1), *coeffs(w, W, filt)) >> PRECISION_BITS
        lo, hi = min(lo, int(raw.min())), max(hi, int(raw.max()))
        img = np.swapaxes(np.clip(raw, 0, 255).astype(np.uint8), 0, 1)
    if h != H:
        raw = apply_axis_raw(img, *coeffs(h, H, filt)) >> PRECISION_BITS
        lo, hi = min(lo, int(raw.min())), max(hi, int(raw.max()))
    return lo, hi


def half_image(h, w, c=3):
    """0 / 255 quadrants: a hard edge in both directions, where LANCZOS overshoots below 0 and above 255"""
    img = np.zeros((h, w, c), np.uint8)
    img[: h // 2, w // 2:] = 255
    img[h // 2:, : w // 2] = 255
    return img


def components(mask):
    """8-connected components of mask == 1 by flood fill -> int32 labels (0 = background, 1.. in raster order of the first pixel)"""
    H, W = mask.shape
    lab = np.zeros((H, W), np.int32)
    fg = mask == 1
    n = 0
    for y0 in range(H):
        for x0 in range(W):
            if not fg[y0, x0] or lab[y0, x0]:
                continue
            n += 1
            lab[y0, x0] = n
            stack = [(y0, x0)]
            while stack:
                y, x = stack.pop()
                for yy in range(max(y - 1, 0), min(y + 2, H)):
                    for xx in range(max(x - 1, 0), min(x + 2, W)):
                        if fg[yy, xx] and not lab[yy, xx]:
                            lab[yy, xx] = n
                            stack.append((yy, xx))
    return lab


def filter_depth_mask(mask):
    """footprint_dataset.py:96-105 for one [H, W] mask of zeros and ones -> same dtype"""
    H, W = mask.shape
    lab = components(mask)
    sizes = np.bincount(lab.reshape(-1))
    keep = sizes < W * H / 100
    keep[0] = False
    return keep[lab].astype(mask.dtype)


# ---- the depth-mask cases of the GPU tests (tile = the labelling kernel's 32 x 8 tile) ----------------------------------------------------
TILE_W, TILE_H = 32, 8


def mask_cases(H, W):
    """name -> [H, W] float64 mask; built for 20 x 30 (limit 6.0) and 24 x 36 (limit 8.64)"""
    z = lambda: np.zeros((H, W))
    out = {"empty": z(), "full": np.ones((H, W))}
    cb = z()
    cb[0::2, 0::2] = 1
    cb[1::2, 1::2] = 1
    out["checkerboard"] = cb
    d = z()                                  # two 2-pixel blobs that touch only diagonally: one component of 4
    d[2, 2:4] = 1
    d[3, 4:6] = 1
    d[10, 10] = 1                            # and an anti-diagonal touch
    d[11, 9] = 1
    out["diagonal"] = d
    if W > TILE_W and H > TILE_H:
        c = z()                              # the same, placed across the corner shared by four tiles: (7, 31) - (8, 32), (7, 32) - (8, 31)
        c[TILE_H - 1, TILE_W - 3:TILE_W] = 1
        c[TILE_H, TILE_W:TILE_W + 3] = 1
        out["diagonal_tile_corner"] = c
        c2 = z()
        c2[TILE_H - 1, TILE_W:TILE_W + 3] = 1
        c2[TILE_H, TILE_W - 3:TILE_W] = 1
        out["antidiagonal_tile_corner"] = c2
    s = z()                                  # one-pixel-wide serpentine over the whole image
    for y in range(0, H, 2):
        s[y, :] = 1
        if y + 1 < H:
            s[y + 1, W - 1 if (y // 2) % 2 == 0 else 0] = 1
    out["serpentine"] = s
    k = z()                                  # components of exactly 5, 6 and 7 pixels (limit 6.0 at 20 x 30: only the 5 stays)
    k[1, 1:6] = 1
    k[4, 1:7] = 1
    k[7, 1:8] = 1
    k[10:13, 1] = 1                          # and 5 as an L across rows
    k[12, 2:4] = 1
    out["sizes_5_6_7"] = k
    b = z()                                  # small components on every border and in every corner, one long one along the bottom
    b[0, 0] = b[0, W - 1] = b[H - 1, 0] = 1
    b[0, W // 2:W // 2 + 2] = 1
    b[H // 2, 0] = b[H // 2 + 1, 0] = 1
    b[H // 2, W - 1] = 1
    b[H - 1, 4:W] = 1
    out["borders"] = b
    return out
