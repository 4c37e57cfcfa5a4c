"""numpy restatement of the label-map resize (csrc/label_resize.hip): OpenCV's cv2.resize on float64 data with INTER_NEAREST or INTER_AREA
(shrinking or equal), written out from its algorithm -- no cv2 is needed.  `restate(m, H, W, method)` is
cv2.resize(m.astype(float), (W, H), interpolation=method); `label_resize` adds what footprint_dataset.py:82-94 wraps around it (fliplr first,
the disparity multiplier last).  numpy never fuses a product into a sum, so `a + b * c` below is two rounded operations, as in OpenCV's
scalar loops.  Vectorised over rows: 375 x 1242 takes well under a second."""
import math

import numpy as np

DBL_EPSILON = 2.220446049250313e-16


def scales(S, D):
    """cv2::resize: inv_scale = dsize / ssize in double, scale = 1 / inv_scale"""
    inv = float(D) / S
    return 1.0 / inv


def area_table(S, D):
    """computeResizeAreaTab of one axis -> (bounds int32 [D, 2] = first entry and count, index int32 [n], weight float32 [n])"""
    scale = scales(S, D)
    bounds, index, weight = np.zeros((D, 2), np.int32), [], []
    for d in range(D):
        f1 = d * scale
        f2 = f1 + scale
        cw = min(scale, S - f1)
        s1 = math.ceil(f1)
        s2 = min(math.floor(f2), S - 1)
        s1 = min(s1, s2)
        first = len(index)
        if s1 - f1 > 1e-3:
            index.append(s1 - 1)
            weight.append(np.float32((s1 - f1) / cw))
        for s in range(s1, s2):
            index.append(s)
            weight.append(np.float32(1.0 / cw))
        if f2 - s2 > 1e-3:
            index.append(s2)
            weight.append(np.float32(min(min(f2 - s2, 1.0), cw) / cw))
        bounds[d] = (first, len(index) - first)
    return bounds, np.asarray(index, np.int32), np.asarray(weight, np.float32)


def is_fast(h, w, H, W):
    sx, sy = scales(w, W), scales(h, H)
    return abs(sx - round(sx)) < DBL_EPSILON and abs(sy - round(sy)) < DBL_EPSILON


def _area_general(m, H, W):
    h, w = m.shape
    bx, ix, ax = area_table(w, W)
    by, iy, ay = area_table(h, H)
    ax, ay = ax.astype(np.float64), ay.astype(np.float64)          # float weights widened when used
    # buf[sy][dx] = ((0.0 + S[sy][sx0] * a0) + S[sy][sx1] * a1) + ...: the same for every dy that reads row sy
    buf = np.zeros((h, W), np.float64)
    for k in range(int(bx[:, 1].max())):
        cols = np.nonzero(bx[:, 1] > k)[0]
        e = bx[cols, 0] + k
        buf[:, cols] = buf[:, cols] + m[:, ix[e]] * ax[e]
    out = np.zeros((H, W), np.float64)
    for k in range(int(by[:, 1].max())):
        rows = np.nonzero(by[:, 1] > k)[0]
        e = by[rows, 0] + k
        t = ay[e][:, None] * buf[iy[e]]
        out[rows] = t if k == 0 else out[rows] + t
    return out


def _area_fast(m, H, W):
    h, w = m.shape
    ix, iy = int(round(scales(w, W))), int(round(scales(h, H)))
    acc = None
    for ky in range(iy):                                            # the block in row-major order, starting from its first element
        for kx in range(ix):
            s = m[ky:ky + iy * H:iy, kx:kx + ix * W:ix]
            acc = s.copy() if acc is None else acc + s
    return acc * float(np.float32(1.0) / np.float32(ix * iy))


def restate(m, H, W, method):
    """cv2.resize(m.astype(float), (W, H), interpolation=INTER_NEAREST | INTER_AREA) for method 'nearest' | 'area'"""
    m = np.asarray(m).astype(np.float64)
    h, w = m.shape
    if (h, w) == (H, W):
        return m.copy()                                             # cv2's early copyTo
    if method == "nearest":
        sx = np.minimum(np.floor(np.arange(W) * scales(w, W)).astype(np.int64), w - 1)
        sy = np.minimum(np.floor(np.arange(H) * scales(h, H)).astype(np.int64), h - 1)
        return m[sy][:, sx]
    if method != "area":
        raise ValueError(method)
    if h < H or w < W:
        raise ValueError("INTER_AREA enlarging is not restated")
    return _area_fast(m, H, W) if is_fast(h, w, H, W) else _area_general(m, H, W)


def label_resize(m, H, W, method, flip=False, multiplier=1.0):
    """load_and_resize_npy without the file: .astype(float), fliplr when flipped, cv2.resize, times the multiplier; None or 'zero' = zeros"""
    if m is None or method == "zero":
        return np.zeros((H, W), np.float64)
    m = np.asarray(m).astype(np.float64)
    if flip:
        m = np.fliplr(m)
    return restate(m, H, W, method) * multiplier


def exact_area(m, H, W):
    """the exact area average in rationals: out[dy][dx] = sum of S weighted by the overlap of source cell and output cell, over the cell's area"""
    from fractions import Fraction
    h, w = m.shape

    def overlaps(S, D):
        rows = []
        for d in range(D):
            lo, hi = Fraction(d * S, D), Fraction((d + 1) * S, D)
            rows.append([(s, min(hi, s + 1) - max(lo, s)) for s in range(int(lo), min(S, math.ceil(hi)))])
        return rows

    ox, oy = overlaps(w, W), overlaps(h, H)
    area = Fraction(h * w, H * W)
    out = [[sum(Fraction(float(m[sy, sx])) * wy * wx for sy, wy in oy[dy] for sx, wx in ox[dx]) / area for dx in range(W)] for dy in range(H)]
    return out
