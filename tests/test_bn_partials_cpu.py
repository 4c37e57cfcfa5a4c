"""CPU: the arithmetic of the BatchNorm statistics that come out of the tile convolution's epilogue (csrc/conv3x3_tile_bf3.hip, round 3)
and, further down, out of the reduce launch of a split grid (csrc/conv_igemm.hip: a streaming Welford form with its own error),
restated in float32 numpy: a lane's 32 values -> two-pass (count, mean, M2) -> Chan merge with the other half-wave -> with the other
M wave -> per pixel tile; bn_stats_final_kernel's merge over the tiles (lane l takes tiles l, l + 64, ..., then a shuffle tree).  The
property checked is the one the GPU test cannot show on benign data: mean and variance stay within 2e-6 of float64 when the channel
mean is a thousand standard deviations away from zero (sum / sum-of-squares partials would lose the variance entirely there)."""
import numpy as np
import pytest

from tests.bn_partials_check import block_of_rows, check_reduce_partials, partial_tolerance, reduce_geometry

f32 = np.float32


def wf_merge(a, b):
    n = f32(a[0] + b[0])
    if n == 0:
        return a
    d = f32(b[1] - a[1])
    f = f32(b[0] / n)
    mean = f32(a[1] + d * f)
    m2 = f32(a[2] + f32(b[2] + f32(f32(d * d) * f32(a[0] * f))))
    return (n, mean, m2)


def lane_stats(v):                       # two passes over the lane's registers
    v = v.astype(f32)
    cnt = f32(len(v))
    s = f32(0)
    for x in v:
        s = f32(s + x)
    mean = f32(s / cnt) if cnt > 0 else f32(0)
    m2 = f32(0)
    for x in v:
        d = f32(x - mean)
        m2 = f32(m2 + d * d)
    return (cnt, mean, m2)


def tile_partial(tile):                  # tile: 128 pixels of one channel = 2 M waves x 2 half-waves x 32 registers' worth... 4 x 32 values
    lanes = [lane_stats(tile[i * 32:(i + 1) * 32]) for i in range(4)]
    w0 = wf_merge(lanes[0], lanes[1])    # half-waves of M wave 0
    w1 = wf_merge(lanes[2], lanes[3])
    return wf_merge(w0, w1)              # M waves in order


def final_merge(parts):                  # bn_stats_final_kernel: lane l merges partials l, l + 64, ...; then offsets 32, 16, ... 1
    lanes = []
    for l in range(64):
        w = (f32(0), f32(0), f32(0))
        for b in range(l, len(parts), 64):
            w = wf_merge(w, parts[b])
        lanes.append(w)
    o = 32
    while o > 0:
        lanes = [wf_merge(lanes[l], lanes[l + o]) if l + o < 64 else lanes[l] for l in range(64)]
        o >>= 1
    return lanes[0]


@pytest.mark.parametrize("mean,std,tiles", [(0.0, 1.0, 180), (3.0, 1.0, 720), (1000.0, 1.0, 180), (-250.0, 0.03, 96), (1e-3, 1e-6, 64)])
def test_tile_welford_partials_match_float64(mean, std, tiles):
    rng = np.random.default_rng(17)
    x = (rng.standard_normal(tiles * 128) * std + mean).astype(f32)
    n, m, m2 = final_merge([tile_partial(x[t * 128:(t + 1) * 128]) for t in range(tiles)])
    xd = x.astype(np.float64)
    assert n == tiles * 128
    assert abs(m - xd.mean()) <= 2e-6 * max(abs(xd.mean()), xd.std())
    assert abs(m2 / n - xd.var()) <= 2e-6 * xd.var() + 1e-30
    # what plain sums would have given in float32 (the form the kernel does NOT use): shown to fail where the mean dominates
    if abs(mean) >= 1000 * std:
        s, q = f32(0), f32(0)
        for v in x[:4096]:
            s = f32(s + v)
            q = f32(q + v * v)
        naive = q / f32(4096) - (s / f32(4096)) ** 2
        assert abs(naive - xd[:4096].var()) > 1e-2 * xd[:4096].var()


def test_empty_lanes_and_ragged_tiles_merge_cleanly():
    """a lane whose pixels all lie outside the image contributes (0, 0, 0); merging it on either side changes nothing"""
    a, z = (f32(7), f32(1.5), f32(0.25)), (f32(0), f32(0), f32(0))
    assert wf_merge(a, z) == a and wf_merge(z, a) == a and wf_merge(z, z) == z


# ---- the reduce launch of a split grid (csrc/conv_igemm.hip, splitk_reduce_stats_kernel): a different arithmetic form -----------------------
# Thread (rr, channel quad) of block b streams fp_wf_add over the rows b * R + rr, + nblk * R, ... (R = 256 / (Nout / 4) row groups, nblk =
# min(512, ceil(M / 4R)) blocks); row group 0 then merges groups 1 .. R - 1 in that order (fp_wf_merge through LDS) and writes the block's
# triple; bn_stats_final_kernel merges the blocks (final_merge above).  One channel is restated: channels do not interact.


def wf_add(a, x, n):                     # fp_wf_add: n = the new count, rn = 1 / n
    rn = f32(f32(1) / n)
    d = f32(x - a[1])
    mean = f32(a[1] + f32(d * rn))
    return (n, mean, f32(a[2] + f32(d * f32(x - mean))))


def reduce_partials(v, R, nblk, row_value=None):
    """[nblk] triples of the column v ([M] float32) in the kernel's order; row_value(m) overrides what the statistics see of row m"""
    parts = []
    for b in range(nblk):
        groups = []
        for rr in range(R):
            w, cnt = (f32(0), f32(0), f32(0)), f32(0)
            for m in range(b * R + rr, len(v), nblk * R):
                cnt = f32(cnt + f32(1))
                w = wf_add(w, v[m] if row_value is None else row_value(m), cnt)
            groups.append(w)
        w = groups[0]
        for r in range(1, R):
            w = wf_merge(w, groups[r])
        parts.append(w)
    return parts


def splitk_sum(p):                       # p: [SK][M] partial copies; four running sums, then a tail loop, then (p0 + p1) + (p2 + p3)
    SK = p.shape[0]
    acc = [np.zeros(p.shape[1], f32) for _ in range(4)]
    s = 0
    while s + 4 <= SK:
        for k in range(4):
            acc[k] = (acc[k] + p[s + k]).astype(f32)
        s += 4
    while s < SK:
        acc[0] = (acc[0] + p[s]).astype(f32)
        s += 1
    return ((acc[0] + acc[1]).astype(f32) + (acc[2] + acc[3]).astype(f32)).astype(f32)


REDUCE_CASES = [(0.0, 1.0, 1440, 512), (3.0, 1.0, 5760, 32), (0.75, 1.2, 234, 64), (1000.0, 1.0, 1440, 512), (1000.0, 1.0, 5760, 32),
                (-250.0, 0.03, 1440, 128), (1000.0, 1.0, 35, 16), (2.0, 1.0, 15, 16)]


@pytest.mark.parametrize("mean,std,M,Nout", REDUCE_CASES)
def test_reduce_welford_partials_match_float64(mean, std, M, Nout):
    """streaming Welford per thread + merges, in float32, against float64.  Measured variance errors: 5e-8 ... 8e-8 of the variance while
    |mean| <= 3 std; 2.7e-6 (M 1440, Nout 512) and 8.6e-7 (M 5760, Nout 32) at a mean of 1000 std, 6.2e-6 at 8333 std, 1.4e-6 at 1000 std
    over 35 rows (other draws of the same distributions: up to 6.1e-6, 2.4e-5 and 3.2e-5): every stored mean is off by up to 2^-24 |mean| and the merges square differences of those means, so the flat 2e-6 of
    the tile form holds only while the mean is of the order of the spread; beyond, 2e-6 + 2^-23 |mean| / std (partial_tolerance)."""
    R, nblk = reduce_geometry(M, Nout)
    rng = np.random.default_rng(23)
    x = (rng.standard_normal(M) * std + mean).astype(f32)
    parts = reduce_partials(x, R, nblk)
    blk = block_of_rows(M, R, nblk)
    assert [float(p[0]) for p in parts] == [float((blk == b).sum()) for b in range(nblk)]          # exact, empty row groups included
    n, m, m2 = final_merge(parts)
    xd = x.astype(np.float64)
    assert n == M
    assert abs(m - xd.mean()) <= 2e-6 * max(abs(xd.mean()), xd.std())
    tol = 2e-6 if abs(mean) <= 3 * std else partial_tolerance(xd.mean(), xd.std())
    err = abs(m2 / n - xd.var()) / xd.var()
    print("reduce form: mean/std %g M %d Nout %d: variance error %.3e (bound %.3e)" % (mean / std, M, Nout, err, tol))
    assert err <= tol
    # ... and the float64 checker of the GPU test accepts these partials
    check_reduce_partials(np.array(parts, dtype=np.float64).reshape(nblk, 1, 3), xd.reshape(M, 1), R)
    if abs(mean) >= 1000 * std:          # plain sums in float32 lose the variance where the mean dominates; this form does not
        s, q = f32(0), f32(0)
        for v in x:
            s = f32(s + v)
            q = f32(q + v * v)
        k = f32(len(x))
        naive = q / k - (s / k) ** 2
        assert abs(naive - xd.var()) > 1e-2 * xd.var() > 100 * abs(m2 / n - xd.var())


def test_reduce_counts_are_exact_with_empty_row_groups():
    """M < R: most row groups of the only block never see a row and merge as (0, 0, 0)"""
    R, nblk = reduce_geometry(35, 16)
    assert (R, nblk) == (64, 1)
    x = (np.arange(35) * 0.37 + 5.0).astype(f32)
    (n, m, m2), = reduce_partials(x, R, nblk)
    assert n == 35 and abs(m - x.astype(np.float64).mean()) <= 2e-6 * abs(m)
    assert abs(m2 - 35 * x.astype(np.float64).var()) <= 2e-6 * m2
    assert reduce_geometry(1440, 24) is None and reduce_geometry(1440, 6) is None and reduce_geometry(70, 40) is None and reduce_geometry(234, 64) == (16, 4)


@pytest.mark.parametrize("defect", ["none", "row missing", "neighbour's mean", "M2 about zero", "tail term dropped"])
def test_partials_checker_has_teeth(defect):
    """the float64 checker of the GPU test must reject: one row missing from one block; a block's mean taken from a neighbouring row group;
    M2 taken about zero; statistics of a split-K sum that lost its tail term"""
    M, Nout, SK = 234, 64, 5
    R, nblk = reduce_geometry(M, Nout)
    rng = np.random.default_rng(5)
    p = (rng.standard_normal((SK, M)) * 0.9 + 0.15).astype(f32)              # the output's mean (0.75) is of the order of its spread (2)
    y = splitk_sum(p)
    assert np.array_equal(y, ((p[0] + p[4]).astype(f32) + p[1]).astype(f32) + (p[2] + p[3]).astype(f32))
    seen = y
    if defect == "tail term dropped":
        q = p.copy()
        q[4] = 0
        seen = splitk_sum(q)
    parts = np.array(reduce_partials(seen, R, nblk), dtype=np.float64).reshape(nblk, 1, 3)
    if defect == "row missing":
        skip = R * nblk + 3              # a row of block 0's second sweep
        parts = np.array(reduce_partials(np.delete(y, skip), R, nblk), dtype=np.float64).reshape(nblk, 1, 3)
        assert parts[:, 0, 0].sum() == M - 1
    if defect == "neighbour's mean":
        parts[1, 0, 1] = parts[2, 0, 1]
    if defect == "M2 about zero":
        blk = block_of_rows(M, R, nblk)
        for b in range(nblk):
            parts[b, 0, 2] = (y[blk == b].astype(np.float64) ** 2).sum()
    if defect == "none":
        check_reduce_partials(parts, y.reshape(M, 1), R)
        return
    with pytest.raises(AssertionError):
        check_reduce_partials(parts, y.reshape(M, 1), R)
