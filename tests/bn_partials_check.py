"""Float64 checker for the BatchNorm partials a split grid's reduce launch writes (csrc/conv_igemm.hip, splitk_reduce_stats_kernel):
block b of nblk owns the rows m with (m // R) % nblk == b, R = 256 / (Nout / 4) row groups of a block, and writes one (count, mean, M2)
triple per channel.  Plain numpy, no GPU: tests/test_gpu_igemm_epilogue.py holds the device's partials against it, and
tests/test_bn_partials_cpu.py shows that it rejects the defects it is there for."""
import numpy as np


def reduce_geometry(M, Nout):
    """(R, nblk) of the reduce launch for an [M][Nout] output, or None where the launch does not emit (the block rule of fp_splitk_finish)"""
    if Nout % 4 or Nout // 4 > 256 or 256 % (Nout // 4):
        return None
    R = 256 // (Nout // 4)
    return R, min(512, -(-M // (R * 4)))


def block_of_rows(M, R, nblk):
    return (np.arange(M) // R) % nblk


def partial_tolerance(mean, std):
    """relative bound on a variance / M2 held in fp32 Welford form: 2e-6 while the mean is of the order of the spread, plus 2^-23 |mean| / std
    where the mean dominates (a partial carries its mean in fp32, off by up to 2^-24 |mean|, and the merge's d^2 term carries twice that
    relative to d ~ std)"""
    return 2e-6 + 2.0 ** -23 * abs(mean) / max(std, 1e-300)


def check_reduce_partials(part, y, R):
    """part: [nblk][C][3] as written by the device; y: [M][C], the tensor the same launch stored.  Raises AssertionError unless every
    block's count is exactly the number of its rows, the counts add up to M per channel, every block's (mean, M2) is that of its own
    rows of y in float64, and the totals merged in float64 are those of y.  Returns the largest relative (mean, M2) error seen."""
    part = np.asarray(part, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    nblk, C, three = part.shape
    M = y.shape[0]
    assert three == 3 and y.shape[1] == C
    blk = block_of_rows(M, R, nblk)
    want_cnt = np.bincount(blk, minlength=nblk).astype(np.float64)
    assert np.array_equal(part[:, :, 0], np.repeat(want_cnt[:, None], C, 1)), "block counts differ from the rows each block owns"
    assert np.array_equal(part[:, :, 0].sum(0), np.full(C, float(M))), "counts do not add up to M"
    worst_mean = worst_m2 = 0.0
    for b in range(nblk):
        rows = y[blk == b]
        if len(rows) == 0:
            assert not part[b, :, 1:].any(), "an empty block must write (0, 0, 0)"
            continue
        mean = rows.mean(0)
        m2 = ((rows - mean) ** 2).sum(0)
        std = np.sqrt(m2 / len(rows))
        scale = np.maximum(np.abs(mean), std)
        e_mean = np.abs(part[b, :, 1] - mean) / np.maximum(scale, 1e-300)
        tol = 2e-6 + 2.0 ** -23 * np.abs(mean) / np.maximum(std, 1e-300)
        e_m2 = np.abs(part[b, :, 2] - m2) / np.maximum(m2, 1e-300)
        ok_m2 = (e_m2 <= tol) | (len(rows) == 1)
        assert (e_mean <= 2e-6).all(), "block %d: mean off by %.3e of max(|mean|, std)" % (b, e_mean.max())
        assert ok_m2.all(), "block %d: M2 off by %.3e (bound %.3e)" % (b, e_m2[~ok_m2].max(), tol[~ok_m2].min())
        if len(rows) == 1:
            assert (np.abs(part[b, :, 2]) <= 1e-12 * np.maximum(mean * mean, 1e-300)).all(), "block %d: M2 of a single row must be 0" % b
        worst_mean = max(worst_mean, float(e_mean.max()))
        worst_m2 = max(worst_m2, float(e_m2.max()) if len(rows) > 1 else 0.0)
    # totals: Chan's merge of the partials in float64 against the tensor itself
    n, mean, m2 = np.zeros(C), np.zeros(C), np.zeros(C)
    for b in range(nblk):
        nb = part[b, :, 0]
        if not nb.any():
            continue
        tot = n + nb
        d = part[b, :, 1] - mean
        m2 = m2 + part[b, :, 2] + d * d * n * nb / tot
        mean = mean + d * nb / tot
        n = tot
    ymean, yvar = y.mean(0), y.var(0)
    ystd = np.sqrt(yvar)
    e_mean = np.abs(mean - ymean) / np.maximum(np.maximum(np.abs(ymean), ystd), 1e-300)
    e_var = np.abs(m2 / M - yvar) / np.maximum(yvar, 1e-300)
    tol = 2e-6 + 2.0 ** -23 * np.abs(ymean) / np.maximum(ystd, 1e-300)
    assert (e_mean <= 2e-6).all(), "merged mean off by %.3e" % e_mean.max()
    assert (e_var <= tol).all() or M == 1, "merged variance off by %.3e" % e_var.max()
    return max(worst_mean, float(e_mean.max())), max(worst_m2, float(e_var.max()))
