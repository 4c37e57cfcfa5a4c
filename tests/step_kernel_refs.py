"""Inputs, float64 references and DERIVED error bounds for the reductions of the step's non-convolution kernels, shared by
tests/test_launch_regimes_cpu.py (is every bound tight enough to see one dropped row?) and tests/test_gpu_step_kernels.py (does the
kernel stay inside it?).  Nothing here touches a GPU.

Bounds are first-order rounding bounds, per output element: (L + k) u sum|terms| + u |result| (tests/launch_regimes.py: L = chain
length of the launch regime, k = roundings inside one term, u = 2^-24), the terms evaluated in float64 from the float32 inputs;
quantities computed from reduced values carry the reduced values' bounds through their expression.  None of them was fitted to what
a kernel returned.

`keep` (a bool row mask or None) evaluates a reference over a subset of the rows: the sensitivity test drops the last row and the
rows of the last workgroup and asks whether that moves a result by more than ten times its bound.
"""
import torch
import torch.nn.functional as F

from tests import launch_regimes as LR

U = LR.U
EPS, MOMENTUM = 1e-5, 0.1


def rnd(shape, seed, lo=-1.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g) * (hi - lo) + lo


def ratio(got, ref, bound):
    """worst error / bound over the elements; an element with bound 0 must be exact (0 / 0 counts as 0)"""
    err = (got.detach().double().cpu() - ref.double()).abs()
    bound = bound.double() if torch.is_tensor(bound) else torch.full_like(err, float(bound))
    r = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
    return float(r.max()) if r.numel() else 0.0


def rel_to_max(bound, ref):
    """the bound in the project's old unit (relative to the tensor's max): must stay below 1e-4 or the inputs are badly conditioned"""
    return float(bound.max() / ref.abs().max().clamp_min(1e-300))


def last_row_mask(M):
    k = torch.ones(M, dtype=torch.bool)
    k[M - 1] = False
    return k


def last_block_mask(M, rows_per_block, nblk):
    """rows of workgroup nblk-1 under the grid-stride mapping m = (b + k nblk) R + r shared by the reductions"""
    m = torch.arange(M)
    return (m // rows_per_block) % nblk != nblk - 1


# ---- BatchNorm ---------------------------------------------------------------------------------------------------------------------
def bn_inputs(shape, seed=400):
    """z [M][C] float32: per-channel offsets, rows alternating +-2.5; channel 1 sits 1000 standard deviations from zero (0.1 +- 1e-4: cancellation in a
    one-pass variance), channel 2 is constant (variance exactly 0, every Welford update exact)"""
    N, H, W, C = shape
    M = N * H * W
    zc = rnd((M, C), seed)
    # (+-2.5 alternating by row, more than the noise spans: with M = 2 or 3 two samples could otherwise sit so close that their variance is all cancellation)
    zv = zc * 2 + ((torch.arange(M) % 2) * 5.0 - 2.5)[:, None]
    z = zv + rnd((1, C), seed + 1) * 3
    z[:, 1] = 0.1 + rnd((M,), seed + 2) * (1e-4 * 3 ** 0.5)
    z[:, 2] = 0.7
    # dy: a per-channel mean and a part that follows z, like a real gradient: sums of pure noise over 24 600 rows are all cancellation,
    # and their bound (on sum|terms|) would exceed 1e-4 of the largest sum
    dy = rnd((M, C), seed + 8) + rnd((1, C), seed + 12) * 0.5 + zv * 0.15
    return {"z": z, "gamma": rnd((C,), seed + 3, 0.5, 1.5), "beta": rnd((C,), seed + 4), "rm": rnd((C,), seed + 5),
            "rv": rnd((C,), seed + 6, 0.5, 2.0), "res": rnd((M, C), seed + 7), "dy": dy, "ro": rnd((M, C), seed + 9),
            "dgamma0": rnd((C,), seed + 10), "dbeta0": rnd((C,), seed + 11)}


def bn_stats_ref(inp, keep=None):
    """-> (ref, bound) dicts over mean, var (biased), invstd, scale, shift, running_mean, running_var.
    mean: a Welford update is mean += (x - mean) / n: six roundings per term (k = 6), each step's error enters the final mean with
    weight <= 1, so the summation bound holds with terms x / M.  var: West's updating M2 has relative error <= n u kappa with
    kappa = sqrt(1 + mean^2 / var) (Chan, Golub & LeVeque 1983, section 3) = (L + k) u sigma rms(x) in absolute terms, k = 8;
    a constant channel gets the bound 0 (every update is exact)."""
    z = inp["z"].double()
    if keep is not None:
        z = z[keep]
    M, C = z.shape
    L = LR.bn_chain(inp["z"].shape[0], C)
    g, b, rm, rv = (inp[k].double() for k in ("gamma", "beta", "rm", "rv"))
    mean = z.mean(0)
    var = ((z - mean) ** 2).mean(0)
    bm = (L + 6) * U * z.abs().mean(0) + U * mean.abs()
    bv = (L + 8) * U * var.sqrt() * (z ** 2).mean(0).sqrt() + U * var
    f = (var + EPS) ** -0.5
    bf = 0.5 * f ** 3 * (bv + U * (var + EPS)) + 4 * U * f
    sc = g * f
    bsc = g.abs() * bf + U * sc.abs()
    sh = b - mean * sc
    bsh = sc.abs() * bm + mean.abs() * bsc + 2 * U * (b.abs() + (mean * sc).abs())
    unb = var * M / (M - 1) if M > 1 else var
    bunb = bv * (M / (M - 1) if M > 1 else 1.0) + 2 * U * unb
    rm2 = (1 - MOMENTUM) * rm + MOMENTUM * mean
    brm = MOMENTUM * bm + 3 * U * (((1 - MOMENTUM) * rm).abs() + (MOMENTUM * mean).abs())
    rv2 = (1 - MOMENTUM) * rv + MOMENTUM * unb
    brv = MOMENTUM * bunb + 3 * U * (((1 - MOMENTUM) * rv).abs() + (MOMENTUM * unb).abs())
    ref = {"mean": mean, "var": var, "invstd": f, "scale": sc, "shift": sh, "running_mean": rm2, "running_var": rv2}
    bound = {"mean": bm, "var": bv, "invstd": bf, "scale": bsc, "shift": bsh, "running_mean": brm, "running_var": brv}
    return ref, bound


def bn_saved(inp):
    """float32 save_mean / save_invstd handed to bn_bwd: the float64 statistics rounded once (not a kernel's output)"""
    ref, _ = bn_stats_ref(inp)
    return ref["mean"].float(), ref["invstd"].float()


def bn_bwd_sums_ref(inp, relu_out, keep=None):
    """-> (ref, bound) over dbeta = sum g, dgamma = sum g xhat with g = dy [ro > 0], xhat = (z - mean) invstd from the float32
    statistics the kernel is given.  k = 0 for dbeta; k = 3 for dgamma (subtract, scale, product)."""
    mean, invstd = bn_saved(inp)
    z, dy = inp["z"].double(), inp["dy"].double()
    g = dy * (inp["ro"] > 0).double() if relu_out else dy
    xh = (z - mean.double()) * invstd.double()
    t2 = g * xh
    if keep is not None:
        g, t2 = g[keep], t2[keep]
    L = LR.bn_chain(*inp["z"].shape)
    s1, s2 = g.sum(0), t2.sum(0)
    ref = {"dbeta": s1, "dgamma": s2}
    bound = {"dbeta": LR.sum_bound(L, 0, g.abs().sum(0), s1), "dgamma": LR.sum_bound(L, 3, t2.abs().sum(0), s2)}
    return ref, bound


def bn_bwd_dz_ref(inp, relu_out):
    """dz = gamma invstd (g - c1 - xhat c2), c = sums / M, with the sums' bounds carried through (c = s * (1 / M): two more roundings)
    and five roundings in the expression itself; -> (dz, bound, g)"""
    mean, invstd = bn_saved(inp)
    sums, bs = bn_bwd_sums_ref(inp, relu_out)
    z, dy = inp["z"].double(), inp["dy"].double()
    M = z.shape[0]
    g = dy * (inp["ro"] > 0).double() if relu_out else dy
    xh = (z - mean.double()) * invstd.double()
    c1, c2 = sums["dbeta"] / M, sums["dgamma"] / M
    b1, b2 = (bs["dbeta"] + 2 * U * sums["dbeta"].abs()) / M, (bs["dgamma"] + 2 * U * sums["dgamma"].abs()) / M
    a = (inp["gamma"].double() * invstd.double())
    dz = a * (g - c1 - xh * c2)
    bound = a.abs() * (b1 + xh.abs() * b2 + 5 * U * (g.abs() + c1.abs() + (xh * c2).abs())) + 2 * U * dz.abs()
    return dz, bound, g


def bn_apply_ref(inp, scale, shift, residual, relu):
    """y = [relu](z scale + shift [+ res]) from float32 coefficients: three roundings on the sum of the magnitudes (relu is monotone)"""
    z = inp["z"].double()
    t = z * scale.double()
    y = t + shift.double()
    mag = t.abs() + shift.double().abs()
    if residual:
        y = y + inp["res"].double()
        mag = mag + inp["res"].double().abs()
    return (y.clamp_min(0) if relu else y), 3 * U * mag


# ---- column sums -------------------------------------------------------------------------------------------------------------------
def colsum_inputs(M, C, seed=430):
    """x = noise + a per-channel mean of magnitude 0.5 .. 1.5 (either sign): a bias gradient, not a sum of pure noise"""
    off = rnd((1, C), seed + 2, 0.5, 1.5) * torch.where(rnd((1, C), seed + 3) < 0, -1.0, 1.0)
    return {"x": rnd((M, C), seed) + off, "out0": rnd((C,), seed + 1)}


def colsum_ref(inp, keep=None):
    x = inp["x"].double()
    L = LR.colsum_chain(*inp["x"].shape)
    if keep is not None:
        x = x[keep]
    s = x.sum(0)
    return {"sum": s}, {"sum": LR.sum_bound(L, 0, x.abs().sum(0), s)}


# ---- heads -------------------------------------------------------------------------------------------------------------------------
def head_inputs(shape, seed=450):
    """x, dz NCHW float32.  x = noise + 0.5 (an activation with a mean).  dz: a dense background at 2^-10 of full amplitude plus every
    4099th pixel and the LAST pixel at 0.5 .. 1 -- gradients of a loss are like that, and a million-term float32 sum can only show one
    dropped pixel when that pixel carries a visible share of sum|terms|"""
    N, h, w, Cin = shape
    x = rnd((N, Cin, h, w), seed) + 0.5
    dz = rnd((N, 2, h, w), seed + 1) * 2.0 ** -10
    big = rnd((N, 2, h, w), seed + 2, 0.5, 1.0)
    flat, bflat = dz.permute(0, 2, 3, 1).reshape(-1, 2), big.permute(0, 2, 3, 1).reshape(-1, 2)
    idx = torch.arange(flat.shape[0])
    sel = (idx % 4099 == 0) | (idx == flat.shape[0] - 1)
    flat[sel] = bflat[sel]
    dz = flat.reshape(N, h, w, 2).permute(0, 3, 1, 2).contiguous()
    return {"x": x, "dz": dz, "w": rnd((2, Cin, 3, 3), seed + 3, -0.2, 0.2), "b": rnd((2,), seed + 4),
            "dw0": rnd((2, Cin, 3, 3), seed + 5), "db0": rnd((2,), seed + 6)}


def _wgrad64(x, dz):
    xp = F.pad(x, (1, 1, 1, 1), mode="reflect")
    H, W = x.shape[2:]
    return torch.stack([torch.stack([torch.einsum("nchw,nohw->oc", xp[:, :, ky:ky + H, kx:kx + W], dz) for kx in range(3)], -1)
                        for ky in range(3)], -2)


def head_wgrad_ref(inp, keep=None):
    """dw [2][Cin][3][3], db [2]; `keep` masks INPUT pixels (the kernel walks input pixels and scatters, head.hip:365-370): a dropped
    pixel loses its x in every tap and its dz in the bias sum.  k = 1 (one fused multiply-add per term)."""
    x, dz = inp["x"].double(), inp["dz"].double()
    N, Cin, h, w = x.shape
    dzb = dz
    if keep is not None:
        k = keep.reshape(N, 1, h, w).double()
        x, dzb = x * k, dz * k
    L = LR.head_wgrad_chain(N, h, w, Cin)
    dw, db = _wgrad64(x, dz), dzb.sum((0, 2, 3))
    return {"dw": dw, "db": db}, {"dw": LR.sum_bound(L, 1, _wgrad64(x.abs(), dz.abs()), dw),
                                  "db": LR.sum_bound(L, 0, dzb.abs().sum((0, 2, 3)), db)}


def head_fwd_ref(inp, sigmoid):
    """low NCHW; k = 1 per product, then the bias add; sigmoid: s(1-s) (dy + 4u) + 2u s (exp, add, divide)"""
    x, w, b = inp["x"].double(), inp["w"].double(), inp["b"].double()
    Cin = x.shape[1]
    y = F.conv2d(F.pad(x, (1, 1, 1, 1), mode="reflect"), w, b)
    mag = F.conv2d(F.pad(x.abs(), (1, 1, 1, 1), mode="reflect"), w.abs(), b.abs())
    by = LR.sum_bound(LR.head_chain(Cin), 1, mag, y)
    if not sigmoid:
        return y, by
    s = torch.sigmoid(y)
    return s, s * (1 - s) * (by + 4 * U) + 2 * U * s


def head_dgrad_base(inp):
    """-> (dx, sum|terms|) of the plain data gradient in float64: the transpose is linear with 0/1 structure, so |dz| and |w| through the
    same transpose give the sum of the terms' magnitudes"""
    x, w, dz = inp["x"].double(), inp["w"].double(), inp["dz"].double()

    def bwd(ww, gg):
        xx = x.clone().requires_grad_(True)
        F.conv2d(F.pad(xx, (1, 1, 1, 1), mode="reflect"), ww).backward(gg)
        return xx.grad
    return bwd(w, dz), bwd(w.abs(), dz.abs())


def head_dgrad_ref(inp, elu, base=None):
    """dx NCHW = conv^T(dz) with the reflection halo folded back [* elu'(x)]: 18 multiply-adds per element (L = 18), up to three
    roundings in a folded dz (k = 3), two more for the ELU factor"""
    dx, mag = base if base is not None else head_dgrad_base(inp)
    k = 3
    if elu:
        x = inp["x"].double()
        fac = torch.where(x > 0, torch.ones_like(x), x + 1)
        dx, mag, k = dx * fac, mag * fac.abs(), 5
    return dx, LR.sum_bound(18, k, mag, dx)
