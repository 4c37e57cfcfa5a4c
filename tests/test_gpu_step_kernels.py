"""GPU: the step's non-convolution kernels (BatchNorm, max-pool, column sums, up2cat backward, the 2-channel heads, Adam, the eval
fold and the layout helpers) in the launch regimes the training step runs them in -- capped grids, grid-stride loops that go round
more than once with a ragged last pass, row rings that wrap, threads without rows -- against torch CPU float64 of the same operation.

Shapes come from tests/test_launch_regimes_cpu.py (CASES; that file proves they reach every regime of the workload); references and the
derived per-element bounds from tests/step_kernel_refs.py.  Every output is a slice of a poisoned buffer with guard bands on both sides.
Where a kernel's arithmetic leaves no freedom the result must be bit-exact.  Each check prints `RATIO <case> <error / bound>` before
it asserts (profiles/step_kernel_edges_notes.md lists them as measured on the MI355X).
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import launch_regimes as LR
from tests import step_kernel_refs as SR
from tests.test_launch_regimes_cpu import BN_BIG, BN_SMALL, CASES, HEAD_BIG, HEAD_R16, HEAD_SMALL

pytestmark = pytest.mark.gpu

U = LR.U
GUARD = 64
POISON_I32 = 0x7FC0DEAD          # a quiet NaN: an element nobody wrote fails every comparison
POISON_U8 = 0xA5


def _ops():
    from footprints_amd import ops
    return ops


class Guarded:
    """an output tensor inside a larger poisoned buffer; `init` = the old contents for accumulating launches"""

    def __init__(self, shape, dtype=torch.float32, init=None):
        n = int(np.prod(shape))
        self.buf = torch.empty(n + 2 * GUARD, dtype=dtype, device="cuda")
        self._raw().fill_(POISON_U8 if dtype == torch.uint8 else POISON_I32)
        self.t = self.buf[GUARD:GUARD + n].view(shape)
        if init is not None:
            self.t.copy_(init)

    def _raw(self):
        return self.buf if self.buf.dtype == torch.uint8 else self.buf.view(torch.int32)

    def intact(self):
        raw, p = self._raw(), (POISON_U8 if self.buf.dtype == torch.uint8 else POISON_I32)
        return bool((raw[:GUARD] == p).all()) and bool((raw[-GUARD:] == p).all())


def guards_ok(*gs):
    torch.cuda.synchronize()
    for i, g in enumerate(gs):
        assert g.intact(), "guard band of output %d was written" % i


def within(case, got, ref, bound):
    r = SR.ratio(got, ref, bound)
    print("RATIO %s %.4f" % (case, r))
    assert r <= 1.0, "%s: error / bound = %.3f" % (case, r)


def exact(case, got, ref):
    print("RATIO %s exact" % case)
    assert torch.equal(got.cpu(), ref.cpu()), "%s: not bit-exact" % case


def dev(t):
    return t.detach().contiguous().cuda()


# ----------------------------------------------------------------------------------------------------------------------------------
# BatchNorm
# ----------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def bn_in(shape):
    return SR.bn_inputs(shape)


@functools.lru_cache(maxsize=2)
def bn_dz(shape, relu_out):
    return SR.bn_bwd_dz_ref(bn_in(shape), relu_out)


@pytest.mark.parametrize("shape", CASES["bn"])
def test_bn_train_stats_and_eval_coeffs(shape):
    ops = _ops()
    inp = bn_in(shape)
    M, C = inp["z"].shape
    ref, bound = SR.bn_stats_ref(inp)
    rm, rv = Guarded((C,), init=inp["rm"]), Guarded((C,), init=inp["rv"])
    outs = {k: Guarded((C,)) for k in ("mean", "invstd", "scale", "shift")}
    nbt = torch.zeros((), dtype=torch.int64, device="cuda")
    ops.bn_train_stats(dev(inp["z"]), dev(inp["gamma"]), dev(inp["beta"]), rm.t, rv.t, nbt, outs["mean"].t, outs["invstd"].t, outs["scale"].t,
                       outs["shift"].t)
    guards_ok(rm, rv, *outs.values())
    assert int(nbt) == 1
    for k, g in list(outs.items()) + [("running_mean", rm), ("running_var", rv)]:
        within("bn_train_stats %s %s" % (shape, k), g.t, ref[k], bound[k])
    # eval coefficients: scale = gamma / sqrt(rv + eps) (add, sqrt, divide), shift = beta - rm scale
    g64, b64, rm64, rv64 = (inp[k].double() for k in ("gamma", "beta", "rm", "rv"))
    sc = g64 / (rv64 + SR.EPS).sqrt()
    bsc = 4 * U * sc.abs()
    sh = b64 - rm64 * sc
    bsh = rm64.abs() * bsc + 2 * U * (b64.abs() + (rm64 * sc).abs())
    s, t = Guarded((C,)), Guarded((C,))
    ops.bn_eval_coeffs(dev(inp["gamma"]), dev(inp["beta"]), dev(inp["rm"]), dev(inp["rv"]), s.t, t.t)
    guards_ok(s, t)
    within("bn_eval_coeffs %s scale" % (shape,), s.t, sc, bsc)
    within("bn_eval_coeffs %s shift" % (shape,), t.t, sh, bsh)


APPLY_VARIANTS = [(shape, res, relu) for shape in CASES["bn"] for res in (True, False) for relu in (True, False)
                  if shape in (BN_BIG, BN_SMALL) or (res and relu)]


@pytest.mark.parametrize("shape,residual,relu", APPLY_VARIANTS)
def test_bn_apply(shape, residual, relu):
    ops = _ops()
    inp = bn_in(shape)
    M, C = inp["z"].shape
    st, _ = SR.bn_stats_ref(inp)
    scale, shift = st["scale"].float(), st["shift"].float()          # float32 coefficients of the test's own making, not a kernel's
    y, by = SR.bn_apply_ref(inp, scale, shift, residual, relu)
    out = Guarded((M, C))
    ops.bn_apply(dev(inp["z"]), dev(scale), dev(shift), out.t, residual=dev(inp["res"]) if residual else None, relu=relu)
    guards_ok(out)
    within("bn_apply %s residual=%d relu=%d" % (shape, residual, relu), out.t, y, by)


BWD_VARIANTS = [(shape, ro, go) for shape in CASES["bn"] for ro in (True, False) for go in (True, False)
                if shape in (BN_BIG, BN_SMALL) or (ro and go)]


@pytest.mark.parametrize("shape,relu_out,g_out", BWD_VARIANTS)
def test_bn_bwd(shape, relu_out, g_out):
    """dz, dgamma, dbeta [, g_out]; then the same launch with accumulate=True on top of old dgamma / dbeta: the kernel adds the finished
    sums to the old values (bn_pool.hip:222-223), so old + fresh in float32 is what must come out, bit for bit"""
    ops = _ops()
    inp = bn_in(shape)
    M, C = inp["z"].shape
    mean, invstd = SR.bn_saved(inp)
    sums, bs = SR.bn_bwd_sums_ref(inp, relu_out)
    dz_ref, dz_bound, g_ref = bn_dz(shape, relu_out)
    d = {k: dev(inp[k]) for k in ("dy", "ro", "z", "gamma")}
    md, isd = dev(mean), dev(invstd)
    tag = "bn_bwd %s relu_out=%d g_out=%d" % (shape, relu_out, g_out)

    def run(accumulate):
        dz, go = Guarded((M, C)), (Guarded((M, C)) if g_out else None)
        dg = Guarded((C,), init=inp["dgamma0"] if accumulate else None)
        db = Guarded((C,), init=inp["dbeta0"] if accumulate else None)
        ops.bn_bwd(d["dy"], d["ro"] if relu_out else None, d["z"], md, isd, d["gamma"], dz.t, dg.t, db.t, g_out=go.t if g_out else None,
                   accumulate=accumulate)
        guards_ok(dz, dg, db, *([go] if g_out else []))
        return dz, go, dg, db
    dz, go, dg, db = run(False)
    within(tag + " dz", dz.t, dz_ref, dz_bound)
    within(tag + " dgamma", dg.t, sums["dgamma"], bs["dgamma"])
    within(tag + " dbeta", db.t, sums["dbeta"], bs["dbeta"])
    if g_out:
        exact(tag + " g_out", go.t, g_ref.float())
    dz2, _, dg2, db2 = run(True)
    exact(tag + " accumulate dz", dz2.t, dz.t)
    exact(tag + " accumulate dgamma", dg2.t, dev(inp["dgamma0"]) + dg.t)
    exact(tag + " accumulate dbeta", db2.t, dev(inp["dbeta0"]) + db.t)


# ----------------------------------------------------------------------------------------------------------------------------------
# max-pool 3x3 / 2 / pad 1
# ----------------------------------------------------------------------------------------------------------------------------------
def pool_input(shape, ties):
    """signed values (whole windows below zero: padding with 0 instead of -inf would win them); ties: quantised to halves"""
    N, H, W, C = shape
    x = SR.rnd((N, C, H, W), 480, -2.0, 1.0)
    return (x * 2).round() / 2 if ties else x


@pytest.mark.parametrize("ties", [False, True])
@pytest.mark.parametrize("shape", CASES["maxpool_fwd"])
def test_maxpool_fwd_bwd(shape, ties):
    ops = _ops()
    N, H, W, C = shape
    x = pool_input(shape, ties)
    y, idx = F.max_pool2d(x, 3, 2, 1, return_indices=True)
    OH, OW = y.shape[2:]
    iy, ix = idx // W, idx % W
    oy, ox = torch.arange(OH).view(1, 1, OH, 1), torch.arange(OW).view(1, 1, 1, OW)
    tap = ((iy - (oy * 2 - 1)) * 3 + (ix - (ox * 2 - 1))).to(torch.uint8)          # ATen's argmax as the kernel's tap number ky * 3 + kx
    ys, am = Guarded((N, OH, OW, C)), Guarded((N, OH, OW, C), torch.uint8)
    ops.maxpool_fwd(dev(x.permute(0, 2, 3, 1)), ys.t, am.t)
    guards_ok(ys, am)
    tag = "maxpool %s ties=%d" % (shape, ties)
    exact(tag + " values", ys.t.permute(0, 3, 1, 2), y)
    exact(tag + " argmax", am.t.permute(0, 3, 1, 2), tap)
    # backward: each input element sums at most four window gradients (L = 4, no rounding inside a term)
    g = SR.rnd(tuple(y.shape), 481)
    x64 = x.double().requires_grad_(True)
    F.max_pool2d(x64, 3, 2, 1).backward(g.double())
    dx_ref = x64.grad
    x64a = x.double().requires_grad_(True)
    F.max_pool2d(x64a, 3, 2, 1).backward(g.double().abs())
    bound = LR.sum_bound(4, 0, x64a.grad, dx_ref)
    gd = dev(g.permute(0, 2, 3, 1))
    dx = Guarded((N, H, W, C))
    ops.maxpool_bwd(gd, am.t, dx.t)
    guards_ok(dx)
    within(tag + " bwd", dx.t.permute(0, 3, 1, 2), dx_ref, bound)
    old = SR.rnd((N, H, W, C), 482)
    dxa = Guarded((N, H, W, C), init=old)
    ops.maxpool_bwd(gd, am.t, dxa.t, accumulate=True)          # the finished window sum is added to the old value (bn_pool.hip:330-333)
    guards_ok(dxa)
    exact(tag + " bwd accumulate", dxa.t, dx.t + dev(old))


# ----------------------------------------------------------------------------------------------------------------------------------
# column sums
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", CASES["colsum"])
def test_colsum(shape):
    ops = _ops()
    M, C = shape
    inp = SR.colsum_inputs(M, C)
    ref, bound = SR.colsum_ref(inp)
    xd = dev(inp["x"])
    out = Guarded((C,))
    ops.colsum(xd, out.t)
    guards_ok(out)
    within("colsum %s" % (shape,), out.t, ref["sum"], bound["sum"])
    acc = Guarded((C,), init=inp["out0"])
    ops.colsum(xd, acc.t, accumulate=True)                      # out[c] + s with s finished (loss_adam_misc.hip:186)
    guards_ok(acc)
    exact("colsum %s accumulate" % (shape,), acc.t, dev(inp["out0"]) + out.t)


# ----------------------------------------------------------------------------------------------------------------------------------
# backward of cat[nearest_x2(low), skip]
# ----------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def up2cat_in(shape):
    N, h, w, C0, C1 = shape
    return {"dxv": SR.rnd((N, 2 * h, 2 * w, C0 + C1), 500), "addend": SR.rnd((N, h, w, C0), 501), "ylow": SR.rnd((N, h, w, C0), 502, -1.5, 1.0),
            "skip0": SR.rnd((N, 2 * h, 2 * w, max(C1, 1)), 503)}


@pytest.mark.parametrize("addend,ylow,acc_skip", [(a, y, s) for a in (False, True) for y in (False, True) for s in (False, True)])
@pytest.mark.parametrize("shape", CASES["up2cat_bwd"])
def test_up2cat_bwd(shape, addend, ylow, acc_skip):
    """the kernel's float32 expression has one order -- ((a + b) + (c + d)) [+ addend] [* elu'] (loss_adam_misc.hip:206-216) -- and the skip
    half is a copy or one addition: torch float32 on the CPU in that order must agree bit for bit"""
    ops = _ops()
    N, h, w, C0, C1 = shape
    inp = up2cat_in(shape)
    v = inp["dxv"]
    lo = v[..., :C0]
    ref = (lo[:, 0::2, 0::2] + lo[:, 0::2, 1::2]) + (lo[:, 1::2, 0::2] + lo[:, 1::2, 1::2])
    if addend:
        ref = ref + inp["addend"]
    if ylow:
        s = inp["ylow"]
        ref = ref * torch.where(s > 0, torch.ones_like(s), s + 1)
    dlow = Guarded((N, h, w, C0))
    dskip = Guarded((N, 2 * h, 2 * w, C1), init=inp["skip0"] if acc_skip else None) if C1 else None
    ops.up2cat_bwd(dev(v), N, h, w, C0, C1, dlow.t, addend=dev(inp["addend"]) if addend else None, ylow=dev(inp["ylow"]) if ylow else None,
                   dskip=dskip.t if C1 else None, accumulate_skip=acc_skip)
    guards_ok(dlow, *([dskip] if C1 else []))
    tag = "up2cat_bwd %s addend=%d ylow=%d acc=%d" % (shape, addend, ylow, acc_skip)
    exact(tag + " dlow", dlow.t, ref)
    if C1:
        exact(tag + " dskip", dskip.t, (inp["skip0"] + v[..., C0:]) if acc_skip else v[..., C0:])


# ----------------------------------------------------------------------------------------------------------------------------------
# heads
# ----------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def head_in(shape):
    return SR.head_inputs(shape)


@functools.lru_cache(maxsize=1)
def head_dgrad_base(shape):
    return SR.head_dgrad_base(head_in(shape))


def to_nhwc(t):
    return dev(t.permute(0, 2, 3, 1))


@pytest.mark.parametrize("sigmoid", [False, True])
@pytest.mark.parametrize("shape", CASES["head"])
def test_head_fwd(shape, sigmoid):
    ops = _ops()
    N, h, w, Cin = shape
    inp = head_in(shape)
    ref, bound = SR.head_fwd_ref(inp, sigmoid)
    low = Guarded((N, h, w, 2))
    ops.head_fwd(to_nhwc(inp["x"]), dev(inp["w"]), dev(inp["b"]), low.t, sigmoid)
    guards_ok(low)
    within("head_fwd %s sigmoid=%d" % (shape, sigmoid), low.t.permute(0, 3, 1, 2), ref, bound)


@pytest.mark.parametrize("elu", [False, True])
@pytest.mark.parametrize("shape", CASES["head"])
def test_head_dgrad(shape, elu):
    ops = _ops()
    N, h, w, Cin = shape
    inp = head_in(shape)
    ref, bound = SR.head_dgrad_ref(inp, elu, head_dgrad_base(shape))
    dx = Guarded((N, h, w, Cin))
    ops.head_dgrad(to_nhwc(inp["dz"]), dev(inp["w"]), dx.t, elu_src=to_nhwc(inp["x"]) if elu else None)
    guards_ok(dx)
    within("head_dgrad %s elu=%d" % (shape, elu), dx.t.permute(0, 3, 1, 2), ref, bound)


@pytest.mark.parametrize("shape", CASES["head_wgrad"])
def test_head_wgrad(shape):
    """fresh, then accumulate=True on old values: the reduce kernel adds its finished sum to the old value (head.hip:589-592)"""
    ops = _ops()
    N, h, w, Cin = shape
    inp = head_in(shape)
    ref, bound = SR.head_wgrad_ref(inp)
    xd, dzd = to_nhwc(inp["x"]), to_nhwc(inp["dz"])
    dw, db = Guarded((2, Cin, 3, 3)), Guarded((2,))
    ops.head_wgrad(xd, dzd, dw.t, db.t)
    guards_ok(dw, db)
    within("head_wgrad %s dw" % (shape,), dw.t, ref["dw"], bound["dw"])
    within("head_wgrad %s db" % (shape,), db.t, ref["db"], bound["db"])
    if shape in (HEAD_SMALL[0], HEAD_BIG):
        dwa, dba = Guarded((2, Cin, 3, 3), init=inp["dw0"]), Guarded((2,), init=inp["db0"])
        ops.head_wgrad(xd, dzd, dwa.t, dba.t, accumulate=True)
        guards_ok(dwa, dba)
        exact("head_wgrad %s accumulate dw" % (shape,), dwa.t, dev(inp["dw0"]) + dw.t)
        exact("head_wgrad %s accumulate db" % (shape,), dba.t, dev(inp["db0"]) + db.t)


# ----------------------------------------------------------------------------------------------------------------------------------
# Adam
# ----------------------------------------------------------------------------------------------------------------------------------
LR_, B1, B2, AEPS, GSCALE = 1e-4, 0.9, 0.999, 1e-8, 0.125
ADAM_STEPS = (1, 2, 100000)


def adam_inputs(n):
    p0 = SR.rnd((n,), 520)
    gs = [SR.rnd((n,), 521 + i, -0.08, 0.08) for i in range(len(ADAM_STEPS))]
    if n > 200:
        for g in gs:
            g[100:200] = 0.0                       # a block of exactly-zero gradients: 0 / (0 + eps) must leave p alone
    return p0, gs


@pytest.mark.parametrize("n", [n for (n,) in CASES["adam"] if n % 4 or n < 1000])
def test_adam_against_float64(n):
    """torch.optim.Adam on float64 tensors; the project's bound: 1.3e-7 per step for |p| <= 1 (one rounding of p per step), 1e-6 of the
    largest moment on the moments"""
    ops = _ops()
    p0, gs = adam_inputs(n)
    pr = p0.double().requires_grad_(True)
    opt = torch.optim.Adam([pr], lr=LR_, betas=(B1, B2), eps=AEPS)
    p, m, v = Guarded((n,), init=p0), Guarded((n,), init=torch.zeros(n)), Guarded((n,), init=torch.zeros(n))
    for k, (step, g) in enumerate(zip(ADAM_STEPS, gs), start=1):
        pr.grad = g.double() * GSCALE
        if step > 2:
            opt.state[pr]["step"] = torch.tensor(float(step - 1))
        opt.step()
        gd = Guarded((n,), init=g)
        ops.adam_step(p.t, gd.t, m.t, v.t, LR_, B1, B2, AEPS, step, GSCALE)
        guards_ok(p, m, v, gd)
        err = (p.t.cpu().double() - pr.detach()).abs().max().item()
        print("RATIO adam n=%d step=%d p %.4f" % (n, step, err / (k * 1.3e-7)))
        assert err <= k * 1.3e-7, "adam n=%d step %d: %.3e" % (n, step, err)
        if n > 200 and k == 1:
            assert torch.equal(p.t[100:200].cpu(), p0[100:200]) and float(m.t[100:200].abs().max()) == 0.0 and float(v.t[100:200].abs().max()) == 0.0
        st = opt.state[pr]
        for name, got, ref in (("exp_avg", m.t, st["exp_avg"]), ("exp_avg_sq", v.t, st["exp_avg_sq"])):
            e = ((got.cpu().double() - ref).abs().max() / ref.abs().max().clamp_min(1e-300)).item()
            print("RATIO adam n=%d step=%d %s %.4f" % (n, step, name, e / 1e-6))
            assert e <= 1e-6, "adam n=%d step %d %s: %.3e" % (n, step, name, e)


def test_adam_hyper_is_float32_of_the_double_formulas():
    ops = _ops()
    for step in ADAM_STEPS:
        bc1, bc2 = 1.0 - B1 ** step, 1.0 - B2 ** step
        want = np.array([1.0 - B1, B2, 1.0 - B2, LR_ / bc1, 1.0 / np.sqrt(bc2), AEPS, GSCALE], dtype=np.float64).astype(np.float32)
        got = ops.adam_hyper(LR_, B1, B2, AEPS, step, GSCALE).numpy()
        assert got.dtype == np.float32 and np.array_equal(got, want), (step, got, want)


def test_adam_step_dev_matches_adam_step_and_refuses_odd_lengths():
    """the graph-replay form (scalars read from device memory) at a length whose grid-stride loop goes round twice"""
    ops = _ops()
    n = 4300004
    assert (n,) in CASES["adam"]
    p0, gs = adam_inputs(n)
    a = [Guarded((n,), init=t) for t in (p0, torch.zeros(n), torch.zeros(n))]
    b = [Guarded((n,), init=t) for t in (p0, torch.zeros(n), torch.zeros(n))]
    for step, g in zip(ADAM_STEPS, gs):
        gd = dev(g)
        ops.adam_step(a[0].t, gd, a[1].t, a[2].t, LR_, B1, B2, AEPS, step, GSCALE)
        ops.adam_step_dev(b[0].t, gd, b[1].t, b[2].t, ops.adam_hyper(LR_, B1, B2, AEPS, step, GSCALE).cuda())
        guards_ok(*a, *b)
        for name, x, y in zip(("p", "exp_avg", "exp_avg_sq"), a, b):
            exact("adam_step_dev step=%d %s" % (step, name), y.t, x.t)
    before = [t.t.clone() for t in b]
    hyper = ops.adam_hyper(LR_, B1, B2, AEPS, 3, GSCALE).cuda()
    with pytest.raises(RuntimeError):
        ops.adam_step_dev(b[0].t[:n - 1], dev(gs[0])[:n - 1], b[1].t[:n - 1], b[2].t[:n - 1], hyper)
    torch.cuda.synchronize()
    for x, y in zip(before, b):
        assert torch.equal(x, y.t), "a refused adam_step_dev touched its buffers"


# ----------------------------------------------------------------------------------------------------------------------------------
# eval fold and layout helpers: bit for bit with torch
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", CASES["scale_rows"])
def test_scale_rows(shape):
    ops = _ops()
    w, s = SR.rnd(shape, 540), SR.rnd((shape[0],), 541, 0.2, 3.0)
    out = Guarded(shape)
    ops.scale_rows(dev(w), dev(s), out.t)
    guards_ok(out)
    exact("scale_rows %s" % (shape,), out.t, w * s.view(-1, 1, 1, 1))


@pytest.mark.parametrize("shape", CASES["layout"])
def test_layouts(shape):
    ops = _ops()
    N, C, H, W = shape
    x = SR.rnd(shape, 542)
    y = Guarded((N, H, W, C))
    ops.nchw_to_nhwc(dev(x), y.t)
    guards_ok(y)
    exact("nchw_to_nhwc %s" % (shape,), y.t, x.permute(0, 2, 3, 1).contiguous())
    z = Guarded(shape)
    ops.nhwc_to_nchw(y.t, z.t)
    guards_ok(z)
    exact("nhwc_to_nchw %s" % (shape,), z.t, x)


@pytest.mark.parametrize("n", [n for (n,) in CASES["fill"]])
def test_fill(n):
    ops = _ops()
    x = Guarded((n,))
    ops.fill(x.t, 2.5)
    guards_ok(x)
    exact("fill %d" % n, x.t, torch.full((n,), 2.5))
