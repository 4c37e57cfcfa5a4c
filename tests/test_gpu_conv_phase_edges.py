"""GPU: the nearest-x2 phase kernels (csrc/conv_up2_phase.hip: forward, data gradient, fold; csrc/wgrad_up2_phase.hip: weight gradient with its
sum / un-collapse / bias-reduce launches; the collapsing packers of csrc/pack.hip) at ragged tiles, with inputs whose answer is exact.
References, inputs and the case tables: tests/conv_phase_refs.py (pinned on the CPU by tests/test_conv_phase_refs_cpu.py); that the cases reach
every launch regime of a train step: tests/test_launch_regimes_cpu.py.

Per case (operand format x geometry), every operand and every output a slice of a larger buffer whose surroundings are NaN:
  * forward, lattice inputs: the plain launch, bias, and bias + in-place addend equal the float64 reference BIT FOR BIT; with ELU the elements
    with a positive pre-activation are bit-equal and the others stay within 3e-6 of the largest; with a skip half (C1 > 0) the real two-launch
    sequence of Engine._conv_dec; the fp16-pair kernel's amax_out is max |y| exactly;
  * data gradient, lattice inputs: the WHOLE extended grid bit for bit, then up2_fold_bwd with addend and ylow bit for bit, its amax_out exact;
  * weight gradient, lattice inputs: store and accumulate bit for bit (dw a channel slice of a wider gradient, db in the split formats);
  * random-valued inputs (the ranges of tests/test_gpu_kernels.py) within the project's bounds -- 1e-4 fp32 and weight gradients, 3e-6 split
    forward and data gradient, 1e-5 bias gradient -- on the whole tensor and again on the border ring plus the partial tiles;
  * cancelling inputs: relative L2 error <= 1/4 (figures: the CPU test).
Every case prints its figures before it asserts (lines "PHASE_EDGE | ...", run with -s to keep them)."""
import os

import pytest
import torch
import torch.nn.functional as F

from tests import conv_phase_refs as PR
from tests import conv_tile_refs as TR
from tests import launch_regimes as LR
from tests.test_gpu_conv_tile_edges import _band_untouched, _banded, _nchw64, _nhwc
from tests.test_gpu_kernels import _ops

pytestmark = pytest.mark.gpu

BOUND = {"f32": 1e-4, "exact": 3e-6, "pair": 3e-6}          # tests/test_gpu_kernels.py, tests/test_gpu_hp.py: test_up2_phase_*
BOUND_WGRAD, BOUND_DB = 1e-4, 1e-5


def _id(c):
    return "%s-%dx%dx%d-%d+%s>%d" % (c[0], c[1], c[2], c[3], c[4], "%d.%d" % c[5] if isinstance(c[5], tuple) else c[5], c[6])


def _by_geometry(table):
    return sorted(table, key=lambda c: repr(c[1:]) + c[0])      # the formats of a geometry side by side: they share inputs and references


_cache = {}


def _shared(what, case, make):
    key = (what,) + tuple(case[1:])
    if key not in _cache:
        if len(_cache) > 6:
            _cache.clear()
        _cache[key] = make()
    return _cache[key]


def _dev(t):
    """(whole buffer, NHWC slice) of an NCHW tensor, or of a vector, inside NaN bands"""
    return _banded(_nhwc(t) if t.dim() == 4 else t.cuda())


def _slot(t):
    ops, _ = _ops()
    return ops.amax_f32(t, ops.new_slot())


class Weights:
    """the channel slice [0, C0) of w [Nout, Cin, 3, 3] packed for one kernel in one format, inside NaN bands; pair: through a one-job table
    (the only packer of that layout, and the engine's) with the slot it was scaled by"""

    def __init__(self, kind, fmt, w, C0):
        ops, L = _ops()
        self.w = w.contiguous().cuda()
        Nout = w.shape[0]
        n = ops.up2_packed_weight_elems(Nout, C0) if kind == "fwd" else ops.up2_packed_weight_elems(C0, Nout)
        self.slot = None
        if fmt == "f32":
            assert kind == "fwd"
            self.buf, self.wp = _banded(shape=(n,))
            ops.pack_up2_weight(self.w, self.wp, 0, C0)
        elif fmt == "exact":
            self.buf, self.wp = _banded(shape=(n * 3 // 2,))
            (ops.pack_up2_weight_bf3 if kind == "fwd" else ops.pack_up2_weight_dgrad_bf3)(self.w, self.wp, 0, C0)
        else:
            self.buf, self.wp = _banded(shape=(n,))
            self.slot = ops.new_slot()
            table = ops.build_pack_table([(L.PACK_UP2_FWD_HP if kind == "fwd" else L.PACK_UP2_DGRAD_HP, self.w, self.wp, 0, C0, self.slot)], "cuda")
            ops.pack_weights_amax(table)
            ops.pack_weights_batched(table)
            assert ops.amax_value(self.slot) == float(w.abs().max())
        torch.cuda.synchronize()
        assert _band_untouched(self.buf), "the packer wrote outside its output"


def _fwd(fmt, low, wts, y, bias=None, addend=None, act=False, amax_out=None):
    ops, L = _ops()
    a = L.ACT_ELU if act else L.ACT_NONE
    if fmt == "f32":
        ops.conv_up2_phase_fwd(low, wts.wp, bias, y, act=a, addend=addend)
    elif fmt == "exact":
        ops.conv_up2_phase_fwd_bf3(low, wts.wp, bias, y, act=a, addend=addend, amax_out=amax_out)
    else:
        ops.conv_up2_phase_fwd_hp(low, wts.wp, bias, y, _slot(low), wts.slot, amax_out=amax_out, act=a, addend=addend)
    torch.cuda.synchronize()
    return y


def _dgrad(fmt, dz, wts, ext):
    ops, _ = _ops()
    if fmt == "exact":
        ops.conv_up2_phase_dgrad_bf3(dz, wts.wp, ext)
    else:
        ops.conv_up2_phase_dgrad_hp(dz, wts.wp, ext, _slot(dz), wts.slot)
    torch.cuda.synchronize()
    return ext


def _mismatch_report(got, ref, th=LR.PH_TH, tw=LR.PH_TW, scale=2):
    """count and the first eight (n, c, y, x) with phase and low-resolution tile coordinates (scale 1: a low-resolution grid)"""
    bad = (got != ref) | torch.isnan(got)
    rows = []
    for n, c, y, x in bad.nonzero()[:8].tolist():
        ly, lx = y // scale, x // scale
        rows.append("(n %d, c %d, y %d, x %d) phase (%d, %d) tile (%d, %d) pixel (%d, %d): got %r, want %r"
                    % (n, c, y, x, y % scale, x % scale, ly // th, lx // tw, ly % th, lx % tw, float(got[n, c, y, x]), float(ref[n, c, y, x])))
    return "%d of %d elements differ:\n%s" % (int(bad.sum()), bad.numel(), "\n".join(rows))


# ---- the library plans the cases as the tables say ------------------------------------------------------------------------------------------
def test_library_plans_the_cases_as_the_tables_say():
    if any(k.startswith("FP_PWGRAD_") for k in os.environ):
        pytest.skip("the launch rules are switched: the regimes of the tables are those of the default build")
    ops, L = _ops()
    lib = L.load()
    for fmt, N, h, w, C0, ks, Nout in PR.PHASE_WGRAD:
        p = LR.phase_wgrad_plan(N, h, w, C0, Nout)
        assert p and ops.up2_phase_wgrad_supported(N, h, w, C0, Nout), (fmt, N, h, w, C0, ks, Nout)
        assert lib.fp_conv_up2_phase_wgrad_workspace(N, h, w, C0, Nout) == p["workspace"] == p["S"] * (16 * C0 * Nout + Nout) * 4


# ---- forward ------------------------------------------------------------------------------------------------------------------------------------
def _fwd_lattice(case):
    def make():
        inp = PR.inputs("fwd", case)
        C0 = case[4]
        ref_lo = PR.fwd_ref(inp["low"].double(), inp["w"][:, :C0].double())
        ref_all = PR.fwd_ref(inp["low"].double(), inp["w"].double(), TR.f64(inp["skip"])) if case[5] else None
        return inp, ref_lo, ref_all
    return _shared("fwd lattice", case, make)


@pytest.mark.parametrize("case", _by_geometry(PR.PHASE_FWD), ids=_id)
def test_fwd_lattice_plain_launch_is_exact(case):
    ops, _ = _ops()
    fmt, N, h, w, C0, C1, Nout = case
    inp, ref, _ = _fwd_lattice(case)
    lbuf, low = _dev(inp["low"])
    wts = Weights("fwd", fmt, inp["w"], C0)
    buf, y = _banded(shape=(N, 2 * h, 2 * w, Nout))
    so = ops.new_slot() if fmt != "f32" else None
    _fwd(fmt, low, wts, y, amax_out=so)
    got = _nchw64(y)
    ok = torch.equal(got, ref)
    print("PHASE_EDGE | fwd lattice | %s | %s | %s" % (_id(case), "equal" if ok else "DIFFERS", sorted(r[2:] for r in PR.case_regimes("fwd", case) if r[2] != "epi")))
    assert ok, _mismatch_report(got, ref)
    assert _band_untouched(buf), "the launch wrote outside its output"
    if so is not None:
        assert ops.amax_value(so) == float(ref.abs().max()), "amax_out is not max |y|"


def _elu_check(got, pre, what):
    """bit-equal where the pre-activation is positive, 3e-6 of the largest element elsewhere (the project's bound of the split forward)"""
    want = F.elu(pre)
    pos = pre > 0
    err = float((got - want).abs().max() / want.abs().max().clamp_min(1e-30))
    print("PHASE_EDGE | fwd lattice elu | %s | positive %s | others %.3e of max" % (what, "equal" if torch.equal(got[pos], pre[pos]) else "DIFFER", err))
    assert not bool(torch.isnan(got).any()) and torch.equal(got[pos], pre[pos]), what + ": " + _mismatch_report(torch.where(pos, got, pre), pre)
    assert err <= 3e-6, (what, err)


@pytest.mark.parametrize("case", _by_geometry(PR.PHASE_FWD), ids=_id)
def test_fwd_lattice_epilogues(case):
    """bias; bias + in-place addend; bias + ELU; bias + addend + ELU.  The addend is a lattice tensor, or for C1 > 0 what Engine._conv_dec
    leaves there: the skip half's raw partial sums from the flattened kernel (exact on lattice inputs), the phase kernel adding in place"""
    ops, L = _ops()
    fmt, N, h, w, C0, C1, Nout = case
    inp, ref_lo, ref_all = _fwd_lattice(case)
    lbuf, low = _dev(inp["low"])
    bbuf, bias = _dev(inp["bias"])
    wts = Weights("fwd", fmt, inp["w"], C0)
    b64 = inp["bias"].double().view(1, -1, 1, 1)
    H, W = 2 * h, 2 * w
    if C1:
        wsk = ops.pack_conv_weight_slice(wts.w, torch.empty(ops.packed_weight_elems(Nout, C1, 3, False, False), device="cuda"), C0, C1)
        dsk = ops.make_desc(N, H, W, H, W, C1, 0, Nout, 3, 1, 1, L.GATHER_FWD_REFLECT)
        skip = _nhwc(inp["skip"])
        pre_add = ref_all + b64
    else:
        pre_add = ref_lo + b64 + inp["prev"].double()

    def in_place():
        if not C1:
            return _banded(_nhwc(inp["prev"]))
        buf, y = _banded(shape=(N, H, W, Nout))
        ops.conv_igemm(dsk, skip, None, wsk, y)
        return buf, y
    for name in PR.FWD_EPIS[1:]:
        addend, act = "addend" in name, "act" in name
        buf, y = in_place() if addend else _banded(shape=(N, H, W, Nout))
        so = ops.new_slot() if fmt != "f32" else None
        _fwd(fmt, low, wts, y, bias=bias, addend=y if addend else None, act=act, amax_out=so)
        got, pre = _nchw64(y), (pre_add if addend else ref_lo + b64)
        what = "%s %s" % (_id(case), "+".join(name))
        if act:
            _elu_check(got, pre, what)
        else:
            ok = torch.equal(got, pre)
            print("PHASE_EDGE | fwd lattice epilogue | %s | %s" % (what, "equal" if ok else "DIFFERS"))
            assert ok, what + ": " + _mismatch_report(got, pre)
        assert _band_untouched(buf), what + ": the launch wrote outside its output"
        if so is not None:
            assert ops.amax_value(so) == float(y.abs().max()), what + ": amax_out is not max |y|"


def _edge_ratios(got, ref, edge):
    err = (got - ref).abs()
    return float(err.max() / ref.abs().max()), float(err[:, :, edge].max() / ref[:, :, edge].abs().max())


@pytest.mark.parametrize("case", _by_geometry(PR.PHASE_FWD), ids=_id)
def test_fwd_random_inputs_within_the_projects_bounds(case):
    fmt, N, h, w, C0, C1, Nout = case

    def make():
        inp = PR.inputs("fwd", case, random=True)
        return inp, F.elu(PR.fwd_ref(inp["low"].double(), inp["w"][:, :C0].double()) + inp["bias"].double().view(1, -1, 1, 1) + inp["prev"].double())
    inp, ref = _shared("fwd random", case, make)
    wts = Weights("fwd", fmt, inp["w"], C0)
    outs = []
    for _ in range(2):
        y = _nhwc(inp["prev"])
        outs.append(_fwd(fmt, _nhwc(inp["low"]), wts, y, bias=inp["bias"].cuda(), addend=y, act=True))
    whole, edges = _edge_ratios(_nchw64(outs[0]), ref, PR.edge_mask(2 * h, 2 * w, LR.PH_TH, LR.PH_TW, 2))
    b = BOUND[fmt]
    print("PHASE_EDGE | fwd random | %s | whole %.3e edge %.3e | bound %.0e | over bound %.3f %.3f" % (_id(case), whole, edges, b, whole / b, edges / b))
    assert whole <= b and edges <= b, (whole, edges, b)
    assert torch.equal(outs[0], outs[1]), "two launches of the same case differ"


# ---- data gradient and fold -------------------------------------------------------------------------------------------------------------------------
def _fold_check(what, ext, inp, N, h, w, C0, ext_ref):
    """up2_fold_bwd over the device's extended grid with (addend, ylow) and with ylow alone, against fold_ref of the reference's"""
    ops, _ = _ops()
    abuf, addend = _dev(inp["addend"])
    ybuf, ylow = _dev(inp["ylow"])
    for with_addend in (True, False):
        buf, dlow = _banded(shape=(N, h, w, C0))
        so = ops.new_slot()
        ops.up2_fold_bwd(ext, dlow, addend=addend if with_addend else None, ylow=ylow, amax_out=so)
        torch.cuda.synchronize()
        want = PR.fold_ref(ext_ref, inp["addend"].double() if with_addend else None, inp["ylow"].double())
        got = _nchw64(dlow)
        ok = torch.equal(got, want)
        print("PHASE_EDGE | fold lattice | %s | %s | %s" % (what, "addend+ylow" if with_addend else "ylow", "equal" if ok else "DIFFERS"))
        assert ok, _mismatch_report(got, want, scale=1)
        assert _band_untouched(buf), "the fold wrote outside its output"
        assert ops.amax_value(so) == float(want.abs().max()), "the fold's amax_out is not max |d(low)|"


@pytest.mark.parametrize("case", _by_geometry(PR.PHASE_DGRAD), ids=_id)
def test_dgrad_lattice_is_exact_on_the_whole_extended_grid(case):
    fmt, N, h, w, C0, C1, Nout = case

    def make():
        inp = PR.inputs("dgrad", case)
        return inp, PR.ext_ref(inp["dz"].double(), inp["w"].double())
    inp, ref = _shared("dgrad lattice", case, make)
    zbuf, dz = _dev(inp["dz"])
    wts = Weights("dgrad", fmt, inp["w"], C0)
    buf, ext = _banded(shape=(N, h + 2, w + 2, C0))
    _dgrad(fmt, dz, wts, ext)
    got = _nchw64(ext)
    ok = torch.equal(got, ref)
    print("PHASE_EDGE | dgrad lattice | %s | %s | %s" % (_id(case), "equal" if ok else "DIFFERS", sorted(r[2:] for r in LR.phase_regime("dgrad", fmt, N, h, w, C0, 0, Nout))))
    assert ok, _mismatch_report(got, ref, scale=1)
    assert _band_untouched(buf), "the launch wrote outside the extended grid"
    _fold_check(_id(case), ext, inp, N, h, w, C0, ref)


@pytest.mark.parametrize("case", PR.PHASE_FOLD, ids=_id)
def test_fold_alone_is_exact(case):
    """the fold over a lattice-valued extended grid of its own: the sizes at which its grid-stride loop runs more than once"""
    fmt, N, h, w, C0, _, _ = case
    inp = PR.inputs("fold", case)
    ebuf, ext = _dev(inp["ext"])
    _fold_check(_id(case), ext, inp, N, h, w, C0, inp["ext"].double())


@pytest.mark.parametrize("case", _by_geometry(PR.PHASE_DGRAD), ids=_id)
def test_dgrad_random_inputs_within_the_projects_bounds(case):
    ops, _ = _ops()
    fmt, N, h, w, C0, C1, Nout = case

    def make():
        inp = PR.inputs("dgrad", case, random=True)
        e = PR.ext_ref(inp["dz"].double(), inp["w"].double())
        return inp, e, PR.fold_ref(e, inp["addend"].double(), inp["ylow"].double())
    inp, eref, fref = _shared("dgrad random", case, make)
    wts = Weights("dgrad", fmt, inp["w"], C0)
    dz = _nhwc(inp["dz"])
    exts = [_dgrad(fmt, dz, wts, torch.full((N, h + 2, w + 2, C0), float("nan"), device="cuda")) for _ in range(2)]
    dlow = ops.up2_fold_bwd(exts[0], torch.full((N, h, w, C0), float("nan"), device="cuda"), addend=_nhwc(inp["addend"]), ylow=_nhwc(inp["ylow"]))
    torch.cuda.synchronize()
    emask = TR.edge_mask(h + 2, w + 2, LR.PH_TH, LR.PH_TW)
    e_whole, e_edge = _edge_ratios(_nchw64(exts[0]), eref, emask)
    f_whole, f_edge = _edge_ratios(_nchw64(dlow), fref, emask[1:-1, 1:-1])
    b = BOUND[fmt]
    print("PHASE_EDGE | dgrad random | %s | ext whole %.3e edge %.3e | folded whole %.3e edge %.3e | bound %.0e | over bound %.3f %.3f %.3f %.3f"
          % (_id(case), e_whole, e_edge, f_whole, f_edge, b, e_whole / b, e_edge / b, f_whole / b, f_edge / b))
    assert max(e_whole, e_edge, f_whole, f_edge) <= b, (e_whole, e_edge, f_whole, f_edge, b)
    assert torch.equal(exts[0], exts[1]), "two launches of the same case differ"


# ---- cancelling inputs ----------------------------------------------------------------------------------------------------------------------------
_CANCEL = [(ck, k, c) for k, c in PR.PHASE_CANCEL for ck in TR.CANCEL_KINDS]


@pytest.mark.parametrize("ckind,kind,case", _CANCEL, ids=["%s-%s-%s" % (ck, k, _id(c)) for ck, k, c in _CANCEL])
def test_cancelling_inputs_keep_the_low_order_products(ckind, kind, case):
    fmt, N, h, w, C0, C1, Nout = case

    def make():
        x, wt = PR.cancel_inputs(kind, ckind, case)
        return x, wt, PR.cancel_ref(kind, x.double(), wt.double())
    x, wt, ref = _shared("cancel %s %s" % (kind, ckind), case, make)
    wts = Weights(kind, fmt, wt, C0)
    if kind == "fwd":
        got = _fwd(fmt, _nhwc(x), wts, torch.full((N, 2 * h, 2 * w, Nout), float("nan"), device="cuda"))
    else:
        got = _dgrad(fmt, _nhwc(x), wts, torch.full((N, h + 2, w + 2, C0), float("nan"), device="cuda"))
    err = TR.rel_l2(_nchw64(got), ref)
    print("PHASE_EDGE | cancelling | %s | %s | %s | relative L2 %.4f" % (ckind, kind, _id(case), err))
    assert err <= 0.25, err


# ---- weight gradient --------------------------------------------------------------------------------------------------------------------------------
def _wgrad_ref(case, random=False):
    def make():
        inp = PR.inputs("wgrad", case, random=random)
        ref = PR.wgrad_ref_mm if case[4] * case[6] > 64 * 64 else PR.wgrad_ref          # (tied to each other on the CPU)
        return (inp,) + tuple(ref(inp["low"].double(), inp["dz"].double()))
    return _shared("wgrad random" if random else "wgrad lattice", case, make)


def _wgrad(fmt, low, dz, dw, kb, acc, db):
    ops, _ = _ops()
    if fmt == "pair":
        ops.conv_up2_phase_wgrad_hp(low, dz, dw, _slot(low), _slot(dz), kb, accumulate=acc, db=db)
    else:
        ops.conv_up2_phase_wgrad(low, dz, dw, kb, accumulate=acc, bf3=fmt == "exact", db=db)
    torch.cuda.synchronize()


@pytest.mark.parametrize("case", _by_geometry(PR.PHASE_WGRAD), ids=_id)
def test_wgrad_lattice_is_exact(case):
    fmt, N, h, w, C0, (kb, ka), Nout = case
    inp, dw_ref, db_ref = _wgrad_ref(case)
    lbuf, low = _dev(inp["low"])
    zbuf, dz = _dev(inp["dz"])
    wbuf, dw = _banded(torch.full((Nout, kb + C0 + ka, 3, 3), 7.0, device="cuda"))
    bbuf, db = _banded(torch.full((Nout,), 3.0, device="cuda")) if fmt != "f32" else (None, None)
    for rep, scale in ((0, 1.0), (1, 2.0)):
        _wgrad(fmt, low, dz, dw, kb, bool(rep), db)
        got = dw[:, kb:kb + C0].double().cpu()
        gb = db.double().cpu() if db is not None else scale * db_ref
        ok = torch.equal(got, scale * dw_ref) and torch.equal(gb, scale * db_ref)
        print("PHASE_EDGE | wgrad lattice | %s | %s | %s | %s" % (_id(case), "accumulate" if rep else "store", "equal" if ok else "DIFFERS",
                                                                   sorted(set(r[2:] for r in PR.case_regimes("wgrad", case)), key=repr)))
        bad = got != scale * dw_ref
        assert ok, "%d of %d dw elements differ, first (o, c, ky, kx): %s; db differs in %d" % (
            int(bad.sum()), bad.numel(), bad.nonzero()[:8].tolist(), int((gb != scale * db_ref).sum()))
        assert bool((dw[:, :kb] == 7.0).all()) and bool((dw[:, kb + C0:] == 7.0).all()), "channels outside the slice were touched"
        assert _band_untouched(wbuf) and (bbuf is None or _band_untouched(bbuf)), "the launch wrote outside dw / db"


@pytest.mark.parametrize("case", _by_geometry(PR.PHASE_WGRAD), ids=_id)
def test_wgrad_random_inputs_within_the_projects_bounds(case):
    fmt, N, h, w, C0, (kb, ka), Nout = case
    inp, dw_ref, db_ref = _wgrad_ref(case, random=True)
    dw = torch.full((Nout, kb + C0 + ka, 3, 3), float("nan"), device="cuda")
    db = torch.full((Nout,), float("nan"), device="cuda") if fmt != "f32" else None
    _wgrad(fmt, _nhwc(inp["low"]), _nhwc(inp["dz"]), dw, kb, False, db)
    got = dw[:, kb:kb + C0].double().cpu()
    whole = float((got - dw_ref).abs().max() / dw_ref.abs().max())
    taps = [float((got[:, :, ky, kx] - dw_ref[:, :, ky, kx]).abs().max() / dw_ref[:, :, ky, kx].abs().max()) for ky in range(3) for kx in range(3)]
    eb = float((db.double().cpu() - db_ref).abs().max() / db_ref.abs().max()) if db is not None else 0.0
    print("PHASE_EDGE | wgrad random | %s | dw whole %.3e worst tap %.3e | db %.3e | over bound %.4f %.4f %.4f"
          % (_id(case), whole, max(taps), eb, whole / BOUND_WGRAD, max(taps) / BOUND_WGRAD, eb / BOUND_DB))
    assert whole <= BOUND_WGRAD and max(taps) <= BOUND_WGRAD and eb <= BOUND_DB, (whole, max(taps), eb)
