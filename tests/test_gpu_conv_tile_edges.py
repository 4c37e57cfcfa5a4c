"""GPU: the 3x3 stride-1 tile kernels (csrc/conv3x3_tile_bf3.hip: forward, data gradient; csrc/wgrad3x3_bf3.hip: weight gradient) at ragged
pixel tiles, with inputs whose answer is exact.  References, inputs and the case tables: tests/conv_tile_refs.py (pinned on the CPU by
tests/test_conv_tile_refs_cpu.py); that the cases reach every launch regime of a train step: tests/test_launch_regimes_cpu.py.

Per case of TILE_CASES (gather x operand format x geometry):
  * lattice inputs, plain launch: equal to the float64 reference BIT FOR BIT (small integers times eighths: every partial sum is exact in
    float32, in any order, in every operand format);
  * lattice inputs, three epilogue sets: bit for bit again; output, addend, mask, actsrc and previous y are slices of larger buffers whose
    surroundings are NaN -- the output's surroundings stay NaN and no NaN comes in;
  * random-valued inputs (the ranges of tests/test_gpu_kernels.py): 2e-6 of max |ref| (test_gpu_kernels.py: test_conv3x3_bf3_kernel,
    test_gpu_hp.py: test_conv3x3_hp_kernel), 3e-6 only for an unsplit chain of K >= 4608 (test_conv3x3_bf3_up2_concat_gather); the same bound
    again with error and maximum both restricted to the border ring plus the partial tiles; a second launch is bit-identical.
Cancelling inputs (CANCEL_CASES): relative L2 error <= 1/4 -- float32 and the fp16 pairs land within 0.05, a kernel that lost a product class
lands 1 away (figures: the CPU test).  The two-term inference mode is selected the way Engine.forward selects it.
Weight gradients (WGRAD_CASES): lattice x and dz into a channel slice of a wider dw, dw and db bit for bit, the rest untouched, a second
accumulating call exactly twice both.

Every case prints its figures before it asserts (lines "TILE_EDGE | ...", run with -s to keep them)."""
import os

import pytest
import torch
import torch.nn.functional as F

from tests import conv_tile_refs as TR
from tests import launch_regimes as LR
from tests.test_gpu_kernels import _ops

pytestmark = pytest.mark.gpu

BAND = 4096               # NaN floats on either side of every output / epilogue operand


def _switched():
    return sorted(k for k in os.environ if k.startswith("FP_TILE_") or k.startswith("FP_WGRAD_"))


def _id(c):
    if len(c) == 8:
        return "%s-%s-%dx%dx%d-%d+%d>%d" % c
    return "%s-%s-%dx%dx%d-%d>%d" % c


def _nhwc(t):
    return None if t is None else t.permute(0, 2, 3, 1).contiguous().cuda()


def _banded(t_nhwc=None, shape=None):
    """(whole buffer, the slice): the slice holds t (or NaN), BAND NaN floats lie before and behind it"""
    shape = tuple(t_nhwc.shape) if shape is None else shape
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 2 * BAND,), float("nan"), device="cuda")
    view = buf[BAND:BAND + n].view(shape)
    if t_nhwc is not None:
        view.copy_(t_nhwc)
    return buf, view


def _band_untouched(buf):
    return bool(torch.isnan(buf[:BAND]).all()) and bool(torch.isnan(buf[-BAND:]).all())


# ---- one launch ----------------------------------------------------------------------------------------------------------------------
_GATHER = {"zero": "GATHER_FWD_ZERO", "reflect": "GATHER_FWD_REFLECT", "up2": "GATHER_FWD_REFLECT_UP2", "dgrad": "GATHER_DGRAD_ZERO",
           "dgrad_reflect": "GATHER_DGRAD_REFLECT"}


class Operands:
    """device copies of src / skip / w of one case in one operand format: packed weights and, for the fp16 pairs, the amax slots"""

    def __init__(self, case, inp):
        ops, L = _ops()
        gather, fmt, N, H, W, C0, C1, Nout = case
        self.case, self.fmt = case, fmt
        self.src, self.skip = _nhwc(inp["src"]), _nhwc(inp["skip"])
        w = inp["w"].contiguous().cuda()
        dg = gather in TR.DGRAD_GATHERS
        Cout, Cin = w.shape[:2]
        self.slots = None
        if fmt == "pair":
            sw = ops.new_slot()
            self.wp = ops.pack_conv_weight_hp(w, torch.empty(ops.packed_weight_elems_hp(Cout, Cin, 3, dg), device="cuda"), sw, dg)
            self.slots = (ops.amax_f32(self.src, ops.new_slot()), ops.amax_f32(self.skip, ops.new_slot()) if self.skip is not None else None, sw)
        else:
            self.wp = ops.pack_conv_weight_bf3(w, torch.empty(ops.packed_weight_elems_bf3(Cout, Cin, 3, dg), device="cuda"), dg)

    def launch(self, y, act=None, actgrad=None, accum=False, **kw):
        ops, L = _ops()
        gather, fmt, N, H, W, C0, C1, Nout = self.case
        epi = (L.EPI_ACTGRAD_ELU if actgrad == "elu" else L.EPI_ACTGRAD_RELU if actgrad == "relu" else 0) | (L.EPI_ACCUM if accum else 0)
        d = ops.make_desc(N, H, W, H, W, C0, C1, Nout, 3, 1, 1, getattr(L, _GATHER[gather]),
                          act={"elu": L.ACT_ELU, "relu": L.ACT_RELU}.get(act, L.ACT_NONE), epi=epi)
        assert ops.conv3x3_bf3_supported(d), "the launcher turns the case down: an error of the case table"
        if fmt == "pair":
            ss, s1, sw = self.slots
            ops.conv3x3_hp(d, self.src, self.wp, y, ss, sw, src1=self.skip, amax_src1=s1, **kw)
        elif fmt == "two":
            assert not ops._bf16x2
            try:
                ops._bf16x2 = True                     # Engine.forward sets it around an eval forward
                ops.conv3x3_bf3(d, self.src, self.wp, y, src1=self.skip, **kw)
            finally:
                ops._bf16x2 = False
        else:
            ops.conv3x3_bf3(d, self.src, self.wp, y, src1=self.skip, **kw)
        torch.cuda.synchronize()
        return y


# one set of inputs and references at a time, shared by the formats of a geometry and by the tests of a case
_cache = {}


def _shared(kind, case, make):
    key = (kind, case[0]) + tuple(case[2:])
    if key not in _cache:
        if len(_cache) > 6:
            _cache.clear()
        _cache[key] = make()
    return _cache[key]


def _lattice(case):
    def make():
        inp = TR.lattice_inputs(case)
        return inp, TR.case_ref(case, inp)
    return _shared("lattice", case, make)


def _mismatch_report(case, got, ref):
    """count and the first eight (n, c, y, x) with their tile coordinates"""
    gather, fmt, N, H, W, C0, C1, Nout = case
    p = LR.tile3_plan(N, H, W, C0, C1, Nout, gather == "up2", fmt)
    bad = (got != ref) | torch.isnan(got)
    idx = bad.nonzero()[:8].tolist()
    rows = ["(n %d, c %d, y %d, x %d) tile (%d, %d) of %d x %d, pixel (%d, %d): got %r, want %r"
            % (n, c, y, x, y // p["th"], x // p["tw"], p["tilesY"], p["tilesX"], y % p["th"], x % p["tw"], float(got[n, c, y, x]), float(ref[n, c, y, x]))
            for n, c, y, x in idx]
    return "%d of %d elements differ (tiles %d x %d, SK %d, %s):\n%s" % (int(bad.sum()), bad.numel(), p["th"], p["tw"], p["SK"], p["inst"], "\n".join(rows))


def _nchw64(y):
    return y.permute(0, 3, 1, 2).double().cpu()


ALL_TILE = sorted(TR.TILE_CASES + TR.TILE_TWO_TERM, key=lambda c: (c[0],) + tuple(c[2:]) + (c[1],))       # the formats of a geometry side by side


# ---- table-dependent: the library plans the cases as the restatement says ---------------------------------------------------------------
def test_library_plans_the_cases_as_the_tables_say():
    if _switched():
        pytest.skip("the launch rules are switched by %s: the regimes of the tables are those of the default build" % ", ".join(_switched()))
    ops, L = _ops()
    for gather, fmt, N, H, W, C0, C1, Nout in ALL_TILE + TR.CANCEL_CASES + TR.CANCEL_TWO_TERM:
        d = ops.make_desc(N, H, W, H, W, C0, C1, Nout, 3, 1, 1, getattr(L, _GATHER[gather]))
        p = LR.tile3_plan(N, H, W, C0, C1, Nout, gather == "up2", fmt)
        assert p and ops.conv3x3_bf3_supported(d), (gather, fmt, N, H, W, C0, C1, Nout)
        assert ops._cached_query("fp_conv3x3_bf3_workspace", d) == p["workspace"]
    for mode, fmt, N, H, W, C0, Nout in TR.WGRAD_CASES:
        d = ops.make_desc(N, H, W, H, W, C0, 0, Nout, 3, 1, 1, getattr(L, _GATHER[mode]))
        assert ops._cached_query("fp_conv_wgrad_bf3_workspace", d) == LR.wgrad3_plan(N, H, W, C0, Nout, mode == "up2")["workspace"]


# ---- lattice inputs ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ALL_TILE, ids=_id)
def test_lattice_plain_launch_is_exact(case):
    inp, ref = _lattice(case)
    o = Operands(case, inp)
    N, H, W, Nout = case[2], case[3], case[4], case[7]
    buf, y = _banded(shape=(N, H, W, Nout))
    o.launch(y)
    got = _nchw64(y)
    ok = torch.equal(got, ref)
    print("TILE_EDGE | lattice | %s | %s | %s" % (_id(case), "equal" if ok else "DIFFERS", sorted(r[2:] for r in LR.tile3_regime(*case))))
    assert ok, _mismatch_report(case, got, ref)
    assert _band_untouched(buf), "the launch wrote outside its output"


EPI_SETS = ("bias", "addend+mask+actgrad_relu+accum", "every stage")


@pytest.mark.parametrize("case", sorted(TR.TILE_CASES, key=lambda c: (c[0],) + tuple(c[2:]) + (c[1],)), ids=_id)
def test_lattice_epilogues_are_exact(case):
    """bias; addend + mask + ReLU gradient + accumulate; and every stage at once with ReLU in place of the forward ELU (which is not exact) --
    for a data gradient the engine's own set instead: ELU gradient + addend"""
    inp, ref = _lattice(case)
    o = Operands(case, inp)
    gather, N, H, W, Nout = case[0], case[2], case[3], case[4], case[7]
    e64 = {k: TR.f64(inp[k]) for k in ("bias", "addend", "mask", "actsrc", "prev")}
    dev = {k: _banded(_nhwc(inp[k])) for k in ("addend", "mask", "actsrc", "prev")}
    bias = inp["bias"].cuda()
    for name in EPI_SETS:
        if name == "bias":
            want, kw, accum = TR.epilogue_ref(ref, bias=e64["bias"]), dict(bias=bias), False
        elif name == "addend+mask+actgrad_relu+accum":
            want = TR.epilogue_ref(ref, addend=e64["addend"], mask=e64["mask"], actgrad="relu", actsrc=e64["actsrc"], prev=e64["prev"])
            kw, accum = dict(addend=dev["addend"][1], addend_mask=dev["mask"][1], actsrc=dev["actsrc"][1], actgrad="relu"), True
        elif gather in TR.DGRAD_GATHERS:
            name = "actgrad_elu+addend"
            want = TR.epilogue_ref(ref, addend=e64["addend"], actgrad="elu", actsrc=e64["actsrc"])
            kw, accum = dict(addend=dev["addend"][1], actsrc=dev["actsrc"][1], actgrad="elu"), False
        else:
            want = TR.epilogue_ref(ref, e64["bias"], e64["addend"], e64["mask"], "elu", e64["actsrc"], "relu", e64["prev"])
            kw = dict(bias=bias, addend=dev["addend"][1], addend_mask=dev["mask"][1], actsrc=dev["actsrc"][1], actgrad="elu", act="relu")
            accum = True
        buf, y = _banded(_nhwc(inp["prev"])) if accum else _banded(shape=(N, H, W, Nout))
        o.launch(y, accum=accum, **kw)
        got = _nchw64(y)
        ok = torch.equal(got, want)
        print("TILE_EDGE | lattice epilogue | %s | %s | %s" % (_id(case), name, "equal" if ok else "DIFFERS"))
        assert ok, name + ": " + _mismatch_report(case, got, want)
        assert _band_untouched(buf), name + ": the launch wrote outside its output"


# ---- random-valued inputs ---------------------------------------------------------------------------------------------------------------
def _random(case):
    def make():
        inp = TR.random_inputs(case)
        ref = TR.case_ref(case, inp)
        if case[0] in TR.FWD_GATHERS:                      # bias + ELU, as the decoder runs its forward convolutions
            return inp, F.elu(TR.epilogue_ref(ref, bias=TR.f64(inp["bias"])))
        if case[0] == "dgrad":                             # + addend (the residual branch's gradient)
            return inp, TR.epilogue_ref(ref, addend=TR.f64(inp["addend"]))
        return inp, TR.epilogue_ref(ref, addend=TR.f64(inp["addend"]), actgrad="elu", actsrc=TR.f64(inp["actsrc"]))      # engine.py: _dgrad_dec
    return _shared("random", case, make)


@pytest.mark.parametrize("case", sorted(TR.TILE_CASES, key=lambda c: (c[0],) + tuple(c[2:]) + (c[1],)), ids=_id)
def test_random_inputs_within_the_projects_bounds(case):
    gather, fmt, N, H, W, C0, C1, Nout = case
    inp, ref = _random(case)
    o = Operands(case, inp)
    if gather in TR.FWD_GATHERS:
        kw = dict(bias=inp["bias"].cuda(), act="elu")
    elif gather == "dgrad":
        kw = dict(addend=_nhwc(inp["addend"]))
    else:
        kw = dict(addend=_nhwc(inp["addend"]), actsrc=_nhwc(inp["actsrc"]), actgrad="elu")
    outs = [o.launch(torch.full((N, H, W, Nout), float("nan"), device="cuda"), **kw) for _ in range(2)]
    p = LR.tile3_plan(N, H, W, C0, C1, Nout, gather == "up2", fmt)
    bound = 3e-6 if (p["SK"] == 1 and 9 * (C0 + C1) >= 4608) else 2e-6
    err = (_nchw64(outs[0]) - ref).abs()
    edge = TR.edge_mask(H, W, p["th"], p["tw"])
    whole = float(err.max() / ref.abs().max())
    edges = float(err[:, :, edge].max() / ref[:, :, edge].abs().max())
    print("TILE_EDGE | random | %s | whole %.3e edge %.3e | bound %.0e | over bound %.2f %.2f" % (_id(case), whole, edges, bound, whole / bound, edges / bound))
    assert whole <= bound, (whole, bound)
    assert edges <= bound, (edges, bound)
    assert torch.equal(outs[0], outs[1]), "two launches of the same case differ"


# ---- cancelling inputs ------------------------------------------------------------------------------------------------------------------
_CANCEL = [(k, c) for c in TR.CANCEL_CASES for k in TR.CANCEL_KINDS] + [(k, c) for c in TR.CANCEL_TWO_TERM for k in sorted(TR.CANCEL_DELTA_TWO)]


@pytest.mark.parametrize("kind,case", _CANCEL, ids=["%s-%s" % (k, _id(c)) for k, c in _CANCEL])
def test_cancelling_inputs_keep_the_low_order_products(kind, case):
    def make():
        inp = TR.cancel_inputs(kind, case, TR.CANCEL_DELTA_TWO[kind] if case[1] == "two" else None)
        return inp, TR.case_ref(case, inp)
    inp, ref = _shared("cancel " + kind + (" two" if case[1] == "two" else ""), case, make)
    N, H, W, Nout = case[2], case[3], case[4], case[7]
    y = Operands(case, inp).launch(torch.full((N, H, W, Nout), float("nan"), device="cuda"))
    err = TR.rel_l2(_nchw64(y), ref)
    print("TILE_EDGE | cancelling | %s | %s | relative L2 %.4f" % (kind, _id(case), err))
    assert err <= 0.25, err


# ---- weight gradient --------------------------------------------------------------------------------------------------------------------
def _wgrad_ref(case):
    def make():
        x, dz = TR.wgrad_lattice_inputs(case)
        return (x, dz) + TR.wgrad_ref(case[0], x.double(), dz.double())
    key = ("wgrad", case[0]) + tuple(case[2:])
    if key not in _cache:
        if len(_cache) > 6:
            _cache.clear()
        _cache[key] = make()
    return _cache[key]


@pytest.mark.parametrize("case", sorted(TR.WGRAD_CASES, key=lambda c: (c[0],) + tuple(c[2:]) + (c[1],)), ids=_id)
def test_wgrad_lattice_is_exact(case):
    ops, L = _ops()
    mode, fmt, N, H, W, C0, Nout = case
    x, dz, dw_ref, db_ref = _wgrad_ref(case)
    d = ops.make_desc(N, H, W, H, W, C0, 0, Nout, 3, 1, 1, getattr(L, _GATHER[mode]))
    assert ops.conv_wgrad_bf3_supported(d), "the launcher turns the case down: an error of the case table"
    pad = 32                                                     # destination = channel slice [pad, pad + C0) of a wider gradient
    dw = torch.full((Nout, C0 + 2 * pad, 3, 3), 7.0, device="cuda")
    db = torch.full((Nout,), 3.0, device="cuda")
    xs, gz = _nhwc(x), _nhwc(dz)
    am = (ops.amax_f32(xs, ops.new_slot()), ops.amax_f32(gz, ops.new_slot())) if fmt == "pair" else None
    for rep, scale in ((0, 1.0), (1, 2.0)):
        ops.conv_wgrad_bf3(d, xs, gz, dw, pad, accumulate=bool(rep), db=db, amax=am)
        torch.cuda.synchronize()
        got, gb = dw[:, pad:pad + C0].double().cpu(), db.double().cpu()
        ok = torch.equal(got, scale * dw_ref) and torch.equal(gb, scale * db_ref)
        print("TILE_EDGE | wgrad lattice | %s | %s | %s | %s" % (_id(case), "accumulate" if rep else "store", "equal" if ok else "DIFFERS",
                                                                  sorted(r[2:] for r in LR.wgrad3_regime(*case))))
        bad = (got != scale * dw_ref)
        assert ok, "%d of %d dw elements differ, first (o, c, ky, kx): %s; db differs in %d" % (
            int(bad.sum()), bad.numel(), bad.nonzero()[:8].tolist(), int((gb != scale * db_ref).sum()))
        assert bool((dw[:, :pad] == 7.0).all()) and bool((dw[:, pad + C0:] == 7.0).all()), "the rest of dw was touched"
