"""CPU: what tests/test_gpu_conv_phase_edges.py relies on, pinned without a GPU (tests/conv_phase_refs.py):

1. the float64 references against autograd, and the restated kernel arithmetic (collapsed weights, K4, un-collapse) against the references;
2. per GPU case, the lattice inputs are exactly summable: every collapsed weight and K4 entry is one term of the case's operand format, the
   sum of |products| behind one output stays below 2^24 units through every later stage, and a float32 evaluation on the CPU equals the
   float64 one bit for bit;
3. each wrong variant differs from the reference on lattice inputs, where it should;
4. the cancelling inputs separate a correct evaluation (float32 and the restated fp16 pairs: below 1/4 by a factor of four) from every
   restatement with one product class of the split operands removed (at least 1 away)."""
import pytest
import torch
import torch.nn.functional as F

from tests import conv_phase_refs as PR
from tests import conv_tile_refs as TR


def _r64(shape, seed):
    return TR.rnd(shape, seed).double()


# ---- 1. the references -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(1, 1), (1, 3), (2, 1), (2, 2), (3, 5), (9, 4)])
def test_references_against_autograd(h, w):
    N, C0, Cout = 2, 3, 4
    wt = _r64((Cout, C0, 3, 3), 1).requires_grad_(True)
    pre = (_r64((N, C0, h, w), 2) * 2).requires_grad_(True)
    low = F.elu(pre)
    extra = _r64((N, C0, h, w), 3)
    y = F.conv2d(F.pad(F.interpolate(low, scale_factor=2, mode="nearest"), (1, 1, 1, 1), mode="reflect"), wt)
    g = _r64(tuple(y.shape), 4)
    ((y * g).sum() + (low * extra).sum()).backward()
    lo, wd = low.detach(), wt.detach()
    assert torch.allclose(PR.fwd_ref(lo, wd), y.detach(), rtol=0, atol=1e-13)
    ext = PR.ext_ref(g, wd)
    assert tuple(ext.shape) == (N, C0, h + 2, w + 2)
    assert torch.allclose(PR.fold_ref(ext, extra, lo), pre.grad, rtol=0, atol=1e-13)           # fold(ext) + addend, times ELU' = autograd's low.grad
    dw, db = PR.wgrad_ref(lo, g)
    assert torch.allclose(dw, wt.grad, rtol=0, atol=1e-13) and torch.allclose(db, g.sum((0, 2, 3)))
    dw2, db2 = PR.wgrad_ref_mm(lo, g)
    assert torch.allclose(dw2, dw, rtol=0, atol=1e-13) and torch.equal(db2, db)
    # the kernels' arithmetic, restated: the same mathematics
    assert torch.allclose(PR.phase_fwd(lo, wd), y.detach(), rtol=0, atol=1e-13)
    assert torch.allclose(PR.ext_by_k4(g, wd), ext, rtol=0, atol=1e-13)                         # the WHOLE extended grid, ring included
    assert torch.allclose(PR.uncollapse(PR.collapsed_wgrad(lo, g)), dw, rtol=0, atol=1e-13)


def test_collapse_and_k4_are_the_packers_tables():
    """pack.hip:64-66 and :80-82 as sums of taps; every tap lands in exactly one collapsed row per phase and in two K4 rows at most"""
    w = torch.zeros(1, 1, 3, 3, dtype=torch.float64)
    w[0, 0] = torch.tensor([[1.0, 2.0, 4.0], [8.0, 16.0, 32.0], [64.0, 128.0, 256.0]])
    wc = PR.collapse(w)
    assert [float(wc[(0, 0, a, b)]) for a in (0, 1) for b in (0, 1)] == [1.0, 6.0, 72.0, 432.0]
    assert [float(wc[(1, 1, a, b)]) for a in (0, 1) for b in (0, 1)] == [27.0, 36.0, 192.0, 256.0]
    for dy in (0, 1):
        for dx in (0, 1):
            assert sum(float(wc[(dy, dx, a, b)]) for a in (0, 1) for b in (0, 1)) == 511.0
    k = PR.k4(w)[0, 0]
    assert k[0].tolist() == [256.0, 384.0, 192.0, 64.0] and k[3].tolist() == [4.0, 6.0, 3.0, 1.0] and float(k.sum()) == 4 * 511.0


# ---- 2. the lattice is exactly summable, case by case ----------------------------------------------------------------------------------
def _distinct(table):
    return sorted({c[1:] for c in table}, key=repr)


def _ids(c):
    return "-".join(str(v) for v in c)


def _weights_are_one_term(w):
    amax = float(w.abs().max())
    for t in list(PR.collapse(w).values()) + [PR.k4(w)]:
        assert float(t.abs().max()) <= 2.0 and bool((t * 8 == (t * 8).round()).all())                  # at most 16 eighths
        for fmt in ("exact", "pair"):
            assert PR.is_one_term(t, fmt, amax), fmt


@pytest.mark.parametrize("case", _distinct(PR.PHASE_FWD), ids=_ids)
def test_fwd_lattice_is_exact(case):
    case = ("exact",) + case
    inp = PR.inputs("fwd", case)
    for k in ("low", "skip", "bias", "prev"):
        if inp[k] is not None:
            assert bool((inp[k] == inp[k].round()).all()) and float(inp[k].abs().max()) <= 4
            assert PR.is_one_term(inp[k], "exact") and PR.is_one_term(inp[k], "pair", target=PR.HP_TARGET_ACT)
    _weights_are_one_term(inp["w"][:, :case[4]])
    assert PR.abs_units("fwd", case, inp) < 2 ** 24
    r64 = PR.fwd_ref(inp["low"].double(), inp["w"].double(), TR.f64(inp["skip"]))
    assert torch.equal(PR.fwd_ref(inp["low"], inp["w"], inp["skip"]).double(), r64)
    e64 = TR.epilogue_ref(r64, bias=inp["bias"].double(), addend=inp["prev"].double())
    e32 = TR.epilogue_ref(PR.fwd_ref(inp["low"], inp["w"], inp["skip"]), bias=inp["bias"], addend=inp["prev"])
    assert torch.equal(e32.double(), e64)
    if case[5] == 0:                                               # the collapsed form, added up in float32 in the kernel's tap order
        assert torch.equal(PR.phase_fwd(inp["low"], inp["w"]).double(), r64)


@pytest.mark.parametrize("case", _distinct(PR.PHASE_DGRAD), ids=_ids)
def test_dgrad_lattice_is_exact(case):
    case = ("exact",) + case
    inp = PR.inputs("dgrad", case)
    _weights_are_one_term(inp["w"])
    assert set(inp["ylow"].unique().tolist()) <= set(PR.ELU_SIDE_VALUES) and float(inp["ylow"].min()) > -1.0
    assert PR.is_one_term(inp["dz"], "exact") and PR.is_one_term(inp["dz"], "pair", target=PR.HP_TARGET_ACT)
    assert PR.abs_units("dgrad", case, inp) < 2 ** 24
    e64 = PR.ext_ref(inp["dz"].double(), inp["w"].double())
    assert torch.equal(PR.ext_ref(inp["dz"], inp["w"]).double(), e64) and torch.equal(PR.ext_by_k4(inp["dz"], inp["w"]).double(), e64)
    f64 = PR.fold_ref(e64, inp["addend"].double(), inp["ylow"].double())
    assert torch.equal(PR.fold_ref(e64.float(), inp["addend"], inp["ylow"]).double(), f64)


@pytest.mark.parametrize("case", _distinct(PR.PHASE_WGRAD), ids=_ids)
def test_wgrad_lattice_is_exact(case):
    case = ("exact",) + case
    N, h, w, C0, ks, Nout = case[1:]
    assert PR.abs_units("wgrad", case, None) == 2.0 * N * 4 * h * w * 16 < 2 ** 24
    inp = PR.inputs("wgrad", case)
    for k in ("low", "dz"):
        assert bool((inp[k] == inp[k].round()).all()) and float(inp[k].abs().max()) <= 4
    if C0 * Nout <= 64 * 64:                                       # (the 1024 x 768 cases: the bound above is the argument)
        dw64, db64 = PR.wgrad_ref(inp["low"].double(), inp["dz"].double())
        dw32, db32 = PR.wgrad_ref(inp["low"], inp["dz"])
        assert torch.equal(dw32.double(), dw64) and torch.equal(db32.double(), db64)
        assert float(dw64.abs().max()) * 2 < 2 ** 24


@pytest.mark.parametrize("case", PR.PHASE_FOLD, ids=_ids)
def test_fold_lattice_is_exact(case):
    assert 4.0 * (9 * 4 + 4) < 2 ** 24                           # nine extended positions of at most 4, the addend, in quarters
    if case[1] * case[2] * case[3] * case[4] < 1 << 16:
        inp = PR.inputs("fold", case)
        assert PR.abs_units("fold", case, inp) < 2 ** 24
        f64 = PR.fold_ref(inp["ext"].double(), inp["addend"].double(), inp["ylow"].double())
        assert torch.equal(PR.fold_ref(inp["ext"], inp["addend"], inp["ylow"]).double(), f64)


# ---- 3. wrong variants -----------------------------------------------------------------------------------------------------------------
def _rows_cols(diff):
    """(rows, columns) of the [.., H, W] positions where anything differs"""
    d = diff.flatten(0, -3).any(0)
    return sorted(set(d.nonzero()[:, 0].tolist())), sorted(set(d.nonzero()[:, 1].tolist()))


@pytest.mark.parametrize("h,w", [(5, 7), (9, 17)])
def test_wrong_variants_differ_where_they_should(h, w):
    case = ("exact", 2, h, w, 32, 0, 32)
    inp = {k: TR.f64(v) for k, v in PR.inputs("fwd", case).items()}
    ref = PR.fwd_ref(inp["low"], inp["w"])
    assert torch.equal(PR.phase_fwd(inp["low"], inp["w"]), ref)
    H, W = 2 * h, 2 * w
    # reflection instead of replicate at low resolution: the outermost hi-res rows and columns, nothing inside
    rows, cols = _rows_cols(PR.wrong_variant("reflect at low resolution", inp["low"], inp["w"]) != ref)
    inner = (PR.wrong_variant("reflect at low resolution", inp["low"], inp["w"]) != ref)[:, :, 1:-1, 1:-1]
    assert not bool(inner.any()) and {0, H - 1} <= set(rows) and {0, W - 1} <= set(cols)
    # phases swapped: the two mixed phases (dy != dx) only
    d = PR.wrong_variant("phases swapped", inp["low"], inp["w"]) != ref
    assert bool(d[:, :, 0::2, 1::2].any()) and bool(d[:, :, 1::2, 0::2].any()) and not bool(d[:, :, 0::2, 0::2].any()) and not bool(d[:, :, 1::2, 1::2].any())
    # rows paired wrongly: the even hi-res rows (dy = 0) only
    d = PR.wrong_variant("rows paired wrongly", inp["low"], inp["w"]) != ref
    assert bool(d[:, :, 0::2].any()) and not bool(d[:, :, 1::2].any())
    assert float(d[:, :, 0::2].double().mean()) > 0.5

    dc = ("exact", 2, h, w, 32, 0, 32)
    di = {k: TR.f64(v) for k, v in PR.inputs("dgrad", dc).items()}
    good = PR.fold_ref(PR.ext_ref(di["dz"], di["w"]))
    # fold onto rows 1 / h-2: rows 0, 1, h-2, h-1 and the same columns, nothing else
    rows, cols = _rows_cols(PR.wrong_variant("fold onto 1 / h-2", di["dz"], di["w"]) != good)
    assert set(rows) | set(cols) and not bool((PR.wrong_variant("fold onto 1 / h-2", di["dz"], di["w"]) != good)[:, :, 2:-2, 2:-2].any())
    assert {0, 1, h - 2, h - 1} <= set(rows) and {0, 1, w - 2, w - 1} <= set(cols)
    # K4 not flipped: everywhere
    d = PR.wrong_variant("K4 not flipped", di["dz"], di["w"]) != good
    assert float(d.double().mean()) > 0.9

    wi = {k: TR.f64(v) for k, v in PR.inputs("wgrad", ("exact", 2, h, w, 32, (0, 0), 32)).items()}
    dw, _ = PR.wgrad_ref(wi["low"], wi["dz"])
    assert torch.equal(PR.uncollapse(PR.collapsed_wgrad(wi["low"], wi["dz"])), dw)
    d = PR.wrong_variant("uncollapse pairing", wi["low"], wi["dz"]) != dw
    taps, cols = _rows_cols(d)                                    # [Nout, C0, ky, kx]: the centre row alone (for dy = 1, ky = 1 sits in a = 0), at every kx
    assert taps == [1] and cols == [0, 1, 2] and float(d[:, :, 1].double().mean()) > 0.9
    assert len(PR.WRONG) == 6


# ---- 4. cancelling inputs --------------------------------------------------------------------------------------------------------------
def _variants(kind, x, w):
    """float64 restatements of the split-operand product with one class of products removed"""
    ref = lambda a, b: PR.cancel_ref(kind, a, b)
    full = ref(x.double(), w.double())
    x1, x2, w1, w2 = TR.bf16_terms(x, 1), TR.bf16_terms(x, 2), TR.bf16_terms(w, 1), TR.bf16_terms(w, 2)
    mm = ref(x2 - x1, w2 - w1)
    (xh, xm), (wh, wm) = PR.fp16_pair_terms(x, PR.HP_TARGET_ACT), PR.fp16_pair_terms(w, PR.HP_TARGET_W)
    pair = ref(xh + xm, wh + wm) - ref(xm, wm)                     # three products: h h + h m + m h
    return full, {"fp16 pairs": pair, "x two terms": ref(x2, w.double()), "x one term": ref(x1, w.double()), "w two terms": ref(x.double(), w2),
                  "w one term": ref(x.double(), w1), "without m x m": full - mm}


ONE_AWAY = 1.0 - 1e-9
_MUST_SEE = {"x-low": ("x two terms", "x one term"), "w-low": ("w two terms", "w one term"), "mid-mid": ("without m x m", "x one term", "w one term")}


@pytest.mark.parametrize("kind", ("fwd", "dgrad"))
@pytest.mark.parametrize("ckind", TR.CANCEL_KINDS)
def test_cancelling_inputs_separate_a_lost_product_class(ckind, kind):
    C = PR.PHASE_CANCEL[0][1][4]
    assert {c[4] for _, c in PR.PHASE_CANCEL} == {C} == {c[6] for _, c in PR.PHASE_CANCEL}
    case = ("exact", 2, 5, 9, C, 0, C)                           # the figures depend on the channel count, not on the geometry
    x, w = PR.cancel_inputs(kind, ckind, case)
    assert not bool(w[:, :, 1].any()) and not bool(w[:, :, :, 1].any()) and bool(w[:, :, 0, 0].any())
    # every collapsed weight and K4 entry is one stored float32 weight or zero: float32 sums of the taps are exact
    for t32, t64 in zip(list(PR.collapse(w).values()) + [PR.k4(w)], list(PR.collapse(w.double()).values()) + [PR.k4(w.double())]):
        assert torch.equal(t32.double(), t64)
    ref, var = _variants(kind, x, w)
    assert float(ref.abs().max()) > 0
    f32 = TR.rel_l2(PR.cancel_ref(kind, x, w), ref)
    figs = {k: TR.rel_l2(v, ref) for k, v in var.items()}
    print("PHASE_CANCEL_SIM | %s | %s | C %d | float32 %.4f | %s" % (ckind, kind, C, f32, " | ".join("%s %.3f" % kv for kv in sorted(figs.items()))))
    assert f32 <= 1 / 16, f32
    assert figs["fp16 pairs"] <= 1 / 16, figs["fp16 pairs"]
    for k in _MUST_SEE[ckind]:
        assert figs[k] >= ONE_AWAY, (k, figs[k])
