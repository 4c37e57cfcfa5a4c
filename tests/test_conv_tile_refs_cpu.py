"""CPU: what tests/test_gpu_conv_tile_edges.py relies on, pinned without a GPU (tests/conv_tile_refs.py):

1. the float64 references against autograd / the padding forms of torch;
2. per GPU case, the lattice inputs are exactly summable: sum |x| |w| stays below 2^24 units and a float32 evaluation on the CPU equals
   the float64 one bit for bit -- so a kernel that differs from the reference in one bit is wrong, in any summation order;
3. each wrong variant (zero for reflection padding, the fold one row out, nearest-x2 before the reflection, the concat switched one chunk
   late, unflipped weights) differs from the reference on lattice inputs where it should;
4. the cancelling inputs separate a correct convolution (float32: at most 1/20 from float64 in relative L2) from every restatement with
   one product class of the split operands removed (at least 1): the GPU criterion 1/4 has a factor of four or more on either side."""
import pytest
import torch
import torch.nn.functional as F

from tests import conv_tile_refs as TR
from tests import launch_regimes as LR


def _r64(shape, seed):
    return TR.rnd(shape, seed).double()


# ---- 1. the references -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(2, 2), (3, 5), (7, 4)])
def test_references_against_autograd(H, W):
    N, Cin, Cout = 2, 3, 4
    w = _r64((Cout, Cin, 3, 3), 1)
    g = _r64((N, Cout, H, W), 2)
    for gather, dg in (("zero", "dgrad"), ("reflect", "dgrad_reflect")):
        x = _r64((N, Cin, H, W), 3).requires_grad_(True)
        wt = w.clone().requires_grad_(True)
        y = F.conv2d(x, wt, None, 1, 1) if gather == "zero" else F.conv2d(F.pad(x, (1, 1, 1, 1), mode="reflect"), wt)
        assert torch.allclose(TR.conv_ref(gather, x.detach(), w), y.detach(), rtol=0, atol=1e-13)
        y.backward(g)
        assert torch.allclose(TR.conv_ref(dg, g, w), x.grad, rtol=0, atol=1e-13), dg
        dw, db = TR.wgrad_ref(gather, x.detach(), g)
        assert torch.allclose(dw, wt.grad, rtol=0, atol=1e-13) and torch.allclose(db, g.sum((0, 2, 3)))
    # the concat gather: cat[nearest_x2(low), skip], then reflection padding
    for C1 in (0, 2):
        lo = _r64((N, Cin, H, W), 4).requires_grad_(True)
        skip = _r64((N, C1, 2 * H, 2 * W), 5) if C1 else None
        wt = _r64((Cout, Cin + C1, 3, 3), 6).requires_grad_(True)
        up = lo.repeat_interleave(2, 2).repeat_interleave(2, 3)
        y = F.conv2d(F.pad(torch.cat([up, skip], 1) if C1 else up, (1, 1, 1, 1), mode="reflect"), wt)
        assert torch.allclose(TR.conv_ref("up2", lo.detach(), wt.detach(), skip), y.detach(), rtol=0, atol=1e-13)
        g2 = _r64(tuple(y.shape), 7)
        y.backward(g2)
        dw, _ = TR.wgrad_ref("up2", lo.detach(), g2, skip)
        assert torch.allclose(dw, wt.grad, rtol=0, atol=1e-13)


def test_epilogue_chain_order():
    """every stage changes the result and the order is the documented one (any two stages swapped show)"""
    acc = torch.tensor([[[[-3.0, 2.0]]]], dtype=torch.float64)
    kw = dict(bias=torch.tensor([1.0], dtype=torch.float64), addend=torch.full_like(acc, 4.0), mask=torch.tensor([[[[1.0, -1.0]]]]).double(),
              actgrad="elu", actsrc=torch.tensor([[[[-0.5, 0.5]]]]).double(), act="relu", prev=torch.full_like(acc, -7.0))
    got = TR.epilogue_ref(acc, **kw)
    # (-3 + 1 + 4) * 0.5 = 1 -> relu 1 -> -6;   (2 + 1 + 0) * 1 = 3 -> 3 -> -4
    assert got.flatten().tolist() == [-6.0, -4.0]
    assert TR.epilogue_ref(acc, actgrad="relu", actsrc=kw["actsrc"]).flatten().tolist() == [0.0, 2.0]
    assert set(TR.SIDE_VALUES) == {-0.75, -0.5, -0.25, 0.0, 0.5, 1.0}


# ---- 2. the lattice is exactly summable, case by case ----------------------------------------------------------------------------------
_DISTINCT_TILE = sorted({(c[0],) + c[2:] for c in TR.TILE_CASES + TR.TILE_TWO_TERM})          # the inputs do not depend on the format


@pytest.mark.parametrize("case", _DISTINCT_TILE, ids=lambda c: "-".join(map(str, c)))
def test_tile_lattice_is_exact(case):
    case = (case[0], "exact") + case[1:]
    inp = TR.lattice_inputs(case)
    for k in ("src", "skip", "addend", "prev", "bias"):
        if inp[k] is not None:
            assert bool((inp[k] == inp[k].round()).all()) and float(inp[k].abs().max()) <= 4
    assert bool((inp["w"] * 8 == (inp["w"] * 8).round()).all()) and float(inp["w"].abs().max()) <= 0.5
    units = TR.abs_sum_units(case, inp)
    assert units < 2 ** 24, "sum |x||w| reaches %.0f units of 1/8" % units
    r64 = TR.case_ref(case, inp)
    r32 = TR.case_ref(case, inp, torch.float32)
    assert torch.equal(r32.double(), r64), "float32 on the CPU differs from float64 on lattice inputs"
    # the epilogue keeps it exact: every stage, with ReLU in place of the forward ELU
    e64 = TR.epilogue_ref(r64, TR.f64(inp["bias"]), TR.f64(inp["addend"]), TR.f64(inp["mask"]), "elu", TR.f64(inp["actsrc"]), "relu", TR.f64(inp["prev"]))
    e32 = TR.epilogue_ref(r32, inp["bias"], inp["addend"], inp["mask"], "elu", inp["actsrc"], "relu", inp["prev"])
    assert torch.equal(e32.double(), e64)


_DISTINCT_WGRAD = sorted({(c[0],) + c[2:] for c in TR.WGRAD_CASES})


@pytest.mark.parametrize("case", _DISTINCT_WGRAD, ids=lambda c: "-".join(map(str, c)))
def test_wgrad_lattice_is_exact(case):
    mode, N, H, W, C0, Nout = case
    assert N * H * W * 16 < 2 ** 24                              # |x| |dz| <= 16 units of 1 per pixel
    x, dz = TR.wgrad_lattice_inputs((mode, "exact") + case[1:])
    dw64, db64 = TR.wgrad_ref(mode, x.double(), dz.double())
    dw32, db32 = TR.wgrad_ref(mode, x, dz)
    assert torch.equal(dw32.double(), dw64) and torch.equal(db32.double(), db64)
    assert float(dw64.abs().max()) * 2 < 2 ** 24                # the accumulate pass doubles it


# ---- 3. wrong variants -----------------------------------------------------------------------------------------------------------------
def _where_differs(a, b):
    d = (a != b).any(0).any(0)                                  # [H, W]
    ring = TR.ring_mask(*d.shape)
    return bool(d[ring].any()), bool(d[~ring].any())


@pytest.mark.parametrize("H,W", [(8, 66), (16, 20)])
def test_wrong_variants_differ_where_they_should(H, W):
    c = ("reflect", "exact", 2, H, W, 32, 0, 32)
    inp = {k: TR.f64(v) for k, v in TR.lattice_inputs(c).items()}
    ref = TR.conv_ref("reflect", inp["src"], inp["w"])
    zero = TR.wrong_variant("zero for reflect", "reflect", inp["src"], inp["w"])
    assert _where_differs(zero, ref) == (True, False)
    border = torch.zeros(H, W, dtype=torch.bool)
    border[0] = border[-1] = True
    border[:, 0] = border[:, -1] = True
    frac = float((zero != ref)[:, :, border].double().mean())
    assert frac > 0.9, "zero against reflection padding differs on %.1f %% of the border elements only" % (100 * frac)

    c = ("dgrad_reflect", "exact", 2, H, W, 32, 0, 32)
    inp = {k: TR.f64(v) for k, v in TR.lattice_inputs(c).items()}
    ref = TR.conv_ref("dgrad_reflect", inp["src"], inp["w"])
    assert _where_differs(TR.wrong_variant("fold at 0 / n-1", "dgrad_reflect", inp["src"], inp["w"]), ref) == (True, False)
    assert _where_differs(TR.conv_ref("dgrad", inp["src"], inp["w"]), ref) == (True, False)          # no fold at all
    assert _where_differs(TR.wrong_variant("weights not flipped", "dgrad_reflect", inp["src"], inp["w"]), ref)[1]

    c = ("up2", "exact", 2, H, W, 32, 32, 32)
    inp = {k: TR.f64(v) for k, v in TR.lattice_inputs(c).items()}
    ref = TR.conv_ref("up2", inp["src"], inp["w"], inp["skip"])
    assert _where_differs(TR.wrong_variant("up2 before reflect", "up2", inp["src"], inp["w"], inp["skip"]), ref) == (True, False)
    assert _where_differs(TR.wrong_variant("concat one chunk late", "up2", inp["src"], inp["w"], inp["skip"]), ref)[1]


# ---- 4. cancelling inputs --------------------------------------------------------------------------------------------------------------
def _variants(case, inp):
    """float64 restatements of the split-operand product with one class of products removed"""
    g = case[0]
    x, w = inp["src"], inp["w"]
    full = TR.conv_ref(g, x.double(), w.double())
    x1, x2, w1, w2 = TR.bf16_terms(x, 1), TR.bf16_terms(x, 2), TR.bf16_terms(w, 1), TR.bf16_terms(w, 2)
    mm = TR.conv_ref(g, x2 - x1, w2 - w1)
    (xh, xm), (wh, wm) = TR.fp16_pair_terms(x), TR.fp16_pair_terms(w)
    pair = TR.conv_ref(g, xh + xm, wh + wm) - TR.conv_ref(g, xm, wm)          # three products: h h + h m + m h
    return full, {"fp16 pairs": pair, "x two terms": TR.conv_ref(g, x2, w.double()), "x one term": TR.conv_ref(g, x1, w.double()),
                  "w two terms": TR.conv_ref(g, x.double(), w2), "w one term": TR.conv_ref(g, x.double(), w1),
                  "without m x m": full - mm, "two-term mode": TR.conv_ref(g, x2, w2) - mm}


# "at least 1 away": a restatement that loses the whole signal returns 0 (the mid-mid inputs: exactly), which is 1 away up to the rounding of the
# float64 evaluation itself
ONE_AWAY = 1.0 - 1e-9
_MUST_SEE = {"x-low": ("x two terms", "x one term"), "w-low": ("w two terms", "w one term"),
             "mid-mid": ("without m x m", "x one term", "w one term")}


@pytest.mark.parametrize("gather,C", sorted({(c[0], c[5]) for c in TR.CANCEL_CASES}))
@pytest.mark.parametrize("kind", TR.CANCEL_KINDS)
def test_cancelling_inputs_separate_a_lost_product_class(kind, gather, C):
    case = (gather, "exact", 2, 9, 21, C, 0, C)                  # the figures depend on the channel count, not on the geometry
    inp = TR.cancel_inputs(kind, case)
    ref, var = _variants(case, inp)
    assert float(ref.abs().max()) > 0
    f32 = TR.rel_l2(TR.conv_ref(gather, inp["src"], inp["w"]), ref)
    figs = {k: TR.rel_l2(v, ref) for k, v in var.items()}
    print("CANCEL_SIM | %s | %s | C %d | float32 %.4f | %s" % (kind, gather, C, f32, " | ".join("%s %.3f" % kv for kv in sorted(figs.items()))))
    assert f32 <= 1 / 20, f32
    assert figs["fp16 pairs"] <= 1 / 16, figs["fp16 pairs"]          # the pair format's own rounding: a factor four inside the GPU criterion
    for k in _MUST_SEE[kind]:
        assert figs[k] >= ONE_AWAY, (k, figs[k])


@pytest.mark.parametrize("kind", sorted(TR.CANCEL_DELTA_TWO))
def test_cancelling_inputs_of_the_two_term_mode(kind):
    """operands of 16 significant bits and no m x m product by design: the pairs are 2^-10 apart; a correct two-term evaluation stays within
    1/20, one bf16 term per operand is at least 1 away"""
    C = TR.CANCEL_TWO_TERM[0][5]
    case = ("reflect", "two", 2, 9, 21, C, 0, C)
    inp = TR.cancel_inputs(kind, case, TR.CANCEL_DELTA_TWO[kind])
    ref, var = _variants(case, inp)
    figs = {k: TR.rel_l2(v, ref) for k, v in var.items()}
    print("CANCEL_SIM two-term | %s | C %d | %s" % (kind, C, " | ".join("%s %.3f" % kv for kv in sorted(figs.items()))))
    assert figs["two-term mode"] <= 1 / 20, figs
    assert figs["x one term" if kind == "x-low" else "w one term"] >= ONE_AWAY, figs


def test_case_tables_name_known_gathers_and_formats():
    for c in TR.TILE_CASES + TR.CANCEL_CASES:
        assert c[0] in TR.GATHERS and c[1] in ("exact", "pair"), c
    for c in TR.TILE_TWO_TERM + TR.CANCEL_TWO_TERM:
        assert c[0] in TR.FWD_GATHERS and c[1] == "two", c
    for c in TR.CANCEL_CASES + TR.CANCEL_TWO_TERM:
        assert LR.tile3_plan(c[2], c[3], c[4], c[5], c[6], c[7], c[0] == "up2", c[1]), c
        assert c[5] % 4 == 0 and c[7] % 4 == 0
    assert len(set(TR.TILE_CASES)) == len(TR.TILE_CASES) and len(set(TR.WGRAD_CASES)) == len(TR.WGRAD_CASES)
