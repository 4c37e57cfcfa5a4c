"""GPU: fp_bn_bwd_frozen / fp_bn_bwd_frozen_partials / fp_bn_eval_coeffs_saved (csrc/bn_frozen.hip) against float64 per element.

References and derived bounds: tests/finetune_refs.py (checked on the CPU by tests/test_finetune_cpu.py, which also shows that the
shapes reach both rows-per-workgroup layouts, the capped grid with a looping row walk, and fewer rows than one workgroup holds).  Every
output is a slice of a poisoned buffer with guard bands (tests/test_gpu_step_kernels.py::Guarded); each check prints
`RATIO <case> <error / bound>` before it asserts."""
import functools

import pytest
import torch

from tests import finetune_refs as FR
from tests.test_finetune_cpu import KERNEL_SHAPES
from tests.test_gpu_step_kernels import Guarded, dev, exact, guards_ok, within

pytestmark = pytest.mark.gpu


def _ops():
    from footprints_amd import ops
    return ops


@functools.lru_cache(maxsize=2)
def _inputs(shape):
    inp = FR.bn_inputs(shape)
    mean, invstd = FR.frozen_stats(inp)
    return inp, mean, invstd


@functools.lru_cache(maxsize=4)
def _ref(shape, relu_out):
    return FR.frozen_bn_bwd_ref(_inputs(shape)[0], relu_out)


# sums: "both" = dgamma and dbeta, "none" = neither (single launch, z never read), "gamma" / "beta" = one of them (once per shape)
VARIANTS = [(sh, ro, go, sm) for sh in KERNEL_SHAPES for ro in (True, False) for go in (False, True) for sm in ("both", "none")] + \
           [(sh, True, False, sm) for sh in KERNEL_SHAPES for sm in ("gamma", "beta")]


@pytest.mark.parametrize("shape,relu_out,g_out,sums", VARIANTS)
def test_bn_bwd_frozen(shape, relu_out, g_out, sums):
    ops = _ops()
    inp, mean, invstd = _inputs(shape)
    ref, bound = _ref(shape, relu_out)
    M, C = inp["z"].shape
    d = {k: dev(inp[k]) for k in ("dy", "ro", "z", "gamma")}
    md, isd = dev(mean), dev(invstd)
    want_g, want_b = sums in ("both", "gamma"), sums in ("both", "beta")
    tag = "bn_bwd_frozen %s relu_out=%d g_out=%d sums=%s" % (shape, relu_out, g_out, sums)
    if sums == "none":                         # z must not be read: a NaN-filled one may not reach dz; mean is not passed at all
        d["z"] = torch.full_like(d["z"], float("nan"))

    def run(accumulate):
        dz, go = Guarded((M, C)), (Guarded((M, C)) if g_out else None)
        dg = Guarded((C,), init=inp["dgamma0"] if accumulate else None)
        db = Guarded((C,), init=inp["dbeta0"] if accumulate else None)
        slot = ops.new_slot()
        ops.bn_bwd_frozen(d["dy"], d["ro"] if relu_out else None, d["z"], md if sums != "none" else None, isd, d["gamma"], dz.t,
                          dg.t if want_g else None, db.t if want_b else None, g_out=go.t if g_out else None, accumulate=accumulate,
                          amax_out=slot)
        guards_ok(dz, dg, db, *([go] if g_out else []))
        assert ops.amax_value(slot) == float(dz.t.abs().max()), tag + ": the amax slot is not max |dz|"
        return dz, go, dg, db
    dz, go, dg, db = run(False)
    assert not bool(torch.isnan(dz.t).any()), tag
    within(tag + " dz", dz.t, ref["dz"], bound["dz"])
    if want_g:
        within(tag + " dgamma", dg.t, ref["dgamma"], bound["dgamma"])
    else:
        assert bool(torch.isnan(dg.t).all()), tag + ": dgamma was written"        # still the poison
    if want_b:
        within(tag + " dbeta", db.t, ref["dbeta"], bound["dbeta"])
    else:
        assert bool(torch.isnan(db.t).all()), tag + ": dbeta was written"
    if g_out:
        exact(tag + " g_out", go.t, ref["g"].float())
    if sums == "none":
        return
    dz2, _, dg2, db2 = run(True)               # accumulate: the finished sums are added to the old values, old + fresh in float32
    exact(tag + " accumulate dz", dz2.t, dz.t)
    if want_g:
        exact(tag + " accumulate dgamma", dg2.t, dev(inp["dgamma0"]) + dg.t)
    else:
        exact(tag + " accumulate dgamma untouched", dg2.t, dev(inp["dgamma0"]))
    if want_b:
        exact(tag + " accumulate dbeta", db2.t, dev(inp["dbeta0"]) + db.t)
    else:
        exact(tag + " accumulate dbeta untouched", db2.t, dev(inp["dbeta0"]))


@pytest.mark.parametrize("sums", [True, False])
@pytest.mark.parametrize("shape", KERNEL_SHAPES)
def test_bn_bwd_frozen_partials(shape, sums):
    """g is the masked gradient; the partials (sum g, sum g * xhat) per tile and channel are written here the way a data gradient's
    epilogue leaves them: float32 sums over consecutive row tiles of 7 rows (nblk not a multiple of 64: the combining lanes are ragged)"""
    ops = _ops()
    inp, mean, invstd = _inputs(shape)
    ref, bound = _ref(shape, True)
    M, C = inp["z"].shape
    g = ref["g"].float()
    xh = ((inp["z"].double() - mean.double()) * invstd.double())
    tile = 7
    nblk = (M + tile - 1) // tile
    pad = nblk * tile - M
    g64 = torch.cat([ref["g"], torch.zeros(pad, C, dtype=torch.float64)]).view(nblk, tile, C)
    t64 = torch.cat([ref["g"] * xh, torch.zeros(pad, C, dtype=torch.float64)]).view(nblk, tile, C)
    part = torch.stack([g64.sum(1).float(), t64.sum(1).float()], dim=-1).contiguous()          # [nblk][C][2]
    # the partials are rounded once each: u * sum |partial| on top of the combination's bound (double accumulation, one final rounding)
    extra_b = FR.U * g64.sum(1).abs().sum(0) + FR.U * ref["dbeta"].abs()
    extra_g = FR.U * t64.sum(1).abs().sum(0) + FR.U * ref["dgamma"].abs()
    tag = "bn_bwd_frozen_partials %s sums=%d" % (shape, sums)
    dz, dg, db = Guarded((M, C)), Guarded((C,)), Guarded((C,))
    slot = ops.new_slot()
    ops.bn_bwd_frozen_partials(dev(g), dev(invstd), dev(inp["gamma"]), dz.t, dg.t if sums else None, db.t if sums else None,
                               dev(part) if sums else None, nblk if sums else 0, amax_out=slot)
    guards_ok(dz, dg, db)
    assert ops.amax_value(slot) == float(dz.t.abs().max()), tag
    within(tag + " dz", dz.t, ref["dz"], bound["dz"])
    if sums:
        within(tag + " dgamma", dg.t, ref["dgamma"], extra_g)
        within(tag + " dbeta", db.t, ref["dbeta"], extra_b)
    else:
        assert bool(torch.isnan(dg.t).all()) and bool(torch.isnan(db.t).all()), tag


@pytest.mark.parametrize("C", [64, 512])
def test_bn_eval_coeffs_saved(C):
    """mean = running_mean (bit-exact), invstd = 1 / sqrt(running_var + eps) within three roundings, scale = gamma * invstd of THAT float32
    invstd (bit-exact product), shift = beta - mean * scale from that scale (two roundings on the magnitudes)"""
    ops = _ops()
    inp = FR.bn_inputs((1, 2, 2, C))
    out = {k: Guarded((C,)) for k in ("scale", "shift", "mean", "invstd")}
    ops.bn_eval_coeffs_saved(dev(inp["gamma"]), dev(inp["beta"]), dev(inp["rm"]), dev(inp["rv"]), out["scale"].t, out["shift"].t,
                             out["mean"].t, out["invstd"].t, FR.EPS)
    guards_ok(*out.values())
    exact("coeffs mean", out["mean"].t, inp["rm"])
    is64 = (inp["rv"].double() + FR.EPS) ** -0.5
    within("coeffs invstd C=%d" % C, out["invstd"].t, is64, 3 * FR.U * is64)
    got_is = out["invstd"].t.cpu()
    exact("coeffs scale", out["scale"].t, inp["gamma"] * got_is)
    sc = out["scale"].t.cpu().double()
    sh64 = inp["beta"].double() - inp["rm"].double() * sc
    within("coeffs shift C=%d" % C, out["shift"].t, sh64, 2 * FR.U * (inp["beta"].double().abs() + (inp["rm"].double() * sc).abs()))
