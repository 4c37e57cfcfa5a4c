"""CPU: the float64 references, planted inputs and bounds of tests/loss_refs.py, checked without a GPU before tests/test_gpu_losses.py
relies on them.

1. Both references agree with the project's oracle (oracle/restatement.py loss_manager / seg_loss) in float64 to 1e-12, values and gradients,
   on every GPU case's inputs.
2. Every planted regime occurs: the pixels per (all_ground, depth_mask, moving) combination, the saturated logits and the exact-kink elements
   are counted in the built tensors.
3. The |.|-kink exclusion stays a vanishing fraction of the depth-channel elements (KINK_MAX_FRACTION of tests/parity.py; at most 2 elements
   below 1000 pixels).
4. The CPU float32 oracle sits below every derived floor of a reduced value: no bound is tighter than the reference's own arithmetic.
5. Nine wrong formulas, evaluated in float64, each move a compared quantity by more than ten times its bound on some GPU case.
"""
from collections import OrderedDict

import pytest
import torch

from oracle import restatement as R
from tests import loss_refs as LF
from tests.parity import KINK_MAX_FRACTION

FP_NAMES = [c.name for c in LF.FP_CASES]
SEG_NAMES = [c.name for c in LF.SEG_CASES]


def _d(ts):
    return [t.double() for t in ts]


def _d_targets(t):
    return OrderedDict((k, v.double()) for k, v in t.items())


# ---- Footprints loss -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FP_NAMES)
def test_footprints_reference_inputs_and_floors(name):
    r = LF.fp_reference(name)
    c, ref = r.case, r.ref
    # 1. the restatement against the oracle, float64
    v64, g64 = LF.oracle_loss(r.preds, r.targets, torch.float64, c.depth_range, c.prior)
    assert float((v64 - ref.values).abs().max()) <= 1e-12 * max(float(v64.abs().max()), 1.0)
    for a, b in zip(g64, ref.grads):
        for ch in range(4):
            assert float((a[:, ch] - b[:, ch]).abs().max()) <= 1e-12 * max(float(a[:, ch].abs().max()), 1e-300)
    # ... and against the analytic derivative of the BCE, sigmoid(x) - t, which autograd on a closed form misses at a logit of exactly 0
    gs, T64 = 1.0 / (4 * c.B * c.H * c.W), _d_targets(r.targets)
    m = ((T64["all_ground"] + T64["depth_mask"]) > 0).double()
    for p, g in zip(r.preds, ref.grads):
        s0, s1 = torch.sigmoid(p[:, 0].double()), torch.sigmoid(p[:, 1].double())
        want1 = (s1 - T64["all_ground"]) * m * (1 - T64["moving_object_mask"]) + c.prior * s1 * (1 - m)
        assert float((g[:, 0] - (s0 - T64["visible_ground"]) * gs).abs().max()) <= 1e-12 * gs
        assert float((g[:, 1] - want1 * gs).abs().max()) <= 1e-12 * gs
    # every input is a finite float32 (no launch may depend on a NaN or an infinity)
    assert all(bool(torch.isfinite(p).all()) and p.dtype == torch.float32 for p in r.preds + list(r.targets.values()))
    # 2. the planted regimes
    want = LF.planted_counts(c)
    T = {k: v.view(c.B, -1) for k, v in r.targets.items()}
    blk = slice(0, LF.N_PLANT if c.planted else 0)
    for ag in (0, 1):
        for dm in (0, 1):
            for mov in (0, 1):
                n = int(((T["all_ground"][:, blk] == ag) & (T["depth_mask"][:, blk] == dm) & (T["moving_object_mask"][:, blk] == mov)).sum())
                assert n == want["combo"], (ag, dm, mov, n)
                if c.H * c.W > 1000:                    # and the dense filler reaches every combination on its own
                    assert int(((T["all_ground"] == ag) & (T["depth_mask"] == dm) & (T["moving_object_mask"] == mov)).sum()) > want["combo"]
    sat = sum(int((p[:, :2].abs() >= LF.SATURATED).sum()) for p in r.preds)
    assert sat == want["saturated"], sat
    assert int(ref.exact.sum()) == want["exact_kink"]
    if c.planted:
        for s, p in enumerate(r.preds):
            pf = p.view(c.B, 4, -1)[:, :, :LF.N_PLANT]
            for ch, tgt in ((0, "visible_ground"), (1, "all_ground")):          # each logit against both targets
                for x in LF.LOGITS:
                    seen = set(T[tgt][:, :LF.N_PLANT][pf[:, ch] == x].tolist())
                    assert seen == {0.0, 1.0}, (s, ch, x, seen)
            if not c.zero_depth:
                for ch, tgt in ((2, "depth"), (3, "ground_depth")):             # disparities exactly 0 and 1 against each depth target
                    pairs = set(zip(pf[:, ch].reshape(-1).tolist(), T[tgt][:, :LF.N_PLANT].reshape(-1).tolist()))
                    assert pairs == {(o, t) for o in (0.0, 1.0) for t in LF.DEPTH_TARGETS}, pairs
    if c.zero_depth:
        assert not bool(r.targets["depth"].any()) and not bool(r.targets["ground_depth"].any())
        assert all(float(g[:, 2:].abs().max()) == 0.0 for g in ref.grads) and all(float(ref.means[4 * s + k]) == 0.0 for s in range(4) for k in (2, 3))
    if tuple(c.depth_range) == LF.EXACT_RANGE:          # on the exact kink the reference's gradient is 0 and its loss term log 1 = 0
        for s in range(4):
            for k in (0, 1):
                assert float(ref.grads[s][:, 2 + k][ref.exact[s, k]].abs().max()) == 0.0
    # 3. the exclusion cap, for the reference alone
    total, kinks = 8 * c.B * c.H * c.W, int(ref.kink.sum())
    print("KINK %s %d of %d (%.2e)" % (name, kinks, total, kinks / total))
    assert kinks <= (2 if c.B * c.H * c.W < 1000 else KINK_MAX_FRACTION * total)
    # 4. the CPU float32 oracle against the derived floors
    e32 = (r.v32 - ref.values).abs()
    ratio = float(LF.value_ratios(r.v32, ref.values, r.value_floor).max())
    print("CPU32 %s worst value error / floor %.3f" % (name, ratio))
    assert ratio <= 1.0, (e32.tolist(), r.value_floor.tolist())
    assert bool((r.value_bound >= LF.FACTOR * r.value_floor).all())
    rel = r.value_floor / ref.values.abs().clamp_min(1e-300)
    assert float(rel[ref.values != 0].max()) < 1e-4, "a value's floor is above 1e-4 of the value: badly conditioned inputs"
    for s in range(4):
        for ch in range(4):
            sels, _ = LF.fp_plane_selections(r, s, ch)
            for label, sel in sels:
                g = ref.grads[s][:, ch]
                mx = float((g.abs() if sel is None else g.abs()[sel]).max())
                ec = LF.plane_err(r.g32[s][:, ch], g, sel)
                assert ec <= LF.anchored(ec, LF.GRAD_FLOOR * mx) and ec <= 16 * LF.GRAD_FLOOR * mx, (s, ch, label, ec, mx)


def _fp_moves(r, variant):
    """largest shift / bound over the quantities the GPU test compares, when the float64 reference evaluates `variant`"""
    c, ref = r.case, r.ref
    wrong = LF.footprints_loss_ref(_d(r.preds), _d_targets(r.targets), c.depth_range, c.prior, variant=variant)
    worst = float(LF.value_ratios(wrong.values, ref.values, r.value_bound).max())
    for s in range(4):
        zero = LF.fp_zero_masks(r, s)
        for ch in range(4):
            if ch in zero and bool((wrong.grads[s][:, ch][zero[ch]] != 0).any()):
                return float("inf")                     # the GPU test asks for == 0 there
            sels, _ = LF.fp_plane_selections(r, s, ch)
            for _, sel in sels:
                g = ref.grads[s][:, ch]
                mx = float((g.abs() if sel is None else g.abs()[sel]).max())
                bound = LF.anchored(LF.plane_err(r.g32[s][:, ch], g, sel), LF.GRAD_FLOOR * mx)
                shift = LF.plane_err(wrong.grads[s][:, ch], g, sel)
                if shift > 0:
                    worst = max(worst, shift / bound if bound > 0 else float("inf"))
    return worst


@pytest.mark.parametrize("variant", LF.VARIANTS_FP)
def test_footprints_bounds_see_a_wrong_formula(variant):
    seen = {}
    for name in ("3x40x72-range", "3x40x72", "2x160x208"):
        seen[name] = _fp_moves(LF.fp_reference(name), variant)
        if seen[name] > 10.0:
            break
    print("MOVES %s %s" % (variant, seen))
    assert max(seen.values()) > 10.0, "%s moves no compared quantity by more than %.2f bounds" % (variant, max(seen.values()))


# ---- segmentation loss ---------------------------------------------------------------------------------------------------------------
def _seg_grad_bounds(r, s):
    g = r.ref.grads[s]
    mx = float(g.abs().max())
    return mx, LF.anchored(LF.plane_err(r.c32.grads[s], g), LF.seg_grad_floor(r.case, s) * mx)


@pytest.mark.parametrize("name", SEG_NAMES)
def test_segmentation_reference_inputs_and_floors(name):
    r = LF.seg_reference(name)
    c, ref = r.case, r.ref
    B = c.B
    outs = [m.double().requires_grad_(True) for m in r.maps]
    tot = R.seg_loss(outs, r.ground.double(), r.labelled.double(), c.H, c.W)
    assert abs(float(tot.detach()) - float(ref.values[5 * B])) <= 1e-12 * max(abs(float(tot.detach())), 1.0)
    if c.backward:
        tot.backward()
        for o, g in zip(outs, ref.grads):
            assert float((o.grad - g).abs().max()) <= 1e-12 * max(float(g.abs().max()), 1e-300)
    assert ref.values.shape == (5 * B + 1,) and bool(torch.isfinite(ref.values).all())
    assert abs(float(ref.values[4 * B:5 * B].mean()) - float(ref.values[5 * B])) <= 1e-15
    if name == "2x16x24-one-none":
        assert ref.valid.tolist() == [1.0, 0.0] and float(r.labelled[0, -1, -1]) == 1.0
        assert all(float(ref.values[s * B + 1]) == 0.0 for s in range(5)) and all(float(g[1].abs().max()) == 0.0 for g in ref.grads)
    if name == "1x8x8":
        assert [tuple(m.shape[2:]) for m in r.maps] == [(1, 1), (2, 2), (4, 4), (8, 8)]
    if name == "2x136x128":
        assert c.H * c.W > 64 * 256
    if c.planted:
        for mp in r.maps:                               # every logit edge in every map of every image, on the border
            for b in range(B):
                border = torch.cat([mp[b, 0, 0, :], mp[b, 0, :, -1]]).tolist()
                assert set(torch.tensor(LF.LOGITS).tolist()) <= set(border), (tuple(mp.shape), b)
        assert bool((r.labelled[:, 0, :] == 1).all()) and set(r.ground[:, 0, :].reshape(-1).tolist()) == {0.0, 1.0}
    ratio = float(LF.value_ratios(r.c32.values, ref.values, r.value_floor).max())
    print("CPU32 %s worst value error / floor %.3f" % (name, ratio))
    assert ratio <= 1.0
    lab = ref.valid > 0
    rel = (r.value_floor[:4 * B].view(4, B) / ref.values[:4 * B].view(4, B).abs().clamp_min(1e-300))[:, lab]
    assert float(rel.max()) < 1e-4
    if c.backward:
        for s in range(4):
            mx, bound = _seg_grad_bounds(r, s)
            assert LF.plane_err(r.c32.grads[s], ref.grads[s]) <= 4 * LF.seg_grad_floor(c, s) * mx, s


def _seg_moves(r, variant):
    c, ref = r.case, r.ref
    wrong = LF.seg_loss_ref(_d(r.maps), r.ground.double(), r.labelled.double(), c.H, c.W, variant=variant, backward=c.backward)
    if not bool(torch.isfinite(wrong.values).all()):
        return float("inf")                             # the GPU test asks for finite values
    worst = float(LF.value_ratios(wrong.values, ref.values, r.value_bound).max())
    if c.backward:
        for s in range(4):
            mx, bound = _seg_grad_bounds(r, s)
            shift = LF.plane_err(wrong.grads[s], ref.grads[s])
            if shift > 0:
                worst = max(worst, shift / bound if bound > 0 else float("inf"))
    return worst


@pytest.mark.parametrize("variant", LF.VARIANTS_SEG)
def test_segmentation_bounds_see_a_wrong_formula(variant):
    seen = {}
    for name in ("2x16x24-one-none", "3x64x96", "2x20x28-fractional"):
        seen[name] = _seg_moves(LF.seg_reference(name), variant)
        if seen[name] > 10.0:
            break
    print("MOVES %s %s" % (variant, seen))
    assert max(seen.values()) > 10.0, "%s moves no compared quantity by more than %.2f bounds" % (variant, max(seen.values()))


def test_tracked_reference_layout():
    v = torch.arange(11, dtype=torch.float64)            # B = 2: scales 0..3 at [0..8), averages at [8, 10), batch mean at 10
    assert LF.tracked_ref(v, 2) == {"ground_loss_0": 0.5, "ground_loss_1": 2.5, "ground_loss_2": 4.5, "ground_loss_3": 6.5, "loss": 8.5}
