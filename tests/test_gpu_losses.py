"""GPU: the two training losses (csrc/loss_adam_misc.hip loss_kernel + loss_final_kernel, csrc/seg_loss.hip) and the test-set metric
reductions (csrc/eval_metrics.hip) at their edges, against float64.

Inputs, float64 references and the derived bounds come from tests/loss_refs.py; tests/test_loss_refs_cpu.py proves there that the references
agree with the oracle, that every planted regime occurs and that the bounds can tell nine wrong formulas from the right one;
tests/test_launch_regimes_cpu.py proves that the shapes here reach the launch regimes of the trainers' shapes.  Every bound is
FACTOR * max(error of the CPU float32 oracle on the same inputs, derived floor).  Every output is a slice of a poisoned buffer with guard
bands.  Each check prints `RATIO <case> <error / bound>` before the test asserts (profiles/loss_kernel_edges_notes.md lists them as
measured on the MI355X); a test collects its failures and reports them together.
"""
import numpy as np
import pytest
import torch

from oracle import filler
from oracle import metrics as M
from tests import loss_refs as LF
from tests.test_gpu_step_kernels import POISON_I32, Guarded, guards_ok

pytestmark = pytest.mark.gpu


def _ops():
    from footprints_amd import ops
    return ops


def dev(t):
    return t.detach().contiguous().cuda()


def _ratio(err, bound):
    return 0.0 if err == 0 else (err / bound if bound > 0 else float("inf"))


class Report:
    def __init__(self, case):
        self.case, self.bad = case, []

    def ratio(self, what, r):
        print("RATIO %s %s %.4f" % (self.case, what, r))
        if not r <= 1.0:
            self.bad.append("%s: error / bound = %.3f" % (what, r))

    def exact(self, what, ok):
        print("RATIO %s %s %s" % (self.case, what, "exact" if ok else "NOT exact"))
        if not ok:
            self.bad.append("%s: not exact" % what)

    def done(self):
        assert not self.bad, "%s: %s" % (self.case, self.bad)


# ----------------------------------------------------------------------------------------------------------------------------------
# Footprints loss
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in LF.FP_CASES])
def test_footprints_loss_edges(name):
    """ops.loss_fwd_bwd on four different prediction tensors: the 21 values per value, the 16 gradient planes per element relative to
    the plane's float64 maximum (on the |.|-kink: the float64 magnitude with either sign), exact zeros where a mask makes the gradient 0,
    finite results, identical bits on a second and on a forward-only call, untouched guard bands"""
    ops = _ops()
    r = LF.fp_reference(name)
    c, ref = r.case, r.ref
    rep = Report("loss " + name)
    pd = [dev(p) for p in r.preds]
    tg = {k: dev(v) for k, v in r.targets.items()}
    out = Guarded((21,))
    dp = [Guarded(tuple(p.shape)) for p in pd]
    ops.loss_fwd_bwd(pd, tg, out.t, [g.t for g in dp], depth_range=c.depth_range, prior=c.prior)
    guards_ok(out, *dp)
    got_v = out.t.cpu()
    rep.exact("values finite", bool(torch.isfinite(got_v).all()))
    ratios = LF.value_ratios(got_v, ref.values, r.value_bound)
    for i, key in enumerate(LF.R.LOSS_KEYS):
        rep.ratio("value %s" % (key,), float(ratios[i]))
    for s in range(4):
        got = dp[s].t.cpu()
        rep.exact("dpred %d finite" % s, bool(torch.isfinite(got).all()))
        zero = LF.fp_zero_masks(r, s)
        for ch in range(4):
            g64, g32, gg = ref.grads[s][:, ch], r.g32[s][:, ch], got[:, ch].double()
            sels, kink = LF.fp_plane_selections(r, s, ch)
            for label, sel in sels:
                mx = float((g64.abs() if sel is None else g64.abs()[sel]).max())
                bound = LF.anchored(LF.plane_err(g32, g64, sel), LF.GRAD_FLOOR * mx)
                rep.ratio("dpred %d channel %d %s" % (s, ch, label), _ratio(LF.plane_err(gg, g64, sel), bound))
            if kink is not None and bool(kink.any()):          # on the kink: the float64 magnitude, either sign
                mx = float(g64.abs().max())
                bound = LF.anchored(LF.plane_err(g32.abs(), g64.abs(), kink), LF.GRAD_FLOOR * mx)
                rep.ratio("dpred %d channel %d kink magnitude (%d elements)" % (s, ch, int(kink.sum())), _ratio(LF.plane_err(gg.abs(), g64.abs(), kink), bound))
            if ch in zero:
                rep.exact("dpred %d channel %d zero where masked (%d elements)" % (s, ch, int(zero[ch].sum())), bool((gg[zero[ch]] == 0).all()))
        if c.zero_depth:
            rep.exact("dpred %d depth planes all zero" % s, bool((got[:, 2:] == 0).all()))
    if c.zero_depth:
        rep.exact("depth terms zero", all(float(got_v[5 * s + k]) == 0.0 for s in range(4) for k in (2, 3)))
    # a second call: identical bits; forward only: the same 21 values bit for bit
    out2 = Guarded((21,))
    dp2 = [torch.empty_like(p) for p in pd]
    ops.loss_fwd_bwd(pd, tg, out2.t, dp2, depth_range=c.depth_range, prior=c.prior)
    rep.exact("second call", torch.equal(out2.t, out.t) and all(torch.equal(a, b.t) for a, b in zip(dp2, dp)))
    out3 = Guarded((21,))
    ops.loss_fwd_bwd(pd, tg, out3.t, None, depth_range=c.depth_range, prior=c.prior)
    guards_ok(out2, out3, *dp)
    rep.exact("forward only", torch.equal(out3.t, out.t))
    rep.done()


# ----------------------------------------------------------------------------------------------------------------------------------
# segmentation loss
# ----------------------------------------------------------------------------------------------------------------------------------
def _seg_maps(r, sliced):
    """-> (maps handed to the kernel, gradient maps addressed like them, the poisoned buffers behind the gradient maps)"""
    if not sliced:
        gs = [Guarded(tuple(m.shape)) for m in r.maps]
        return [dev(m) for m in r.maps], [g.t for g in gs], gs
    maps, grads, bufs = [], [], []
    for m in r.maps:            # [B,2,h,w] buffers, channel 0 handed out (how Segmentor hands its outputs out)
        B, _, h, w = m.shape
        pb = torch.zeros(B, 2, h, w, device="cuda")
        pb[:, 0] = m.cuda()[:, 0]
        gb = torch.empty(B, 2, h, w, device="cuda")
        gb.view(torch.int32).fill_(POISON_I32)
        maps.append(pb[:, :1])
        grads.append(gb[:, :1])
        bufs.append(gb)
    return maps, grads, bufs


@pytest.mark.parametrize("sliced", [False, True], ids=["dense", "sliced"])
@pytest.mark.parametrize("name", [c.name for c in LF.SEG_CASES])
def test_segmentation_loss_edges(name, sliced):
    """ops.seg_loss_fwd_bwd on dense maps and on channel slices of wider buffers: the 5 B + 1 values per value, each gradient map per
    element relative to the map's float64 maximum, loss 0 and an all-zero gradient for an image without a labelled pixel, finite results,
    identical bits on a second call; SegmentationLoss on the same maps: the same bits, and tracked() per key"""
    from footprints_amd.preprocessing.segmentation.losses import SegmentationLoss
    ops = _ops()
    r = LF.seg_reference(name)
    c, ref = r.case, r.ref
    B = c.B
    rep = Report("seg %s %s" % (name, "sliced" if sliced else "dense"))
    gm, lm = dev(r.ground), dev(r.labelled)
    maps, grads, bufs = _seg_maps(r, sliced)
    losses = Guarded((5 * B + 1,))
    if not c.backward:          # non-integer ratios: forward only; a call that asks for gradients is refused by name
        with pytest.raises(RuntimeError, match="not an integer fraction"):
            ops.seg_loss_fwd_bwd(maps, gm, lm, losses.t, dpreds=grads)
        with pytest.raises(RuntimeError, match="not an integer fraction"):
            SegmentationLoss()([m.detach().requires_grad_(True) for m in maps], gm, lm)
        grads = None
    ops.seg_loss_fwd_bwd(maps, gm, lm, losses.t, dpreds=grads)
    guards_ok(losses, *([] if sliced else bufs))
    got_v = losses.t.cpu()
    rep.exact("values finite", bool(torch.isfinite(got_v).all()))
    ratios = LF.value_ratios(got_v, ref.values, r.value_bound)
    for s in range(5):
        rep.ratio("values %s" % ("scale %d" % s if s < 4 else "average"), float(ratios[s * B:(s + 1) * B].max()))
    rep.ratio("value batch mean", float(ratios[5 * B]))
    unlabelled = [b for b in range(B) if float(ref.valid[b]) == 0.0]
    for b in unlabelled:
        rep.exact("image %d without labels: loss 0" % b, all(float(got_v[s * B + b]) == 0.0 for s in range(5)))
    if c.backward:
        for s in range(4):
            got = grads[s].cpu()
            if sliced:
                rep.exact("map %d: the buffer's other channel untouched" % s, bool((bufs[s][:, 1].view(torch.int32) == POISON_I32).all()))
            rep.exact("map %d gradient finite" % s, bool(torch.isfinite(got).all()))
            g64 = ref.grads[s]
            mx = float(g64.abs().max())
            bound = LF.anchored(LF.plane_err(r.c32.grads[s], g64), LF.seg_grad_floor(c, s) * mx)
            rep.ratio("map %d gradient" % s, _ratio(LF.plane_err(got, g64), bound))
            for b in unlabelled:
                rep.exact("map %d image %d without labels: gradient 0" % (s, b), bool((got[b] == 0).all()))
    # a second call: identical bits
    losses2 = Guarded((5 * B + 1,))
    grads2 = [torch.empty_like(g, memory_format=torch.contiguous_format) for g in grads] if c.backward else None
    maps2 = [m.contiguous() for m in maps] if sliced else maps
    ops.seg_loss_fwd_bwd(maps2, gm, lm, losses2.t, dpreds=grads2)
    guards_ok(losses2)
    same = torch.equal(losses2.t, losses.t) and (not c.backward or all(torch.equal(a, b) for a, b in zip(grads2, grads)))
    rep.exact("second call (dense copies)" if sliced else "second call", same)
    if c.backward:              # the trainer's entry point: same launches, and the Evaluator's bookkeeping
        sl = SegmentationLoss()
        gp = [m.detach().requires_grad_(True) for m in maps]
        loss = sl(gp, gm, lm)
        loss.backward()
        rep.exact("SegmentationLoss value", float(loss) == float(got_v[5 * B]))
        rep.exact("SegmentationLoss gradients", all(torch.equal(p.grad, g) for p, g in zip(gp, grads)))
        tr, want = sl.tracked(), LF.tracked_ref(ref.values, B)
        rep.exact("tracked keys", set(tr) == set(want) and sl.tracked() == {})
        for i, key in enumerate(["ground_loss_%d" % s for s in range(4)] + ["loss"]):
            mag = float(ref.values[i * B:(i + 1) * B].abs().mean())
            bound = float(r.value_bound[i * B:(i + 1) * B].mean()) + (B + 1) * LF.U * mag      # the mean of B values: B roundings
            rep.ratio("tracked %s" % key, _ratio(abs(float(tr[key]) - want[key]), bound))
    rep.done()


# ----------------------------------------------------------------------------------------------------------------------------------
# metrics
# ----------------------------------------------------------------------------------------------------------------------------------
METRIC_SHAPES = [(1, 5, 7), (2, 33, 37), (3, 48, 65)]       # fewer pixels than the 1024 threads; one pass and a tail; three passes and a tail


def metric_inputs(B, H, W, dt):
    """tests/golden/metrics_inputs.py's construction at another shape: the threshold neighbours planted again; for B >= 2 the last image
    has empty free space and image 1 no hidden depth, for B >= 3 image 0 has no hidden ground"""
    tag = "medge%dx%dx%d" % (B, H, W)
    pred = filler.uniform(tag + ".pred", (B, 4, H, W)).astype(np.float32)
    edge = np.array([0.5, 0.5 - 2.0 ** -12, 0.5 + 2.0 ** -11, 0.5 - 2.0 ** -25, 0.5 + 2.0 ** -24, 0.49987793, 0.50024414], np.float32)
    pred[:, 1, 0, :edge.size] = edge
    pred[:, 1, 1, :edge.size] = edge
    pred[:, 3, 0, :4] = np.array([0.0, 1.0, 2.0 ** -14, 0.999], np.float32)
    pred = pred.astype(dt)
    gt_kitti = filler.bernoulli(tag + ".gt.kitti", (B, H, W), 0.3) > 0.5
    free = filler.bernoulli(tag + ".free", (B, H, W), 0.6) > 0.5
    gt_mp = filler.bernoulli(tag + ".gt.mp", (B, H, W), 0.4) * filler.uniform(tag + ".gt.mp.v", (B, H, W), 0.0, 1.2)
    gt_mp[:, 2, :6] = np.array([0.1, 0.10000001, 0.9, 0.89999998, 0.05, 1.0], np.float32)
    gt_mp = gt_mp.astype(np.float32)
    gt_depth = (filler.bernoulli(tag + ".gt.depth.m", (B, H, W), 0.5) * filler.uniform(tag + ".gt.depth", (B, H, W), 0.0, 30.0)).astype(np.float32)
    gt_depth[:, 0, :4] = 7.0                                 # the planted disparities are scored
    free[:, :3, :8] = True                                   # ... and the planted thresholds lie inside the free space
    if B >= 2:
        free[B - 1] = False
        gt_depth[1] = 0.0
    if B >= 3:
        gt_kitti[0] = False
        gt_mp[0] = 0.0
    return pred, gt_kitti, gt_mp, free, gt_depth


def _mask_counts(true, pred):
    """evaluate_model.py:72-99's four integers"""
    t, p = true > 0.1, pred > 0.5
    return [int(t.sum()), int((t & p).sum()), int((~t & p).sum()), int((t & ~p).sum())]


def _depth_sums(gt, pred4, max_depth=20):
    """evaluate_model.py:50-69's terms in the arrays' own dtypes, summed in float64"""
    pred = M.sigmoid_to_depth(pred4[M.HIDDEN_DEPTH])
    mask = gt > 0
    g, p = np.clip(gt[mask], 0.5, max_depth), np.clip(pred[mask], 0.5, max_depth)
    sq = (g - p) ** 2
    assert sq.dtype == np.float32
    return [float(g.size), float((np.maximum(g / p, p / g) < 1.25).sum()), float(sq.astype(np.float64).sum()),
            float((np.abs(g - p) / g).astype(np.float64).sum()), float((sq / g).astype(np.float64).sum())]


def _same(a, b):
    return (np.isnan(a) and np.isnan(b)) or a == b


@pytest.mark.parametrize("dense", [False, True], ids=["slice", "dense"])
@pytest.mark.parametrize("dt", [np.float16, np.float32], ids=["float16", "float32"])
@pytest.mark.parametrize("B,H,W", METRIC_SHAPES)
def test_metric_kernels_edges(B, H, W, dt, dense):
    """fp_eval_mask_counts / fp_eval_depth_sums through evaluate_model and directly, against oracle.metrics.score_image on the same arrays:
    confusion counts and a1 exact, depth means within 1e-5 of numpy's float32 means and within 1e-12 of a float64 sum of the same terms"""
    from footprints_amd.evaluation import evaluate_model as EM
    ops = _ops()
    pred, gt_kitti, gt_mp, free, gt_depth = metric_inputs(B, H, W, dt)
    rep = Report("metrics %dx%dx%d %s %s" % (B, H, W, np.dtype(dt).name, "dense" if dense else "slice"))
    hidden = np.ascontiguousarray(pred[:, M.HIDDEN_GROUND]) if dense else pred
    disp = np.ascontiguousarray(pred[:, M.HIDDEN_DEPTH]) if dense else pred
    pd = torch.from_numpy(pred).cuda()
    p_mask = torch.from_numpy(hidden).cuda() if dense else pd[:, M.HIDDEN_GROUND]
    p_disp = torch.from_numpy(disp).cuda() if dense else pd[:, M.HIDDEN_DEPTH]
    fs = torch.from_numpy(free.astype(np.uint8)).cuda()
    for flavour, gt in (("kitti", gt_kitti), ("matterport", gt_mp)):
        scores = EM.mask_scores(hidden, gt, free)
        gtd = torch.from_numpy(gt.astype(np.float32)).cuda()
        a = ops.eval_mask_counts(p_mask, gtd).cpu().tolist()
        b = ops.eval_mask_counts(p_mask, gtd, region=fs, invert=True).cpu().tolist()
        ok_scores = ok_counts = True
        for i in range(B):
            want = M.score_image(pred[i], gt[i], free[i], "iou")
            for part in ("freespace", "footprint"):
                ok_scores &= all(_same(scores[i][part][k], want[part][k]) for k in ("iou", "precision", "recall", "f1"))
            h = pred[i][M.HIDDEN_GROUND]
            ok_counts &= a[i] == _mask_counts(gt[i], h) and b[i] == _mask_counts(1 - gt[i][free[i]], 1 - h[free[i]])
        rep.exact("%s mask scores" % flavour, ok_scores)
        rep.exact("%s confusion counts" % flavour, ok_counts)
    dscores = EM.depth_scores(disp, gt_depth)
    sums = ops.eval_depth_sums(p_disp, torch.from_numpy(gt_depth).cuda(), clip=(0.5, 20.0)).cpu().numpy()
    worst5, worst12, ok_a1 = 0.0, 0.0, True
    for i in range(B):
        want = M.score_image(pred[i], gt_depth[i], None, "depth")
        s64 = _depth_sums(gt_depth[i], pred[i])
        ok_a1 &= sums[i][0] == s64[0] and sums[i][1] == s64[1]
        if s64[0] == 0:
            ok_a1 &= all(np.isnan(dscores[i][k]) and np.isnan(want[k]) for k in ("a1", "abs_rel", "sq_rel", "rmse")) and not sums[i].any()
            continue
        ok_a1 &= dscores[i]["a1"] == want["a1"]
        n = s64[0]
        mine = {"abs_rel": s64[3] / n, "sq_rel": s64[4] / n, "rmse": float(np.sqrt(s64[2] / n))}
        for k in ("abs_rel", "sq_rel", "rmse"):
            worst5 = max(worst5, abs(dscores[i][k] - float(want[k])) / (1e-5 * abs(float(want[k]))))
            worst12 = max(worst12, abs(dscores[i][k] - mine[k]) / (1e-12 * abs(mine[k])))
        for j in (2, 3, 4):
            worst12 = max(worst12, abs(sums[i][j] - s64[j]) / (1e-12 * abs(s64[j])))
    rep.exact("depth counts and a1", bool(ok_a1))
    rep.ratio("depth means against numpy (1e-5)", worst5)
    rep.ratio("depth means and sums against float64 sums of the same terms (1e-12)", worst12)
    rep.done()
