"""GPU: fine-tuning -- frozen parameters (requires_grad=False) and frozen BatchNorm statistics (the encoder's BatchNorm2d modules in eval
mode while the network trains) through the drop-in surface, TrainStep with and without its recorded launch plan, and the checkpoints.

Semantics are PyTorch's: a frozen tensor gets no .grad, is never written and has no optimiser state; a trainable tensor's gradient is
bit-identical to the unfrozen run's (same kernels, same order); frozen statistics are never written and gradients still flow through
the layer.  Whole-network cases run at 2x64x64 (layer 4 is 2 x 2: every split and wrapped regime of the small levels), one at 2x96x128.
Gradients under frozen statistics are held to the float64 eval-mode oracle evaluated under the engine's own ReLU / max-pool decisions
(tests/parity.py FORCED_* bounds, relative L2 per tensor); measured figures: profiles/finetune_notes.md."""
import os
import subprocess
import sys
from collections import OrderedDict

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOW = ("encoder.layer0", "encoder.layer1")


def _mm(P, B, folder=None):
    from footprints_amd.model_manager import ModelManager
    mm = ModelManager(save_folder=folder)
    mm.model.load_state_dict({**P, **B})
    return mm


def _lm():
    from footprints_amd.training.losses import LossManager
    return LossManager((0.1, 100), 0.25, compute_viz=False)


def _dropin(mm, batch, lm, step=True):
    """forward + loss + zero_grad + backward [+ optimiser.step] through the nn.Module surface -> the loss"""
    mm.model.train()
    out = mm.model(batch["image"])
    losses = lm(out, batch)
    mm.model.zero_grad()
    losses["loss"].backward()
    if step:
        mm.optimiser.step()
    return losses["loss"].detach().clone()


def _grads(model):
    return OrderedDict((n, None if p.grad is None else p.grad.detach().clone()) for n, p in model.named_parameters())


def _state(model):
    return OrderedDict((k, v.detach().clone()) for k, v in model.state_dict().items())


def _is_buffer(k):
    return k.endswith(("running_mean", "running_var", "num_batches_tracked"))


def _hooked(eng):
    calls = []
    eng.debug_hook = lambda i, d: calls.append(i)
    return calls


def _pair(tag, frozen_prefixes):
    """an unfrozen and a frozen model on the same state and batch, one drop-in forward + backward each (no step yet)"""
    from oracle import restatement as R
    P, B = R.make_state(tag=tag)
    batch = {k: v.cuda() for k, v in R.make_batch(2, 64, 64, tag=tag).items()}
    a, b = _mm(P, B), _mm(P, B)
    b.model.freeze(frozen_prefixes)
    calls = _hooked(b.model.engine())
    lm = _lm()
    la, lb = _dropin(a, batch, lm, step=False), _dropin(b, batch, lm, step=False)
    assert torch.equal(la, lb)
    return P, a, b, calls


def _check_frozen_run(P, a, b, prefixes):
    from footprints_amd.network import is_dead_param
    ga, gb = _grads(a.model), _grads(b.model)
    for n in ga:
        if n.startswith(prefixes) or is_dead_param(n):
            assert gb[n] is None, "%s: a frozen / dead tensor has a .grad" % n
        else:
            assert gb[n] is not None and torch.equal(ga[n], gb[n]), "%s: gradient differs from the unfrozen run's" % n
    a.optimiser.step()
    b.optimiser.step()
    torch.cuda.synchronize()
    sa, sb = _state(a.model), _state(b.model)
    for k in sa:
        if k in P and k.startswith(prefixes):
            assert torch.equal(sb[k].cpu(), P[k]), "%s: a frozen tensor was written" % k
        else:                                   # trainable tensors, dead ones and the running statistics (they did move: train-mode BatchNorm)
            assert torch.equal(sa[k], sb[k]), k
    return sa, sb


# ---- 1. frozen encoder, train-mode BatchNorm, drop-in surface --------------------------------------------------------------------------
def test_frozen_encoder_dropin():
    from footprints_amd.network import is_dead_param
    P, a, b, calls = _pair("ft1", ("encoder",))
    assert calls == [], "the encoder's backward ran for blocks %s" % calls
    sa, sb = _check_frozen_run(P, a, b, ("encoder",))
    params = list(b.model.parameters())
    names = [n for n, _ in b.model.named_parameters()]
    want = {i for i, n in enumerate(names) if not n.startswith("encoder") and not is_dead_param(n)}
    got = set(b.optimiser.state_dict()["state"].keys())
    assert got == want
    # ... which is what torch.optim.Adam keeps when the frozen (and dead) parameters never had a gradient
    cpu = [torch.zeros(1, requires_grad=True) for _ in params]
    for i in want:
        cpu[i].grad = torch.zeros(1)
    ref = torch.optim.Adam(cpu, lr=1e-4)
    ref.step()
    assert set(ref.state_dict()["state"].keys()) == got
    assert len(a.optimiser.state_dict()["state"]) == 196


def test_frozen_encoder_running_statistics_move():
    """train-mode BatchNorm keeps updating its running statistics when its affine parameters are frozen, as in PyTorch"""
    from oracle import restatement as R
    P, B = R.make_state(tag="ft1b")
    batch = {k: v.cuda() for k, v in R.make_batch(2, 64, 64, tag="ft1b").items()}
    b = _mm(P, B)
    b.model.freeze(("encoder",))
    _dropin(b, batch, _lm())
    sb = _state(b.model)
    for k, v in B.items():
        if k.startswith("encoder"):
            assert not torch.equal(sb[k].cpu(), v), "%s did not move" % k


def test_freezing_after_a_backward_wants_the_stale_grad_gone():
    """a tensor frozen after a backward pass still holds its view of the flat gradient buffer: refused (tests/test_gpu_trainer.py pins the
    message) until that .grad is set to None; then the frozen tensor stays without one and the others get theirs"""
    from oracle import restatement as R
    P, B = R.make_state(tag="ft1c")
    batch = {k: v.cuda() for k, v in R.make_batch(2, 64, 64, tag="ft1c").items()}
    mm, lm = _mm(P, B), _lm()
    _dropin(mm, batch, lm, step=False)
    p0 = mm.model.encoder.layer0[0].weight
    assert p0.grad is not None
    p0.requires_grad_(False)
    out = mm.model(batch["image"])
    with pytest.raises(RuntimeError, match="frozen parameters"):
        lm(out, batch)["loss"].backward()
    _dropin(mm, batch, lm)                       # zero_grad(), backward, step
    assert p0.grad is None and torch.equal(p0.detach().cpu(), P["encoder.layer0.0.weight"])
    assert mm.model.encoder.layer0[1].weight.grad is not None


# ---- 2. frozen prefix ------------------------------------------------------------------------------------------------------------------
def test_frozen_prefix_dropin():
    P, a, b, calls = _pair("ft2", LOW)
    assert sorted(calls) == list(range(3, 16)), "encoder blocks whose backward ran: %s" % sorted(calls)      # layers 2-4 (layer 1 = blocks 0-2)
    _check_frozen_run(P, a, b, LOW)


# ---- 3. frozen statistics, everything trainable ----------------------------------------------------------------------------------------
def _frozen_stats_case(Bn, Hn, Wn):
    from oracle import restatement as R
    from tests import finetune_refs as FR
    from tests.gpu_child import engine_decisions
    from tests.parity import FLIP_MAX_FRACTION, FORCED_MAX_ERR, FORCED_MEDIAN_ERR, chan_relerr, rel_l2, tie_free_batch
    from footprints_amd._format import operand_format
    tag = "frozen statistics %dx%dx%d %s" % (Bn, Hn, Wn, operand_format())
    P, B = R.make_state(tag="ft3")
    cpu_batch = R.make_batch(Bn, Hn, Wn, tag="ft3")
    out64, _, g64, cpu_batch = FR.oracle_grads_eval(P, B, cpu_batch, torch.float64, fix_batch=lambda b, o: tie_free_batch(b, o)[0])
    out32, _, g32, _ = FR.oracle_grads_eval(P, B, cpu_batch, torch.float32)
    mm = _mm(P, B)
    model = mm.model
    model.freeze_bn_stats()
    model.train()
    batch = {k: v.cuda() for k, v in cpu_batch.items()}
    out = model(batch["image"])
    torch.cuda.synchronize()
    decisions = engine_decisions(model.engine())            # before backward: the saved activations are the engine's own buffers
    losses = _lm()(out, batch)
    model.zero_grad()
    losses["loss"].backward()
    gpu = _grads(model)
    mm.optimiser.step()
    torch.cuda.synchronize()
    for k, v in model.state_dict().items():
        if _is_buffer(k):
            assert torch.equal(v.cpu(), B[k]), "%s: %s was written" % (tag, k)
    for k in R.SCALES:
        e32, e64 = max(chan_relerr(out[k], out32[k])), max(chan_relerr(out[k], out64[k]))
        print("FIGURE %s output %s: %.2e vs float32, %.2e vs float64 (bound 1e-4)" % (tag, k, e32, e64))
        assert e32 <= 1e-4 and e64 <= 1e-4, (tag, k, e32, e64)
    imposed = R.ReluDecisions(impose=decisions["relu"], pool_impose=decisions["pool"])
    g64f = FR.oracle_grads_eval(P, B, cpu_batch, torch.float64, relu_decisions=imposed)[2]
    n_relu, n_pool = sum(m.numel() for m in imposed.taken), decisions["pool"].numel()
    print("FIGURE %s imposed decisions: %d of %d ReLU (worst at %.2e x RMS), %d of %d max-pool (worst %.2e x RMS)" % (
        tag, imposed.relu_flips, n_relu, imposed.relu_flip_worst, imposed.pool_flips, n_pool, imposed.pool_flip_worst))
    assert imposed.relu_flips <= max(FLIP_MAX_FRACTION * n_relu, 2) and imposed.pool_flips <= max(FLIP_MAX_FRACTION * n_pool, 2), tag
    errs = []
    for n, r in g64f.items():
        if r is None:
            assert gpu[n] is None, n
            continue
        assert gpu[n] is not None, "%s: missing gradient" % n
        errs.append((rel_l2(gpu[n], r), rel_l2(g32[n], g64[n]), n))
    errs.sort(reverse=True)
    med = sorted(e for e, _, _ in errs)[len(errs) // 2]
    print("FIGURE %s gradients vs float64 under the engine's decisions: max %.2e (%s; the CPU float32 oracle's own error there %.2e), "
          "median %.2e over %d tensors (bounds %.0e / %.0e)" % (tag, errs[0][0], errs[0][2], errs[0][1], med, len(errs), FORCED_MAX_ERR,
                                                                FORCED_MEDIAN_ERR))
    for e, e32, n in errs[:5]:
        print("FIGURE %s   %s gpu %.2e cpu32 %.2e" % (tag, n, e, e32))
    assert errs[0][0] <= FORCED_MAX_ERR, (tag, errs[:3])
    assert med <= FORCED_MEDIAN_ERR, (tag, med)


@pytest.mark.parametrize("Bn,Hn,Wn", [(2, 64, 64), (2, 96, 128)])
def test_frozen_statistics_against_the_eval_mode_oracle(Bn, Hn, Wn):
    _frozen_stats_case(Bn, Hn, Wn)


def test_frozen_statistics_against_the_eval_mode_oracle_fp16_pair():
    """the same case at 2x64x64 in a fresh process with the fp16-pair operand format (fixed when the engine module is imported)"""
    from footprints_amd._format import format_env
    env = dict(os.environ)
    env.update(format_env("fp16_pair"))
    r = subprocess.run([sys.executable, "-m", "tests.test_gpu_finetune", "2", "64", "64"], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=600)
    print(r.stdout[-4000:])
    assert r.returncode == 0, (r.stderr or r.stdout)[-4000:]
    assert "fp16_pair" in r.stdout


# ---- 4. mixed BatchNorm modes ----------------------------------------------------------------------------------------------------------
def test_mixed_batchnorm_modes_raise_and_the_flag_is_sticky():
    from oracle import restatement as R
    P, B = R.make_state(tag="ft4")
    img = R.make_batch(2, 64, 64, tag="ft4")["image"].cuda()
    model = _mm(P, B).model
    model.train()
    model.encoder.layer2[1].bn1.eval()
    with pytest.raises(RuntimeError, match=r"encoder\.layer\d.*train mode.*encoder\.layer2\.1\.bn1 in eval mode"):
        model(img)
    with pytest.raises(RuntimeError, match="mixed modes"), torch.no_grad():
        model(img)
    model.train()
    model.freeze_bn_stats()
    model.eval()
    model.train()
    eng = model.engine()
    assert eng.bn_training() is False and model.training
    model.freeze_bn_stats(False)
    assert eng.bn_training() is True
    model.encoder.eval()                        # the plain PyTorch idiom
    assert eng.bn_training() is False
    model.train()
    assert eng.bn_training() is True


# ---- 5. frozen encoder with frozen statistics: the BN-folded forward ---------------------------------------------------------------------
def test_frozen_encoder_with_frozen_statistics_takes_the_folded_forward():
    from oracle import restatement as R
    from tests import finetune_refs as FR
    from tests.parity import FORCED_MAX_ERR, FORCED_MEDIAN_ERR, rel_l2, tie_free_batch
    from tests.test_gpu_network import relerr
    P, B = R.make_state(tag="ft5")
    cpu_batch = R.make_batch(2, 64, 64, tag="ft5")
    outs = {}
    for fold in (True, False):
        mm = _mm(P, B)
        model, eng = mm.model, mm.model.engine()
        model.freeze(("encoder",))
        model.freeze_bn_stats()
        model.train()
        eng.fold_eval = fold
        calls = _hooked(eng)
        assert not eng._fold_ready
        out = model(cpu_batch["image"].cuda())
        torch.cuda.synchronize()
        assert eng._fold_ready == fold and (eng.saved["blocks"] == []) == fold
        feats = [f.detach().permute(0, 3, 1, 2).contiguous().cpu() for f in eng.saved["feats"]]
        _, out64 = FR.decoder_grads64(P, feats, cpu_batch, grads=False)
        fixed = tie_free_batch(cpu_batch, out64)[0]
        g64, _ = FR.decoder_grads64(P, feats, fixed)
        losses = _lm()(out, {k: v.cuda() for k, v in fixed.items()})
        model.zero_grad()
        losses["loss"].backward()
        torch.cuda.synchronize()
        assert calls == []
        gpu = _grads(model)
        assert all(gpu[n] is None for n in gpu if n.startswith("encoder"))
        errs = sorted(((rel_l2(gpu[n], r), n) for n, r in g64.items()), reverse=True)
        med = sorted(e for e, _ in errs)[len(errs) // 2]
        print("FIGURE folded=%d decoder gradients vs float64 on the engine's features: max %.2e (%s), median %.2e" % (fold, errs[0][0], errs[0][1], med))
        assert errs[0][0] <= FORCED_MAX_ERR and med <= FORCED_MEDIAN_ERR, errs[:3]
        mm.optimiser.step()                      # the fold survives the decoders' update: nothing of the encoder was written
        if fold:
            model(cpu_batch["image"].cuda())
            assert eng._fold_ready
        for k, v in model.state_dict().items():
            if k.startswith("encoder"):
                assert torch.equal(v.cpu(), {**P, **B}[k]), k
        outs[fold] = OrderedDict((k, v.detach().cpu()) for k, v in out.items())
    for k in outs[True]:
        e = relerr(outs[True][k], outs[False][k])
        print("FIGURE folded vs unfolded output %s: %.2e (bound 2e-5)" % (k, e))
        assert e <= 2e-5, (k, e)


# ---- 6. TrainStep ------------------------------------------------------------------------------------------------------------------------
def _configure(model, variant):
    if variant in ("encoder", "stats+encoder"):
        model.freeze(("encoder",))
    if variant == "prefix":
        model.freeze(LOW)
    if variant in ("stats", "stats+encoder"):
        model.freeze_bn_stats()
    model.train()


def _trainable_flat(eng):
    return torch.cat([eng.flat_grad[lo:hi] for lo, hi in eng.adam_ranges]).clone()


def _opt_state(opt):
    return OrderedDict((i, (float(s["step"]), s["exp_avg"].clone(), s["exp_avg_sq"].clone())) for i, s in opt.state_dict()["state"].items())


def _same_opt_state(a, b, what):
    assert a.keys() == b.keys(), what
    for i in a:
        assert a[i][0] == b[i][0] and torch.equal(a[i][1], b[i][1]) and torch.equal(a[i][2], b[i][2]), (what, i)


@pytest.mark.parametrize("variant", ["encoder", "prefix", "stats", "stats+encoder"])
def test_trainstep_plan_eager_and_dropin_agree(variant):
    from footprints_amd.training.train import TrainStep
    from oracle import restatement as R
    P, B = R.make_state(tag="ft6")
    batch = {k: v.cuda().contiguous() for k, v in R.make_batch(2, 64, 64, tag="ft6").items()}
    mms = [_mm(P, B) for _ in range(3)]
    for mm in mms:
        _configure(mm.model, variant)
    plan, eager, drop = mms
    tp, te = TrainStep(plan.model, plan.optimiser, plan=True), TrainStep(eager.model, eager.optimiser, plan=False)
    lm = _lm()
    for step in range(6):                       # plan=True: two eager steps, one recording step, then replays
        lp, le = tp(batch).clone(), te(batch).clone()
        ld = _dropin(drop, batch, lm)
        torch.cuda.synchronize()
        assert torch.equal(lp, le), (variant, step)
        assert torch.equal(lp[20], ld), (variant, step)
        gp, ge, gd = (_trainable_flat(m.model.engine()) for m in mms)
        assert torch.equal(gp, ge) and torch.equal(gp, gd), (variant, step)
    assert len(tp._plans) == 1 and not te._plans
    frozen = {"encoder": ("encoder",), "prefix": LOW, "stats": (), "stats+encoder": ("encoder",)}[variant]
    sp, se, sd = (_state(m.model) for m in mms)
    for k in sp:
        assert torch.equal(sp[k], se[k]) and torch.equal(sp[k], sd[k]), (variant, k)
        if (frozen and k.startswith(frozen)) and k in P:
            assert torch.equal(sp[k].cpu(), P[k]), "%s: frozen tensor %s was written" % (variant, k)
        if "stats" in variant and _is_buffer(k):
            assert torch.equal(sp[k].cpu(), B[k]), "%s: %s was written" % (variant, k)
    op, oe, od = (_opt_state(m.optimiser) for m in mms)
    _same_opt_state(op, oe, variant + " plan / eager")
    _same_opt_state(op, od, variant + " plan / drop-in")
    # the frozen set is fixed by the optimiser's first step
    p = plan.model.mask_decoder.block1.pre_concat_conv.conv1.weight
    p.requires_grad_(False)
    with pytest.raises(RuntimeError, match="frozen parameters changed"):
        tp(batch)
    p.requires_grad_(True)
    # the BatchNorm mode may change at any time: the plans go, and the next steps are the eager run's
    for mm in (plan, eager):
        mm.model.freeze_bn_stats("stats" not in variant)
    for step in range(4):
        lp, le = tp(batch).clone(), te(batch).clone()
        torch.cuda.synchronize()
        assert torch.equal(lp, le), (variant, "after the toggle", step)
        assert len(tp._plans) == (1 if step >= 2 else 0), (variant, step, len(tp._plans))
    sp, se = _state(plan.model), _state(eager.model)
    for k in sp:
        assert torch.equal(sp[k], se[k]), (variant, "after the toggle", k)


def test_trainstep_graph_replay_with_a_frozen_prefix():
    """the opt-in hipGraph replay (TrainStep(graph=True)) captures the ranged Adam update and the shortened backward: same losses,
    trainable gradients and state as the eager schedule, frozen tensors untouched"""
    from footprints_amd.training.train import TrainStep
    from oracle import restatement as R
    P, B = R.make_state(tag="ft6g")
    batch = {k: v.cuda().contiguous() for k, v in R.make_batch(2, 64, 64, tag="ft6g").items()}
    res = []
    for graph in (False, True):
        mm = _mm(P, B)
        _configure(mm.model, "prefix")
        mm.model.freeze_bn_stats()
        ts = TrainStep(mm.model, mm.optimiser, graph=graph, plan=False)
        losses, grads = [], []
        for _ in range(5):                                       # graph mode: 2 eager + capture + 2 replays
            losses.append(ts(batch).clone())
            grads.append(_trainable_flat(ts.eng))
        assert (ts._graph is not None) == graph
        res.append((losses, grads, _state(mm.model), _opt_state(mm.optimiser)))
    for a, b in zip(res[0][0] + res[0][1], res[1][0] + res[1][1]):
        assert torch.equal(a, b)
    for k in res[0][2]:
        assert torch.equal(res[0][2][k], res[1][2][k]), k
        if k.startswith(LOW) and k in P:
            assert torch.equal(res[1][2][k].cpu(), P[k]), k
    _same_opt_state(res[0][3], res[1][3], "graph / eager")


# ---- 7. checkpoint round trip --------------------------------------------------------------------------------------------------------------
def test_checkpoint_round_trip_of_a_frozen_run(tmp_path):
    from footprints_amd.network import is_dead_param
    from footprints_amd.training.train import TrainStep
    from oracle import restatement as R
    P, B = R.make_state(tag="ft7")
    batch = {k: v.cuda().contiguous() for k, v in R.make_batch(2, 64, 64, tag="ft7").items()}
    mm = _mm(P, B, str(tmp_path))
    mm.model.freeze(("encoder",))
    ts = TrainStep(mm.model, mm.optimiser)
    for _ in range(2):
        ts(batch)
    mm.save_model("weights_0")
    osd = torch.load(tmp_path / "weights_0" / "optimiser.pth", map_location="cpu")
    live_dec = [n for n, _ in mm.model.named_parameters() if not n.startswith("encoder") and not is_dead_param(n)]
    assert len(osd["state"]) == len(live_dec) and len(osd["param_groups"][0]["params"]) == 268
    from footprints_amd.model_manager import ModelManager
    free, same = ModelManager(save_folder=str(tmp_path)), ModelManager(save_folder=str(tmp_path))
    same.model.freeze(("encoder",))
    for m in (free, same):
        m.load_model(str(tmp_path / "weights_0"), load_optimiser=True)
    assert free.optimiser._step == 2 and same.optimiser._step == 2
    lf = TrainStep(free.model, free.optimiser)(batch)          # all-trainable continuation of a decoder-only run: loads and steps
    assert bool(torch.isfinite(lf).all())
    ts2 = TrainStep(same.model, same.optimiser)
    for step in range(2):
        l1, l2 = ts(batch).clone(), ts2(batch).clone()
        assert torch.equal(l1, l2), step
    for (k, va), vb in zip(mm.model.state_dict().items(), same.model.state_dict().values()):
        assert torch.equal(va, vb), k
    _same_opt_state(_opt_state(mm.optimiser), _opt_state(same.optimiser), "continued run")


# ---- the segmentation network shares the engine ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frozen", [("encoder",), ("decoder.PSP",), ("encoder.layer0", "encoder.layer1", "decoder.outconv1")])
def test_segmentor_frozen_parameters(frozen):
    """Segmentor with pyramid pooling, drop-in surface: trainable gradients bit-equal to the unfrozen run's, frozen tensors without .grad and
    unchanged by the optimiser -- a frozen encoder, frozen PSP convolutions under a trainable encoder, and a frozen 1-channel head"""
    from footprints_amd.optim import FusedAdam
    from footprints_amd.preprocessing.segmentation.network import Segmentor
    from oracle import filler, restatement as R
    B, H, W = 2, 64, 96
    image = torch.from_numpy(filler.uniform("ftseg:image", (B, 3, H, W))).cuda()
    gmask = torch.from_numpy(filler.bernoulli("ftseg:gmask", (B, H, W), 0.4)).cuda()
    lmask = torch.from_numpy(filler.bernoulli("ftseg:lmask", (B, H, W), 0.7)).cuda()
    P, Bf = R.make_seg_state(True, tag="ftseg")
    runs = []
    for prefixes in ((), frozen):
        m = Segmentor(pretrained=False, use_PSP=True)
        m.load_state_dict({**P, **Bf})
        m.cuda().train()
        if prefixes:
            m.freeze(prefixes)
        opt = FusedAdam(m, lr=1e-4)
        loss = R.seg_loss(m(image), gmask, lmask, H, W)
        loss.backward()
        grads = _grads(m)
        opt.step()
        torch.cuda.synchronize()
        runs.append((float(loss.detach()), grads, _state(m)))
    (la, ga, sa), (lb, gb, sb) = runs
    assert la == lb
    for n in ga:
        if n.startswith(frozen):
            assert gb[n] is None and torch.equal(sb[n].cpu(), P[n]), n
        else:
            assert (ga[n] is None and gb[n] is None) or torch.equal(ga[n], gb[n]), n
            assert torch.equal(sa[n], sb[n]), n


if __name__ == "__main__":                      # the fp16-pair child of case 3
    _frozen_stats_case(*(int(v) for v in sys.argv[1:4]))
