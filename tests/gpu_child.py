"""One train-mode forward + loss + backward of the HIP engine in a CHOSEN operand format (test infrastructure).

The operand format (footprints_amd/_format.py: exact bf16x3 split = default, scaled fp16 pairs = opt-in) is fixed when footprints_amd.engine is
imported, so the format the test session itself runs in executes in-process and the other one in a child process:
`gpu_step(P, B, cpu_batch, fmt)` hides the difference and returns plain CPU tensors either way --

    out        {scale: [B,4,H,W]}            the network outputs (network.py:26-30)
    losses     {key: float}                  the 21 scalars of LossManager (training/losses.py:31-92)
    grads      {name: tensor | None}         d loss / d parameter
    decisions  {"relu": [33 bool NCHW masks], the engine's discrete decisions: ReLU masks (stem, then (bn1's ReLU, block output) per BasicBlock) and the
                "pool": int64 [N,64,OH,OW]}  max-pool's winning window positions -- what tests/parity.py imposes on the float64 oracle to separate
                                             decisions from arithmetic
    state      {key: tensor}                 state_dict after the step (BatchNorm running statistics)
    taps       {name: tensor}                (tap_block = i) g / d out / z2 / out of encoder block i, see test_gpu_parity_fullsize.py
    format     str                           what the engine that ran really used
    train      {...}                         (train_steps = K > 0) K TrainSteps of a fresh model on the same state and batch (with the
                                             default launch plan: 2 eager steps, 1 recording step, then replays) -- digests, not buffers:
        losses      [K x 21 floats]
        grads       [K x {name: sha256}]     each live parameter's slice of the engine's flat gradient buffer after the step
        state       {key: sha256}            model.state_dict() after the last step (parameters and BatchNorm statistics)
        exp_avg, exp_avg_sq {name: sha256}   the optimiser's moments after the last step
    grad_sha   {name: sha256}                the drop-in step's gradients in the same form as train["grads"][i]
    legacy_losses [4 x 21 floats]            (train_steps > 0) four TrainSteps from the seeded default initialisation on a synthetic 2x128x192 batch

`gpu_step(..., env=...)` always runs in a child: every switch of the table in tests/test_gpu_switches.py (and the two spellings of the
operand format) is removed from the child's environment first, then `env` applied -- so that a stray variable of the parent cannot leak
into a run; the format is then whatever `env` selects.  A child that dies by a signal or an abort stops every later child of the session
(test runs never start programs on a GPU that may just have faulted).
"""
import hashlib
import os
import subprocess
import sys
import tempfile
from collections import OrderedDict

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _nchw_mask(t):
    return (t > 0).permute(0, 3, 1, 2).contiguous().cpu()


def engine_decisions(eng):
    """the discrete decisions of the engine's last train-mode forward (call before backward): {"relu": 33 bool NCHW masks, "pool": winners}"""
    S = eng.saved
    relu = [_nchw_mask(S["feats"][0])]
    for Bk in S["blocks"]:
        relu += [_nchw_mask(Bk["a1"]), _nchw_mask(Bk["out"])]
    f0 = S["feats"][0]
    hp, wp = (f0.shape[1] + 1) // 2, (f0.shape[2] + 1) // 2
    am = eng._bufs["pool.argmax"][:f0.shape[0] * hp * wp * 64].view(f0.shape[0], hp, wp, 64)          # uint8 ky * 3 + kx (csrc/bn_pool.hip maxpool_fwd_kernel)
    return {"relu": relu, "pool": am.permute(0, 3, 1, 2).contiguous().cpu().to(torch.int64)}


def _step_here(P, B, cpu_batch, tap_block=None, train_steps=0):
    from footprints_amd import FootprintNetwork
    from footprints_amd._format import operand_format
    from footprints_amd.training.losses import LossManager
    model = FootprintNetwork(pretrained=False)
    model.load_state_dict({**P, **B})
    model.cuda().train()
    eng = model.engine()
    taps = {}
    if tap_block is not None:
        def hook(i, d):
            if i == tap_block:
                taps.update(dout=d["dout"].detach().cpu(), g=d["g"].detach().cpu(), z2=d["B"]["z2"].detach().cpu(), out=d["B"]["out"].detach().cpu())
        eng.debug_hook = hook
    batch = {k: v.cuda() for k, v in cpu_batch.items()}
    out = model(batch["image"])
    torch.cuda.synchronize()
    decisions = engine_decisions(eng)
    losses = LossManager((0.1, 100), 0.25, compute_viz=False)(out, batch)
    losses["loss"].backward()
    torch.cuda.synchronize()
    grad_sha = flat_digests(eng.flat_grad, eng)
    res = {"out": OrderedDict((k, v.detach().cpu()) for k, v in out.items()),
           "losses": OrderedDict((k, float(v)) for k, v in losses.items()),
           "grads": OrderedDict((n, None if p.grad is None else p.grad.detach().cpu()) for n, p in model.named_parameters()),
           "decisions": decisions,
           "state": OrderedDict((k, v.detach().cpu()) for k, v in model.state_dict().items()),
           "taps": taps, "format": operand_format(), "grad_sha": grad_sha}
    eng.debug_hook = None
    del model, eng, out, losses, batch
    torch.cuda.empty_cache()
    if train_steps:
        res["train"] = _train_leg(P, B, cpu_batch, train_steps)
        res["legacy_losses"] = _legacy_leg()
    return res


def _legacy_leg(steps=4):
    """the switch sweep's original run: four TrainSteps from the seeded default initialisation on a small synthetic batch -> [steps x 21]"""
    from footprints_amd.model_manager import ModelManager
    from footprints_amd.training.train import SEED, TrainStep, synthetic_batch
    torch.manual_seed(SEED)
    mm = ModelManager(use_cuda=True)
    ts = TrainStep(mm.model, mm.optimiser)
    batch = synthetic_batch(2, 128, 192, "cuda")
    out = []
    for _ in range(steps):
        ts(batch)
        out.append([float(v) for v in ts.losses.cpu()])
    del mm, ts, batch
    torch.cuda.empty_cache()
    return out


def _sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def flat_digests(flat, eng):
    """{live parameter name: sha256 of its slice of a flat buffer laid out like eng.flat_param}"""
    flat = flat.detach().cpu()
    return OrderedDict((n, _sha(flat[o:o + p.numel()])) for n, p, o in zip(eng.live_names, eng.live_params, eng.offsets))


def _train_leg(P, B, cpu_batch, steps):
    from footprints_amd.model_manager import ModelManager
    from footprints_amd.training.train import TrainStep
    mm = ModelManager(use_cuda=True)
    mm.model.load_state_dict({**P, **B})
    ts = TrainStep(mm.model, mm.optimiser)
    eng = ts.eng
    batch = {k: v.cuda().contiguous() for k, v in cpu_batch.items()}
    losses, grads = [], []
    for _ in range(steps):
        lv = ts(batch)
        torch.cuda.synchronize()
        losses.append([float(v) for v in lv.cpu()])
        grads.append(flat_digests(eng.flat_grad, eng))
    m, v = mm.optimiser._buffers(eng)
    res = {"losses": losses, "grads": grads, "plans": len(ts._plans),
           "state": OrderedDict((k, _sha(t)) for k, t in mm.model.state_dict().items()),
           "exp_avg": flat_digests(m, eng), "exp_avg_sq": flat_digests(v, eng)}
    del mm, ts, eng, batch
    torch.cuda.empty_cache()
    return res


_CRASHED = []          # children of this session that died by a signal / abort / time limit


def gpu_step(P, B, cpu_batch, fmt=None, tap_block=None, env=None, train_steps=0):
    """fmt: the operand format to run in (None: the one `env` selects); env (optional): switches of the run -- see the module docstring"""
    from footprints_amd._format import format_env, operand_format
    if env is None:
        if fmt == operand_format() and not train_steps:
            return _step_here(P, B, cpu_batch, tap_block)
        child_env = dict(os.environ)
        child_env.update(format_env(fmt))
    else:
        from tests.test_gpu_switches import swept_switches
        child_env = {k: v for k, v in os.environ.items() if k not in swept_switches() | {"FP_OPERANDS", "FP_HP"}}
        child_env.update(env)
        fmt = operand_format(child_env) if fmt is None else fmt
    assert not _CRASHED, "not started: an earlier child engine of this session died (%s)" % _CRASHED[0]
    with tempfile.TemporaryDirectory(prefix="fp_gpu_child_") as tmp:
        src, dst = os.path.join(tmp, "in.pt"), os.path.join(tmp, "out.pt")
        torch.save({"P": P, "B": B, "batch": cpu_batch, "tap_block": tap_block, "train_steps": train_steps}, src)
        try:
            r = subprocess.run([sys.executable, "-m", "tests.gpu_child", src, dst], cwd=ROOT, env=child_env, capture_output=True, text=True,
                               timeout=1200)
        except subprocess.TimeoutExpired:
            _CRASHED.append("%s %s: time limit" % (fmt, env))
            raise
        if r.returncode < 0 or r.returncode in (134, 137, 139):
            _CRASHED.append("%s %s: exit status %d" % (fmt, env, r.returncode))
        assert r.returncode == 0, "child engine (%s, %s) failed:\n%s" % (fmt, env, (r.stderr or r.stdout)[-3000:])
        res = torch.load(dst, weights_only=False)
    assert res["format"] == fmt, (res["format"], fmt)
    return res


if __name__ == "__main__":
    job = torch.load(sys.argv[1], weights_only=False)
    torch.save(_step_here(job["P"], job["B"], job["batch"], job["tap_block"], job.get("train_steps", 0)), sys.argv[2])
