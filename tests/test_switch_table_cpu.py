"""CPU: (1) the tripwire of the switch table -- every FP_* environment variable the package (Python) or its library (C / HIP) reads is swept by
tests/test_gpu_switches.py or exempt there with a reason, and no entry of the table names a switch that no longer exists; (2) why the switch
cases compare gradients: a gradient scaled by 1.01 fails the fp64-anchored rule of tests/parity.py on exactly that tensor, while three Adam
steps with it move the parameters -- and the losses -- by far less than a 1e-4 loss tolerance can see."""
import glob
import os
import re
from collections import OrderedDict

import torch

from tests import test_gpu_switches as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "footprints_amd")
_PY_READ = re.compile(r"""(?:environ|env)\.get\(\s*["'](FP_[A-Za-z0-9_]+)["']|environ\[\s*["'](FP_[A-Za-z0-9_]+)["']\s*\]|getenv\(\s*["'](FP_[A-Za-z0-9_]+)["']""")
_C_READ = re.compile(r"""(?:getenv|fp_env_flag)\(\s*"(FP_[A-Za-z0-9_]+)"\s*\)""")


def switches_read(pkg=PKG):
    """{name: [files]} of the FP_* variables read by footprints_amd/**/*.py (os.environ.get / [] / getenv; `env.get` in _format.py) and footprints_amd/csrc/*
    (getenv, fp_env_flag)"""
    found = {}
    for path in glob.glob(os.path.join(pkg, "**", "*.py"), recursive=True):
        for m in _PY_READ.finditer(open(path).read()):
            found.setdefault(next(g for g in m.groups() if g), []).append(os.path.relpath(path, pkg))
    for path in glob.glob(os.path.join(pkg, "csrc", "*")):
        if os.path.isfile(path):
            for m in _C_READ.finditer(open(path, errors="replace").read()):
                found.setdefault(m.group(1), []).append(os.path.relpath(path, pkg))
    return found


def _exempt(name):
    return name in S.EXEMPT or any(k.endswith("*") and name.startswith(k[:-1]) for k in S.EXEMPT)


def test_the_scan_sees_both_sides():
    read = switches_read()
    assert "FP_SERIAL" in read and "FP_NO_SPLITK" in read and "FP_STREAM_LAYOUT" in read          # engine.py, ops.py (__import__ form), a default
    assert "FP_OPERANDS" in read and "FP_HP" in read                                                # _format.py reads a mapping it is given
    assert "FP_NO_TILE" in read and "FP_WGRAD_SPLIT_REDUCE" in read                                # getenv, fp_env_flag in csrc/


def test_every_switch_is_swept_or_exempt():
    read = switches_read()
    missing = sorted("%s (%s)" % (n, ", ".join(sorted(set(f)))) for n, f in read.items() if n not in S.swept_switches() and not _exempt(n))
    assert not missing, "FP_* switches read by the package but neither swept by tests/test_gpu_switches.py nor in its EXEMPT: %s" % missing


def test_no_table_entry_names_a_dead_switch():
    read = set(switches_read())
    dead = sorted(n for n in S.swept_switches() if n not in read)
    dead += sorted(k for k in S.EXEMPT if not (any(n.startswith(k[:-1]) for n in read) if k.endswith("*") else k in read))
    assert not dead, "switch table entries that nothing reads any more: %s" % dead
    assert all(isinstance(r, str) and r.strip() for r in S.EXEMPT.values())
    assert not (S.swept_switches() - {"FP_OPERANDS", "FP_HP"}) & set(S.EXEMPT), "a switch is both swept and exempt"


def test_switch_table_shape():
    keys = [S._key(env) for env, _, _ in S.SWITCH_CASES]
    assert len(keys) == len(set(keys)), "a case appears twice"
    for env, ref, exact in S.SWITCH_CASES:
        assert env and isinstance(exact, bool) and ref in ({}, S.PAIR)
        assert all(k.startswith("FP_") and isinstance(v, str) for k, v in env.items())
    for env, _, _ in S.SWITCH_CASES:                  # at most three side streams: the engine's streams stay within four hardware queues
        if "FP_STREAM_LAYOUT" in env:
            assert max(int(v) for v in env["FP_STREAM_LAYOUT"].split(",")) <= 2


def test_the_tripwire_fires_on_a_new_switch(tmp_path):
    """a copy of the package with one more os.environ.get("FP_...") in engine.py: the scan reports it, the table does not cover it"""
    pkg = tmp_path / "footprints_amd"
    (pkg / "csrc").mkdir(parents=True)
    src = open(os.path.join(PKG, "engine.py")).read()
    (pkg / "engine.py").write_text(src + '\n_FOO = bool(int(os.environ.get("FP_FOO", "0")))\n')
    (pkg / "csrc" / "x.hip").write_text('static const bool b = fp_env_flag("FP_BAR");\n')
    read = switches_read(str(pkg))
    assert set(read["FP_FOO"]) == {"engine.py"} and read["FP_BAR"] == [os.path.join("csrc", "x.hip")]
    assert not _exempt("FP_FOO") and "FP_FOO" not in S.swept_switches()


def test_a_scaled_gradient_fails_the_anchored_rule_but_not_a_loss_comparison_after_adam():
    from oracle import restatement as R
    from tests.parity import anchored_gradient_failures, oracle_grads
    P, B = R.make_state(tag="teeth")
    batch = R.make_batch(1, 64, 96, tag="teeth")
    dec64, dec32 = R.ReluDecisions(), R.ReluDecisions()
    _, l64, g64, _, _ = oracle_grads(P, B, batch, torch.float64, relu_decisions=dec64)
    _, _, g32, _, _ = oracle_grads(P, B, batch, torch.float32, relu_decisions=dec32)
    decisions = {"relu": dec32.taken}
    # the fp32 oracle as "the engine": it passes, exactly as it is
    assert anchored_gradient_failures(P, B, batch, decisions, dec64.taken, g32, g32, g64, "fp32 oracle") == []
    name = "depth_decoder.block1.post_concat_conv.conv1.weight"
    wrong = OrderedDict((n, None if g is None else (g * 1.01 if n == name else g.clone())) for n, g in g32.items())
    bad = anchored_gradient_failures(P, B, batch, decisions, dec64.taken, wrong, g32, g64, "1.01x " + name)
    assert bad and {b.split(" ")[0] for b in bad} == {name}, bad

    # ... while three Adam steps (lr 1e-4, the reference's optimiser) with the right and the 1.01x gradient end within round-off of each other
    p0 = P[name].double()
    moved = []
    for scale in (1.0, 1.01):
        p = torch.nn.Parameter(p0.clone())
        opt = torch.optim.Adam([p], lr=1e-4)
        for _ in range(3):
            p.grad = g64[name].double() * scale
            opt.step()
        moved.append(p.detach())
    step = (moved[0] - p0).abs().mean().item()
    diff = (moved[1] - moved[0]).abs().max().item()
    assert step > 1e-4 and diff < 1e-2 * step, (step, diff)            # measured: 3e-4 and 7e-7
    # ... and the losses of the next forward pass with either set of parameters agree far inside the old 1e-4 loss tolerance
    losses = []
    for p in moved:
        Pd = OrderedDict((k, v.double()) for k, v in P.items())
        Pd[name] = p
        Bd = OrderedDict((k, v.double() if v.is_floating_point() else v.clone()) for k, v in B.items())
        with torch.no_grad():
            out = R.footprint_network(batch["image"].double(), Pd, Bd, True)
            losses.append(R.loss_manager(out, OrderedDict((k, v.double()) for k, v in batch.items()))[0])
    worst = max(abs(float(losses[1][k]) - float(losses[0][k])) / max(abs(float(losses[0][k])), 1e-3) for k in R.LOSS_KEYS)
    assert worst < 1e-6, worst
