"""CPU: the pure layout planner (footprints_amd/weight_layouts.py) reproduces, for every convolution, where each packed copy lay in
Engine.packed and what the four pack tables held before the table existed.

tests/golden/weight_layouts.json was dumped from the engine of the commit before the planner (one fresh Engine per configuration on the
device): per convolution its facts and {"role.format": [offset in Engine.packed (-1: a buffer of its own), numel]}, and the four pack tables
(stem + layer1 / rest / rest forward / rest data gradient) as [kind, destination offset, c_begin, c_count, has an amax slot] -- in full for
FootprintNetwork in both operand formats (also with the two-term inference mode on), as digests per convolution / per table for
FP_NO_PHASE=1, FP_NO_BF3=1, FP_PACK_LAZY32=0 and the pyramid-pooling Segmentor.  The planner only uses the library's host-side size
queries, so this runs without a device.

Two things the fixture and this test are NOT.  The `up2` fact is structural -- (C0, C1) of every conv fed by cat[nearest_x2(low), skip],
derived from the conv's name when the fixture was written -- while the engine leaves ConvRec.up2 unset with FP_NO_PHASE=1: in that
configuration the test reaches `plan` with up2 set and the phase switch off, a combination the engine never produces (both give the same
layouts).  And `_planned` below restates the engine's side of the pack tables (first / rest / forward / data-gradient split, the lazy
filter of a fresh engine, which jobs carry an amax slot): Engine.refresh_packed itself needs a device and is covered by the GPU suite only
(tests/test_gpu_switches.py: FP_PACK_LAZY32, FP_PACK_DGRAD_LATE, both operand formats)."""
import hashlib
import json
import os

import pytest

from footprints_amd import _lib as L
from footprints_amd import weight_layouts as WL

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "weight_layouts.json")) as _f:
    GOLD = json.load(_f)
KIND = {getattr(L, n): n for n in dir(L) if n.startswith("PACK_")}
TABLES = ("stem + layer1", "rest", "rest, forward", "rest, data gradient")


def _sha(x):
    return hashlib.sha256(json.dumps(x, sort_keys=True, separators=(",", ":")).encode()).hexdigest()[:16]


def _planned(cfg, two_term=False):
    """-> ([{role.format: [offset, numel]} per conv], the four tables) as the planner lays them out"""
    fl = WL.Flags(**{k: cfg["flags"][k] for k in WL.Flags._fields})
    where, tables, o = [], [[], [], [], []], 0
    for c in cfg["convs"]:
        f = WL.Facts(**{**c["facts"], "up2": tuple(c["facts"]["up2"]) if c["facts"]["up2"] else None})
        pairs = []
        for l in WL.plan(f, fl):
            pairs.append((l, [o if l.pooled else -1, l.numel]))
            o += l.numel if l.pooled else 0
        where.append({"%s.%s" % (l.role, l.fmt): w for l, w in pairs})
        for l, w in WL.pack_jobs(pairs, WL.classify(f, fl)[1], cfg["flags"]["hp_tile"], two_term):
            if l.lazy and cfg["flags"]["lazy32"]:
                continue                         # a fresh engine: no launch has read an fp32 layout yet
            job = [KIND[l.kind], w[0], l.c_begin, l.c_count, l.fmt == "hp"]
            for t in ([0] if c["first"] else [1, 3 if l.role.endswith("dgrad") else 2]):
                tables[t].append(job)
    return where, tables, o


@pytest.mark.parametrize("name", sorted(GOLD))
def test_planner_reproduces_the_recorded_layouts(name):
    cfg = GOLD[name]
    where, _, total = _planned(cfg)
    for c, got in zip(cfg["convs"], where):
        if isinstance(c["lay"], str):
            assert _sha(got) == c["lay"], (name, c["name"], got)
            continue
        for key in sorted(set(got) | set(c["lay"])):
            assert got.get(key) == c["lay"].get(key), (name, c["name"], key, got.get(key), c["lay"].get(key))
    assert total == cfg["total"], (name, total, cfg["total"])


@pytest.mark.parametrize("name,key", [(n, k) for n in sorted(GOLD) for k in ("tables", "tables_bf16x2") if k in GOLD[n]])
def test_planner_reproduces_the_recorded_pack_tables(name, key):
    cfg = GOLD[name]
    _, tables, _ = _planned(cfg, two_term=key == "tables_bf16x2")
    by_offset = {tuple(w): (c["name"], k) for c in cfg["convs"] if not isinstance(c["lay"], str) for k, w in c["lay"].items()}
    for title, got, want in zip(TABLES, tables, cfg[key]):
        if isinstance(want, str):
            assert _sha(got) == want, (name, key, title, len(got))
            continue
        for i, (a, b) in enumerate(zip(got, want)):
            who = next((v for (off, _), v in by_offset.items() if off == b[1]), None)
            assert a == b, (name, key, title, "job %d" % i, who, a, b)
        assert len(got) == len(want), (name, key, title, len(got), len(want))
