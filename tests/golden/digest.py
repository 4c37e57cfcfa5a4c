"""Compact, comparison-friendly digests of large tensors for the golden fixtures.

A tensor with <= full_limit elements is stored whole; a larger one is stored as
float64 sum, float64 abs-sum and a strided sample (stride 61, coprime to every
power-of-two / small-factor dimension in the network, so the samples walk all
channels and positions).  The same function digests oracle / HIP results in tests.
"""
import os

import numpy as np
import torch

GOLDEN_DIR = os.path.dirname(os.path.abspath(__file__))
STRIDE = 61


def fill(name, shape, lo=-1.0, hi=1.0):
    from oracle import filler
    return torch.from_numpy(filler.uniform(name, shape, lo, hi))


def fill_value(tag, key, shape, is_int=False):
    """Deterministic value for state entry `key` of a block fixture (shared by the
    generator and the tests so both sides rebuild identical weights)."""
    if is_int:
        return torch.zeros(shape, dtype=torch.int64)
    if key.endswith("running_var"):
        return fill(tag + ":" + key, shape, 0.5, 2.0)
    if key.endswith("weight") and len(shape) == 4:
        b = float(np.sqrt(3.0 / (shape[1] * shape[2] * shape[3])))
        return fill(tag + ":" + key, shape, -b, b)
    return fill(tag + ":" + key, shape, -0.3, 0.3)


def digest(name, t, full_limit=1 << 15):
    t = t.detach().cpu().contiguous()
    flat = t.reshape(-1)
    if flat.numel() <= full_limit:
        return {name: t.numpy().copy()}
    d = flat.double()
    return {name + "#sum": np.float64(d.sum().item()), name + "#abs": np.float64(d.abs().sum().item()),
            name + "#sample": flat[::STRIDE].numpy().copy(), name + "#shape": np.array(t.shape)}


def sparse_sample(t, n=512):
    """strided sample of at most `n` elements of the flattened tensor (shared by the generator and the tests)"""
    flat = t.detach().cpu().reshape(-1)
    return flat[::max(1, -(-flat.numel() // n))]


PART_LIMIT = 1 << 20               # bytes: a fixture that does not fit one file goes on in <name>.part2.npz, <name>.part3.npz, ...


def _part_path(name, k):
    return os.path.join(GOLDEN_DIR, name + (".npz" if k == 1 else ".part%d.npz" % k))


class _Parts:
    """the parts of one fixture seen as one archive (`.files`, `[name]`, like np.load's)"""

    def __init__(self, parts):
        self.parts = parts
        self.files = [f for p in parts for f in p.files]

    def __getitem__(self, key):
        for p in self.parts:
            if key in p.files:
                return p[key]
        raise KeyError(key)


def save(name, arrays):
    """np.savez_compressed of `arrays` as tests/golden/<name>.npz, split into consecutive parts when one file would reach PART_LIMIT"""
    keys = list(arrays)
    for n in range(1, len(keys) + 1):
        cut = [len(keys) * i // n for i in range(n + 1)]
        for k in range(n):
            np.savez_compressed(_part_path(name, k + 1), **{key: arrays[key] for key in keys[cut[k]:cut[k + 1]]})
        if all(os.path.getsize(_part_path(name, k + 1)) < PART_LIMIT for k in range(n)):
            break
    k = n + 1
    while os.path.exists(_part_path(name, k)):     # parts of an earlier, larger version
        os.remove(_part_path(name, k))
        k += 1
    return [_part_path(name, k + 1) for k in range(n)]


def load(name):
    parts, k = [], 1
    while k == 1 or os.path.exists(_part_path(name, k)):
        parts.append(np.load(_part_path(name, k), allow_pickle=False))
        k += 1
    return parts[0] if len(parts) == 1 else _Parts(parts)


def compare(gold, name, t, rtol=1e-4, atol_scale=1e-4):
    """Max-normalised error of tensor `t` against golden entry `name` (full or digest form).

    Returns err = max|a-b| / max|b| (tensor-scale relative error).  For digests also
    checks the float64 sum against abs-sum scale.  Asserts err <= rtol.
    """
    t = t.detach().cpu().contiguous()
    if name in gold.files:
        ref = torch.from_numpy(gold[name])
        assert tuple(ref.shape) == tuple(t.shape), (name, ref.shape, t.shape)
        scale = max(ref.abs().max().item(), 1e-30)
        err = (t.double() - ref.double()).abs().max().item() / scale
        assert err <= rtol, "%s: rel-to-max error %.3e > %.1e" % (name, err, rtol)
        return err
    shape = tuple(gold[name + "#shape"])
    assert shape == tuple(t.shape), (name, shape, t.shape)
    ref = torch.from_numpy(gold[name + "#sample"])
    got = t.reshape(-1)[::STRIDE]
    scale = max(ref.abs().max().item(), 1e-30)
    err = (got.double() - ref.double()).abs().max().item() / scale
    assert err <= rtol, "%s: sample rel-to-max error %.3e > %.1e" % (name, err, rtol)
    s_ref, a_ref = float(gold[name + "#sum"]), float(gold[name + "#abs"])
    s = t.double().sum().item()
    serr = abs(s - s_ref) / max(a_ref, 1e-30)
    assert serr <= atol_scale, "%s: sum error %.3e (abs-sum scale)" % (name, serr)
    return err
