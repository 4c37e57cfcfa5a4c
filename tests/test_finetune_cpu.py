"""CPU: the references of the fine-tuning tests check themselves (tests/finetune_refs.py) -- the frozen-statistics BatchNorm backward is
torch.autograd's, its bounds can see one dropped row, and the optimiser's ranges cover exactly the trainable slots of the flat buffers."""
import random

import pytest
import torch

from tests import finetune_refs as FR
from tests import launch_regimes as LR

# the kernel shapes of tests/test_gpu_finetune_kernels.py (N, H, W, C): both rows-per-workgroup layouts (C = 64: R = 16, C = 512: R = 2),
# M no multiple of R; one M below a workgroup's rows, one that reaches the capped grid with the row loop going round more than once
CAP = LR.bn_blocks(1 << 30, 64)            # the launcher's grid cap, as tests/launch_regimes.py restates it (512)
KERNEL_SHAPES = [(1, 3, 3, 64), (1, 1, 1, 512), (1, 7, 11, 64), (1, 5, 7, 512), (1, 1, 16 * 4 * CAP * 2 + 5, 64), (1, 1, 2 * 4 * CAP * 2 + 3, 512)]


def test_kernel_shapes_reach_the_regimes_they_claim():
    seen = set()
    for shape in KERNEL_SHAPES:
        N, H, W, C = shape
        M, R = N * H * W, 256 // (C // 4)
        nblk = LR.bn_blocks(M, C)
        assert M % R != 0, shape
        capped = LR.ceil_div(M, R * 4) > CAP
        loops = LR.ceil_div(M, nblk * R) > 1
        seen.add((R, "small" if M < R else ("capped+loop" if capped and loops else "one pass" if not loops else "loop")))
        assert nblk <= CAP
    for R in (16, 2):
        assert (R, "small") in seen and (R, "capped+loop") in seen, seen


@pytest.mark.parametrize("shape", [(1, 7, 11, 64), (1, 5, 7, 512)])
def test_frozen_bn_backward_formulas_are_autograds(shape):
    """dz, dgamma, dbeta of relu(batch_norm(training=False)) in float64 == the reference formulas evaluated with the same float64
    statistics (the GPU tests evaluate them with the float32 statistics the kernel is handed)"""
    inp = FR.bn_inputs(shape)
    auto, y, invstd64 = FR.frozen_bn_autograd(inp)
    assert 0.05 < float((y > 0).double().mean()) < 0.95          # the mask is neither empty nor full
    ref, _ = FR.frozen_bn_bwd_ref(inp, True, mean=inp["rm"].double(), invstd=invstd64, ro=y)
    for k in ("dz", "dgamma", "dbeta"):
        err = float((auto[k] - ref[k]).abs().max() / ref[k].abs().max())
        assert err < 1e-13, (k, err)
    # without the mask: plain batch_norm
    z = inp["z"].double().requires_grad_(True)
    g = inp["gamma"].double().requires_grad_(True)
    b = inp["beta"].double().requires_grad_(True)
    out = torch.nn.functional.batch_norm(z, inp["rm"].double(), inp["rv"].double(), g, b, False, 0.1, FR.EPS)
    dz, dg, db = torch.autograd.grad(out, (z, g, b), inp["dy"].double())
    ref, _ = FR.frozen_bn_bwd_ref(inp, False, mean=inp["rm"].double(), invstd=invstd64)
    for k, v in (("dz", dz), ("dgamma", dg), ("dbeta", db)):
        assert float((v - ref[k]).abs().max() / ref[k].abs().max()) < 1e-13, k


@pytest.mark.parametrize("shape", KERNEL_SHAPES)
@pytest.mark.parametrize("relu_out", [True, False])
def test_frozen_bn_bounds_see_a_dropped_row(shape, relu_out):
    """dropping the last row moves dbeta / dgamma by more than ten times their bound, and zeroing the last row of dz shows against
    its per-element bound -- the trick of tests/test_launch_regimes_cpu.py"""
    inp = FR.bn_inputs(shape)
    M = inp["z"].shape[0]
    full, bound = FR.frozen_bn_bwd_ref(inp, relu_out)
    if M > 1:
        dropped, _ = FR.frozen_bn_bwd_ref(inp, relu_out, keep=FR.last_row_mask(M))
        for k in ("dbeta", "dgamma"):
            mv = float(((full[k] - dropped[k]).abs() / bound[k].clamp_min(1e-300)).max())
            assert mv > 10.0, "%s %s: dropping the last row moves %s by %.2f bounds" % (shape, relu_out, k, mv)
            # and the bound is small against the result it guards: well-conditioned inputs
            assert float(bound[k].max() / full[k].abs().max()) < 1e-4, k
    lost = full["dz"].clone()
    lost[M - 1] = 0
    assert FR.ratio(lost.float(), full["dz"], bound["dz"]) > 10.0
    assert FR.ratio(full["dz"].float(), full["dz"], bound["dz"]) <= 1.0       # one rounding of the exact value passes


def _check_ranges(offs, total, shapes, flags):
    ranges = FR.trainable_ranges(offs, total, flags)
    covered = torch.zeros(total, dtype=torch.bool)
    prev_hi = -1
    for lo, hi in ranges:
        assert lo % 4 == 0 and hi % 4 == 0 and lo < hi and lo > prev_hi, (lo, hi, prev_hi)      # ascending, disjoint, NOT adjacent (maximal)
        assert not bool(covered[lo:hi].any())
        covered[lo:hi] = True
        prev_hi = hi
    ends = offs[1:] + [total]
    for o, e, sh, t in zip(offs, ends, shapes, flags):
        n = 1
        for d in sh:
            n *= d
        assert bool(covered[o:o + n].all()) == t and bool(covered[o:o + n].any()) == t, (o, sh, t)      # exactly the trainable elements
        assert bool(covered[o + n:e].all()) == t or e == o + n                                       # padding goes with its slot
    return ranges


def test_trainable_ranges_on_the_real_layout():
    names, shapes = FR.live_shapes()
    assert len(names) == 196
    offs, total = FR.flat_layout(shapes)
    assert _check_ranges(offs, total, shapes, [True] * 196) == [(0, total)]
    assert _check_ranges(offs, total, shapes, [False] * 196) == []
    enc = [not n.startswith("encoder") for n in names]
    r = _check_ranges(offs, total, shapes, enc)
    assert len(r) == 1 and r[0][1] == total                       # the decoders are one contiguous tail
    rng = random.Random(7)
    for _ in range(10):
        flags = [rng.random() < 0.5 for _ in names]
        ranges = _check_ranges(offs, total, shapes, flags)
        want = sum(e - o for o, e, t in zip(offs, offs[1:] + [total], flags) if t)
        assert sum(hi - lo for lo, hi in ranges) == want          # the union = the trainable slots with their padding, nothing else


def test_layout_matches_the_module():
    """the layout the range test uses is the engine's: live parameters of the module tree in named_parameters order"""
    from footprints_amd import FootprintNetwork
    names, shapes = FR.live_shapes()
    live = FootprintNetwork(pretrained=False).live_named_parameters()
    assert [n for n, _ in live] == names and [tuple(p.shape) for _, p in live] == shapes


def test_mode_rule_and_sticky_flag_on_the_module():
    """freeze_bn_stats is sticky under train() / eval(); freeze() takes prefixes; nothing here needs a device"""
    from footprints_amd import FootprintNetwork
    m = FootprintNetwork(pretrained=False)
    bns = [x for x in m.encoder.modules() if isinstance(x, torch.nn.BatchNorm2d)]
    assert len(bns) == 36
    m.train()
    assert all(b.training for b in bns)
    m.freeze_bn_stats()
    assert not any(b.training for b in bns) and m.training
    m.eval()
    m.train()
    assert not any(b.training for b in bns) and m.mask_decoder.training
    m.freeze_bn_stats(False)
    assert all(b.training for b in bns)
    frozen = m.freeze(("encoder.layer0", "encoder.layer1"))
    assert frozen and all(n.startswith(("encoder.layer0", "encoder.layer1")) for n in frozen)
    for n, p in m.named_parameters():
        assert p.requires_grad != n.startswith(("encoder.layer0", "encoder.layer1")), n
    with pytest.raises(ValueError):
        m.freeze(("no_such_prefix",))


def test_cli_flags_are_absent_unless_given():
    from footprints_amd.options import Options
    assert "freeze" not in vars(Options().parse([])) and "freeze_bn" not in vars(Options().parse([]))
    o = Options().parse(["--freeze", "encoder", "mask_decoder.block1", "--freeze_bn"])
    assert o.freeze == ["encoder", "mask_decoder.block1"] and o.freeze_bn is True
