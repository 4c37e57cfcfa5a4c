"""GPU: the epilogues and the BatchNorm side output of the flattened convolutions (csrc/conv_igemm.hip: igemm_hp_kernel<TN, NP> behind
fp_conv_igemm_bf3 / fp_conv_igemm_hp, igemm_kernel behind fp_conv_igemm, igemm_store_tile, and the reduce launch fp_splitk_finish picks for a
split grid: splitk_reduce_kernel or splitk_reduce_stats_kernel), every launch against float64 of the same fp32 operands:

    acc (+bias) -> +addend * (mask > 0) -> * actgrad (ELU: sv > 0 ? 1 : sv + 1; ReLU: sv > 0) -> act -> + previous y

The matrix is epilogue set x geometry x operand format; the geometries are chosen so that every set meets the four grid forms of the
launcher -- unsplit, split-K without a tail (SK % 4 == 0), split-K with the tail loop of the reduce (SK % 4 != 0) and the parity-major
rows of a 3x3 stride-2 data gradient -- and a table-level test says so from a restatement of the launcher's split rule, which a second test
holds against the library (a split grid is the only one that answers an armed statistics sink).

Bounds: split operand formats relative L2 <= 1e-6 (test_gpu_hp.py's test_igemm_hp_against_float64), fp32 operands 1e-4 of the largest
element (test_gpu_kernels.TOL); every launch is repeated and must be bit-identical.  The epilogue adds at most two fp32 roundings per
element on top of the plain launch's error.

Every case prints its figure before it asserts (lines "IGEMM_EPI | format | epilogue set | geometry | form SK | error", IGEMM_RULE,
IGEMM_STATS, IGEMM_NOEMIT; run with -s to keep them).  The same matrix with a float32 CPU convolution in place of the launches gives
1e-7 ... 5e-7 relative L2 in every epilogue set, the plain convolution's own figure: the epilogue's roundings do not show at this bound."""
import itertools
import math
import os

import pytest
import torch
import torch.nn.functional as F

from tests.bn_partials_check import check_reduce_partials, reduce_geometry
from tests.test_gpu_kernels import TOL, _ops, relerr

pytestmark = pytest.mark.gpu

FORMATS = ("exact", "fp16_pair", "f32")          # fp_conv_igemm_bf3, fp_conv_igemm_hp, fp_conv_igemm
SPLIT_FORMATS = FORMATS[:2]
L2_BOUND = 1e-6

# name: (N, H, W, Cin, Cout, K, stride, mode); H x W is the forward convolution's input, mode "dgrad" = its data gradient (Nout = Cin, C0 = Cout)
GEOMS = {
    "L2 fwd": (12, 48, 160, 64, 128, 3, 2, "fwd"),            # layer 2 / 3 / 4 block 0 conv1, KITTI at batch 12
    "L3 fwd": (12, 24, 80, 128, 256, 3, 2, "fwd"),
    "L4 fwd": (12, 12, 40, 256, 512, 3, 2, "fwd"),            # 96 tiles, 144 steps: SK = 8
    "L4 1x1 fwd": (12, 12, 40, 256, 512, 1, 2, "fwd"),        # the downsample: 16 steps, SK = 2
    "80>40 fwd": (2, 18, 26, 80, 40, 3, 2, "fwd"),            # M = 234 (ragged), Nout % 32 != 0, 45 steps: SK = 5
    "36>40 fwd": (2, 10, 14, 36, 40, 3, 2, "fwd"),            # M = 70 < one tile, C0 % 16 != 0, 27 steps: SK = 3
    "4>8 1x1 fwd": (3, 7, 5, 4, 8, 1, 1, "fwd"),              # one K-step, M = 105
    "96>16 fwd": (1, 6, 10, 96, 16, 3, 2, "fwd"),             # M = 15: fewer rows than one wave, SK = 6
    "L2 dgrad": (12, 48, 160, 64, 128, 3, 2, "dgrad"),        # parity-major
    "L3 dgrad": (12, 24, 80, 128, 256, 3, 2, "dgrad"),
    "L4 dgrad": (12, 12, 40, 256, 512, 3, 2, "dgrad"),
    "36>40 dgrad": (2, 10, 14, 36, 40, 3, 2, "dgrad"),        # parity-major with ragged classes (70 rows each), Nout = 36, C0 = 40
    "24>64 odd dgrad": (2, 9, 13, 24, 64, 3, 2, "dgrad"),     # odd dims: all nine taps, M = 234, 36 steps: SK = 4
    "24>48 odd dgrad": (2, 9, 13, 24, 48, 3, 2, "dgrad"),     # 27 steps: SK = 3
    "L4 1x1 dgrad": (12, 12, 40, 256, 512, 1, 2, "dgrad"),    # 180 tiles: unsplit
    "64>64 s1 dgrad": (2, 16, 24, 64, 64, 3, 1, "dgrad"),     # a stride-1 3x3 the tile kernel's tiling rejects (the 64 x 96 fixtures): SK = 4
}

# name: (bias, addend, addend_mask, actgrad, act, accumulate, backward sink armed)
EPI_SETS = {
    "bias": (1, 0, 0, None, None, 0, 0),                              # the engine's seven ...
    "bias+relu": (1, 0, 0, None, "relu", 0, 0),
    "bias+addend+relu": (1, 1, 0, None, "relu", 0, 0),
    "accum": (0, 0, 0, None, None, 1, 0),
    "addend": (0, 1, 0, None, None, 0, 0),
    "actgrad_relu": (0, 0, 0, "relu", None, 0, 0),
    "addend+actgrad_relu+bwd_sink": (0, 1, 0, "relu", None, 0, 1),
    "addend+mask": (0, 1, 1, None, None, 0, 0),                       # ... and the rest of the flag set
    "actgrad_elu": (0, 0, 0, "elu", None, 0, 0),
    "elu": (0, 0, 0, None, "elu", 0, 0),
    "addend+mask+actgrad_relu+accum": (0, 1, 1, "relu", None, 1, 0),
    "every stage": (1, 1, 1, "elu", "elu", 1, 0),                     # any two stages swapped show here
}
ALL_FORMS = {"unsplit", "split, no tail", "split, tail", "parity-major"}


def _cdiv(a, b):
    return -(-a // b)


def _dims(g):
    """(M, Nout, C0, taps, parity-major) of the launch"""
    N, H, W, Cin, Cout, K, stride, mode = g
    if mode == "fwd":
        pad = K // 2
        OH, OW = (H + 2 * pad - K) // stride + 1, (W + 2 * pad - K) // stride + 1
        return N * OH * OW, Cout, Cin, K * K, False
    pm = K == 3 and stride == 2 and H % 2 == 0 and W % 2 == 0
    return N * H * W, Cin, Cout, K * K, pm


def grid_form(fmt, g):
    """the launcher's decision restated (conv_igemm.hip: fp_conv_igemm / igemm_split_operands pick the tile; fp_conv_igemm_workspace, the
    clamp of igemm_fill and plan_grid with pick_splitk the split): (form, SK)"""
    M, Nout, C0, T, pm = _dims(g)
    if pm:
        return "parity-major", 1
    if fmt == "f32":
        if Nout <= 32:
            BM, BN = (256 if _cdiv(M, 256) >= 512 else 128), 32
        elif Nout % 128 == 0 and _cdiv(M, 128) * (Nout // 128) >= 256:
            BM, BN = 128, 128
        else:
            BM, BN = (128, 64) if M >= 256 else (64, 64)
    else:
        BM = 128
        wide = fmt == "fp16_pair" and Nout % 128 == 0 and _cdiv(M, 128) * (Nout // 128) >= 512
        BN = 32 if Nout <= 32 else 128 if wide else 64
    tiles, steps = _cdiv(M, BM) * _cdiv(Nout, BN), T * _cdiv(C0, 16)
    if _cdiv(M, 128) * _cdiv(Nout, 64) >= 384 or tiles >= 160:         # no workspace / the grid fills the chip
        return "unsplit", 1
    sk = min(_cdiv(768, tiles), steps // 8, 24)                          # ~3 workgroups per CU, >= 8 steps each, 24 partial copies at most
    if sk < 2:
        return "unsplit", 1
    SK = _cdiv(steps, _cdiv(steps, sk))
    return ("split, no tail" if SK % 4 == 0 else "split, tail"), SK


def _switched():
    return [k for k in ("FP_IGEMM_SK1_FROM", "FP_NO_PM", "FP_NO_SPLITK") if os.environ.get(k)]


def test_every_epilogue_set_meets_every_grid_form():
    """a condition on the table, not a measurement: the matrix below cannot collapse onto the unsplit path.  Every epilogue set runs on every
    geometry, so each set reaches all four forms as soon as the geometries do, in every operand format; the SK values named by the issue
    (2, 8 and one of 3 / 5 / 6) are among them"""
    if _switched():
        pytest.skip("the split rule is switched by %s: the forms of the table are those of the default build" % ", ".join(_switched()))
    for fmt in FORMATS:
        forms = {}
        for name, g in GEOMS.items():
            form, SK = grid_form(fmt, g)
            forms.setdefault(form, []).append((name, SK))
        assert set(forms) == ALL_FORMS, (fmt, forms)
        for epi in EPI_SETS:                                              # the cases test_epilogue_against_float64 is parametrized with
            hit = {grid_form(f, GEOMS[n])[0] for (f, e, n) in MATRIX if f == fmt and e == epi}
            assert hit == ALL_FORMS, (fmt, epi, hit)
        sks = {SK for v in forms.values() for _, SK in v}
        assert {2, 8} <= sks and sks & {3, 5, 6}, sks
        assert len(forms["split, tail"]) >= 3 and len(forms["parity-major"]) >= 4
    assert grid_form("exact", GEOMS["L4 fwd"]) == ("split, no tail", 8) and grid_form("exact", GEOMS["L4 1x1 fwd"]) == ("split, tail", 2)
    assert [grid_form("exact", (2, 18, 26, c, 64, 3, 2, "fwd"))[1] for c in (48, 80, 96)] == [3, 5, 6]


# ---- operands and float64 references, one geometry at a time --------------------------------------------------------------------------
_cache = {}


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _geometry(name, g, stats_inputs=False):
    """fp32 operands of the geometry, the float64 convolution / data gradient of them (NHWC, on the CPU) and the device copies"""
    key = (name, g, stats_inputs)
    if key in _cache:
        return _cache[key]
    _cache.clear()
    ops, L = _ops()
    N, H, W, Cin, Cout, K, stride, mode = g
    gen = torch.Generator().manual_seed(1000 * K + 7 * Cin + 3 * H + Cout)
    pad = K // 2
    OH, OW = (H + 2 * pad - K) // stride + 1, (W + 2 * pad - K) // stride + 1
    x = torch.rand(N, Cin, H, W, generator=gen) * 2 - 1
    w = (torch.rand(Cout, Cin, K, K, generator=gen) * 2 - 1) * 0.1
    if stats_inputs:                  # a per-channel mean of the order of the spread, like post-ReLU activations (see test_bn_partials_cpu.py)
        x = x * 2.0 + 0.75
        w = w + 0.1 / math.sqrt(Cin * K * K)
    if mode == "fwd":
        ref = _nhwc(F.conv2d(x.double(), w.double(), stride=stride, padding=pad))
        src = _nhwc(x).cuda()
        d = (N, OH, OW, H, W, Cin, 0, Cout, K, stride, pad, L.GATHER_FWD_ZERO)
    else:
        dz = (torch.rand(N, Cout, OH, OW, generator=gen) * 2 - 1) * 1e-6          # gradients are small numbers
        xin = torch.zeros(N, Cin, H, W, dtype=torch.float64, requires_grad=True)
        F.conv2d(xin, w.double(), stride=stride, padding=pad).backward(dz.double())
        ref = _nhwc(xin.grad)
        src = _nhwc(dz).cuda()
        d = (N, H, W, OH, OW, Cout, 0, Cin, K, stride, pad, L.GATHER_DGRAD_ZERO)
    shape = tuple(ref.shape)
    top = float(ref.abs().max())
    e = {"desc": d, "ref": ref, "src": src, "w": w.cuda(), "dgrad": mode == "dgrad", "shape": shape, "packed": {},
         # addend and previous y at the scale of the largest output element; mask and activation source from continuous distributions
         "bias": (torch.rand(shape[3], generator=gen) * 2 - 1) * (0.5 * top),
         "addend": (torch.rand(shape, generator=gen) * 2 - 1) * top,
         "prev": (torch.rand(shape, generator=gen) * 2 - 1) * top,
         "mask": torch.randn(shape, generator=gen),
         "actsrc": (torch.randn(shape, generator=gen) * 0.5).clamp_min(-0.99)}
    e["dev"] = {k: e[k].cuda() for k in ("bias", "addend", "prev", "mask", "actsrc")}
    _cache[key] = e
    return e


def _packed(e, fmt):
    """(packed weights, source amax slot, weight amax slot) of the format"""
    if fmt not in e["packed"]:
        ops, _ = _ops()
        w, dg = e["w"], e["dgrad"]
        Cout, Cin, K, _k = w.shape
        if fmt == "exact":
            p = (ops.pack_conv_weight_bf3(w, torch.empty(ops.packed_weight_elems_bf3(Cout, Cin, K, dg), device="cuda"), dg), None, None)
        elif fmt == "fp16_pair":
            sw = ops.new_slot()
            wp = ops.pack_conv_weight_hp(w, torch.empty(ops.packed_weight_elems_hp(Cout, Cin, K, dg), device="cuda"), sw, dg)
            p = (wp, ops.amax_f32(e["src"], ops.new_slot()), sw)
        else:
            wp = torch.empty(ops.packed_weight_elems(Cout, Cin, K, dg, False), device="cuda")
            p = (ops.pack_conv_weight_dgrad(w, wp) if dg else ops.pack_conv_weight(w, wp, False), None, None)
        e["packed"][fmt] = p
    return e["packed"][fmt]


def _launch(fmt, e, y, act=0, epi=0, **kw):
    ops, _ = _ops()
    d = ops.make_desc(*e["desc"], act=act, epi=epi)
    wp, ss, sw = _packed(e, fmt)
    if fmt == "exact":
        ops.conv_igemm_bf3(d, e["src"], wp, y, **kw)
    elif fmt == "fp16_pair":
        assert ops.conv_igemm_hp_supported(d)
        ops.conv_igemm_hp(d, e["src"], wp, y, ss, sw, **kw)
    else:
        ops.conv_igemm(d, e["src"], None, wp, y, **kw)
    torch.cuda.synchronize()
    return y


def _error(fmt, y, ref):
    """(figure, bound): relative L2 for the split formats, largest deviation over largest element for fp32 operands"""
    if fmt == "f32":
        return relerr(y, ref), TOL
    return ((y.double().cpu() - ref).norm() / ref.norm().clamp_min(1e-300)).item(), L2_BOUND


MATRIX = [(fmt, epi, name) for name, fmt, epi in itertools.product(GEOMS, FORMATS, EPI_SETS)]           # geometry outermost: one reference each


@pytest.mark.parametrize("fmt,epi_name,geom", MATRIX, ids=["%s-%s-%s" % m for m in MATRIX])
def test_epilogue_against_float64(fmt, epi_name, geom):
    """one launch per (operand format, epilogue set, geometry) against float64 in the documented order; twice, bit-identical.  An armed
    backward sink (bn_bwd_out) must be answered with "nothing emitted" by all three entry points: the engine then takes its own pass."""
    ops, L = _ops()
    g = GEOMS[geom]
    e = _geometry(geom, g)
    bias, addend, mask, actgrad, act, accum, bwd_sink = EPI_SETS[epi_name]
    ref, dev = e["ref"], e["dev"]
    v = ref.clone()
    if bias:
        v += e["bias"].double()
    if addend:
        v += e["addend"].double() * (e["mask"] > 0).double() if mask else e["addend"].double()
    if actgrad == "elu":
        sv = e["actsrc"].double()
        v *= torch.where(sv > 0, torch.ones_like(sv), sv + 1.0)
    if actgrad == "relu":
        v *= (e["actsrc"] > 0).double()
    if act == "elu":
        v = F.elu(v)
    if act == "relu":
        v = v.clamp_min(0.0)
    if accum:
        v += e["prev"].double()
    flags = (L.EPI_ACTGRAD_ELU if actgrad == "elu" else L.EPI_ACTGRAD_RELU if actgrad == "relu" else 0) | (L.EPI_ACCUM if accum else 0)
    kw = {}
    if bias:
        kw["bias"] = dev["bias"]
    if addend:
        kw["addend"] = dev["addend"]
    if mask:
        kw["addend_mask"] = dev["mask"]
    if actgrad:
        kw["actsrc"] = dev["actsrc"]
    M, Nout = ref.numel() // ref.shape[3], ref.shape[3]
    outs = []
    for rep in range(2):
        y = dev["prev"].clone() if accum else torch.full(e["shape"], float("nan"), device="cuda")
        cell = part = None
        if bwd_sink:
            part = torch.full((ops_engine_cap(g, Nout, 2) + 5,), float("nan"), device="cuda")
            z = torch.randn(M, Nout, device="cuda")
            cell = ops.bn_bwd_out(part, z, z.mean(0), 1.0 / torch.sqrt(z.var(0, unbiased=False) + 1e-5))
            kw["bn_out"] = cell
        _launch(fmt, e, y, act={"elu": L.ACT_ELU, "relu": L.ACT_RELU}.get(act, L.ACT_NONE), epi=flags, **kw)
        if bwd_sink:
            assert cell.nblk == 0 and bool(torch.isnan(part).all()), "the flattened kernels do not emit backward sums"
        outs.append(y)
    form, SK = grid_form(fmt, g)
    err, bound = _error(fmt, outs[0], v)
    print("IGEMM_EPI | %s | %s | %s | %s SK %d | %.3e" % (fmt, epi_name, geom, form, SK, err))
    assert err <= bound, (err, bound)
    assert torch.equal(outs[0], outs[1]), "two launches of the same case differ"


def ops_engine_cap(g, Nout, per):
    """the engine's partials buffer for this output (Engine._partials_cap)"""
    from footprints_amd.engine import Engine
    N, H, W, Cin, Cout, K, stride, mode = g
    if mode == "fwd":
        pad = K // 2
        H, W = (H + 2 * pad - K) // stride + 1, (W + 2 * pad - K) // stride + 1
    return Engine._partials_cap(N, H, W, Nout, per)


@pytest.mark.parametrize("fmt", SPLIT_FORMATS)
@pytest.mark.parametrize("geom", [n for n, g in GEOMS.items() if g[7] == "fwd"])
def test_split_rule_agrees_with_library(geom, fmt):
    """the restated split rule against the library on every forward geometry: only the reduce launch of a split grid answers an armed
    statistics sink, so nblk > 0 <=> the rule says split, where the reduce launch takes the channel count"""
    if _switched():
        pytest.skip("switched by %s" % ", ".join(_switched()))
    ops, _ = _ops()
    g = GEOMS[geom]
    e = _geometry(geom, g)
    M, Nout = _dims(g)[:2]
    part = torch.full((ops_engine_cap(g, Nout, 3) + 5,), float("nan"), device="cuda")
    cell = ops.bn_stats_out(part)
    _launch(fmt, e, torch.empty(e["shape"], device="cuda"), bn_out=cell)
    form, SK = grid_form(fmt, g)
    print("IGEMM_RULE | %s | %s | %s SK %d | nblk %d" % (fmt, geom, form, SK, cell.nblk))
    if reduce_geometry(M, Nout) is None:
        assert cell.nblk == 0
    else:
        assert (cell.nblk > 0) == (SK > 1), (cell.nblk, form, SK)


# ---- the statistics side output of the reduce launch -----------------------------------------------------------------------------------
STATS_EMIT = {
    "256>512 3x3/2, SK 8": (12, 12, 40, 256, 512, 3, 2, "fwd"),
    "256>512 1x1/2, SK 2": (12, 12, 40, 256, 512, 1, 2, "fwd"),
    "80>64 3x3/2, SK 5": (2, 18, 26, 80, 64, 3, 2, "fwd"),        # M = 234: ragged last sweep, 4 blocks of 16 row groups
    "96>16 3x3/2, SK 6": (1, 6, 10, 96, 16, 3, 2, "fwd"),         # M = 15 < R = 64: most row groups are empty
    "48>32 3x3/2, SK 3": (2, 18, 26, 48, 32, 3, 2, "fwd"),
}


@pytest.mark.parametrize("fmt", SPLIT_FORMATS)
@pytest.mark.parametrize("case", list(STATS_EMIT))
def test_reduce_launch_emits_batchnorm_partials(case, fmt):
    """fp_aux.bn_part behind fp_conv_igemm_bf3 / fp_conv_igemm_hp: the reduce launch of a split grid stores y and one (count, mean, M2) per
    block and channel of what it stores (splitk_reduce_stats_kernel); fp_bn_train_stats_partials turns them into the coefficients
    fp_bn_train_stats gets from the tensor -- the numbers of test_conv3x3_hp_emits_batchnorm_partials"""
    ops, L = _ops()
    g = STATS_EMIT[case]
    e = _geometry(case, g, stats_inputs=True)
    M, Nout = _dims(g)[:2]
    form, SK = grid_form(fmt, g)
    assert SK == int(case.rsplit(" ", 1)[1]) or _switched()
    R, nblk = reduce_geometry(M, Nout)
    part = torch.full((ops_engine_cap(g, Nout, 3) + 5,), float("nan"), device="cuda")
    cell = ops.bn_stats_out(part)
    y = _launch(fmt, e, torch.full(e["shape"], float("nan"), device="cuda"), bn_out=cell)
    y0 = _launch(fmt, e, torch.full(e["shape"], float("nan"), device="cuda"))
    err, bound = _error(fmt, y, e["ref"])
    print("IGEMM_STATS | %s | %s | SK %d nblk %d | y %.3e" % (fmt, case, SK, cell.nblk, err))
    assert err <= bound, err
    assert torch.equal(y, y0), "the sink changed the stored tensor"
    if _switched():
        return
    assert cell.nblk == nblk == min(512, _cdiv(M, R * 4))
    used = nblk * Nout * 3
    assert not bool(torch.isnan(part[:used]).any()) and bool(torch.isnan(part[used:]).all())
    y2d = y.view(M, Nout).cpu()
    worst = check_reduce_partials(part[:used].view(nblk, Nout, 3).cpu().numpy(), y2d.numpy(), R)
    print("IGEMM_STATS | %s | %s | partials: mean %.3e M2 %.3e" % (fmt, case, worst[0], worst[1]))
    gam, bet = (torch.rand(Nout) + 0.5).cuda(), (torch.rand(Nout) * 2 - 1).cuda()
    outs = [[torch.zeros(Nout, device="cuda") for _ in range(4)] for _ in range(2)]
    rms, rvs = [torch.zeros(Nout, device="cuda") for _ in range(2)], [torch.ones(Nout, device="cuda") for _ in range(2)]
    nbt = [torch.zeros((), dtype=torch.int64, device="cuda") for _ in range(2)]
    ops.bn_train_stats_partials(part, nblk, Nout, gam, bet, rms[0], rvs[0], nbt[0], *outs[0])
    ops.bn_train_stats(y.view(M, Nout), gam, bet, rms[1], rvs[1], nbt[1], *outs[1])
    yd, gc, bc = y2d.double(), gam.double().cpu(), bet.double().cpu()
    mean, var = yd.mean(0), yd.var(0, unbiased=False)
    invstd = 1.0 / torch.sqrt(var + 1e-5)
    for k, want in enumerate((mean, invstd, gc * invstd, bc - mean * gc * invstd)):
        for o in outs:
            assert relerr(o[k], want) < 2e-6, (k, relerr(o[k], want))
    assert relerr(rms[0], rms[1].cpu()) < 1e-6 and relerr(rvs[0], rvs[1].cpu()) < 1e-6 and int(nbt[0]) == int(nbt[1]) == 1


# name: (geometry, format(s), launch options, what arms the sink, capacity)
NO_EMIT = {
    "unsplit grid": ((2, 18, 26, 64, 64, 1, 2, "fwd"), SPLIT_FORMATS, {}, "stats", 0),                       # 4 steps
    "bias": ((12, 12, 40, 256, 512, 1, 2, "fwd"), SPLIT_FORMATS, {"bias": 1}, "stats", 0),
    "activation": ((12, 12, 40, 256, 512, 1, 2, "fwd"), SPLIT_FORMATS, {"act": "relu"}, "stats", 0),
    "parity-major data gradient": ((2, 10, 14, 32, 48, 3, 2, "dgrad"), SPLIT_FORMATS, {}, "stats", 0),
    "Nout 24": ((2, 18, 26, 48, 24, 3, 2, "fwd"), SPLIT_FORMATS, {}, "stats", 0),                            # 256 % 6 != 0; SK = 3
    "capacity one float short": ((2, 18, 26, 80, 64, 3, 2, "fwd"), SPLIT_FORMATS, {}, "stats", -1),
    "backward sink": ((2, 16, 24, 64, 64, 3, 1, "dgrad"), SPLIT_FORMATS, {"addend": 1, "actgrad": "relu"}, "backward", 0),
    "fp32 operands": ((12, 12, 40, 256, 512, 1, 2, "fwd"), ("f32",), {}, "stats", 0),
}
NO_EMIT_CASES = [(n, f) for n, c in NO_EMIT.items() for f in c[1]]


@pytest.mark.parametrize("case,fmt", NO_EMIT_CASES, ids=["%s-%s" % c for c in NO_EMIT_CASES])
def test_launches_that_must_not_emit(case, fmt):
    """every launch the reduce-with-statistics path does not take reports nblk == 0, leaves the partials buffer untouched and stores the
    right tensor: engine.py then runs the BatchNorm's own pass (its `nblk == 0` branches)"""
    ops, L = _ops()
    g, _f, opt, sink, cap_delta = NO_EMIT[case]
    e = _geometry("no-emit " + case, g, stats_inputs=True)
    M, Nout = _dims(g)[:2]
    form, SK = grid_form(fmt, g)
    if not _switched():
        assert (SK > 1) == (case not in ("unsplit grid", "parity-major data gradient")), (form, SK)
    ref, dev, kw, flags = e["ref"].clone(), e["dev"], {}, 0
    if opt.get("bias"):
        ref += e["bias"].double()
        kw["bias"] = dev["bias"]
    if opt.get("addend"):
        ref += e["addend"].double()
        kw["addend"] = dev["addend"]
    if opt.get("actgrad"):
        ref *= (e["actsrc"] > 0).double()
        kw["actsrc"], flags = dev["actsrc"], L.EPI_ACTGRAD_RELU
    if opt.get("act"):
        ref = ref.clamp_min(0.0)
    if cap_delta:
        R, nblk = reduce_geometry(M, Nout)
        cap = nblk * Nout * 3 + cap_delta
    else:
        cap = ops_engine_cap(g, Nout, 3) + 5
    part = torch.full((cap,), float("nan"), device="cuda")
    if sink == "backward":
        z = torch.randn(M, Nout, device="cuda")
        cell = ops.bn_bwd_out(part, z, z.mean(0), 1.0 / torch.sqrt(z.var(0, unbiased=False) + 1e-5))
    else:
        cell = ops.bn_stats_out(part)
    y = _launch(fmt, e, torch.full(e["shape"], float("nan"), device="cuda"), act=L.ACT_RELU if opt.get("act") else 0, epi=flags, bn_out=cell, **kw)
    err, bound = _error(fmt, y, ref)
    print("IGEMM_NOEMIT | %s | %s | %s SK %d | nblk %d | y %.3e" % (fmt, case, form, SK, cell.nblk, err))
    assert cell.nblk == 0, cell.nblk
    assert bool(torch.isnan(part).all()), "a launch that reports nothing emitted wrote into the partials buffer"
    assert err <= bound, err
