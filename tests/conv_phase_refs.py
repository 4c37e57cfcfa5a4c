"""Float64 references, exactly summable inputs and the GPU case tables for the nearest-x2 phase kernels (csrc/conv_up2_phase.hip,
csrc/wgrad_up2_phase.hip, the collapsing packers of csrc/pack.hip).  tests/test_conv_phase_refs_cpu.py pins what is here on the CPU;
tests/test_gpu_conv_phase_edges.py runs the cases; tests/test_launch_regimes_cpu.py asserts that the cases reach every launch regime of a
train step.  Built on tests/conv_tile_refs.py (TR): the forward is TR.conv_ref("up2", ...), the weight gradient TR.wgrad_ref("up2", ...).

Tensors are NCHW here, float64 unless said otherwise; h x w is the LOW-resolution grid.  A case row is (fmt, N, h, w, C0, C1, Nout) with fmt in
("f32", "exact", "pair"):
    forward          low [N, C0, h, w] (+ skip [N, C1, 2h, 2w], run by another kernel), w [Nout, C0 + C1, 3, 3] -> y [N, Nout, 2h, 2w]
    data gradient    dz [N, Nout, 2h, 2w], w [Nout, C0, 3, 3] -> ext [N, C0, h + 2, w + 2] -> fold -> d(low) [N, C0, h, w];  C1 = 0
    weight gradient  low, dz -> dw [Nout, k_begin + C0 + k_after, 3, 3]; the sixth entry is (k_begin, k_after) in place of C1

The references are stated WITHOUT the phase arithmetic (upsample, pad, convolve; transposed convolution, summed over 2 x 2 blocks).  The
kernels' arithmetic -- collapsed weights, the 4 x 4 stride-2 kernel K4, the un-collapse -- is restated separately (phase_fwd, ext_by_k4,
collapsed_wgrad / uncollapse), tied to the references on the CPU, and carries the wrong variants.

LATTICE INPUTS as in TR: activations, gradients, addend, previous y integers in [-4, 4], weights integers in [-4, 4] over 8, ylow from
SIDE_VALUES.  A collapsed weight is a sum of up to four taps: at most 16 eighths, still one bf16 term and, scaled by the weight tensor's amax to
[2^11, 2^12) (fp_common.h: FP_HP_TARGET_W = 11, four taps of headroom), still one fp16 term.  Every partial sum stays below 2^24 units
(asserted per case on the CPU), so any order of float32 additions gives the float64 result bit for bit in all three formats.

CANCELLING INPUTS: TR.cancel_inputs with the weights kept in the four corner taps only (centre row and column zero): every collapsed weight
and every K4 entry is then exactly one stored float32 weight, and the float64 reference sees what the kernel sees whatever order the packer
adds in."""
import math

import torch
import torch.nn.functional as F

from tests import conv_tile_refs as TR
from tests import launch_regimes as LR

FORMATS = LR.PHASE_FORMATS


# ---- float64 references --------------------------------------------------------------------------------------------------------------
def fwd_ref(low, w, skip=None):
    return TR.conv_ref("up2", low, w, skip)


def ext_ref(dz, w):
    """gradient on the extended (h + 2) x (w + 2) low-resolution grid, before the fold: the gradient of the reflection-padded upsampled
    image (conv_transpose2d: [N, C0, 2h + 2, 2w + 2]) summed over the 2 x 2 blocks that one low-resolution pixel was repeated into.  Padded
    row Y shows hi-res row Y - 1, i.e. virtual low-res row floor((Y - 1) / 2) in -1 .. h: extended row e collects Y = 2e - 1 and 2e."""
    g = F.pad(F.conv_transpose2d(dz, w), (1, 1, 1, 1))
    N, C, H2, W2 = g.shape
    return g.view(N, C, H2 // 2, 2, W2 // 2, 2).sum((3, 5))


def fold_ref(ext, addend=None, ylow=None, onto=0):
    """the extended grid's border rows / columns folded onto rows 0 / h-1 (the padding is a REPLICATE padding at low resolution), then the
    addend, then the ELU-gradient factor of ylow; onto = 1 is the wrong variant (the reflection rule)"""
    return TR.epilogue_ref(TR.fold_ring(ext, onto), addend=addend, actgrad="elu" if ylow is not None else None, actsrc=ylow)


def wgrad_ref(low, dz):
    return TR.wgrad_ref("up2", low, dz)


def wgrad_ref_mm(low, dz):
    """the same as nine matrix products (pixels contracted by a GEMM): for the one case whose 768 channel tiles make conv2d slow"""
    p = TR.padded("up2", low)
    N, C, H2, W2 = p.shape
    H, W = H2 - 2, W2 - 2
    z = dz.permute(1, 0, 2, 3).reshape(dz.shape[1], -1)
    dw = torch.empty(dz.shape[1], C, 3, 3, dtype=low.dtype)
    for ky in range(3):
        for kx in range(3):
            dw[:, :, ky, kx] = z @ p[:, :, ky:ky + H, kx:kx + W].permute(0, 2, 3, 1).reshape(-1, C)
    return dw, dz.sum((0, 2, 3))


# ---- the kernels' arithmetic, restated (and its wrong variants) ----------------------------------------------------------------------------
ROWS = {(0, 0): (0,), (0, 1): (1, 2), (1, 0): (0, 1), (1, 1): (2,)}          # (dy, a) -> the ky collapsed into tap row a of phase dy (pack.hip:64)
K4ROWS = ((2,), (1, 2), (0, 1), (0,))                                        # K4[r] (pack.hip:80)
WRONG = ("reflect at low resolution", "phases swapped", "rows paired wrongly", "fold onto 1 / h-2", "K4 not flipped", "uncollapse pairing")


def collapse(w, wrong=None):
    """{(dy, dx, a, b): Wc [Nout, C]}; "rows paired wrongly": Wc[dy = 0][a = 1] = W[0] + W[1]"""
    rows = dict(ROWS)
    if wrong == "rows paired wrongly":
        rows[(0, 1)] = (0, 1)
    return {(dy, dx, a, b): sum(w[:, :, ky, kx] for ky in rows[(dy, a)] for kx in ROWS[(dx, b)])
            for dy in (0, 1) for dx in (0, 1) for a in (0, 1) for b in (0, 1)}


def phase_fwd(low, w, wrong=None):
    """out[2y + dy][2x + dx] = sum_ab Wc[dy, dx][a][b] . low[clamp(y + dy - 1 + a)][clamp(x + dx - 1 + b)] (conv_up2_phase.hip:6)"""
    N, C, h, wd = low.shape
    p = F.pad(low, (1, 1, 1, 1), mode="reflect" if wrong == "reflect at low resolution" else "replicate")
    wc = collapse(w, wrong)
    out = torch.zeros(N, w.shape[0], 2 * h, 2 * wd, dtype=low.dtype)
    for dy in (0, 1):
        for dx in (0, 1):
            wy, wx = (dx, dy) if wrong == "phases swapped" else (dy, dx)
            out[:, :, dy::2, dx::2] = sum(torch.einsum("nchw,oc->nohw", p[:, :, dy + a:dy + a + h, dx + b:dx + b + wd], wc[(wy, wx, a, b)])
                                          for a in (0, 1) for b in (0, 1))
    return out


def k4(w, flipped=True):
    """the 4 x 4 stride-2 kernel of the data gradient [Cout, C0, 4, 4]: K4[0] = W[2], K4[1] = W[1] + W[2], K4[2] = W[0] + W[1], K4[3] = W[0]"""
    rows = K4ROWS if flipped else K4ROWS[::-1]
    out = torch.zeros(w.shape[0], w.shape[1], 4, 4, dtype=w.dtype)
    for r in range(4):
        for s in range(4):
            out[:, :, r, s] = sum(w[:, :, ky, kx] for ky in rows[r] for kx in rows[s])
    return out


def ext_by_k4(dz, w, flipped=True):
    """ext[e] = sum_r K4[r] dz[2e - 3 + r]: K = 4, stride 2, zero padding 3 (conv_up2_phase.hip:537-540)"""
    return F.conv2d(dz, k4(w, flipped).transpose(0, 1).contiguous(), stride=2, padding=3)


def collapsed_wgrad(low, dz):
    """{(dy, dx, a, b): dWc [Nout, C0]} (wgrad_up2_phase.hip:4)"""
    N, C, h, wd = low.shape
    p = F.pad(low, (1, 1, 1, 1), mode="replicate")
    return {(dy, dx, a, b): torch.einsum("nchw,nohw->oc", p[:, :, dy + a:dy + a + h, dx + b:dx + b + wd], dz[:, :, dy::2, dx::2])
            for dy in (0, 1) for dx in (0, 1) for a in (0, 1) for b in (0, 1)}


def uncollapse(dwc, wrong=None):
    """dW[ky] = dWc over the (dy, a) whose collapsed row holds ky: ky = 0: (0,0) (1,0); 1: (0,1) (1,0); 2: (0,1) (1,1) (wgrad_up2_phase.hip:359);
    "uncollapse pairing": (dy = 1) paired with the a of dy = 0"""
    a_of = lambda d, k: (0 if k == 0 else 1) if (d == 0 or wrong == "uncollapse pairing") else (1 if k == 2 else 0)
    b_of = lambda d, k: (0 if k == 0 else 1) if d == 0 else (1 if k == 2 else 0)
    any_ = next(iter(dwc.values()))
    dw = torch.zeros(tuple(any_.shape) + (3, 3), dtype=any_.dtype)
    for ky in range(3):
        for kx in range(3):
            dw[:, :, ky, kx] = sum(dwc[(dy, dx, a_of(dy, ky), b_of(dx, kx))] for dy in (0, 1) for dx in (0, 1))
    return dw


def wrong_variant(name, *a):
    """forward variants take (low, w) -> y; data-gradient variants (dz, w) -> d(low) after the fold; "uncollapse pairing" (low, dz) -> dw"""
    if name in ("reflect at low resolution", "phases swapped", "rows paired wrongly"):
        return phase_fwd(a[0], a[1], name)
    if name == "fold onto 1 / h-2":
        return fold_ref(ext_ref(a[0], a[1]), onto=1)
    if name == "K4 not flipped":
        return fold_ref(ext_by_k4(a[0], a[1], flipped=False))
    if name == "uncollapse pairing":
        return uncollapse(collapsed_wgrad(a[0], a[1]), name)
    raise KeyError(name)


# ---- the operand formats (fp_common.h) -------------------------------------------------------------------------------------------------
HP_TARGET_ACT, HP_TARGET_W = 12, 11          # fp_common.h:195-196


def hp_exponent(amax, target):
    """fp_common.h:226 fp_hp_exponent: k with amax 2^k in [2^target, 2^(target + 1)); 0 for an all-zero tensor"""
    return min(target - (math.frexp(float(amax))[1] - 1), 126) if amax else 0


def is_one_term(t, fmt, amax=None, target=HP_TARGET_W):
    """is every element of the float32 tensor a single term of the format (bf16; fp16 after the scaling by the TENSOR's amax -- for collapsed
    weights the amax is that of the 3 x 3 weights they were summed from)?"""
    if fmt == "f32":
        return True
    if fmt == "exact":
        return torch.equal(t.bfloat16().float(), t.float())
    v = t.double() * 2.0 ** hp_exponent(float(t.abs().max()) if amax is None else amax, target)
    return bool(torch.isfinite(v.half()).all()) and torch.equal(v.half().double(), v)


def fp16_pair_terms(t, target):
    """(h, m) of the scaled fp16-pair format as float64 (TR.fp16_pair_terms with the target exponent of the operand)"""
    s = 2.0 ** hp_exponent(float(t.abs().max()), target)
    v = t.double() * s
    h = v.half().double()
    return h / s, (v - h).half().double() / s


# ---- inputs --------------------------------------------------------------------------------------------------------------------------
ELU_SIDE_VALUES = tuple(v for v in TR.SIDE_VALUES if v > -1.0)          # what an ELU output can be: all of them


def _seed(kind, case):
    fmt, N, h, w, C0, C1, Nout = case
    c1 = sum(C1) if isinstance(C1, tuple) else C1
    return 7 * h + 13 * w + 3 * C0 + 5 * c1 + Nout + 1000 * ("fwd", "dgrad", "wgrad", "fold").index(kind) + 20000


def lattice_side(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.tensor(ELU_SIDE_VALUES)[torch.randint(0, len(ELU_SIDE_VALUES), tuple(shape), generator=g)]


def inputs(kind, case, random=False):
    """dict of float32 tensors of a case: lattice values, or the ranges of tests/test_gpu_kernels.py (activations and gradients in [-1, 1],
    weights in [-0.1, 0.1], ylow = an ELU output)"""
    fmt, N, h, w, C0, C1, Nout = case
    s = _seed(kind, case) + (50 if random else 0)
    act = (lambda shape, k: TR.rnd(shape, s + k)) if random else (lambda shape, k: TR.lattice(shape, s + k))
    wt = (lambda shape, k: TR.rnd(shape, s + k, -0.1, 0.1)) if random else (lambda shape, k: TR.lattice(shape, s + k, step=0.125))
    side = (lambda shape, k: F.elu(TR.rnd(shape, s + k, -2.0, 2.0))) if random else (lambda shape, k: lattice_side(shape, s + k))
    if kind == "fwd":
        return {"low": act((N, C0, h, w), 0), "skip": act((N, C1, 2 * h, 2 * w), 1) if C1 else None, "w": wt((Nout, C0 + C1, 3, 3), 2),
                "bias": act((Nout,), 3), "prev": act((N, Nout, 2 * h, 2 * w), 4)}
    if kind == "dgrad":
        return {"dz": act((N, Nout, 2 * h, 2 * w), 0), "w": wt((Nout, C0, 3, 3), 2), "addend": act((N, C0, h, w), 4), "ylow": side((N, C0, h, w), 5)}
    if kind == "wgrad":
        return {"low": act((N, C0, h, w), 0), "dz": act((N, Nout, 2 * h, 2 * w), 1)}
    assert kind == "fold"
    return {"ext": act((N, C0, h + 2, w + 2), 0), "addend": act((N, C0, h, w), 4), "ylow": side((N, C0, h, w), 5)}


def corner_taps(w):
    out = w.clone()
    out[:, :, 1, :] = 0
    out[:, :, :, 1] = 0
    return out


def cancel_inputs(kind, ckind, case):
    """(operand, w): kind "fwd": low and w [Nout, C0, 3, 3]; "dgrad": dz and w [Nout, C0, 3, 3]; the reduction channels in cancelling pairs /
    groups of four (TR.cancel_inputs), the weights in the corner taps only"""
    fmt, N, h, w, C0, C1, Nout = case
    tc = ("up2", fmt, N, 2 * h, 2 * w, C0, 0, Nout) if kind == "fwd" else ("dgrad", fmt, N, 2 * h, 2 * w, Nout, 0, C0)
    t = TR.cancel_inputs(ckind, tc)
    return t["src"], corner_taps(t["w"])


def cancel_ref(kind, x, w):
    """forward: y; data gradient: the extended grid"""
    return fwd_ref(x, w) if kind == "fwd" else ext_ref(x, w)


def abs_units(kind, case, inp):
    """the largest sum of |products| behind one output, in the lattice's units (forward, data gradient: eighths; weight gradient: ones),
    every later stage included: bias and addend; the fold of up to nine extended positions and its addend; the sum over the splits, the
    four-term un-collapse and the accumulating second call.  Below 2^24 every float32 partial sum is exact."""
    fmt, N, h, w, C0, C1, Nout = case
    if kind == "wgrad":
        return 2.0 * N * 4 * h * w * 16           # |low| |dz| <= 16 per hi-res pixel and tap; all four collapsed entries behind one dw; twice
    a = {k: (None if v is None else v.double().abs()) for k, v in inp.items()}
    if kind == "fwd":
        return float((fwd_ref(a["low"], a["w"], a["skip"]) + a["bias"].view(1, -1, 1, 1) + a["prev"]).max()) * 8.0
    if kind == "dgrad":
        return float((fold_ref(ext_ref(a["dz"], a["w"])) + a["addend"]).max()) * 8.0
    return float((fold_ref(a["ext"]) + a["addend"]).max()) * 4.0          # the ELU-gradient factor is a multiple of 1/4


def edge_mask(H, W, th, tw, scale=1):
    """TR.edge_mask for a grid tiled at `scale` times finer tiles (the forward's output: scale 2, tiles 16 x 32 hi-res pixels)"""
    return TR.edge_mask(H, W, th * scale, tw * scale)


# ---- the GPU cases -------------------------------------------------------------------------------------------------------------------
# the epilogue sets every forward case runs (test_gpu_conv_phase_edges.py): plain; bias; bias + in-place addend; bias + ELU (the decoder's o41);
# bias + addend + ELU (the decoder's post1)
FWD_EPIS = ((), ("bias",), ("addend", "bias"), ("act", "bias"), ("act", "addend", "bias"))


def case_regimes(kind, case):
    fmt, N, h, w, C0, C1, Nout = case
    if kind == "fwd":
        out = frozenset()
        for e in FWD_EPIS:
            out |= LR.phase_regime("fwd", fmt, N, h, w, C0, C1, Nout, epi=e)
        return out
    if kind == "dgrad":
        return LR.phase_regime("dgrad", fmt, N, h, w, C0, 0, Nout) | LR.fold_regime(N, h, w, C0, True, True) | LR.fold_regime(N, h, w, C0, False, True)
    if kind == "wgrad":
        return LR.phase_regime("wgrad", fmt, N, h, w, C0, 0, Nout, kslice=C1)
    return LR.fold_regime(N, h, w, C0, True, True) | LR.fold_regime(N, h, w, C0, False, True)


# Chosen by a greedy cover over small shapes (smallest N h w C0 Nout first) of: every regime tuple the four training workloads produce
# (tests/test_launch_regimes_cpu.py: phase_workload) plus, per compiled kernel, every value of every axis of LR.phase_regime that the
# launcher can reach.  Each row is there for a tuple no earlier row produces.
PHASE_FWD = [('f32', 1, 1, 1, 12, 0, 20),
 ('exact', 1, 1, 1, 12, 0, 20),
 ('pair', 1, 1, 1, 12, 0, 20),
 ('f32', 1, 1, 1, 12, 0, 64),
 ('exact', 1, 1, 1, 12, 0, 64),
 ('pair', 1, 1, 1, 12, 0, 64),
 ('f32', 2, 2, 2, 32, 32, 32),
 ('exact', 2, 2, 2, 32, 32, 32),
 ('pair', 2, 2, 2, 32, 32, 32),
 ('f32', 1, 2, 2, 32, 0, 72),
 ('exact', 1, 2, 2, 32, 0, 72),
 ('pair', 1, 2, 2, 32, 0, 72),
 ('f32', 2, 8, 16, 36, 20, 64),
 ('exact', 2, 8, 16, 36, 20, 64),
 ('pair', 2, 8, 16, 36, 20, 64),
 ('f32', 1, 8, 16, 36, 0, 20),
 ('exact', 1, 8, 16, 36, 0, 20),
 ('pair', 1, 8, 16, 36, 0, 20),
 ('f32', 2, 3, 3, 56, 0, 72),
 ('exact', 2, 3, 3, 56, 0, 72),
 ('pair', 2, 3, 3, 56, 0, 72),
 ('f32', 1, 3, 3, 56, 0, 20),
 ('exact', 1, 3, 3, 56, 0, 20),
 ('pair', 1, 3, 3, 56, 0, 20),
 ('f32', 1, 9, 17, 72, 0, 20),
 ('exact', 1, 9, 17, 72, 0, 20),
 ('pair', 1, 9, 17, 72, 0, 20),
 ('f32', 1, 9, 17, 72, 16, 64),
 ('exact', 1, 9, 17, 72, 16, 64),
 ('pair', 1, 9, 17, 72, 16, 64),
 ('f32', 1, 10, 18, 12, 12, 20),
 ('exact', 1, 10, 18, 12, 12, 20),
 ('pair', 1, 10, 18, 12, 12, 20),
 ('f32', 1, 11, 19, 12, 0, 20),
 ('exact', 1, 11, 19, 12, 0, 20),
 ('pair', 1, 11, 19, 12, 0, 20),
 ('f32', 1, 16, 32, 12, 0, 20),
 ('exact', 1, 16, 32, 12, 0, 20),
 ('pair', 1, 16, 32, 12, 0, 20),
 ('f32', 1, 10, 18, 12, 0, 64),
 ('exact', 1, 10, 18, 12, 0, 64),
 ('pair', 1, 10, 18, 12, 0, 64),
 ('f32', 1, 11, 19, 12, 0, 64),
 ('exact', 1, 11, 19, 12, 0, 64),
 ('pair', 1, 11, 19, 12, 0, 64),
 ('f32', 1, 16, 32, 12, 0, 64),
 ('exact', 1, 16, 32, 12, 0, 64),
 ('pair', 1, 16, 32, 12, 0, 64)]
PHASE_DGRAD = [('exact', 1, 1, 1, 20, 0, 12),
 ('exact', 1, 8, 2, 64, 0, 12),
 ('pair', 1, 1, 1, 20, 0, 12),
 ('pair', 1, 1, 1, 64, 0, 12),
 ('exact', 1, 1, 16, 72, 0, 32),
 ('exact', 2, 6, 14, 32, 0, 32),
 ('pair', 2, 6, 14, 32, 0, 32),
 ('pair', 1, 6, 14, 72, 0, 32),
 ('pair', 2, 8, 16, 64, 0, 36),
 ('exact', 2, 6, 1, 64, 0, 36),
 ('exact', 1, 8, 16, 20, 0, 36),
 ('pair', 1, 8, 16, 20, 0, 36),
 ('exact', 2, 7, 14, 72, 0, 56),
 ('pair', 2, 7, 15, 72, 0, 56),
 ('exact', 1, 7, 15, 20, 0, 56),
 ('pair', 1, 7, 15, 20, 0, 56),
 ('exact', 1, 9, 17, 20, 0, 72),
 ('pair', 1, 9, 17, 20, 0, 72),
 ('exact', 1, 9, 15, 64, 0, 72),
 ('pair', 1, 9, 17, 64, 0, 72),
 ('exact', 1, 14, 30, 20, 0, 12),
 ('pair', 1, 14, 30, 20, 0, 12),
 ('exact', 1, 14, 17, 64, 0, 12),
 ('pair', 1, 14, 30, 64, 0, 12),
 ('exact', 1, 1, 30, 64, 0, 12)]
PHASE_WGRAD = [('f32', 7, 5, 15, 32, (0, 0), 32),
 ('exact', 7, 5, 15, 32, (0, 0), 32),
 ('pair', 7, 5, 15, 32, (0, 0), 32),
 ('f32', 1, 28, 50, 32, (0, 32), 32),
 ('exact', 1, 28, 50, 32, (0, 32), 32),
 ('pair', 1, 28, 50, 32, (0, 32), 32),
 ('f32', 19, 31, 48, 64, (32, 0), 64),
 ('exact', 9, 11, 29, 64, (32, 0), 32),
 ('pair', 9, 11, 29, 64, (32, 0), 32),
 ('exact', 1, 31, 65, 64, (32, 32), 32),
 ('pair', 1, 31, 65, 64, (32, 32), 32),
 ('f32', 14, 7, 29, 64, (32, 32), 32),
 ('exact', 2, 7, 32, 1024, (0, 0), 768),
 ('pair', 2, 7, 32, 1024, (0, 0), 768),
 ('f32', 1, 31, 16, 1024, (0, 0), 768),
 ('exact', 4, 7, 16, 32, (0, 0), 64),
 ('pair', 4, 7, 16, 32, (0, 0), 64),
 ('f32', 1, 8, 65, 64, (0, 0), 32),
 ('f32', 1, 8, 50, 32, (0, 0), 64),
 ('f32', 2, 4, 50, 32, (0, 0), 64),
 ('exact', 1, 8, 50, 32, (0, 0), 64),
 ('pair', 1, 8, 50, 32, (0, 0), 64),
 ('exact', 1, 8, 50, 64, (0, 0), 64),
 ('pair', 1, 8, 50, 64, (0, 0), 64)]
# the fold kernel alone: its grid-stride loop runs more than once from 2^20 float4 items (the 4096-workgroup cap), as at 4 x 256 x 320 x 64
# (4 x 256 x 320 x 64 is five full passes, 12 x 96 x 320 x 64 five and a part); the format entry is unused
PHASE_FOLD = [("f32", 1, 33, 130, 1024, 0, 0), ("f32", 2, 64, 64, 1024, 0, 0), ("f32", 3, 5, 7, 12, 0, 0)]

# cancelling inputs: one aligned and one ragged geometry per kernel and split format (C0 = Nout = 64: the figures of the CPU test)
PHASE_CANCEL = [(k, (f,) + s) for k in ("fwd", "dgrad") for f in ("exact", "pair") for s in ((3, 16, 32, 64, 0, 64), (5, 9, 17, 64, 0, 64))]
