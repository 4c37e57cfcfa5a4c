"""Float64 references, exactly summable inputs and the GPU case tables for the 3x3 stride-1 tile kernels (csrc/conv3x3_tile_bf3.hip,
csrc/wgrad3x3_bf3.hip).  tests/test_conv_tile_refs_cpu.py pins what is here on the CPU; tests/test_gpu_conv_tile_edges.py runs the cases;
tests/test_launch_regimes_cpu.py asserts that the cases reach every launch regime of a train step.

Tensors are NCHW here, float64 unless said otherwise.  The five gathers:

    zero            conv2d, zero padding 1
    reflect         reflection padding 1, then conv2d
    up2             cat[nearest_x2(low), skip], reflection padding 1, then conv2d
    dgrad           gradient of "zero" with respect to its input
    dgrad_reflect   gradient of "reflect" with respect to its input: the gradient of the padded image, its ring folded onto rows /
                    columns 1 and n-2

LATTICE INPUTS: activations, gradients, addend and previous y are integers in [-4, 4], weights integers in [-4, 4] over 8, bias integers,
mask and actsrc from {-0.75, -0.5, -0.25, 0, 0.5, 1}.  Every product is a multiple of 1/8 and every partial sum stays below 2^24 of
these units (asserted per case on the CPU), so ANY order of float32 additions gives the float64 result bit for bit: in the exact
bf16 split (an integer up to 4 is its own first term), in the scaled fp16 pairs (the largest magnitude maps into [2^12, 2^13): the
first plane holds the value, the second is zero) and in the two-term mode.

CANCELLING INPUTS: channels come in pairs (x, x + d) with weights (w, -w): the result -sum w d is carried by the operands' low-order
terms alone.  A group of four, (x, x + d, x, x + d) with weights (w, -w, -(w + e), w + e), leaves e d: the middle x middle product
(x and w of one bf16 term there, d and e their middle terms).
The second member of a pair is built from the STORED float32 value of the first, so the float64 reference sees what the kernel sees."""
import torch
import torch.nn.functional as F

FWD_GATHERS = ("zero", "reflect", "up2")
DGRAD_GATHERS = ("dgrad", "dgrad_reflect")
GATHERS = FWD_GATHERS + DGRAD_GATHERS


# ---- float64 references --------------------------------------------------------------------------------------------------------------
def _up2_cat(low, skip):
    up = F.interpolate(low, scale_factor=2, mode="nearest")
    return torch.cat([up, skip], 1) if skip is not None else up


def padded(gather, x, skip=None):
    """the (H + 2) x (W + 2) image the nine taps of a forward gather read"""
    if gather == "zero":
        return F.pad(x, (1, 1, 1, 1))
    if gather == "up2":
        x = _up2_cat(x, skip)
    return F.pad(x, (1, 1, 1, 1), mode="reflect")


def conv_ref(gather, src, w, skip=None):
    """forward gathers: src [N, C0, H, W] (up2: the half-resolution tensor, skip [N, C1, 2H, 2W] or None), w [Nout, C, 3, 3];
    data gradients: src = the gradient [N, Cout, H, W], w = the FORWARD convolution's weights [Cout, Cin, 3, 3] -> [N, Cin, H, W]"""
    if gather in FWD_GATHERS:
        return F.conv2d(padded(gather, src, skip), w)
    ext = F.conv_transpose2d(src, w)                       # gradient of the padded image: [N, Cin, H + 2, W + 2]
    if gather == "dgrad":
        return ext[:, :, 1:-1, 1:-1].clone()
    return fold_ring(ext, 1)


def fold_ring(ext, onto):
    """the padded image's gradient -> the image's: padded row 0 mirrors image row 1 and padded row n+1 mirrors row n-2 (`onto` = 1);
    `onto` = 0 is the wrong variant that folds onto rows 0 / n-1"""
    e = ext[:, :, 1:-1, :].clone()
    e[:, :, onto, :] += ext[:, :, 0, :]
    e[:, :, e.shape[2] - 1 - onto, :] += ext[:, :, -1, :]
    out = e[:, :, :, 1:-1].clone()
    out[:, :, :, onto] += e[:, :, :, 0]
    out[:, :, :, out.shape[3] - 1 - onto] += e[:, :, :, -1]
    return out


def wgrad_ref(gather, src, dz, skip=None):
    """weight and bias gradient of a forward gather: dw [Nout, C, 3, 3] = sum over pixels of dz x the tap's input, db = column sums of dz"""
    p = padded(gather, src, skip)
    dw = F.conv2d(p.transpose(0, 1), dz.transpose(0, 1)).transpose(0, 1)
    return dw.contiguous(), dz.sum((0, 2, 3))


def epilogue_ref(acc, bias=None, addend=None, mask=None, actgrad=None, actsrc=None, act=None, prev=None):
    """acc (+bias) -> + addend * (mask > 0) -> * actgrad (ELU: sv > 0 ? 1 : sv + 1; ReLU: sv > 0) -> act -> + previous y
    (the chain tests/test_gpu_igemm_epilogue.py states); bias broadcasts over dim 1"""
    v = acc.clone()
    if bias is not None:
        v = v + bias.view(1, -1, 1, 1)
    if addend is not None:
        v = v + (addend * (mask > 0).to(addend.dtype) if mask is not None else addend)
    if actgrad == "elu":
        v = v * torch.where(actsrc > 0, torch.ones_like(actsrc), actsrc + 1.0)
    elif actgrad == "relu":
        v = v * (actsrc > 0).to(v.dtype)
    if act == "elu":
        v = F.elu(v)
    elif act == "relu":
        v = v.clamp_min(0.0)
    if prev is not None:
        v = v + prev
    return v


# ---- wrong variants (each a plausible kernel mistake) --------------------------------------------------------------------------------
def wrong_variant(name, gather, src, w, skip=None):
    if name == "zero for reflect":
        assert gather == "reflect"
        return conv_ref("zero", src, w)
    if name == "fold at 0 / n-1":
        assert gather == "dgrad_reflect"
        return fold_ring(F.conv_transpose2d(src, w), 0)
    if name == "up2 before reflect":                       # reflection at half resolution, then nearest x2 of the padded image (`sy >> 1` first)
        assert gather == "up2"
        p = F.interpolate(F.pad(src, (1, 1, 1, 1), mode="reflect"), scale_factor=2, mode="nearest")[:, :, 1:-1, 1:-1]
        if skip is not None:
            p = torch.cat([p, F.pad(skip, (1, 1, 1, 1), mode="reflect")], 1)
        return F.conv2d(p, w)
    if name == "concat one chunk late":                    # the first 16 skip channels still read from the upsampled tensor's last 16
        assert gather == "up2" and skip is not None and skip.shape[1] >= 16 and src.shape[1] >= 16
        up = F.interpolate(src, scale_factor=2, mode="nearest")
        late = torch.cat([up, up[:, -16:], skip[:, 16:]], 1)
        return F.conv2d(F.pad(late, (1, 1, 1, 1), mode="reflect"), w)
    if name == "weights not flipped":
        assert gather in DGRAD_GATHERS
        return conv_ref(gather, src, w.flip(2, 3))
    raise KeyError(name)


def ring_mask(H, W, width=2):
    """True on the outer `width` rows and columns"""
    m = torch.zeros(H, W, dtype=torch.bool)
    m[:width] = m[-width:] = True
    m[:, :width] = m[:, -width:] = True
    return m


def edge_mask(H, W, th, tw):
    """the border ring plus every pixel of a partial last tile row / column"""
    m = ring_mask(H, W)
    if H % th:
        m[H - H % th:] = True
    if W % tw:
        m[:, W - W % tw:] = True
    return m


# ---- inputs --------------------------------------------------------------------------------------------------------------------------
def rnd(shape, seed, lo=-1.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g) * (hi - lo) + lo


def lattice(shape, seed, lo=-4, hi=4, step=1.0):
    """float32 tensor of integers in [lo, hi] times `step`"""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, tuple(shape), generator=g).float() * step


SIDE_VALUES = (-0.75, -0.5, -0.25, 0.0, 0.5, 1.0)        # mask / actsrc: `> 0` both ways, and the ELU-gradient factor sv + 1 is exact


def lattice_side(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.tensor(SIDE_VALUES)[torch.randint(0, len(SIDE_VALUES), tuple(shape), generator=g)]


def _seed(case):
    gather, fmt, N, H, W, C0, C1, Nout = case
    return 7 * H + 13 * W + 3 * C0 + 5 * C1 + Nout + 1000 * GATHERS.index(gather)


def operand_shapes(case):
    """(src, skip or None, w, out) shapes of a tile case (gather, fmt, N, H, W, C0, C1, Nout): H x W is the launch's output; for a data
    gradient C0 = channels of the incoming gradient and Nout = channels of the result, w is the forward weight [C0, Nout, 3, 3]"""
    gather, fmt, N, H, W, C0, C1, Nout = case
    if gather == "up2":
        return (N, C0, H // 2, W // 2), ((N, C1, H, W) if C1 else None), (Nout, C0 + C1, 3, 3), (N, Nout, H, W)
    if gather in DGRAD_GATHERS:
        return (N, C0, H, W), None, (C0, Nout, 3, 3), (N, Nout, H, W)
    return (N, C0, H, W), None, (Nout, C0, 3, 3), (N, Nout, H, W)


def lattice_inputs(case):
    """dict of float32 tensors: src, skip, w, and the epilogue's bias, addend, mask, actsrc, prev"""
    s = _seed(case)
    ss, ks, ws, os_ = operand_shapes(case)
    return {"src": lattice(ss, s), "skip": lattice(ks, s + 1) if ks else None, "w": lattice(ws, s + 2, step=0.125),
            "bias": lattice((os_[1],), s + 3), "addend": lattice(os_, s + 4), "mask": lattice_side(os_, s + 5),
            "actsrc": lattice_side(os_, s + 6), "prev": lattice(os_, s + 7)}


def random_inputs(case):
    """the ranges of tests/test_gpu_kernels.py: activations and gradients in [-1, 1], weights in [-0.1, 0.1]"""
    s = _seed(case) + 50
    ss, ks, ws, os_ = operand_shapes(case)
    return {"src": rnd(ss, s), "skip": rnd(ks, s + 1) if ks else None, "w": rnd(ws, s + 2, -0.1, 0.1), "bias": rnd((os_[1],), s + 3),
            "addend": rnd(os_, s + 4), "actsrc": rnd(os_, s + 6, -0.99, 1.0)}


def wgrad_lattice_inputs(case):
    """(x, dz) of a weight-gradient case (mode, fmt, N, H, W, C0, Nout): integers in [-4, 4]; up2: x at half resolution"""
    mode, fmt, N, H, W, C0, Nout = case
    s = 11 * H + 17 * W + C0 + 3 * Nout + 1000 * FWD_GATHERS.index(mode)
    xs = (N, C0, H // 2, W // 2) if mode == "up2" else (N, C0, H, W)
    return lattice(xs, s), lattice((N, Nout, H, W), s + 1)


def f64(t):
    return None if t is None else t.double()


def case_ref(case, inp, dtype=torch.float64):
    """the plain launch's result for the inputs, evaluated in `dtype`"""
    c = (lambda t: None if t is None else t.to(dtype))
    return conv_ref(case[0], c(inp["src"]), c(inp["w"]), c(inp["skip"]))


def abs_sum_units(case, inp):
    """max over outputs of sum |x| |w| in units of 1/8 (the lattice's product unit): below 2^24 every float32 partial sum is exact"""
    a = {k: (None if v is None else v.abs()) for k, v in inp.items()}
    return float(case_ref(case, a).max()) * 8.0


# cancelling inputs ---------------------------------------------------------------------------------------------------------------------
CANCEL_KINDS = ("x-low", "w-low", "mid-mid")
# x-low / w-low: 2^-19.  At 2^-18 and 64 channels an operand cut to two bf16 terms (the signed terms carry 17 to 18 bits) still lands
# 0.92 from float64, short of the separation the CPU test asks for; at 2^-19 it lands 1.5 away, float32 0.014 and the fp16 pairs 0.034
# mid-mid: the base values are rounded to bf16 (one term) and raised by 2^-9, which is then exactly their middle term: e d = 2^-18 x w is the
# m x m product and nothing else.  (Raising a random float32 by 2^-8 moves its FIRST term half of the time; a kernel without m x m then
# still lands within 0.37.)
CANCEL_DELTA = {"x-low": 2.0 ** -19, "w-low": 2.0 ** -19, "mid-mid": 2.0 ** -9}
CANCEL_DELTA_TWO = {"x-low": 2.0 ** -10, "w-low": 2.0 ** -10}          # the two-term mode (16 significant bits per operand, no m x m)


def _paired(base, dim, pattern, delta):
    """interleave along `dim` the members base * f for f in pattern (1 -> the stored value, "+" -> fl32(value * (1 + delta)),
    "-" -> the negated value, "-+" -> minus the raised value): [.., K, ..] -> [.., len(pattern) * K, ..]"""
    up = (base.double() * (1.0 + delta)).float()
    members = {"1": base, "+": up, "-": -base, "-+": -up}
    st = torch.stack([members[p] for p in pattern], dim + 1)
    shape = list(base.shape)
    shape[dim] *= len(pattern)
    return st.reshape(shape).contiguous()


def cancel_inputs(kind, case, delta=None):
    """src / skip / w for a tile case whose reduction channels come in cancelling pairs (x-low, w-low) or groups of four (mid-mid)"""
    gather, fmt, N, H, W, C0, C1, Nout = case
    delta = CANCEL_DELTA[kind] if delta is None else delta
    xpat, wpat = {"x-low": (("1", "+"), ("1", "-")), "w-low": (("1", "-"), ("1", "+")),
                  "mid-mid": (("1", "+", "1", "+"), ("1", "-", "-+", "+"))}[kind]
    g = len(xpat)
    s = _seed(case) + 100 + CANCEL_KINDS.index(kind)
    ss, ks, ws, _ = operand_shapes(case)
    rdim = 0 if gather in DGRAD_GATHERS else 1                   # the weight's reduction dimension

    one_term = (lambda t: t.bfloat16().float()) if kind == "mid-mid" else (lambda t: t)

    def src_of(shape, seed):
        assert shape[1] % g == 0, (case, kind)
        return _paired(one_term(rnd((shape[0], shape[1] // g) + tuple(shape[2:]), seed)), 1, xpat, delta)

    def w_of(k, seed):
        shape = list(ws)
        shape[rdim] = k // g
        return _paired(one_term(rnd(shape, seed, -0.1, 0.1)), rdim, wpat, delta)
    src = src_of(ss, s)
    skip = src_of(ks, s + 10) if ks else None
    w = w_of(C0, s + 20) if not ks else torch.cat([w_of(C0, s + 20), w_of(C1, s + 30)], rdim)
    return {"src": src, "skip": skip, "w": w}


def bf16_terms(t, n):
    """the first n terms of the exact bf16 split of a float32 tensor (h = bf16(x), m = bf16(x - h), l = bf16(x - h - m)), as float64"""
    out, r = torch.zeros_like(t, dtype=torch.float64), t.clone()
    for _ in range(n):
        term = r.bfloat16().float()
        out += term.double()
        r = r - term
    return out


def fp16_pair_terms(t):
    """the two planes of the scaled fp16-pair format as float64: the largest magnitude maps into [2^12, 2^13), h = fp16(x s), m = fp16(x s - h)"""
    import math
    s = 2.0 ** (12 - math.floor(math.log2(float(t.abs().max()))))
    v = t.double() * s
    h = v.half().double()
    return h / s, (v - h).half().double() / s


def rel_l2(got, ref):
    return float((got.double() - ref).norm() / ref.norm().clamp_min(1e-300))


# ---- the GPU cases -------------------------------------------------------------------------------------------------------------------
# (gather, fmt, N, H, W, C0, C1, Nout); H x W = the launch's output.  The first 30 rows put one launch of each format on every geometry
# that is the smallest of its remainder class (8 x 16 tiles: 8x65 one column, 8x66, 33x16 one row, 26x16, 7x15 a single partial tile,
# 15x82 both axes, 32x40, 8x26; 6 x 20 tiles: 6x121, 6x122, 31x20, 11x19, 16x20), N the smallest the launcher takes, and the weights
# past 4 MiB (wmajor).  The rest was added until the coverage assertion of tests/test_launch_regimes_cpu.py held: each row is there
# for a regime tuple that a train step runs and no earlier row does.
TILE_CASES = [('zero', 'exact', 26, 8, 65, 32, 0, 32),
 ('dgrad', 'pair', 13, 8, 65, 40, 0, 112),
 ('reflect', 'exact', 13, 8, 66, 64, 0, 64),
 ('dgrad_reflect', 'pair', 26, 8, 66, 16, 0, 12),
 ('dgrad', 'exact', 13, 33, 16, 72, 0, 20),
 ('dgrad_reflect', 'pair', 5, 33, 16, 96, 0, 80),
 ('dgrad_reflect', 'exact', 16, 26, 16, 40, 0, 112),
 ('zero', 'pair', 32, 26, 16, 32, 0, 32),
 ('dgrad_reflect', 'exact', 128, 7, 15, 16, 0, 12),
 ('reflect', 'pair', 64, 7, 15, 64, 0, 64),
 ('zero', 'exact', 3, 15, 82, 80, 0, 96),
 ('dgrad', 'pair', 6, 15, 82, 72, 0, 20),
 ('reflect', 'exact', 11, 32, 40, 32, 0, 32),
 ('dgrad_reflect', 'pair', 6, 32, 40, 40, 0, 112),
 ('dgrad', 'exact', 32, 8, 26, 64, 0, 64),
 ('up2', 'pair', 16, 8, 26, 64, 64, 64),
 ('dgrad_reflect', 'exact', 10, 6, 121, 72, 0, 20),
 ('zero', 'pair', 5, 6, 121, 80, 0, 96),
 ('up2', 'exact', 10, 6, 122, 32, 20, 64),
 ('reflect', 'pair', 19, 6, 122, 32, 0, 32),
 ('zero', 'exact', 22, 31, 20, 12, 0, 16),
 ('dgrad', 'pair', 11, 31, 20, 64, 0, 64),
 ('reflect', 'exact', 16, 11, 19, 80, 0, 96),
 ('dgrad_reflect', 'pair', 32, 11, 19, 72, 0, 20),
 ('dgrad', 'exact', 43, 16, 20, 32, 0, 32),
 ('up2', 'pair', 43, 16, 20, 16, 0, 32),
 ('reflect', 'exact', 8, 6, 20, 512, 0, 256),
 ('dgrad_reflect', 'exact', 4, 16, 20, 256, 0, 512),
 ('reflect', 'pair', 8, 6, 20, 512, 0, 256),
 ('dgrad_reflect', 'pair', 4, 16, 20, 256, 0, 512),
 ('dgrad_reflect', 'pair', 22, 16, 20, 20, 0, 72),
 ('dgrad_reflect', 'exact', 32, 16, 32, 12, 0, 16),
 ('dgrad_reflect', 'exact', 32, 8, 26, 64, 0, 40),
 ('dgrad', 'exact', 22, 16, 20, 20, 0, 72),
 ('dgrad_reflect', 'exact', 11, 6, 122, 20, 0, 72),
 ('dgrad_reflect', 'pair', 26, 16, 52, 20, 0, 72),
 ('reflect', 'pair', 22, 16, 20, 20, 0, 72),
 ('up2', 'exact', 32, 26, 16, 16, 0, 32),
 ('dgrad_reflect', 'pair', 32, 26, 16, 16, 0, 32),
 ('up2', 'pair', 64, 8, 26, 16, 0, 32),
 ('zero', 'pair', 16, 26, 16, 20, 0, 72),
 ('zero', 'pair', 26, 16, 52, 20, 0, 72),
 ('dgrad', 'pair', 26, 16, 52, 20, 0, 72),
 ('dgrad_reflect', 'pair', 2, 6, 20, 512, 0, 256),
 ('up2', 'exact', 1, 8, 26, 256, 256, 256),
 ('dgrad', 'exact', 2, 6, 20, 512, 0, 256),
 ('up2', 'pair', 2, 6, 20, 256, 256, 256),
 ('dgrad_reflect', 'pair', 1, 8, 26, 512, 0, 256),
 ('zero', 'exact', 16, 26, 16, 20, 0, 72),
 ('dgrad', 'exact', 16, 26, 16, 20, 0, 72),
 ('zero', 'exact', 32, 11, 19, 20, 0, 72),
 ('dgrad', 'pair', 64, 6, 20, 20, 0, 72),
 ('dgrad_reflect', 'exact', 32, 26, 16, 32, 0, 32),
 ('dgrad', 'pair', 16, 26, 16, 64, 0, 64),
 ('dgrad_reflect', 'exact', 1, 8, 26, 512, 0, 256),
 ('reflect', 'pair', 32, 26, 16, 12, 0, 16),
 ('zero', 'pair', 68, 16, 20, 20, 0, 72),
 ('dgrad', 'pair', 68, 16, 20, 20, 0, 72),
 ('up2', 'pair', 26, 26, 16, 64, 64, 64),
 ('dgrad', 'pair', 32, 8, 26, 20, 0, 72),
 ('dgrad', 'pair', 1, 6, 121, 512, 0, 256),
 ('dgrad_reflect', 'pair', 16, 12, 40, 20, 0, 72),
 ('dgrad_reflect', 'pair', 32, 6, 121, 20, 0, 72),
 ('dgrad_reflect', 'pair', 32, 26, 16, 32, 0, 32),
 ('dgrad', 'pair', 13, 26, 16, 128, 0, 128),
 ('dgrad_reflect', 'pair', 13, 26, 16, 128, 0, 128),
 ('dgrad_reflect', 'pair', 16, 26, 16, 64, 0, 40),
 ('zero', 'pair', 1, 8, 26, 1024, 0, 256),
 ('dgrad', 'exact', 1, 8, 26, 1024, 0, 256),
 ('up2', 'exact', 11, 16, 20, 64, 64, 64),
 ('reflect', 'pair', 26, 16, 52, 20, 0, 72),
 ('dgrad_reflect', 'pair', 43, 8, 65, 20, 0, 72),
 ('zero', 'exact', 32, 8, 65, 64, 0, 32),
 ('zero', 'pair', 32, 8, 65, 64, 0, 32),
 ('zero', 'exact', 32, 8, 65, 64, 0, 40),
 ('dgrad', 'pair', 32, 8, 65, 64, 0, 40),
 ('dgrad_reflect', 'exact', 32, 8, 65, 64, 0, 40),
 ('dgrad_reflect', 'pair', 32, 8, 65, 64, 0, 40),
 ('zero', 'exact', 81, 11, 19, 64, 0, 40),
 ('zero', 'pair', 81, 11, 19, 64, 0, 40),
 ('dgrad', 'exact', 81, 11, 19, 64, 0, 40),
 ('dgrad', 'pair', 81, 11, 19, 64, 0, 40),
 ('dgrad_reflect', 'exact', 81, 11, 19, 64, 0, 40),
 ('dgrad_reflect', 'pair', 81, 11, 19, 64, 0, 40),
 ('zero', 'pair', 7, 7, 15, 512, 0, 256),
 ('zero', 'pair', 81, 8, 65, 64, 0, 40),
 ('dgrad', 'pair', 81, 8, 65, 64, 0, 40),
 ('dgrad_reflect', 'pair', 81, 8, 65, 64, 0, 40),
 ('zero', 'pair', 68, 31, 20, 64, 0, 40),
 ('dgrad', 'pair', 68, 31, 20, 64, 0, 40)]

# split-K edges no train step runs today: a ragged last split of ONE chunk (112 channels: 3 + 3 + 1, SK % 4 = 3; the concat gather with the
# switch to the skip tensor on a split boundary), and unsplit loops of five and seven chunks on both tile shapes
TILE_CASES += [("reflect", "exact", 9, 8, 65, 112, 0, 40), ("reflect", "pair", 9, 8, 65, 112, 0, 40), ("up2", "exact", 9, 8, 66, 48, 64, 40),
               ("up2", "pair", 9, 8, 66, 48, 64, 40), ("dgrad_reflect", "exact", 9, 8, 65, 112, 0, 40), ("dgrad", "pair", 9, 33, 16, 112, 0, 40),
               ("zero", "exact", 32, 8, 65, 80, 0, 32), ("dgrad_reflect", "pair", 23, 6, 121, 112, 0, 32), ("reflect", "exact", 23, 6, 121, 80, 0, 96),
               ("up2", "pair", 13, 8, 66, 32, 20, 64), ("up2", "exact", 16, 26, 16, 32, 20, 64)]      # the skip tensor's channel tail on 8 x 16 tiles

# the opt-in two-term inference mode (forward gathers only), selected the way Engine.forward selects it
TILE_TWO_TERM = [("zero", "two", 13, 8, 65, 64, 0, 64), ("reflect", "two", 6, 32, 40, 20, 0, 72), ("up2", "two", 10, 6, 122, 32, 20, 64)]

# cancelling inputs: (gather, fmt, N, H, W, C0, C1, Nout), one aligned and one ragged geometry per format and family
CANCEL_CASES = [(g, f) + s for f in ("exact", "pair") for g in ("reflect", "dgrad", "dgrad_reflect")
                for s in ((6, 32, 48, 64, 0, 64), (13, 8, 65, 64, 0, 64))]
CANCEL_TWO_TERM = [("reflect", "two", 6, 32, 48, 64, 0, 64), ("reflect", "two", 13, 8, 65, 64, 0, 64)]

# weight gradients: (mode, fmt, N, H, W, C0, Nout).  First the shapes picked by hand for the chunk remainders, the transposing reduce
# (512 -> 256), the capped plain reduce (480 -> 256) and 256 -> 256 at 8x26, in every mode the shape allows; then the rows the coverage
# assertion asked for
_WGRAD_SHAPES = [(4, 8, 65, 32, 32), (2, 33, 16, 32, 64), (3, 26, 16, 64, 32), (16, 7, 15, 32, 32), (2, 15, 82, 32, 96), (6, 10, 34, 32, 32),
                 (1, 24, 70, 32, 32), (3, 13, 35, 96, 32), (5, 6, 122, 32, 32), (4, 16, 20, 512, 256), (4, 6, 20, 480, 256), (12, 8, 26, 256, 256)]
WGRAD_CASES = [(m, f) + s for s in _WGRAD_SHAPES for m in ("zero", "reflect", "up2") if m != "up2" or (s[1] % 2 == 0 and s[2] % 2 == 0)
               for f in ("exact", "pair")]
WGRAD_CASES += [c for c in [('zero', 'exact', 2, 10, 36, 32, 32),
 ('zero', 'pair', 2, 10, 36, 32, 32),
 ('reflect', 'exact', 2, 10, 36, 32, 32),
 ('reflect', 'pair', 2, 10, 36, 32, 32),
 ('up2', 'exact', 2, 12, 40, 32, 32),
 ('up2', 'pair', 2, 12, 40, 32, 32),
 ('reflect', 'exact', 3, 16, 20, 32, 32),
 ('reflect', 'pair', 3, 16, 20, 32, 32),
 ('zero', 'exact', 22, 4, 13, 32, 32),
 ('zero', 'pair', 22, 4, 13, 32, 32),
 ('reflect', 'exact', 4, 26, 16, 32, 32),
 ('reflect', 'pair', 4, 26, 16, 32, 32),
 ('up2', 'exact', 4, 26, 16, 32, 32),
 ('up2', 'pair', 4, 26, 16, 32, 32),
 ('zero', 'exact', 7, 6, 20, 32, 32),
 ('zero', 'pair', 7, 6, 20, 32, 32),
 ('reflect', 'exact', 9, 6, 20, 32, 32),
 ('reflect', 'pair', 9, 6, 20, 32, 32),
 ('zero', 'exact', 3, 33, 16, 32, 32),
 ('zero', 'pair', 3, 33, 16, 32, 32),
 ('up2', 'exact', 7, 8, 66, 32, 32),
 ('up2', 'pair', 7, 8, 66, 32, 32),
 ('zero', 'exact', 4, 6, 20, 512, 256),
 ('zero', 'pair', 4, 6, 20, 512, 256),
 ('reflect', 'exact', 4, 6, 20, 512, 256),
 ('reflect', 'pair', 4, 6, 20, 512, 256)] if c not in WGRAD_CASES]
