"""Float64 references, planted inputs and DERIVED bounds for the two training losses (csrc/loss_adam_misc.hip loss_kernel +
loss_final_kernel, csrc/seg_loss.hip), shared by tests/test_loss_refs_cpu.py (are the references right, do the planted regimes occur,
can the bounds see a wrong formula?) and tests/test_gpu_losses.py (do the kernels stay inside them?).  Nothing here touches a GPU.

Every bound has the shape of the anchored rule of tests/parity.py:  err(GPU vs float64) <= FACTOR * max(err(CPU float32 vs float64),
floor), FACTOR = 4.  The CPU term is the oracle's own float32 arithmetic on the same inputs.  The floor is derived:
  * a reduced value: the first-order summation bound of tests/launch_regimes.py over the kernel's chain length, plus a per-term
    evaluation allowance (the roundings inside one pixel's term, written out at `_bce_parts` / `_depth_parts` / `seg_loss_ref`);
  * a Footprints gradient element: 8 * 2^-24 of its plane's float64 maximum (one sigmoid or one reciprocal-square, two multiplies, the
    scale);
  * a segmentation gradient element of the map of scale S: (4 S^2 + 8) * 2^-24 of the map's maximum (the non-zero weights the gather adds).
None of them was fitted to what a kernel returned.

`variant` evaluates a WRONG formula with the same float64 arithmetic (the CPU test asks whether the bounds can tell it from the right one).
"""
import functools
from collections import OrderedDict, namedtuple
from types import SimpleNamespace

import torch
import torch.nn.functional as F

from oracle import filler
from oracle import restatement as R
from tests import launch_regimes as LR
from tests.parity import FACTOR, TIE

U = LR.U
FLUSH = 2.0 ** -125                 # a term that is denormal in float32 may be flushed to zero
GRAD_FLOOR = 8 * U                  # of the plane's maximum
TARGET_KEYS = ("visible_ground", "all_ground", "depth", "ground_depth", "moving_object_mask", "depth_mask")

# ---- planted pixels of the Footprints loss -------------------------------------------------------------------------------------------
LOGITS = (0.0, 1e-4, -1e-4, 30.0, -30.0, 88.0, -88.0, 104.0, -104.0)      # expf(104) = inf, expf(-88) is denormal, log1pf(expf(-30)) ~ 1e-13
SATURATED = 88.0                    # |logit| from which expf leaves the normal range
TINY = 2.0 ** -126                  # the smallest normal float32: a valid depth (> 0) that no subtraction can see
DEPTH_TARGETS = (0.0, TINY, 80.0)
N_PLANT = 8 * len(LOGITS)           # pixels 0 .. 71 of every image: eight mask combinations x nine logits
N_EXACT = 2                         # pixels 72, 73 (exact-kink range only): predicted depth == target on both depth channels
EXACT_RANGE = (0.125, 64.0)         # min_disp = 1/64 and disp_range = 7.984375 are exact in float32: disparity 0 -> 64, 1 -> 0.125

FpCase = namedtuple("FpCase", "name B H W tag planted depth_range prior zero_depth")
FP_CASES = [
    FpCase("1x5x7", 1, 5, 7, "lossedge5x7", False, (0.1, 100.0), 0.25, False),
    FpCase("3x40x72", 3, 40, 72, "lossbig", True, (0.1, 100.0), 0.25, False),
    FpCase("3x40x72-range", 3, 40, 72, "lossbig", True, EXACT_RANGE, 0.4, False),
    FpCase("2x40x72-nodepth", 2, 40, 72, "lossnodepth", True, (0.1, 100.0), 0.25, True),
    FpCase("2x160x208", 2, 160, 208, "loss65", False, (0.1, 100.0), 0.25, False),
    FpCase("2x1024x1030", 2, 1024, 1030, "losscap", False, (0.1, 100.0), 0.25, False),
]
FP_BY_NAME = {c.name: c for c in FP_CASES}


def plant_plan(j, scale):
    """what pixel j < N_PLANT of every image holds at prediction `scale` -> (logit, vg, ag, dm, mov, disp2, depth, disp3, gdepth)"""
    c = j % 8
    ag, dm, mov = c & 1, (c >> 1) & 1, (c >> 2) & 1
    k2, k3 = j % 6, (j + 3) % 6
    return (LOGITS[(j // 8 + scale) % len(LOGITS)], dm, ag, dm, mov, float(k2 % 2), DEPTH_TARGETS[k2 // 2], float(k3 % 2), DEPTH_TARGETS[k3 // 2])


def fp_inputs(case):
    """-> (preds: four float32 [B,4,H,W], channels 0/1 logits in [-4, 4), channels 2/3 disparities in (0, 1); targets: OrderedDict of
    float32 [B,H,W]).  Dense filler values, then the planted block over the first pixels of every image."""
    B, H, W = case.B, case.H, case.W
    u, bern = filler.uniform, filler.bernoulli
    tag = case.tag
    t = OrderedDict()                                   # R.make_batch's distributions without its image
    t["visible_ground"] = torch.from_numpy(bern(tag + ":vg", (B, H, W), 0.4))
    t["depth"] = torch.from_numpy(u(tag + ":depth", (B, H, W), 0.0, 80.0) * bern(tag + ":dv", (B, H, W), 0.8))
    t["ground_depth"] = torch.from_numpy(u(tag + ":gdepth", (B, H, W), 0.0, 30.0) * bern(tag + ":gv", (B, H, W), 0.5))
    t["moving_object_mask"] = torch.from_numpy(bern(tag + ":mov", (B, H, W), 0.05))
    t["depth_mask"] = torch.from_numpy(bern(tag + ":dm", (B, H, W), 0.1))
    t["all_ground"] = ((t["ground_depth"] + t["visible_ground"]) > 0).float()
    preds = []
    for i in range(4):
        p = torch.from_numpy(u("%s:pred%d" % (tag, i), (B, 4, H, W), -4.0, 4.0))
        p[:, 2:] = torch.sigmoid(p[:, 2:])
        preds.append(p)
    if case.planted:
        flat = {k: v.view(B, H * W) for k, v in t.items()}
        for j in range(N_PLANT):
            for i, p in enumerate(preds):
                x, vg, ag, dm, mov, o2, dep, o3, gdep = plant_plan(j, i)
                pf = p.view(B, 4, H * W)
                pf[:, 0, j], pf[:, 1, j], pf[:, 2, j], pf[:, 3, j] = x, x, o2, o3
            flat["visible_ground"][:, j], flat["all_ground"][:, j], flat["depth_mask"][:, j] = vg, ag, dm
            flat["moving_object_mask"][:, j], flat["depth"][:, j], flat["ground_depth"][:, j] = mov, dep, gdep
        if tuple(case.depth_range) == EXACT_RANGE:
            lo, hi = case.depth_range
            for n, (o2, dep, o3, gdep) in enumerate(((0.0, hi, 1.0, lo), (1.0, lo, 0.0, hi))):
                j = N_PLANT + n
                for p in preds:
                    pf = p.view(B, 4, H * W)
                    pf[:, 2, j], pf[:, 3, j] = o2, o3
                flat["depth"][:, j], flat["ground_depth"][:, j] = dep, gdep
    if case.zero_depth:
        t["depth"].zero_()
        t["ground_depth"].zero_()
    return preds, t


def planted_counts(case):
    """what fp_inputs planted, as the CPU test counts it: pixels per (all_ground, depth_mask, moving) combination inside the block,
    saturated logits and exact-kink elements in the whole case"""
    if not case.planted:
        return {"combo": 0, "saturated": 0, "exact_kink": 0}
    sat = sum(abs(x) >= SATURATED for x in LOGITS) * 8 * 2 * 4 * case.B
    exact = N_EXACT * 2 * 4 * case.B if (tuple(case.depth_range) == EXACT_RANGE and not case.zero_depth) else 0
    return {"combo": len(LOGITS) * case.B, "saturated": sat, "exact_kink": exact}


# ---- Footprints loss in float64 ------------------------------------------------------------------------------------------------------
def _bce_parts(x, t):
    """-> (term, magnitude, allowance) of max(x, 0) - x t + log1p(exp(-|x|)) per element.  Float32 evaluation: t is 0 or 1, so x t is exact;
    expf within 2 u moves log1p(z) by <= 2 u z / (1 + z) <= 2 u log1p(z); log1pf within 2 u; two additions, each within u of a partial sum
    that the magnitude bounds: allowance = u (4 c + 2 (a + |b| + c)) + one flushed denormal.  max(x, 0) is written (x + |x|) / 2 so that
    autograd gives sigmoid(0) - t = 1/2 - t at a logit of exactly 0 (clamp's one-sided derivative would give 1 - t)"""
    a, b, c = 0.5 * (x + x.abs()), x * t, torch.log1p(torch.exp(-x.abs()))
    mag = a + b.abs() + c
    return a - b + c, mag, U * (4 * c + 2 * mag) + FLUSH


def _depth_parts(o, target, lo, hi, valid, sign0_is_1=False):
    """-> (term, magnitude, allowance, d) of log(|1 / (lo + (hi - lo) o) - target| + 1) * valid.  Float32 evaluation: lo and hi - lo are
    rounded once each, the product and the sum once each (all terms positive: 3 u on the sum), the reciprocal once: d within 4 u d;
    e = d - target within 4 u d + u |e|; y = |e| + 1 within that + u y; logf within 2 u:
    allowance = u (4 d + |e| + y) / y + 2 u log y"""
    d = 1 / (lo + (hi - lo) * o)
    e = d - target
    ae = torch.where(e >= 0, e, -e) if sign0_is_1 else e.abs()
    y = ae + 1
    term = torch.log(y) * valid
    dd, yy = d.detach(), y.detach()
    return term, term.detach().abs(), valid * (U * (4 * dd + (yy - 1) + yy) / yy + 2 * U * torch.log(yy)), dd


VARIANTS_FP = ("no_keep", "no_depth_mask", "no_prior", "prior_off", "no_valid", "sign0")


def footprints_loss_ref(preds64, targets64, depth_range=(0.1, 100.0), prior=0.25, variant=None):
    """A straightforward restatement of training/losses.py:31-152 in the dtype of its inputs (float64 for the reference).
    -> namespace: values [21] in R.LOSS_KEYS order; grads: four [B,4,H,W] (autograd); kink [4,2,B,H,W] bool: |d - target| <= TIE *
    max(target, 1) & target > 0 per scale and depth channel; exact: the same with |d - target| == 0; means [16], abs_terms [16],
    allow [16]: per scale (visible_ground, all_ground, depth, ground_depth) the mean, the sum of the terms' magnitudes and the sum of
    their evaluation allowances"""
    assert variant in (None,) + VARIANTS_FP
    T = targets64
    vg, ag, depth, gdepth = T["visible_ground"], T["all_ground"], T["depth"], T["ground_depth"]
    keep = torch.ones_like(vg) if variant == "no_keep" else 1 - T["moving_object_mask"]
    m = ((ag > 0) if variant == "no_depth_mask" else ((ag + T["depth_mask"]) > 0)).to(vg.dtype)
    ones = torch.ones_like(depth)
    vd, vgd = (ones, ones) if variant == "no_valid" else ((depth > 0).to(vg.dtype), (gdepth > 0).to(vg.dtype))
    pw = {"no_prior": 0.0, "prior_off": prior * 1.001}.get(variant, prior)
    lo, hi = 1 / depth_range[1], 1 / depth_range[0]
    preds = [p.detach().clone().requires_grad_(True) for p in preds64]
    n = vg.numel()
    values, means, mags, allows, kink, exact = [], [], [], [], [], []
    total = 0
    for o in preds:
        t0, m0, a0 = _bce_parts(o[:, 0], vg)
        ta, ma, aa = _bce_parts(o[:, 1], ag)
        tz, mz, az = _bce_parts(o[:, 1], torch.zeros_like(ag))
        w1, w0 = m * keep, pw * (1 - m)
        t1 = ta * w1 + tz * w0                           # the prior is rounded to float32 and multiplied in: u bce each; the sum: u |term|
        m1, a1 = ma * w1 + mz * w0, (aa * w1 + (az + 2 * U * mz) * w0 + U * (ma * w1 + mz * w0)).detach()
        t2, m2, a2, d2 = _depth_parts(o[:, 2], depth, lo, hi, vd, variant == "sign0")
        t3, m3, a3, d3 = _depth_parts(o[:, 3], gdepth, lo, hi, vgd, variant == "sign0")
        four = [t.mean() for t in (t0, t1, t2, t3)]
        ls = four[2] + four[0] + four[1] + four[3]
        total = total + ls
        values += four + [ls]
        means += [v.detach() for v in four]
        mags += [x.detach().sum() for x in (m0, m1, m2, m3)]
        allows += [x.detach().sum() for x in (a0, a1, a2, a3)]
        ks, es = [], []
        for d, tg in ((d2, depth), (d3, gdepth)):
            ks.append(((d - tg).abs() <= TIE * tg.clamp_min(1.0)) & (tg > 0))
            es.append(((d - tg) == 0) & (tg > 0))
        kink.append(torch.stack(ks))
        exact.append(torch.stack(es))
    loss = total / 4
    loss.backward()
    return SimpleNamespace(values=torch.stack([v.detach() for v in values] + [loss.detach()]), grads=[p.grad for p in preds], kink=torch.stack(kink),
                           exact=torch.stack(exact), means=torch.stack(means), abs_terms=torch.stack(mags), allow=torch.stack(allows), n=n)


def loss_value_floor(ref):
    """[21] derived bounds of the values the kernel reports, from the float64 evaluation `ref`: a term mean carries the summation bound
    over loss_kernel + loss_final_kernel's chain and its pixels' evaluation allowances, then the scaling by 1 / n and the rounding to
    float32 (2 u); a scale's loss adds four of them (3 u on the magnitudes); the total adds four of those and divides (5 u)"""
    L = LR.loss_chain(ref.n)
    b16 = (LR.sum_bound(L, 0, ref.abs_terms, ref.means * ref.n) + ref.allow) / ref.n + U * ref.means.abs()
    out = []
    lsb, lsm = [], []
    for s in range(4):
        b = b16[4 * s:4 * s + 4]
        out += list(b)
        mag = ref.means[4 * s:4 * s + 4].abs().sum()
        lsb.append(b.sum() + 3 * U * mag)
        lsm.append(mag)
        out.append(lsb[-1])
    out.append(sum(lsb) / 4 + 5 * U * sum(lsm) / 4)
    return torch.stack(out)


def oracle_loss(preds, targets, dtype, depth_range, prior):
    """the project's CPU oracle (oracle/restatement.py loss_manager) in `dtype` -> (values [21] float64, grads)"""
    pr = OrderedDict((k, p.detach().to(dtype).requires_grad_(True)) for k, p in zip(R.SCALES, preds))
    losses, _ = R.loss_manager(pr, OrderedDict((k, v.to(dtype)) for k, v in targets.items()), depth_range=depth_range, prior=prior)
    losses["loss"].backward()
    return torch.stack([losses[k].detach().double() for k in R.LOSS_KEYS]), [pr[k].grad for k in R.SCALES]


def anchored(err_cpu, floor):
    """the bound of the anchored rule; tensors or floats"""
    if torch.is_tensor(err_cpu) or torch.is_tensor(floor):
        return FACTOR * torch.maximum(torch.as_tensor(err_cpu, dtype=torch.float64), torch.as_tensor(floor, dtype=torch.float64))
    return FACTOR * max(err_cpu, floor)


def plane_err(got, ref, sel=None):
    """max |got - ref| over the selected elements of one plane (absolute; the caller divides by the plane's maximum)"""
    d = (got.detach().double().cpu() - ref.double()).abs()
    if sel is not None:
        d = d[sel]
    return float(d.max()) if d.numel() else 0.0


@functools.lru_cache(maxsize=1)
def fp_reference(name):
    """everything the checks of one Footprints case need, computed once: inputs, float64 reference, CPU float32 oracle, value bounds"""
    case = FP_BY_NAME[name]
    preds, targets = fp_inputs(case)
    ref = footprints_loss_ref([p.double() for p in preds], OrderedDict((k, v.double()) for k, v in targets.items()), case.depth_range, case.prior)
    v32, g32 = oracle_loss(preds, targets, torch.float32, case.depth_range, case.prior)
    floor = loss_value_floor(ref)
    return SimpleNamespace(case=case, preds=preds, targets=targets, ref=ref, v32=v32, g32=g32, value_floor=floor,
                           value_bound=anchored((v32 - ref.values).abs(), floor))


def fp_plane_selections(r, s, ch):
    """the element sets one gradient plane (scale s, channel ch) is compared over -> list of (label, bool [B,H,W] selection or None)
    and, for a depth channel, the kink selection.  `all`: every element off the kink, relative to the plane's own maximum (a planted
    d = 100 pixel carries ~1e3 times an ordinary pixel's gradient and sets that maximum); `dense`: in a planted case, the unplanted pixels
    on their own, relative to THEIR maximum, so the ordinary pixels are not measured against the planted ones"""
    case = r.case
    kink = r.ref.kink[s, ch - 2] if ch >= 2 else None
    off = None if kink is None else ~kink
    sels = [("all", off)]
    if case.planted:
        dense = torch.ones(case.B, case.H * case.W, dtype=torch.bool)
        dense[:, :N_PLANT + N_EXACT] = False
        dense = dense.view(case.B, case.H, case.W)
        sels.append(("dense", dense if off is None else dense & off))
    return sels, kink


def fp_zero_masks(r, s):
    """per channel 1..3 of scale s: where the reference gradient is exactly 0 BY A MASK (moving == 1 where m == 1; depth == 0; the exact kink)"""
    T = r.targets
    m = (T["all_ground"] + T["depth_mask"]) > 0
    return {1: m & (T["moving_object_mask"] == 1), 2: (T["depth"] == 0) | r.ref.exact[s, 0], 3: (T["ground_depth"] == 0) | r.ref.exact[s, 1]}


# ---- segmentation loss ---------------------------------------------------------------------------------------------------------------
SegCase = namedtuple("SegCase", "name B H W sizes planted backward")
SEG_CASES = [
    SegCase("1x8x8", 1, 8, 8, None, False, True),
    SegCase("2x16x24-one-none", 2, 16, 24, None, False, True),
    SegCase("3x64x96", 3, 64, 96, None, True, True),
    SegCase("2x136x128", 2, 136, 128, None, False, True),
    SegCase("2x512x1032", 2, 512, 1032, None, False, True),      # B H W above 4096 * 256: seg_down_kernel's grid is capped at scale 1, as at 12x192x640
    SegCase("2x20x28-fractional", 2, 20, 28, ((3, 4), (5, 7), (10, 14), (20, 28)), False, False),
]
SEG_BY_NAME = {c.name: c for c in SEG_CASES}
VARIANTS_SEG = ("no_eps", "all_pixels", "align_corners")


def seg_sizes(case):
    return case.sizes or tuple((case.H // s, case.W // s) for s in (8, 4, 2, 1))


def seg_inputs(case):
    """-> (maps: four float32 [B,1,h,w] logits in [-4, 4), ground [B,H,W] 0/1, labelled [B,H,W] 0/1)"""
    B, H, W = case.B, case.H, case.W
    tag = "segedge:" + case.name
    maps = [torch.from_numpy(filler.uniform("%s:map%d" % (tag, i), (B, 1, h, w), -4.0, 4.0)) for i, (h, w) in enumerate(seg_sizes(case))]
    ground = torch.from_numpy(filler.bernoulli(tag + ":ground", (B, H, W), 0.4))
    labelled = torch.from_numpy(filler.bernoulli(tag + ":labelled", (B, H, W), 0.7))
    if case.name == "2x16x24-one-none":
        labelled.zero_()
        labelled[0, H - 1, W - 1] = 1.0                 # image 0: one labelled pixel, in a corner; image 1: none
    elif case.B > 1:
        labelled[0, : H // 2] = 0.0                     # an image with a large unlabelled region
    if case.planted:                                    # the logit edges along the first row and the last column of every map, both targets
        for mp in maps:
            h, w = mp.shape[2:]
            for j in range(min(w, 2 * len(LOGITS))):
                mp[:, 0, 0, j] = LOGITS[j % len(LOGITS)]
            for j in range(min(h, 2 * len(LOGITS))):
                mp[:, 0, h - 1 - j, w - 1] = LOGITS[j % len(LOGITS)]
        ground[:, 0, ::2], ground[:, 0, 1::2] = 1.0, 0.0
        labelled[:, 0, :] = 1.0
        labelled[:, :, W - 1] = 1.0
        ground[:, ::2, W - 1], ground[:, 1::2, W - 1] = 0.0, 1.0
    return maps, ground, labelled


def _pow2_ratio(n_out, n_in):
    q = n_out // n_in
    return n_out % n_in == 0 and q & (q - 1) == 0


def seg_loss_ref(maps64, ground, labelled, H, W, variant=None, backward=True):
    """segmentation/train.py:184-193 + evaluation.py:39-58 in the dtype of its inputs -> namespace: values [5 B + 1] in seg_final_kernel's
    layout (scale-major per-image means, their average per image, the batch mean); grads: four maps; valid [B]; abs_terms, allow [4,B]:
    per scale and image the sum of the labelled terms' magnitudes and of their evaluation allowances.
    Allowance of one term: the sampled logit v is three lerps of four corners (6 u max|corner|; the weights are exact where out / in is a
    power of two, else the source coordinate (dst + 0.5) r - 0.5 carries 2 u (s + 1) per axis against a span of 2 max|corner|), BCE moves
    by at most |dv| (|sigmoid - t| <= 1), plus the BCE's own roundings (_bce_parts)"""
    assert variant in (None,) + VARIANTS_SEG
    B = ground.shape[0]
    maps = [m.detach().clone().requires_grad_(True) for m in maps64]
    lab = torch.ones_like(labelled) if variant == "all_pixels" else labelled
    valid = lab.sum(dim=[1, 2])
    den = valid if variant == "no_eps" else valid + 1e-7
    per, mags, allows = [], [], []
    for mp in maps:
        h, w = mp.shape[2:]
        pred = F.interpolate(mp, size=(H, W), mode="bilinear", align_corners=(variant == "align_corners")).squeeze(1)
        term, mag, allow = _bce_parts(pred, ground)
        amax = mp.detach().abs().amax(dim=(1, 2, 3)).view(B, 1, 1)
        werr = (0.0 if _pow2_ratio(H, h) else 2 * U * (h + 1)) + (0.0 if _pow2_ratio(W, w) else 2 * U * (w + 1))
        allow = allow.detach() + (6 * U + 2 * werr) * amax
        per.append((term * lab).sum(dim=[1, 2]) / den)
        mags.append((mag.detach() * lab).sum(dim=[1, 2]))
        allows.append((allow * lab).sum(dim=[1, 2]))
    avg = (per[0] + per[1] + per[2] + per[3]) / 4
    loss = avg.mean()
    if backward:
        loss.backward()
    return SimpleNamespace(values=torch.cat([p.detach() for p in per] + [avg.detach(), loss.detach().view(1)]), grads=[m.grad for m in maps],
                           valid=valid.detach(), abs_terms=torch.stack(mags), allow=torch.stack(allows), B=B, HW=H * W)


def seg_value_floor(ref):
    """[5 B + 1] derived bounds: a per-scale mean is a sum over seg_loss_kernel + seg_final_kernel's chain divided by valid + 1e-7 (the
    labelled count is a sum of 0/1 below 2^24: exact; the epsilon's rounding and the division: 3 u); the average adds four and divides
    (4 u on the magnitudes); the batch mean adds B of those and divides"""
    L = LR.seg_loss_chain(ref.HW)
    B = ref.B
    v = ref.values
    den = (ref.valid + 1e-7).view(1, B)
    vs = v[:4 * B].view(4, B)
    b = (LR.sum_bound(L, 0, ref.abs_terms, vs * den) + ref.allow) / den + 2 * U * vs.abs()
    mag = v[:4 * B].view(4, B).abs().sum(0)
    bavg = b.sum(0) / 4 + 4 * U * mag / 4
    btot = bavg.sum() / B + (B + 1) * U * v[4 * B:5 * B].abs().sum() / B
    return torch.cat([b.reshape(-1), bavg, btot.view(1)])


def seg_grad_floor(case, s):
    h, w = seg_sizes(case)[s]
    S = max(case.H // h, case.W // w)
    return (4 * S * S + 8) * U


@functools.lru_cache(maxsize=1)
def seg_reference(name):
    case = SEG_BY_NAME[name]
    maps, ground, labelled = seg_inputs(case)
    ref = seg_loss_ref([m.double() for m in maps], ground.double(), labelled.double(), case.H, case.W, backward=case.backward)
    c32 = seg_loss_ref(maps, ground, labelled, case.H, case.W, backward=case.backward)
    floor = seg_value_floor(ref)
    return SimpleNamespace(case=case, maps=maps, ground=ground, labelled=labelled, ref=ref, c32=c32, value_floor=floor,
                           value_bound=anchored((c32.values.double() - ref.values).abs(), floor))


def tracked_ref(values, B):
    """what SegmentationLoss.tracked() reports after one call: the means over the images of each key's per-image values"""
    out = {"ground_loss_%d" % s: float(values[s * B:(s + 1) * B].mean()) for s in range(4)}
    out["loss"] = float(values[4 * B:5 * B].mean())
    return out


# ---- shared reporting ----------------------------------------------------------------------------------------------------------------
def value_ratios(got, ref_values, bound):
    """per value error / bound; a value with bound 0 must be exact"""
    err = (got.detach().double().cpu() - ref_values).abs()
    return torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
