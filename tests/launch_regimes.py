"""The host launch arithmetic of the step's non-convolution kernels and (at the end) of the 3x3 stride-1 tile kernels and the nearest-x2 phase kernels, restated in plain Python, and what follows from it for a
test: which launch REGIME a shape runs in, and how long the longest chain of dependent float32 additions behind one reduced output is.

Every function names the file:line it restates.  tests/test_launch_regimes_cpu.py sweeps these against the library's own answers
(the workspace queries and fp_head_grid), so a changed launch rule fails there before the small GPU shapes silently stop reaching
what the product runs.

A regime is a small tuple; a launch maps to a frozenset of them (a head launch holds workgroups of several kinds: full row groups, the
tail group, the part-dead last column block).  "covered" means: every tuple the workload produces is produced by some GPU case.
"""
import math

U = 2.0 ** -24            # unit roundoff of float32 (round to nearest)


def ceil_div(a, b):
    return -(-a // b)


# ---- grids -------------------------------------------------------------------------------------------------------------------------
def head_grid(N, H, W, Cin, max_rows=16):
    """csrc/head.hip:597 head_grid -> (colblocks, rows, groups per image); fp_head_grid answers the same"""
    colblocks = ceil_div(W * (Cin // 4), 256)
    rows = max_rows
    while rows > 4 and colblocks * N * ceil_div(H, rows) < 2048:
        rows >>= 1
    return colblocks, rows, ceil_div(H, rows)


def head_wgrad_blocks(M, Cin):
    """csrc/head.hip:606 head_wgrad_blocks"""
    ppb = 256 // (Cin // 4)
    return max(1, min(1024, ceil_div(M, ppb * 8)))


def bn_blocks(M, C, iters=4):
    """csrc/bn_pool.hip:20 bn_blocks (FP_BN_ROWS_PER_THREAD unset: 4 rows per thread)"""
    rows = 256 // (C // 4)
    return max(1, min(512, ceil_div(M, rows * iters)))


def colsum_blocks(M, C):
    """csrc/loss_adam_misc.hip:153 colsum_blocks"""
    rows = 256 // (C // 4)
    return max(1, min(512, ceil_div(M, rows * 16)))


def loss_blocks(npix):
    """csrc/loss_adam_misc.hip:109 loss_blocks"""
    return max(1, min(2048, ceil_div(npix, 256 * 4)))


SEG_BLK = 64              # csrc/seg_loss.hip:15: partial-sum workgroups per image


def seg_loss_workspace(B, H, W):
    """csrc/seg_loss.hip:141 fp_seg_loss_workspace: four full-resolution gradient planes, then per image SEG_BLK labelled-pixel partials and
    SEG_BLK x 4 loss partials"""
    return (4 * B * H * W + B * SEG_BLK * 5) * 4


def seg_down_grid(B, h, w):
    """csrc/seg_loss.hip:174: one thread per low-resolution element, capped at 4096 workgroups"""
    return min(4096, ceil_div(B * h * w, 256))


def ew_grid(total, cap=8192):
    """csrc/bn_pool.hip:339 and csrc/loss_adam_misc.hip:11 ew_grid (same rule, default cap 8192); csrc/psp.hip:150 grid_for is the
    same rule with cap 4096"""
    return max(1, min(cap, ceil_div(total, 256)))


def adam_grid(n):
    """csrc/loss_adam_misc.hip:301,346: ew_grid(n / 4 + 1, 4096) over float4 items; the n % 4 tail is workgroup 0's"""
    return ew_grid(n // 4 + 1, 4096)


def _prod(shape):
    p = 1
    for s in shape:
        p *= s
    return p


# kernel -> (work items of one launch, grid cap): the element-wise kernels, items as the kernel counts them (float4 where it loads float4)
EW = {
    "bn_apply": (lambda M, C: M * (C // 4), 8192),                                     # bn_pool.hip:394-395
    "bn_bwd_apply": (lambda M, C: M * (C // 4), 8192),                                 # bn_pool.hip:414-415
    "maxpool_fwd": (lambda N, H, W, C: N * ((H + 1) // 2) * ((W + 1) // 2) * (C // 4), 8192),   # bn_pool.hip:440-441
    "maxpool_bwd": (lambda N, H, W, C: N * H * W * (C // 4), 8192),                    # bn_pool.hip:449-450
    "up2cat_bwd": (lambda N, h, w, C0, C1: max(N * h * w * (C0 // 4), N * 4 * h * w * (C1 // 4)), 8192),   # loss_adam_misc.hip:401-403
    "nchw_to_nhwc": (lambda N, C, H, W: N * C * H * W, 8192),                          # loss_adam_misc.hip:410
    "nhwc_to_nchw": (lambda N, C, H, W: N * C * H * W, 8192),                          # loss_adam_misc.hip:415
    "fill": (lambda n: n, 8192),                                                       # loss_adam_misc.hip:421
    "scale_rows": (lambda *shape: _prod(shape), 8192),                                 # loss_adam_misc.hip:359
    "adam": (lambda n: n // 4, 4096),                                                  # loss_adam_misc.hip:123-124 (grid: adam_grid)
    "psp": (lambda total: total, 4096),                                                # psp.hip:150 (any of its five kernels)
}


def ew_launch(kernel, *shape):
    items, cap = EW[kernel]
    n = items(*shape)
    grid = adam_grid(shape[0]) if kernel == "adam" else ew_grid(n, cap)
    return n, grid


# ---- regimes -----------------------------------------------------------------------------------------------------------------------
def ew_regime(kernel, *shape):
    """("ew", kernel, passes, ragged_last_pass): passes = grid-stride iterations of the busiest thread, reported as 1 or 2 (2 = "more than once":
    the loop has no third path); ragged = the last pass does not fill the grid (for one pass: the last workgroup is not full)"""
    n, grid = ew_launch(kernel, *shape)
    passes = ceil_div(n, grid * 256) if n else 0
    ragged = (n % (grid * 256) != 0) if passes > 1 else (n % 256 != 0)
    return frozenset([("ew", kernel, min(passes, 2), ragged)])


def adam_regime(n):
    """the float4 body as an "ew" regime plus ("adam_tail", n % 4): the scalar tail (loss_adam_misc.hip:140)"""
    return ew_regime("adam", n) | frozenset([("adam_tail", n % 4)])


def head_regime(N, H, W, Cin):
    """("head", rows, ring_wraps, tail_rows, dead_lanes) per KIND of workgroup in the launch.  rows = row-group height; ring_wraps = how
    many times the four-buffer row ring goes round for that workgroup (head.hip:99-107: four rows per turn); tail_rows = rows the last
    group of an image walks when that is fewer than `rows` (0 for a full group); dead_lanes = the last column block holds lanes past W"""
    colblocks, rows, gpi = head_grid(N, H, W, Cin)
    tail = H - (gpi - 1) * rows
    heights = {rows} if gpi > 1 or tail == rows else set()
    if tail != rows:
        heights.add(tail)
    deads = {False} if (colblocks > 1 or W * (Cin // 4) == 256 * colblocks) else set()
    if W * (Cin // 4) != 256 * colblocks:
        deads.add(True)
    return frozenset(("head", rows, ceil_div(hh, 4), 0 if hh == rows else hh, d) for hh in heights for d in deads)


def _final_lanes(nblk):
    """the one-wave-per-output final kernels: lane l takes partials l, l + 64, ...: 0 = some lanes get none, 1 = one pass, 2 = a loop"""
    return 0 if nblk < 64 else min(ceil_div(nblk, 64), 2)


def head_wgrad_regime(N, H, W, Cin):
    """("head_wgrad", capped, grid_stride_loop, final_lanes_loop)"""
    M = N * H * W
    ppb = 256 // (Cin // 4)
    nblk = head_wgrad_blocks(M, Cin)
    return frozenset([("head_wgrad", ceil_div(M, ppb * 8) > 1024, ceil_div(M, nblk * ppb) > 1, _final_lanes(nblk))])


def bn_reduce_regime(M, C):
    """("bn_reduce", capped, zero_row_threads, final_lanes_loop) for bn_stats_kernel and bn_bwd_reduce_kernel (same mapping)"""
    R = 256 // (C // 4)
    nblk = bn_blocks(M, C)
    return frozenset([("bn_reduce", ceil_div(M, R * 4) > 512, nblk * R > M, _final_lanes(nblk))])


def colsum_regime(M, C):
    """("colsum", capped, zero_row_threads, idle_threads, final_lanes_loop); idle_threads: C / 4 does not divide 256
    (loss_adam_misc.hip:162)"""
    C4 = C // 4
    R = 256 // C4
    nblk = colsum_blocks(M, C)
    return frozenset([("colsum", ceil_div(M, R * 16) > 512, nblk * R > M, 256 % C4 != 0, _final_lanes(nblk))])


def loss_regime(B, H, W):
    """("loss", capped, passes, ragged_last_pass, final_lanes_loop) for loss_kernel + loss_final_kernel (loss_adam_misc.hip:33,85):
    passes = grid-stride iterations of the busiest thread as 1 or 2 (2 = more than one); ragged = the last pass does not fill the grid
    (for one pass: the last workgroup is not full)"""
    npix = B * H * W
    nblk = loss_blocks(npix)
    passes = ceil_div(npix, nblk * 256)
    ragged = (npix % (nblk * 256) != 0) if passes > 1 else (npix % 256 != 0)
    return frozenset([("loss", ceil_div(npix, 1024) > 2048, min(passes, 2), ragged, _final_lanes(nblk))])


def seg_loss_regime(B, H, W):
    """("seg_loss", passes, ragged_last_pass) of seg_valid_kernel / seg_loss_kernel (seg_loss.hip:37,57: SEG_BLK x 256 threads stride over one
    image) and ("seg_down", scale index, capped) per gradient map of the decoder's sizes H / 8 .. H / 1 (seg_loss.hip:113,174)"""
    HW = H * W
    passes = ceil_div(HW, SEG_BLK * 256)
    ragged = (HW % (SEG_BLK * 256) != 0) if passes > 1 else (HW % 256 != 0)
    down = [("seg_down", i, ceil_div(B * (H // s) * (W // s), 256) > 4096) for i, s in enumerate((8, 4, 2, 1))]
    return frozenset([("seg_loss", min(passes, 2), ragged)] + down)


# ---- chain lengths -----------------------------------------------------------------------------------------------------------------
# L = the longest chain of dependent float32 additions behind one reduced output: iterations of one thread, then the in-LDS merges, then
# the shuffle tree, then the final kernel's per-lane loop (and its tree).  Stages a kernel runs in double are counted all the same: the
# bound stays an upper bound.
def bn_chain(M, C):
    """bn_stats_kernel / bn_bwd_reduce_kernel (bn_pool.hip:31,156) + their final kernels (:71,:203)"""
    R = 256 // (C // 4)
    nblk = bn_blocks(M, C)
    return ceil_div(M, nblk * R) + (R - 1) + ceil_div(nblk, 64) + 6


def colsum_chain(M, C):
    """colsum_kernel + colsum_final_kernel (loss_adam_misc.hip:160,179)"""
    R = 256 // (C // 4)
    nblk = colsum_blocks(M, C)
    return ceil_div(M, nblk * R) + (R - 1) + ceil_div(nblk, 64) + 6


def head_wgrad_chain(N, H, W, Cin):
    """head_wgrad_kernel + head_wgrad_reduce_kernel (head.hip:433,576).  A pixel on row/column 1 or n-2 is also a mirror source: up to
    four multiply-adds into one accumulator per iteration (head.hip:508-518); then the slot tree (log2(64 / Q) steps), the four waves
    in LDS (3), the reduce kernel's lane loop and its tree (6)"""
    M = N * H * W
    Q = Cin // 4
    ppb = 256 // Q
    nblk = head_wgrad_blocks(M, Cin)
    return 4 * ceil_div(M, nblk * ppb) + int(math.log2(64 // Q) if Q < 64 else 0) + 3 + ceil_div(nblk, 64) + 6


def head_chain(Cin):
    """head_fwd_kernel (head.hip:79-88): 9 taps x 4 channels in one lane, then log2(Q) shuffle steps, then the bias"""
    Q = Cin // 4
    return 36 + int(math.log2(Q)) + 1


def loss_chain(npix):
    """loss_kernel + loss_final_kernel (loss_adam_misc.hip:33,85): one thread's pixels, the wave tree (6), the four waves in LDS (3), the final
    kernel's lane loop over the partial blocks and its tree (6)"""
    nblk = loss_blocks(npix)
    return ceil_div(npix, nblk * 256) + 6 + 3 + ceil_div(nblk, 64) + 6


def seg_loss_chain(HW):
    """seg_loss_kernel + seg_final_kernel (seg_loss.hip:51,88): one thread's pixels, the wave tree (6), the four waves in LDS as two pairs
    (2), then SEG_BLK partial blocks added serially by one thread (64)"""
    return ceil_div(HW, SEG_BLK * 256) + 6 + 2 + SEG_BLK


def sum_bound(L, k, abs_terms, result):
    """first-order summation bound: (L + k) u sum|terms| + u |result|; k = roundings inside one term"""
    return (L + k) * U * abs_terms + U * abs(result)


# ---- the 3x3 stride-1 tile kernels (conv3x3_tile_bf3.hip, wgrad3x3_bf3.hip) ---------------------------------------------------------
# Operand formats: "exact" (three bf16 terms, six products), "pair" (scaled fp16 pairs), "two" (two bf16 terms: the opt-in inference mode,
# forward gathers only).  Families: "fwd" (gathers zero / reflect / up2), "flip" (data gradient, zero padding), "fold" (data gradient
# of reflection padding).
TILE3_GATHERS = {"zero": "fwd", "reflect": "fwd", "up2": "fwd", "dgrad": "flip", "dgrad_reflect": "fold"}


def tile3_plan(N, H, W, C0, C1, Nout, up2=False, fmt="exact"):
    """conv3x3_tile_bf3.hip:811 plan3 (every FP_TILE_* variable unset) and what run_tile3 adds (:925-926 wmajor, :940-951 the
    instantiation) -> dict, or None where fp_conv3x3_bf3_supported answers 0.  H x W = output = input size (stride 1, pad 1)"""
    if C0 % 4:
        return None
    if up2:
        if C0 % 16 or C1 % 4 or C1 < 0 or H % 2 or W % 2:
            return None
    elif C1:
        return None
    if H < 2 or W < 2:
        return None

    def waste_ok(th, tw):                                       # :824 at most 25 % padded work
        return ceil_div(H, th) * ceil_div(W, tw) * 128 * 4 <= H * W * 5
    if waste_ok(8, 16):
        th, tw = 8, 16
    elif waste_ok(6, 20):
        th, tw = 6, 20
    else:
        return None
    bn = 32 if Nout <= 32 else 64
    tx, ty, tn = ceil_div(W, tw), ceil_div(H, th), ceil_div(Nout, bn)
    tiles = N * ty * tx * tn
    KC16 = (C0 + C1 + 15) // 16
    sk = 1
    if tiles < 160:                                             # :853 no split from 160 tiles
        sk = max(1, min(768 // tiles, KC16 // 2, 16))           # :855-859 target 768, >= 2 chunks per split, <= 16 partial copies
    cps = ceil_div(KC16, sk)
    SK = ceil_div(KC16, cps)
    if tiles * SK < 128:                                        # :863
        return None
    nwg = tiles * SK
    hp = fmt == "pair"
    inst = ("pair_wpf" if (bn == 64 and nwg <= 400) else "pair") if hp else fmt          # :943
    return {"th": th, "tw": tw, "bn": bn, "tilesX": tx, "tilesY": ty, "tilesN": tn, "KC16": KC16, "SK": SK, "cps": cps, "nwg": nwg,
            "wmajor": 9 * (C0 + C1) * Nout * (4 if hp else 6) > (4 << 20), "inst": inst,
            "workspace": SK * N * H * W * Nout * 4 if SK > 1 else 0}                         # :873


def _chunk_class(n):
    """trips of a loop that is unrolled by two with up to two items in flight ahead: 1, 2, 3, an even count >= 4, an odd count >= 5"""
    return n if n <= 3 else ("even" if n % 2 == 0 else "odd")


def _rem_class(n, t):
    """pixels of the last tile along one axis: 0 (a full tile), 1, 2, or 3 = three and more"""
    return min(n % t, 3)


def tile3_regime(gather, fmt, N, H, W, C0, C1, Nout):
    """frozenset of ("tile3", instantiation key, axis, value).  key = (family, tile height, BN, instantiation): one compiled kernel;
    the axes are what differs between launches of one kernel:
      gather   zero / reflect / up2 (a.mode, a.Clo at :299-311)
      split    (False, 0) unsplit, or (True, SK % 4): the tail loop of the reduce launch
      chunks   class of c_end - c_begin (:330-331), every split of the launch counted; the loop is unrolled by two and the halo sets
               prefetch up to two chunks ahead (:746-751)
      ctail    C % 16 != 0 (zero_tail, :355);  c1: for the concat gather "none" / "tail" (C1 % 16 != 0) / "whole"
      ntail    Nout % BN != 0 (:314, :517);  wmajor (:926)
      ragx / ragy   pixels of the last tile of a row / column of tiles (:512 the epilogue's `interior`, :300-302 the halo's validity)
      foldy / foldx (fold only, :316-317) (rows 1 and OH-2 share a tile, OH-2 lies in the last tile or in the one before it)"""
    family = TILE3_GATHERS[gather]
    assert fmt != "two" or family == "fwd"
    p = tile3_plan(N, H, W, C0, C1, Nout, gather == "up2", fmt)
    assert p is not None, (gather, fmt, N, H, W, C0, C1, Nout)
    key = (family, p["th"], p["bn"], p["inst"])
    C = C0 + C1
    out = [("gather", gather), ("split", (p["SK"] > 1, p["SK"] % 4 if p["SK"] > 1 else 0)), ("ctail", C % 16 != 0),
           ("ntail", Nout % p["bn"] != 0), ("wmajor", p["wmajor"]), ("ragx", _rem_class(W, p["tw"])), ("ragy", _rem_class(H, p["th"]))]
    for s in range(p["SK"]):
        out.append(("chunks", _chunk_class(min(p["KC16"], (s + 1) * p["cps"]) - s * p["cps"])))
    if gather == "up2":
        out.append(("c1", "none" if C1 == 0 else "tail" if C1 % 16 else "whole"))
    if family == "fold":
        for ax, n, t, tiles in (("foldy", H, p["th"], p["tilesY"]), ("foldx", W, p["tw"], p["tilesX"])):
            out.append((ax, (1 // t == (n - 2) // t, "last" if (n - 2) // t == tiles - 1 else "before")))
    return frozenset(("tile3", key) + o for o in out)


W3_CH, W3_CW = 4, 16      # wgrad3x3_bf3.hip:45 pixel chunk of the weight gradient: 4 rows x 16 columns


def wgrad3_plan(N, H, W, C0, Nout, up2=False):
    """wgrad3x3_bf3.hip:797 eligible and :812 plan (FP_WGRAD_* unset) -> dict, or None where fp_conv_wgrad_bf3_workspace answers -1"""
    if up2 and (H % 2 or W % 2):
        return None
    if H < 2 or W < 2 or C0 % 32 or Nout % 32:
        return None
    cy, cx = ceil_div(H, W3_CH), ceil_div(W, W3_CW)
    if cy * W3_CH * cx * W3_CW * 10 > H * W * 22:               # :807 padded work up to 2.2x
        return None
    if N * cy * cx < 16:                                        # :808
        return None
    nchunks = N * cy * cx
    citiles, cotiles = C0 // 32, Nout // 32
    S = max(1, min(ceil_div(256, citiles * cotiles), nchunks // 4, 512))       # :822-825
    cps = ceil_div(nchunks, S)
    S = ceil_div(nchunks, cps)
    return {"S": S, "cps": cps, "nchunks": nchunks, "cy": cy, "cx": cx, "citiles": citiles, "cotiles": cotiles,
            "workspace": S * (9 * C0 * Nout + Nout) * 4}         # :837


def wgrad3_regime(mode, fmt, N, H, W, C0, Nout):
    """frozenset of ("wgrad3", key, axis, value).  key = (kernel, mode, fmt): "ring" = wgrad3x3_hp_pf_kernel, "v3" = the third
    generation, which keeps the exact format's up2 gather (:900).  Axes:
      remy / remx   rows / columns of the last 4 x 16 chunk (0 = full)
      chunks   "border" or "both": does a launch hold fast (interior) chunks beside the border ones (:415; never for up2)
      cnt      parity of the chunk count of a split (:362; two ring slots, two LDS buffers), every split counted
      stride   (S >= chunks per image: dcn > 0, S % chunksX == 0: dcx == 0) (:365)
      reduce   "plain", "capped" (its 4096-block cap), "transposing" (:935-949);  s4: S % 4 (the partial-sum loops' tail)"""
    p = wgrad3_plan(N, H, W, C0, Nout, mode == "up2")
    assert p is not None, (mode, fmt, N, H, W, C0, Nout)
    key = ("v3" if (fmt == "exact" and mode == "up2") else "ring", mode, fmt)
    fast = mode != "up2" and any(y0 >= 1 and y0 + W3_CH + 1 <= H and x0 >= 1 and x0 + W3_CW + 1 <= W
                                 for y0 in range(0, H, W3_CH) for x0 in range(0, W, W3_CW))
    if (Nout // 32) * (C0 // 8) >= 512:
        reduce = "transposing"
    else:
        reduce = "capped" if ceil_div(9 * C0 * Nout, 256) > 4096 else "plain"
    S = p["S"]
    out = [("remy", H % W3_CH), ("remx", _rem_class(W, W3_CW)), ("chunks", "both" if fast else "border"),
           ("stride", (S >= p["cy"] * p["cx"], S % p["cx"] == 0)), ("reduce", reduce), ("s4", S % 4)]
    out += [("cnt", ((p["nchunks"] - 1 - s) // S + 1) % 2) for s in range(S)]
    return frozenset(("wgrad3", key) + o for o in out)


# ---- the nearest-x2 phase kernels (conv_up2_phase.hip, wgrad_up2_phase.hip) ---------------------------------------------------------
# Operand formats: "f32" (fp32 MFMA), "exact" (three bf16 terms), "pair" (scaled fp16 pairs).  h x w is the LOW-resolution grid throughout.
PH_TH, PH_TW = 8, 16      # conv_up2_phase.hip:23 the low-resolution tile of the forward and data-gradient kernels
PW_CH, PW_CW = 2, 16      # wgrad_up2_phase.hip:30 pixel chunk of the weight gradient: 2 rows x 16 columns
PHASE_FORMATS = ("f32", "exact", "pair")


def phase_ok(h, w):
    """engine.py:895 _phase_ok: the caller keeps the fused-gather path when under 60 % of the 8 x 16 tiles would be pixels"""
    return h * w * 10 >= ceil_div(h, 8) * 8 * ceil_div(w, 16) * 16 * 6


def phase_fwd_plan(N, h, w, C0, Nout, fmt="exact"):
    """conv_up2_phase.hip:593-608 (f32) and :615-636 (split formats) -> dict, or None where the launcher refuses the arguments"""
    if min(N, h, w, C0, Nout) < 1 or C0 % 4:
        return None
    if fmt != "f32" and (N * 4 * h * w * Nout >= 1 << 29 or N * h * w * C0 >= 1 << 29):          # :617 32-bit byte offsets
        return None
    bn = 32 if Nout <= 32 else 64                                # :626
    tx, ty, tn = ceil_div(w, PH_TW), ceil_div(h, PH_TH), ceil_div(Nout, bn)
    return {"bn": bn, "tilesX": tx, "tilesY": ty, "tilesN": tn, "KC16": ceil_div(C0, 16), "nwg": N * ty * tx * tn * 4}


def phase_dgrad_plan(N, h, w, Cout, C0, fmt="exact"):
    """conv_up2_phase.hip:654-674: tiles of the EXTENDED (h + 2) x (w + 2) grid, BN over the C0 result channels, chunks over Cout; one
    workgroup runs all four phases (4 KC16 steps)"""
    if min(N, h, w, Cout, C0) < 1 or Cout % 4 or fmt == "f32":          # (no fp32 phase data gradient: that path is conv_igemm)
        return None
    if N * 4 * h * w * Cout >= 1 << 29 or N * (h + 2) * (w + 2) * C0 >= 1 << 29:
        return None
    bn = 32 if C0 <= 32 else 64                                  # :664
    tx, ty, tn = ceil_div(w + 2, PH_TW), ceil_div(h + 2, PH_TH), ceil_div(C0, bn)
    kc = ceil_div(Cout, 16)
    return {"bn": bn, "tilesX": tx, "tilesY": ty, "tilesN": tn, "KC16": kc, "nsteps": 4 * kc, "nwg": N * ty * tx * tn}


def phase_wgrad_plan(N, h, w, C0, Nout):
    """wgrad_up2_phase.hip:371 eligible and :378 plan (FP_PWGRAD_TARGET_WGS unset: 768) -> dict, or None where
    fp_conv_up2_phase_wgrad_workspace answers -1"""
    if C0 % 32 or Nout % 32 or h < 1 or w < 1 or C0 < 1 or Nout < 1:
        return None
    cy, cx = ceil_div(h, PW_CH), ceil_div(w, PW_CW)
    if cy * PW_CH * cx * PW_CW * 10 > h * w * 13:                # :374 more than 30 % padded work
        return None
    if N * cy * cx < 16:                                         # :375
        return None
    nchunks = N * cy * cx
    citiles, cotiles = C0 // 32, Nout // 32
    S = max(1, min(ceil_div(768, citiles * cotiles), nchunks // 4, 512))       # :385-388 one round of three workgroups per CU
    cps = ceil_div(nchunks, S)
    S = ceil_div(nchunks, cps)
    return {"S": S, "cps": cps, "nchunks": nchunks, "cy": cy, "cx": cx, "citiles": citiles, "cotiles": cotiles,
            "workspace": (S * 16 * C0 * Nout + S * Nout) * 4}    # :400


def _clamp_class(n, t):
    """does the halo of ONE tile leave the image on both sides of an axis: "no", "both" (n < t), "one" (a single row / column: every
    halo row is the same pixel row)"""
    return "one" if n == 1 else "both" if n < t else "no"


def _cnt_class(n):
    """chunks of one split of the weight gradient (one-deep prefetch, two LDS buffers in the fp32 kernel): 1, 2, an even count, an odd count"""
    return n if n <= 2 else ("even" if n % 2 == 0 else "odd")


def phase_wgrad_split_counts(p, fmt):
    """chunks per split: the fp32 kernel takes `cps` contiguous chunks (wgrad_up2_phase.hip:45-46, the last split short), the split-operand
    kernels stride them: c = s, s + S, ... (:176)"""
    if fmt == "f32":
        return [min(p["nchunks"], (s + 1) * p["cps"]) - s * p["cps"] for s in range(p["S"])]
    return [len(range(s, p["nchunks"], p["S"])) for s in range(p["S"])]


def phase_wgrad_sum_groups(S):
    """up2_wgrad_sum_kernel (wgrad_up2_phase.hip:340-345): group g of four walks s = g, g + 4, ...: (trips of the 16-stride loop > 0, trips of the tail)"""
    out = []
    for g in range(4):
        s, main = g, 0
        while s + 12 < S:
            s += 16
            main += 1
        out.append((main > 0, len(range(s, S, 4))))
    return out


def phase_regime(kind, fmt, N, h, w, C0, C1, Nout, epi=(), kslice=(0, 0)):
    """frozenset of ("phase", key, axis, value); key = (kind, BN or the weight-gradient kernel, fmt): one compiled instantiation.
    kind "fwd": low [N, h, w, C0] -> y [N, 2h, 2w, Nout] (C1 = channels of the skip half, which another kernel runs: it decides the
    `addend` epilogue only); "dgrad": dz [N, 2h, 2w, Nout] -> ext [N, h + 2, w + 2, C0]; "wgrad": dw [Nout, k_begin + C0 + k_after, 3, 3],
    kslice = (k_begin, k_after).  Axes:
      ragx / ragy   (pixels of the last 8 x 16 tile as _rem_class, more than one tile along the axis) (dgrad: of the extended grid; wgrad: of
                    the last 2 x 16 chunk, ragy = h % 2: an eligible shape has two rows at least)
      grid          (N > 1, more than one tile of result channels) (wgrad: N > 1, more than one tile of 32 input / output channels)
      chunks        class of KC16 (fwd: over C0, :110; dgrad: over Nout, :404 -- with one chunk every step changes phase)
      ctail / ntail contracted channels % 16 != 0 (hzero, :262 :435) / result channels % BN != 0 (:278 :341 :451 :524)
      clampy / clampx   "no" / "both" / "one" (_clamp_class; wgrad: clampx alone, a single row is not eligible)
      epi (fwd)     the sorted subset of bias / addend / act (:342-364)
    wgrad: s1 (S == 1: no sum launch, :432), s4 (S % 4, the bias reduce's tail :327), sum (per group of up2_wgrad_sum_kernel), cnt (per
    split), short (fp32: the last split is shorter), db, kslice (k_begin > 0, channels behind the slice)"""
    assert fmt in PHASE_FORMATS, fmt
    if kind == "fwd":
        p = phase_fwd_plan(N, h, w, C0, Nout, fmt)
        assert p is not None, (kind, fmt, N, h, w, C0, C1, Nout)
        key = ("fwd", p["bn"], fmt)
        out = [("ragx", (_rem_class(w, PH_TW), p["tilesX"] > 1)), ("ragy", (_rem_class(h, PH_TH), p["tilesY"] > 1)),
               ("chunks", _chunk_class(p["KC16"])), ("ctail", C0 % 16 != 0), ("ntail", Nout % p["bn"] != 0), ("clampy", _clamp_class(h, PH_TH)),
               ("clampx", _clamp_class(w, PH_TW)), ("grid", (N > 1, p["tilesN"] > 1)), ("epi", tuple(sorted(epi)))]
    elif kind == "dgrad":
        p = phase_dgrad_plan(N, h, w, Nout, C0, fmt)
        assert p is not None, (kind, fmt, N, h, w, C0, C1, Nout)
        key = ("dgrad", p["bn"], fmt)
        out = [("ragx", (_rem_class(w + 2, PH_TW), p["tilesX"] > 1)), ("ragy", (_rem_class(h + 2, PH_TH), p["tilesY"] > 1)),
               ("chunks", _chunk_class(p["KC16"])), ("ctail", Nout % 16 != 0), ("ntail", C0 % p["bn"] != 0), ("clampy", _clamp_class(h, PH_TH)),
               ("clampx", _clamp_class(w, PH_TW)), ("grid", (N > 1, p["tilesN"] > 1))]
    else:
        assert kind == "wgrad", kind
        p = phase_wgrad_plan(N, h, w, C0, Nout)
        assert p is not None, (kind, fmt, N, h, w, C0, C1, Nout)
        key = ("wgrad", "fp32" if fmt == "f32" else "split", fmt)
        S = p["S"]
        counts = phase_wgrad_split_counts(p, fmt)
        out = [("ragx", (_rem_class(w, PW_CW), p["cx"] > 1)), ("ragy", h % PW_CH), ("s1", S == 1), ("s4", S % 4), ("db", fmt != "f32"),
               ("kslice", (kslice[0] > 0, kslice[1] > 0)), ("clampx", _clamp_class(w, PW_CW)), ("grid", (N > 1, p["citiles"] > 1, p["cotiles"] > 1))]
        out += [("cnt", _cnt_class(c)) for c in counts]
        if S > 1:
            out += [("sum", g) for g in phase_wgrad_sum_groups(S)]
        if fmt == "f32":
            out.append(("short", counts[-1] < p["cps"]))
    return frozenset(("phase", key) + o for o in out)


EW["up2_fold"] = (lambda N, h, w, C: N * h * w * (C // 4), 4096)                           # conv_up2_phase.hip:584-586, :691


def fold_regime(N, h, w, C, addend, ylow):
    """up2_fold_bwd_kernel (conv_up2_phase.hip:543): the grid-stride loop as an "ew" regime, the optional operands, and how many extended
    positions fold onto one pixel along each axis (1 / 2 inside and on a border, 3 where h == 1: :556-561)"""
    return ew_regime("up2_fold", N, h, w, C) | frozenset([("fold", "operands", (bool(addend), bool(ylow))), ("fold", "ny", min(h, 2) == 1),
                                                          ("fold", "nx", min(w, 2) == 1)])
