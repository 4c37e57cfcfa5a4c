"""CPU: do the small shapes of tests/test_gpu_step_kernels.py still reach the launch regimes the product runs, and are the error
bounds those tests use tight enough to see one dropped row?

1. tests/launch_regimes.py restates the host launch arithmetic; here it is swept against the library's own answers.
2. WORKLOAD lists, per kernel, the shapes the engine launches (footprints network at 12x192x640 and 4x512x640, the PSP segmentor at
   12x192x640), read off footprints_amd/engine.py; CASES lists the GPU test shapes.  Every regime tuple of WORKLOAD must occur in CASES:
   when a launch rule changes, this is the test that says which small shape stopped standing in for the product's.
3. For every reduction case the float64 reference is recomputed without the last row and without the last workgroup's rows; one
   reduced output at least must move by more than ten times its bound (tests/step_kernel_refs.py), else the bound could not see it.
4. The two training losses: the launch arithmetic of csrc/seg_loss.hip against fp_seg_loss_workspace, and the regimes the trainers' shapes
   run (Footprints 12x192x640, 4x512x640, 12x512x640; segmentor 12x192x640) against the cases of tests/test_gpu_losses.py.
5. The 3x3 stride-1 tile kernels: plan3 / run_tile3 (csrc/conv3x3_tile_bf3.hip) and eligible / plan (csrc/wgrad3x3_bf3.hip) restated and
   swept against fp_conv3x3_bf3_supported, fp_conv3x3_bf3_workspace and fp_conv_wgrad_bf3_workspace; TILE_WORKLOAD lists the 3x3 stride-1
   convolutions of one train step with their data and weight gradients (footprints 12x192x640, 4x512x640, 12x128x416; segmentor
   12x192x640), and every regime tuple of it must occur among the cases of tests/test_gpu_conv_tile_edges.py (tests/conv_tile_refs.py).
6. The nearest-x2 phase kernels that run beside them (csrc/conv_up2_phase.hip, csrc/wgrad_up2_phase.hip): the launchers' tiling restated,
   eligible / plan swept against fp_conv_up2_phase_wgrad_workspace, phase_workload lists the phase launches of the same four train steps,
   and every regime tuple of it must occur among the cases of tests/test_gpu_conv_phase_edges.py (tests/conv_phase_refs.py).
"""
import ctypes

import pytest
import torch

from tests import conv_phase_refs as PR
from tests import conv_tile_refs as TR
from tests import launch_regimes as LR
from tests import step_kernel_refs as SR

ADAM_N = 31021392          # parameters of the footprints network = length of the flat buffers optim.py:44,54,83 hand to Adam


def network_shapes(N, H, W, psp=False):
    """kernel -> shapes of one train step, by engine.py line.  Encoder levels: stem H/2 (64), layer1 H/4 (64), layer2 H/8 (128), layer3
    H/16 (256), layer4 H/32 (512) (engine.py:670-698, 876-880); decoder block bi: pre convs at level 4-bi, post convs at level 3-bi with
    chans[bi][1] channels (engine.py:152, 987-1000), outconv4 at full resolution with 32 (engine.py:1005-1007).  Where a switch decides
    between one of these kernels and a fused path, the shape is listed: the table is a superset."""
    lv = [(H >> s, W >> s, c) for s, c in ((1, 64), (2, 64), (3, 128), (4, 256), (5, 512))]
    bn = [(N * h * w, c) for h, w, c in lv]
    (h0, w0, _), (h1, w1, _), (h2, w2, _), (h3, w3, _), (h4, w4, _) = lv
    out = {
        "bn_reduce": bn,                       # engine.py:522 (statistics), :1163 :1177 :1208 :1212 :1261 (backward sums)
        "bn_apply": bn,                        # engine.py:530
        "bn_bwd_apply": bn,                    # engine.py:1163 ... :1261
        "maxpool_fwd": [(N, h0, w0, 64)],      # engine.py:705
        "maxpool_bwd": [(N, h0, w0, 64)],      # engine.py:1232 (dx = the stem feature gradient, accumulate=True)
        # bias gradients of the decoder convolutions, engine.py:1032 :1075: pre1/pre2 and post1/post2 of the four blocks, o41/o42
        "colsum": [(N * h4 * w4, 256), (N * h3 * w3, 256), (N * h3 * w3, 128), (N * h2 * w2, 128), (N * h2 * w2, 64), (N * h1 * w1, 64),
                   (N * h1 * w1, 64), (N * h0 * w0, 64), (N * H * W, 32)],
        # engine.py:1391 (outconv4's input), :1427 (blocks 4..1: hl, wl = the pre-concat resolution, C0 = C1 = cout)
        "up2cat_bwd": [(N, h0, w0, 64, 0), (N, h1, w1, 64, 64), (N, h2, w2, 64, 64), (N, h3, w3, 128, 128), (N, h4, w4, 256, 256)],
        # engine.py:979 (forward), :1359 :1370 (data gradient), :552 (weight gradient): heads on blocks 2, 3, 4 and outconv4
        "head": [(N, h2, w2, 128), (N, h1, w1, 64), (N, h0, w0, 64), (N, H, W, 32)],
        "head_wgrad": [(N, h2, w2, 128), (N, h1, w1, 64), (N, h0, w0, 64), (N, H, W, 32)],
        "adam": [(ADAM_N,)],                   # optim.py:44 :54 :83
        # engine.py:655: every encoder convolution's OIHW weights (ResNet-34: stem, 3x3 pairs, 1x1 shortcuts)
        "scale_rows": [(64, 3, 7, 7), (64, 64, 3, 3), (128, 64, 3, 3), (128, 128, 3, 3), (128, 64, 1, 1), (256, 128, 3, 3), (256, 256, 3, 3),
                       (256, 128, 1, 1), (512, 256, 3, 3), (512, 512, 3, 3), (512, 256, 1, 1)],
    }
    if psp:                                    # the segmentor's decoder starts from the 1024-channel pyramid concatenation (engine.py:152):
        out = dict(out)                        # the shapes of THESE kernels do not change (its heads: engine.py:148-150, no sigmoid, scale 1)
        del out["adam"]
    return out


WORKLOAD = {"footprints 12x192x640": network_shapes(12, 192, 640), "footprints 4x512x640": network_shapes(4, 512, 640),
            "psp segmentor 12x192x640": network_shapes(12, 192, 640, psp=True)}

BN_BIG = (3, 82, 100, 512)
BN_SMALL = (2, 6, 6, 128)
HEAD_BIG = (2, 1027, 500, 16)
HEAD_R16 = (2, 2050, 500, 16)
HEAD_SMALL = [(2, 6, 10, 16), (2, 40, 56, 128)]

# the GPU test shapes (tests/test_gpu_step_kernels.py takes them from here)
CASES = {
    "bn": [BN_BIG, (2, 1, 1, 512), (2, 2, 2, 128), BN_SMALL, (1, 3, 1, 16), (3, 10, 10, 4), (3, 10, 10, 1024)],        # (N, H, W, C)
    "maxpool_fwd": [(1, 1, 5, 4), (2, 2, 2, 8), (1, 7, 9, 8), (2, 8, 12, 16), (2, 8, 16, 32), (3, 211, 209, 64)],
    "maxpool_bwd": [(1, 1, 5, 4), (2, 2, 2, 8), (1, 7, 9, 8), (2, 8, 12, 16), (2, 8, 16, 32), (3, 211, 209, 64)],
    "colsum": [(M, C) for C in (4, 20, 36, 72, 1024) for M in (1, 3, 1000)] + [(1100, 1024), (24600, 512)],
    "up2cat_bwd": [(1, 1, 1, 4, 4), (1, 3, 5, 8, 4), (2, 4, 6, 8, 0), (2, 4, 8, 16, 16), (2, 129, 128, 64, 64)],
    "head": HEAD_SMALL + [HEAD_BIG, HEAD_R16],
    "head_wgrad": HEAD_SMALL + [HEAD_BIG],
    "adam": [(n,) for n in (1, 2, 3, 4, 5, 1023, 4300003, 4300004)],
    "scale_rows": [(512, 512, 3, 3), (64, 3, 7, 7), (64, 64, 3, 3)],
    "layout": [(2, 5, 7, 9), (3, 5, 373, 401)],                                                                  # (N, C, H, W)
    "fill": [(1,), (2097153,)],
}


def regimes(kernel, shape):
    if kernel == "bn_reduce":
        return LR.bn_reduce_regime(*shape)
    if kernel == "colsum":
        return LR.colsum_regime(*shape)
    if kernel == "head":
        return LR.head_regime(*shape)
    if kernel == "head_wgrad":
        return LR.head_wgrad_regime(*shape)
    if kernel == "adam":
        return LR.adam_regime(*shape)
    return LR.ew_regime(kernel, *shape)


def case_shapes(kernel):
    """the CASES rows that exercise `kernel`, in the kernel's own argument order"""
    if kernel in ("bn_reduce", "bn_apply", "bn_bwd_apply"):
        return [(N * H * W, C) for N, H, W, C in CASES["bn"]]
    if kernel in ("nchw_to_nhwc", "nhwc_to_nchw"):
        return CASES["layout"]
    return CASES[kernel]


KERNELS = sorted({k for w in WORKLOAD.values() for k in w})


def _lib():
    from footprints_amd import _lib as L
    return L.load()


# ---- 1. restatement against the library ----------------------------------------------------------------------------------------------
def _sweep(seed, n, lo, hi):
    g = torch.Generator().manual_seed(seed)
    return [int(v) for v in torch.randint(lo, hi, (n,), generator=g)]


def test_bn_blocks_match_library():
    lib = _lib()
    Ms = [1, 2, 3, 8, 72, 255, 256, 257, 2047, 2048, 2049, 24600, 368640, 1474560] + _sweep(1, 40, 1, 3000000)
    for C in (4, 8, 16, 32, 64, 128, 256, 512, 1024):
        for M in Ms:
            nblk = (lib.fp_bn_workspace(M, C) - C * 2 * 4) // (C * 3 * 4)
            assert nblk == LR.bn_blocks(M, C), (M, C)


def test_colsum_blocks_match_library():
    lib = _lib()
    Ms = [1, 3, 1000, 1100, 8191, 8192, 8193, 24600, 1474560] + _sweep(2, 30, 1, 3000000)
    for C in (4, 20, 32, 36, 64, 72, 128, 256, 512, 1024):
        for M in Ms:
            assert lib.fp_colsum_workspace(M, C) == LR.colsum_blocks(M, C) * C * 4, (M, C)


def test_head_grids_match_library():
    lib = _lib()
    hs, ws = [2, 3, 6, 24, 37, 96, 192, 512, 1027, 2050] + _sweep(3, 6, 2, 2100), [2, 5, 8, 56, 80, 320, 500, 640] + _sweep(4, 4, 2, 700)
    out = (ctypes.c_int32 * 3)()
    for Cin in (4, 8, 16, 32, 64, 128):
        for N in (1, 2, 12, 20):
            for h in hs:
                for w in ws:
                    assert lib.fp_head_grid(N, h, w, Cin, out) == 0
                    assert tuple(out) == LR.head_grid(N, h, w, Cin), (N, h, w, Cin)
                    per = (9 * Cin * 2 + 2) * 4
                    assert lib.fp_head_wgrad_workspace(N, h, w, Cin) == LR.head_wgrad_blocks(N * h * w, Cin) * per, (N, h, w, Cin)
    assert lib.fp_head_grid(2, 6, 10, 12, out) != 0 and lib.fp_head_grid(2, 1, 10, 16, out) != 0        # what the launches refuse


def test_loss_blocks_match_library():
    lib = _lib()
    for B, H, W in [(1, 1, 1), (1, 32, 32), (1, 32, 33), (12, 192, 640), (4, 512, 640), (3, 40, 72), (20, 192, 640), (2, 1024, 1024),
                    (2, 1024, 1025)] + [(2, h, 37) for h in _sweep(5, 30, 1, 40000)]:
        assert lib.fp_loss_workspace(B, H, W) == LR.loss_blocks(B * H * W) * 16 * 4, (B, H, W)


def test_seg_loss_launch_matches_library():
    lib = _lib()
    for B, H, W in [(1, 8, 8), (2, 16, 24), (3, 64, 96), (2, 136, 128), (12, 192, 640), (2, 512, 1032)] + [(3, h, 41) for h in _sweep(6, 20, 1, 20000)]:
        assert lib.fp_seg_loss_workspace(B, H, W) == LR.seg_loss_workspace(B, H, W), (B, H, W)
    assert LR.SEG_BLK * 256 == 16384 and LR.seg_down_grid(12, 192, 640) == 4096 and LR.seg_down_grid(2, 136, 128) == 136


# ---- the two losses: which regimes the trainers' shapes run, and that the GPU cases of tests/test_gpu_losses.py reach them ----------
LOSS_WORKLOAD = [(12, 192, 640), (4, 512, 640), (12, 512, 640)]       # Footprints trainer: KITTI, Matterport, Matterport at the KITTI batch size
SEG_LOSS_WORKLOAD = [(12, 192, 640)]                                  # segmentation trainer


def test_loss_regimes_of_the_trainers_occur_in_the_gpu_cases():
    from tests import loss_refs as LF
    assert LR.loss_regime(12, 192, 640) == LR.loss_regime(4, 512, 640) == frozenset([("loss", False, 2, False, 2)])
    assert LR.loss_regime(12, 512, 640) == frozenset([("loss", True, 2, True, 2)])          # 3840 blocks wanted, capped at 2048
    have = set().union(*(LR.loss_regime(c.B, c.H, c.W) for c in LF.FP_CASES))
    for shape in LOSS_WORKLOAD:
        missing = LR.loss_regime(*shape) - have
        assert not missing, "Footprints loss at %s runs %s: no GPU case does (cases reach %s)" % (shape, sorted(missing), sorted(have))
    # the structural edges the cases add on purpose: one partial workgroup; lanes of the final kernel without a partial block
    assert ("loss", False, 1, True, 0) in have and LR.loss_blocks(2 * 160 * 208) == 65 and LR.ceil_div(2 * 1024 * 1030, 1024) == 2060
    assert (2 * 1024 * 1030) % (2048 * 256) != 0            # under the cap some threads take five trips, the others four
    # an image boundary inside a workgroup: 1024 x 1030 pixels are a multiple of 256, so the capped case does not have one; 40 x 72 does
    assert (1024 * 1030) % 256 == 0 and (40 * 72) % 256 != 0 and any(c.B > 1 and (c.H, c.W) == (40, 72) for c in LF.FP_CASES)
    assert LR.seg_loss_regime(12, 192, 640) == frozenset([("seg_loss", 2, True), ("seg_down", 0, False), ("seg_down", 1, False),
                                                          ("seg_down", 2, False), ("seg_down", 3, True)])
    seg = set().union(*(LR.seg_loss_regime(c.B, c.H, c.W) for c in LF.SEG_CASES if c.backward))
    for shape in SEG_LOSS_WORKLOAD:
        missing = LR.seg_loss_regime(*shape) - seg
        assert not missing, "segmentation loss at %s runs %s: no GPU case does (cases reach %s)" % (shape, sorted(missing), sorted(seg))
    assert ("seg_loss", 1, True) in seg and ("seg_loss", 1, False) in seg


def test_issue_table_rows():
    """the launch regimes of the 12x192x640 step that the kernel tests did not reach before this file existed"""
    assert LR.head_grid(12, 96, 320, 64)[1] == 8 and LR.head_grid(12, 192, 640, 32)[1] == 16          # the row ring wraps
    assert [LR.ceil_div(12 * h * w, (256 // (c // 4)) * 8) for h, w, c in ((192, 640, 32), (96, 320, 64))] == [5760, 2880]   # capped at 1024
    assert [LR.ceil_div(m, (256 // (c // 4)) * 4) for m, c in ((368640, 64), (92160, 64), (23040, 128))] == [5760, 1440, 720]    # capped at 512
    assert LR.ew_launch("scale_rows", 512, 512, 3, 3) == (2359296, 8192) and 2359296 > 8192 * 256
    assert LR.ew_launch("adam", ADAM_N)[1] == 4096 and ADAM_N // 4 > 4096 * 256
    assert LR.colsum_blocks(12 * 192 * 640, 32) == 512 and LR.ceil_div(12 * 192 * 640, 32 * 16) > 512


# ---- 2. the workload is covered by the cases ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", KERNELS)
def test_workload_regimes_occur_in_cases(kernel):
    have = set()
    for shape in case_shapes(kernel):
        have |= regimes(kernel, shape)
    for name, table in WORKLOAD.items():
        for shape in table.get(kernel, ()):
            missing = regimes(kernel, shape) - have
            assert not missing, "%s, %s %s runs %s: no GPU case does (cases reach %s)" % (name, kernel, shape, sorted(missing), sorted(have))


def test_cases_reach_the_structural_edges():
    """regimes no workload runs today that the cases add on purpose"""
    bn = set().union(*(LR.bn_reduce_regime(N * H * W, C) for N, H, W, C in CASES["bn"]))
    assert any(r[2] for r in bn), "no BatchNorm case leaves threads without rows"
    cs = set().union(*(LR.colsum_regime(*s) for s in CASES["colsum"]))
    assert any(r[3] for r in cs) and any(r[2] for r in cs), "no column-sum case with idle threads / threads without rows"
    hd = set().union(*(LR.head_regime(*s) for s in CASES["head"]))
    assert ("head", 8, 1, 3, True) in hd and ("head", 16, 1, 2, True) in hd and ("head", 16, 4, 0, False) in hd
    ad = set().union(*(LR.adam_regime(*s) for s in CASES["adam"]))
    assert {("adam_tail", r) for r in range(4)} <= ad


# ---- 3. the bounds can see a dropped row -------------------------------------------------------------------------------------------
def _moves(full, dropped, bound):
    """largest (shift of a reduced output) / (its bound) over all outputs of the case"""
    worst = 0.0
    for k in full:
        b = bound[k].double()
        shift = (full[k] - dropped[k]).abs()
        ok = b > 0
        if bool(ok.any()):
            worst = max(worst, float((shift[ok] / b[ok]).max()))
        if bool((shift[~ok] > 0).any()):
            worst = float("inf")              # bound 0: the output must be exact, any shift shows
    return worst


def _drops(M, rows_per_block, nblk, empty_ok=False):
    d = [("last row", SR.last_row_mask(M))] if (M > 1 or empty_ok) else []
    if nblk > 1:
        d.append(("last workgroup", SR.last_block_mask(M, rows_per_block, nblk)))
    return d


def _assert_sensitive(what, ref_fn, M, rows_per_block, nblk, conditioned=(), empty_ok=False):
    full, bound = ref_fn(None)
    for k in conditioned:
        r = SR.rel_to_max(bound[k], full[k])
        assert r < 1e-4, "%s: the bound on %s is %.2e of the tensor's max: badly conditioned inputs" % (what, k, r)
    for name, keep in _drops(M, rows_per_block, nblk, empty_ok):
        dropped, _ = ref_fn(keep)
        mv = _moves(full, dropped, bound)
        assert mv > 10.0, "%s: dropping the %s moves no output by more than %.2f bounds" % (what, name, mv)


@pytest.mark.parametrize("shape", CASES["bn"])
def test_bn_bounds_see_a_dropped_row(shape):
    inp = SR.bn_inputs(shape)
    M, C = inp["z"].shape
    R, nblk = 256 // (C // 4), LR.bn_blocks(M, C)

    def stats(keep):
        ref, bound = SR.bn_stats_ref(inp, keep)
        return {k: ref[k] for k in ("mean", "var")}, {k: bound[k] for k in ("mean", "var")}
    _assert_sensitive("bn_train_stats %s" % (shape,), stats, M, R, nblk)
    ref, bound = SR.bn_stats_ref(inp)
    for k in ref:
        r = SR.rel_to_max(bound[k], ref[k])
        assert r < 1e-4, "bn_train_stats %s: the bound on %s is %.2e of the tensor's max" % (shape, k, r)
    for relu_out in (True, False):
        _assert_sensitive("bn_bwd %s" % (shape,), lambda keep: SR.bn_bwd_sums_ref(inp, relu_out, keep), M, R, nblk, ("dbeta", "dgamma"))
    if shape in (BN_BIG, BN_SMALL):
        dz, bdz, _ = SR.bn_bwd_dz_ref(inp, True)
        assert SR.rel_to_max(bdz, dz) < 1e-4


@pytest.mark.parametrize("shape", CASES["colsum"])
def test_colsum_bounds_see_a_dropped_row(shape):
    M, C = shape
    inp = SR.colsum_inputs(M, C)
    _assert_sensitive("colsum %s" % (shape,), lambda keep: SR.colsum_ref(inp, keep), M, 256 // (C // 4), LR.colsum_blocks(M, C),
                      ("sum",), empty_ok=True)       # (a sum over no rows is 0: M = 1 can drop its only row)


@pytest.mark.parametrize("shape", CASES["head_wgrad"])
def test_head_wgrad_bounds_see_a_dropped_pixel(shape):
    N, h, w, Cin = shape
    inp = SR.head_inputs(shape)
    _assert_sensitive("head_wgrad %s" % (shape,), lambda keep: SR.head_wgrad_ref(inp, keep), N * h * w, 256 // (Cin // 4),
                      LR.head_wgrad_blocks(N * h * w, Cin), ("dw", "db"))


# ---- 5. the 3x3 stride-1 tile kernels: restatement against the library, workload against the cases of test_gpu_conv_tile_edges.py ----
TILE_CHANNELS = [(32, 0, 32), (64, 0, 64), (20, 0, 72), (112, 0, 40), (12, 0, 16), (80, 0, 96), (32, 20, 64), (16, 0, 32), (64, 64, 64),
                 (512, 0, 256), (256, 256, 256), (30, 0, 32)]
_GATHER_ID = {"zero": 0, "reflect": 1, "up2": 2, "dgrad": 3, "dgrad_reflect": 4}


def _desc(N, H, W, C0, C1, Nout, gather):
    from footprints_amd import ops
    return ops.make_desc(N, H, W, H, W, C0, C1, Nout, 3, 1, 1, _GATHER_ID[gather])


def _tile_sweep_shapes():
    hs = sorted(set([2, 3, 5, 6, 7, 8, 11, 12, 15, 16, 20, 24, 26, 31, 32, 33, 40, 48, 64, 65, 96, 128, 140] + _sweep(11, 14, 2, 141)))
    ws = sorted(set([2, 3, 15, 16, 19, 20, 26, 40, 65, 66, 80, 82, 104, 121, 122, 140] + _sweep(12, 12, 2, 141)))
    ns = [1, 2, 3, 4, 7, 12, 13, 26, 43, 64]
    return hs, ws, ns


def _tile_switched():
    import os
    return sorted(k for k in os.environ if k.startswith("FP_TILE_") or k.startswith("FP_WGRAD_"))


def test_tile3_plan_matches_library():
    """fp_conv3x3_bf3_supported and fp_conv3x3_bf3_workspace (host-only queries) against tile3_plan over ~60 000 descriptors"""
    if _tile_switched():
        pytest.skip("the launch rules are switched by %s: the restatement is that of the default build" % ", ".join(_tile_switched()))
    import ctypes as C
    lib = _lib()
    assert _GATHER_ID == {"zero": 0, "reflect": 1, "up2": 2, "dgrad": 3, "dgrad_reflect": 4}
    hs, ws, ns = _tile_sweep_shapes()
    n = 0
    for C0, C1, Nout in TILE_CHANNELS:
        for gather in (("up2",) if C1 else ("zero", "up2", "dgrad_reflect")):
            for H in hs:
                for W in ws:
                    for N in ns:
                        d = _desc(N, H, W, C0, C1, Nout, gather)
                        p = LR.tile3_plan(N, H, W, C0, C1, Nout, gather == "up2")
                        assert bool(lib.fp_conv3x3_bf3_supported(C.byref(d))) == (p is not None), (gather, N, H, W, C0, C1, Nout)
                        assert lib.fp_conv3x3_bf3_workspace(C.byref(d)) == (p["workspace"] if p else 0), (gather, N, H, W, C0, C1, Nout)
                        if p and p["SK"] > 1:
                            assert p["workspace"] == p["SK"] * N * H * W * Nout * 4
                        n += 1
    assert n > 3000


def test_wgrad3_plan_matches_library():
    """fp_conv_wgrad_bf3_workspace against wgrad3_plan: S (9 C0 Nout + Nout) 4 bytes, or -1"""
    if _tile_switched():
        pytest.skip("the launch rules are switched by %s: the restatement is that of the default build" % ", ".join(_tile_switched()))
    import ctypes as C
    lib = _lib()
    hs, ws, ns = _tile_sweep_shapes()
    n = 0
    for C0, Nout in [(32, 32), (32, 64), (64, 32), (32, 96), (96, 32), (256, 256), (512, 256), (480, 256), (20, 32), (32, 40), (128, 128)]:
        for mode in ("zero", "reflect", "up2"):
            for H in hs:
                for W in ws:
                    for N in ns:
                        p = LR.wgrad3_plan(N, H, W, C0, Nout, mode == "up2")
                        got = lib.fp_conv_wgrad_bf3_workspace(C.byref(_desc(N, H, W, C0, 0, Nout, mode)))
                        assert got == (p["workspace"] if p else -1), (mode, N, H, W, C0, Nout)
                        if p:
                            assert p["workspace"] == p["S"] * (9 * C0 * Nout + Nout) * 4
                        n += 1
    assert n > 3000


def tile_workload(N, H, W, psp=False):
    """the 3x3 stride-1 convolutions of one train step as (tile cases without format, weight-gradient cases without format), by
    engine.py line; a superset where a switch or a shape test decides between the tile kernels and another path.
    Encoder (engine.py:787 forward, :1318 data gradient, :1122 weight gradient): conv2 of every block and conv1 of the stride-1 blocks.
    Decoder block bi at (h, w) = level 4 - bi (engine.py:1091-1096): pre1 cin -> cout, pre2 at (h, w); post1 over cat[up2(y2), skip]
    (or its skip half alone beside the phase kernels, :900), post2 at (2h, 2w); o41 / o42 at full resolution (:1105-1106).
    Data gradients :1183 (:1501 :1508 :1530 :1545 :1549 :1559 :1570-1573), weight gradients :1129 :1152-1154 :1173 (:1500 :1503 :1529-1565)"""
    tile, wg = [], []
    for s, c in ((2, 64), (3, 128), (4, 256), (5, 512)):
        h, w = H >> s, W >> s
        tile += [("zero", N, h, w, c, 0, c), ("dgrad", N, h, w, c, 0, c)]
        wg.append(("zero", N, h, w, c, c))
    chans = [(1024 if psp else 512, 256), (256, 128), (128, 64), (64, 64)]
    for bi, (cin, cout) in enumerate(chans):
        h, w = (H >> 5) << bi, (W >> 5) << bi
        hh, ww = 2 * h, 2 * w
        tile += [("reflect", N, h, w, cin, 0, cout), ("reflect", N, h, w, cout, 0, cout), ("up2", N, hh, ww, cout, cout, cout),
                 ("reflect", N, hh, ww, cout, 0, cout),                                   # post1's skip half, and post2
                 ("dgrad_reflect", N, h, w, cout, 0, cin), ("dgrad_reflect", N, h, w, cout, 0, cout),
                 ("dgrad_reflect", N, hh, ww, cout, 0, cout), ("dgrad_reflect", N, hh, ww, cout, 0, 2 * cout)]
        wg += [("reflect", N, h, w, cin, cout), ("reflect", N, h, w, cout, cout), ("reflect", N, hh, ww, cout, cout),
               ("up2", N, hh, ww, cout, cout)]
    tile += [("up2", N, H, W, 64, 0, 32), ("reflect", N, H, W, 32, 0, 32), ("dgrad_reflect", N, H, W, 32, 0, 32),
             ("dgrad_reflect", N, H, W, 32, 0, 64)]
    wg += [("up2", N, H, W, 64, 32), ("reflect", N, H, W, 32, 32)]
    return tile, wg


TILE_WORKLOAD = {"footprints 12x192x640": tile_workload(12, 192, 640), "footprints 4x512x640": tile_workload(4, 512, 640),
                 "footprints 12x128x416": tile_workload(12, 128, 416), "psp segmentor 12x192x640": tile_workload(12, 192, 640, psp=True)}
TILE_FORMATS = ("exact", "pair")


def tile_workload_regimes():
    """{regime tuple: (workload name, launch) of its first occurrence} over both training formats; launches the planners turn down
    (they take the flattened kernels) are no part of it"""
    need = {}
    for name, (tile, wg) in TILE_WORKLOAD.items():
        for fmt in TILE_FORMATS:
            for gather, N, H, W, C0, C1, Nout in tile:
                if LR.tile3_plan(N, H, W, C0, C1, Nout, gather == "up2", fmt):
                    for r in LR.tile3_regime(gather, fmt, N, H, W, C0, C1, Nout):
                        need.setdefault(r, (name, (gather, fmt, N, H, W, C0, C1, Nout)))
            for mode, N, H, W, C0, Nout in wg:
                if LR.wgrad3_plan(N, H, W, C0, Nout, mode == "up2"):
                    for r in LR.wgrad3_regime(mode, fmt, N, H, W, C0, Nout):
                        need.setdefault(r, (name, (mode, fmt, N, H, W, C0, Nout)))
    return need


def tile_case_regimes():
    have = set()
    for c in TR.TILE_CASES:
        have |= LR.tile3_regime(*c)
    for c in TR.WGRAD_CASES:
        have |= LR.wgrad3_regime(*c)
    return have


def test_tile_cases_are_launchable():
    """every GPU case is a shape its launcher takes (an unsupported case is an error of the table, never a skip)"""
    for gather, fmt, N, H, W, C0, C1, Nout in TR.TILE_CASES + TR.TILE_TWO_TERM:
        assert LR.tile3_plan(N, H, W, C0, C1, Nout, gather == "up2", fmt), (gather, fmt, N, H, W, C0, C1, Nout)
    for mode, fmt, N, H, W, C0, Nout in TR.WGRAD_CASES:
        assert LR.wgrad3_plan(N, H, W, C0, Nout, mode == "up2"), (mode, fmt, N, H, W, C0, Nout)


def test_tile_workload_regimes_occur_in_cases():
    have = tile_case_regimes()
    missing = {r: w for r, w in tile_workload_regimes().items() if r not in have}
    lines = ["%s: first run by %s %s" % (r, w[0], w[1]) for r, w in sorted(missing.items(), key=repr)]
    assert not missing, "%d launch regimes of the train step that no GPU case of tests/conv_tile_refs.py runs:\n%s" % (len(lines), "\n".join(lines))


def _split_sizes(c):
    gather, fmt, N, H, W, C0, C1, Nout = c
    p = LR.tile3_plan(N, H, W, C0, C1, Nout, gather == "up2", fmt)
    return p, tuple(min(p["KC16"], (s + 1) * p["cps"]) - s * p["cps"] for s in range(p["SK"]))


def test_tile_cases_reach_the_structural_edges():
    """edges the cases add on purpose, whether or not a train step runs them today"""
    have = tile_case_regimes()
    axes = {}
    for r in have:
        if r[0] == "tile3":
            axes.setdefault((r[1][1], r[2]), set()).add(r[3])          # (tile height, axis) -> values over all kernels
    for th in (8, 6):
        assert axes[(th, "ragx")] == {0, 1, 2, 3} and axes[(th, "ragy")] >= {0, 1, 3}, (th, axes[(th, "ragx")], axes[(th, "ragy")])
        assert axes[(th, "chunks")] == {1, 2, 3, "even", "odd"}, (th, axes[(th, "chunks")])
        assert {(False, "before"), (False, "last")} <= axes[(th, "foldx")] and (True, "last") in axes[(th, "foldy")]
        assert {True, False} <= axes[(th, "ctail")] and {True, False} <= axes[(th, "ntail")] and {True, False} <= axes[(th, "wmajor")]
    assert axes[(8, "c1")] == {"none", "tail", "whole"} and axes[(6, "c1")] >= {"none", "whole"}
    sizes = {(c[0], c[1]): _split_sizes(c)[1] for c in TR.TILE_CASES if _split_sizes(c)[1] == (3, 3, 1)}
    assert {"fwd", "fold", "flip"} <= {LR.TILE3_GATHERS[g] for g, _ in sizes} and {"exact", "pair"} <= {f for _, f in sizes}, sizes
    p, s = _split_sizes(("up2", "pair", 9, 8, 66, 48, 64, 40))
    assert s == (3, 3, 1) and p["cps"] * 16 == 48                      # the concat gather switches sources exactly where the second split begins
    single = [c for c in TR.TILE_CASES if c[3:5] == (7, 15)]           # one partial tile per image, in both formats
    assert {c[1] for c in single} == {"exact", "pair"}
    assert any(_split_sizes(c)[0]["inst"] == "pair" and _split_sizes(c)[0]["bn"] == 64 for c in TR.TILE_CASES)       # above 400 workgroups
    wg = {}
    for r in have:
        if r[0] == "wgrad3":
            wg.setdefault(r[2], set()).add(r[3])
    assert wg["remy"] == {0, 1, 2, 3} and wg["remx"] == {0, 1, 2, 3} and wg["reduce"] == {"plain", "capped", "transposing"}
    assert wg["chunks"] == {"border", "both"} and wg["cnt"] == {0, 1} and wg["s4"] == {0, 1, 2, 3}


# ---- 6. the nearest-x2 phase kernels: restatement against the library, workload against the cases of test_gpu_conv_phase_edges.py ----
def _phase_switched():
    import os
    return sorted(k for k in os.environ if k.startswith("FP_PWGRAD_"))


def test_phase_wgrad_plan_matches_library():
    """fp_conv_up2_phase_wgrad_workspace against phase_wgrad_plan: (S 16 C0 Nout + S Nout) 4 bytes, or -1; the bytes give S"""
    if _phase_switched():
        pytest.skip("the launch rules are switched by %s: the restatement is that of the default build" % ", ".join(_phase_switched()))
    lib = _lib()
    hs = sorted(set([1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 13, 16, 24, 26, 32, 48, 64, 96, 128, 256] + _sweep(21, 8, 1, 130)))
    ws = sorted(set([1, 2, 12, 13, 14, 15, 16, 17, 18, 19, 20, 26, 29, 32, 33, 40, 48, 52, 80, 104, 160, 208, 320] + _sweep(22, 8, 1, 330)))
    ns = [1, 2, 3, 4, 5, 7, 8, 12, 16, 64]
    n = 0
    for C0, Nout in [(32, 32), (32, 64), (64, 32), (64, 64), (96, 32), (128, 128), (256, 256), (1024, 768), (512, 1536), (20, 32), (32, 40), (0, 32), (32, 0), (-32, 32)]:      # (no channels: the query once divided by zero tiles)
        for h in hs:
            for w in ws:
                for N in ns:
                    p = LR.phase_wgrad_plan(N, h, w, C0, Nout)
                    got = lib.fp_conv_up2_phase_wgrad_workspace(N, h, w, C0, Nout)
                    assert got == (p["workspace"] if p else -1), (N, h, w, C0, Nout, got, p)
                    if p:
                        assert got % ((16 * C0 * Nout + Nout) * 4) == 0 and got // ((16 * C0 * Nout + Nout) * 4) == p["S"]
                        assert sum(LR.phase_wgrad_split_counts(p, "f32")) == p["nchunks"] == sum(LR.phase_wgrad_split_counts(p, "exact"))
                        assert min(LR.phase_wgrad_split_counts(p, "f32")) >= 1
                    n += 1
    assert n > 3000


def test_phase_tile_plans():
    """the forward and data-gradient launchers have no host query: the restatement is checked against its own definition at the shapes of a
    train step (workgroups = tiles x phases; the data gradient tiles the extended grid and runs the four phases inside a workgroup)"""
    p = LR.phase_fwd_plan(12, 48, 160, 64, 64)
    assert (p["bn"], p["tilesY"], p["tilesX"], p["tilesN"], p["KC16"], p["nwg"]) == (64, 6, 10, 1, 4, 12 * 60 * 4)
    p = LR.phase_fwd_plan(12, 96, 320, 64, 32, "pair")
    assert (p["bn"], p["tilesN"], p["nwg"]) == (32, 1, 12 * 12 * 20 * 4)
    p = LR.phase_dgrad_plan(12, 96, 320, 32, 64)
    assert (p["bn"], p["tilesY"], p["tilesX"], p["KC16"], p["nsteps"], p["nwg"]) == (64, 13, 21, 2, 8, 12 * 13 * 21)
    p = LR.phase_dgrad_plan(4, 8, 10, 256, 256)
    assert (p["tilesY"], p["tilesX"], p["tilesN"], p["KC16"]) == (2, 1, 4, 16)
    assert LR.phase_fwd_plan(1, 4, 4, 18, 16) is None and LR.phase_dgrad_plan(1, 4, 4, 18, 16) is None           # channels % 4
    assert LR.phase_dgrad_plan(1, 4, 4, 16, 16, "f32") is None                                                       # that path is conv_igemm
    assert LR.phase_fwd_plan(64, 512, 512, 16, 8, "exact") is None and LR.phase_fwd_plan(64, 512, 512, 16, 8, "f32")  # 2^29 elements: split formats only
    assert LR.phase_ok(12, 40) and LR.phase_ok(8, 26) and not LR.phase_ok(6, 20) and not LR.phase_ok(4, 13)
    assert LR.phase_ok(26, 42) and LR.phase_ok(6, 15) and not LR.phase_ok(18, 22) and not LR.phase_ok(10, 28)       # extended grids


def phase_workload(N, H, W):
    """the phase launches of one train step: (forward (N, h, w, C0, C1, Nout), data gradient (N, h, w, C0, Nout), fold (N, h, w, C0, addend,
    ylow), weight gradient (N, h, w, C0, C1, Nout)) at LOW resolution h x w, by engine.py line.
    Decoder block bi (engine.py:1091-1096): post1 over cat[up2(y2), skip] with C0 = C1 = Nout = cout at level 4 - bi; o41 over up2(x4) alone
    with 64 -> 32 at H/2 x W/2 (:1105).  Forward :897-910 (the skip half first, then the phase kernel adds in place, bias + ELU); weight
    gradient :1136-1179 (k_begin = 0 of a gradient of C0 + C1 channels, the bias gradient in the same pass); data gradient :1186-1196 on the
    extended grid; fold :1503-1540 (o41: + the head's gradient, * ELU'; blocks: * ELU')"""
    fwd, dg, fold, wg = [], [], [], []
    for bi, cout in enumerate((256, 128, 64, 64)):
        h, w = (H >> 5) << bi, (W >> 5) << bi
        fwd.append((N, h, w, cout, cout, cout))
        dg.append((N, h, w, cout, cout))
        fold.append((N, h, w, cout, False, True))
        wg.append((N, h, w, cout, cout, cout))
    h0, w0 = H // 2, W // 2
    return fwd + [(N, h0, w0, 64, 0, 32)], dg + [(N, h0, w0, 64, 32)], fold + [(N, h0, w0, 64, True, True)], wg + [(N, h0, w0, 64, 0, 32)]


PHASE_WORKLOAD = {"footprints 12x192x640": phase_workload(12, 192, 640), "footprints 4x512x640": phase_workload(4, 512, 640),
                  "footprints 12x128x416": phase_workload(12, 128, 416), "psp segmentor 12x192x640": phase_workload(12, 192, 640)}


def phase_workload_regimes():
    """({regime tuple: (workload name, launch) of its first occurrence}, [launches the gates turn down]) over both training formats.
    Gates: forward engine.py:898 _phase_ok(h, w); data gradient :1190 _phase_ok(h + 2, w + 2); weight gradient :1142 eligible.  The fold
    runs either way (:1512 :1540: a turned-down data gradient fills the same extended grid through conv_igemm)."""
    need, down = {}, []
    for name, (fwd, dg, fold, wg) in PHASE_WORKLOAD.items():
        for fmt in TILE_FORMATS:
            for N, h, w, C0, C1, Nout in fwd:
                if not LR.phase_ok(h, w):
                    down.append((name, "fwd", N, h, w))
                    continue
                epi = ("act", "bias") + (("addend",) if C1 else ())
                for r in LR.phase_regime("fwd", fmt, N, h, w, C0, C1, Nout, epi=epi):
                    need.setdefault(r, (name, ("fwd", fmt, N, h, w, C0, C1, Nout)))
            for N, h, w, C0, Nout in dg:
                if not LR.phase_ok(h + 2, w + 2):
                    down.append((name, "dgrad", N, h, w))
                    continue
                for r in LR.phase_regime("dgrad", fmt, N, h, w, C0, 0, Nout):
                    need.setdefault(r, (name, ("dgrad", fmt, N, h, w, C0, Nout)))
            for N, h, w, C0, C1, Nout in wg:
                if not LR.phase_wgrad_plan(N, h, w, C0, Nout):
                    down.append((name, "wgrad", N, h, w))
                    continue
                for r in LR.phase_regime("wgrad", fmt, N, h, w, C0, 0, Nout, kslice=(0, C1)):
                    need.setdefault(r, (name, ("wgrad", fmt, N, h, w, C0, C1, Nout)))
        for N, h, w, C0, addend, ylow in fold:
            for r in LR.fold_regime(N, h, w, C0, addend, ylow):
                need.setdefault(r, (name, ("fold", N, h, w, C0, addend, ylow)))
    return need, sorted(set(down))


def phase_case_regimes():
    have = set()
    for kind, table in (("fwd", PR.PHASE_FWD), ("dgrad", PR.PHASE_DGRAD), ("wgrad", PR.PHASE_WGRAD), ("fold", PR.PHASE_FOLD)):
        for c in table:
            have |= PR.case_regimes(kind, c)
    return have


def test_phase_gates_turn_down_the_deepest_levels():
    """which launches of a train step the gates keep away from the phase kernels.  The forward gate looks at h x w, the data gradient's at the
    extended (h + 2) x (w + 2): 6 x 20 fails as a forward (62 % of 8 x 32 is under the 60 % rule's 6/10 of 256) and passes as 8 x 22;
    16 x 20 passes as a forward and fails as 18 x 22; 8 x 26 passes and 10 x 28 fails; 4 x 13 fails and its 6 x 15 -- one partial tile --
    passes.  The weight gradient's own rule (30 % padded 2 x 16 chunks) turns down 6 x 20 and 16 x 20 and takes 4 x 13."""
    _, down = phase_workload_regimes()
    assert down == [("footprints 12x128x416", "dgrad", 12, 8, 26), ("footprints 12x128x416", "fwd", 12, 4, 13),
                    ("footprints 12x192x640", "fwd", 12, 6, 20), ("footprints 12x192x640", "wgrad", 12, 6, 20),
                    ("footprints 4x512x640", "dgrad", 4, 16, 20), ("footprints 4x512x640", "wgrad", 4, 16, 20),
                    ("psp segmentor 12x192x640", "fwd", 12, 6, 20), ("psp segmentor 12x192x640", "wgrad", 12, 6, 20)], down


def test_phase_cases_are_launchable():
    """an unsupported row in a table is an error, never a skip"""
    for fmt, N, h, w, C0, C1, Nout in PR.PHASE_FWD:
        assert fmt in LR.PHASE_FORMATS and LR.phase_fwd_plan(N, h, w, C0, Nout, fmt) and C1 % 4 == 0, (fmt, N, h, w, C0, C1, Nout)
    for fmt, N, h, w, C0, C1, Nout in PR.PHASE_DGRAD:
        assert fmt in ("exact", "pair") and C1 == 0 and C0 % 4 == 0 and LR.phase_dgrad_plan(N, h, w, Nout, C0, fmt), (fmt, N, h, w, C0, Nout)
    for fmt, N, h, w, C0, ks, Nout in PR.PHASE_WGRAD:
        assert fmt in LR.PHASE_FORMATS and len(ks) == 2 and LR.phase_wgrad_plan(N, h, w, C0, Nout), (fmt, N, h, w, C0, ks, Nout)
    for kind, c in PR.PHASE_CANCEL:
        assert c[0] in ("exact", "pair") and c[4] % 4 == 0 and c[6] % 4 == 0
        assert LR.phase_fwd_plan(*c[1:5], c[6], c[0]) if kind == "fwd" else LR.phase_dgrad_plan(c[1], c[2], c[3], c[6], c[4], c[0])
    for t in (PR.PHASE_FWD, PR.PHASE_DGRAD, PR.PHASE_WGRAD, PR.PHASE_FOLD):
        assert len(set(t)) == len(t)


def test_phase_workload_regimes_occur_in_cases():
    have = phase_case_regimes()
    need, _ = phase_workload_regimes()
    missing = {r: w for r, w in need.items() if r not in have}
    lines = ["%s: first run by %s %s" % (r, w[0], w[1]) for r, w in sorted(missing.items(), key=repr)]
    assert not missing, "%d launch regimes of the train step that no GPU case of tests/conv_phase_refs.py runs:\n%s" % (len(lines), "\n".join(lines))


def test_phase_cases_reach_the_structural_edges():
    """edges the cases add on purpose, whether or not a train step runs them today -- per compiled kernel, not only over all of them"""
    axes = {}
    for r in phase_case_regimes():
        if r[0] == "phase":
            axes.setdefault(r[1], {}).setdefault(r[2], set()).add(r[3])
    keys = [(k, bn, f) for k, fmts in (("fwd", LR.PHASE_FORMATS), ("dgrad", ("exact", "pair"))) for bn in (32, 64) for f in fmts]
    for key in keys:
        a = axes[key]
        assert a["chunks"] == {1, 2, 3, "even", "odd"}, (key, a["chunks"])            # KC16 = 1: every step of the data gradient changes phase
        many = {(r, True) for r in (0, 1, 2, 3)}                                     # every remainder behind a full tile, and a single partial tile
        assert many <= a["ragx"] and many <= a["ragy"] and any(not m for _, m in a["ragx"]) and any(not m for _, m in a["ragy"]), (key, a["ragx"], a["ragy"])
        assert a["grid"] == {(n, t) for n in (False, True) for t in (False, True) if key[1] == 64 or not t}, (key, a["grid"])
        assert a["ctail"] == {True, False} and a["ntail"] == {True, False}, (key, a["ctail"], a["ntail"])
        assert a["clampy"] == {"no", "both", "one"} and a["clampx"] == {"no", "both", "one"}, (key, a["clampy"], a["clampx"])       # h == 1, w == 1, h < 8
        if key[0] == "fwd":
            assert a["epi"] == set(PR.FWD_EPIS), (key, a["epi"])
    for fmt in ("exact", "pair"):                                                     # h == w == 1: nine extended positions fold onto one pixel
        assert any(c[0] == fmt and c[2] == c[3] == 1 for c in PR.PHASE_DGRAD) and any(c[0] == fmt and c[2] == c[3] == 1 for c in PR.PHASE_FWD)
    for key in [("wgrad", "fp32", "f32"), ("wgrad", "split", "exact"), ("wgrad", "split", "pair")]:
        a = axes[key]
        assert {(r, True) for r in (0, 1, 2, 3)} <= a["ragx"] and a["ragy"] == {0, 1} and a["clampx"] == {"no", "both"}, (key, a)
        assert {(True, False, False), (True, True, False), (True, False, True), (True, True, True), (False, True, True)} <= a["grid"], (key, a["grid"])
        assert a["s1"] == {True, False} and a["s4"] == {0, 1, 2, 3}, (key, a["s1"], a["s4"])
        assert a["kslice"] == {(False, False), (False, True), (True, False), (True, True)}, (key, a["kslice"])
        assert {"even", "odd"} <= a["cnt"], (key, a["cnt"])
        assert {(False, 1), (False, 2), (False, 3), (True, 0), (True, 1), (True, 2), (True, 3)} <= a["sum"], (key, a["sum"])
        assert a["db"] == {key[2] != "f32"}
    f32 = axes[("wgrad", "fp32", "f32")]
    assert f32["short"] == {True, False} and {1, 2, "even", "odd"} <= f32["cnt"], (f32["short"], f32["cnt"])
    fold = {}
    for r in phase_case_regimes():
        if r[0] == "fold":
            fold.setdefault(r[1], set()).add(r[2])
    assert fold["ny"] == {True, False} and fold["nx"] == {True, False} and fold["operands"] == {(True, True), (False, True)}
    assert {("ew", "up2_fold", 1, True), ("ew", "up2_fold", 2, True), ("ew", "up2_fold", 2, False)} <= phase_case_regimes()
