"""GPU: the ground-segmentation network (reference footprints/preprocessing/segmentation/network.py)
on the HIP engine: pyramid-pooling kernels against torch CPU ops, the Segmentor against the G9 fixture (the reference's own
module) and against the CPU oracle at the KITTI resolution, forward and backward through the segmentation trainer's loss."""
from collections import OrderedDict

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def relerr(got, ref):
    ref = ref.double().cpu()
    return ((got.double().cpu() - ref).abs().max() / ref.abs().max().clamp_min(1e-30)).item()


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().cuda()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous().cpu()


def rnd(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g) - 0.5


@pytest.mark.parametrize("N,H,W,C,P", [(2, 6, 20, 512, 1), (2, 6, 20, 512, 2), (2, 6, 20, 512, 4), (2, 6, 20, 512, 6), (1, 16, 20, 64, 6), (3, 2, 3, 8, 4)])
def test_adaptive_avgpool_fwd_bwd(N, H, W, C, P):
    from footprints_amd import ops
    x = rnd((N, C, H, W), 1).requires_grad_(True)
    y = F.adaptive_avg_pool2d(x, (P, P))
    g = rnd(tuple(y.shape), 2)
    y.backward(g)
    got = ops.adaptive_avgpool_fwd(nhwc(x.detach()), torch.empty((N, P, P, C), device="cuda"))
    assert relerr(nchw(got), y.detach()) <= 1e-6
    base = rnd((N, C, H, W), 3)
    dx = nhwc(base)
    ops.adaptive_avgpool_bwd(nhwc(g), dx, accumulate=True)
    assert relerr(nchw(dx), base + x.grad) <= 1e-6
    ops.adaptive_avgpool_bwd(nhwc(g), dx, accumulate=False)
    assert relerr(nchw(dx), x.grad) <= 1e-6


@pytest.mark.parametrize("N,P,C,H,W", [(2, 1, 128, 6, 20), (2, 2, 128, 6, 20), (2, 4, 128, 6, 20), (2, 6, 128, 6, 20), (1, 6, 16, 16, 20), (2, 4, 8, 2, 3)])
def test_bilinear_align_corners_fwd_bwd_into_channel_slice(N, P, C, H, W):
    from footprints_amd import ops
    src = rnd((N, C, P, P), 4).requires_grad_(True)
    y = F.interpolate(src, size=(H, W), mode="bilinear", align_corners=True)
    g = rnd(tuple(y.shape), 5)
    y.backward(g)
    dstC, off = C * 3, C
    dst = torch.full((N, H, W, dstC), 7.0, device="cuda")
    ops.bilinear_ac_fwd(nhwc(src.detach()), dst, off)
    assert relerr(nchw(dst[..., off:off + C]), y.detach()) <= 1e-6
    assert bool((dst[..., :off] == 7.0).all()) and bool((dst[..., off + C:] == 7.0).all())       # neighbours of the slice untouched
    gd = torch.zeros((N, H, W, dstC), device="cuda")
    gd[..., off:off + C] = nhwc(g)
    dsrc = ops.bilinear_ac_bwd(gd, torch.empty((N, P, P, C), device="cuda"), off)
    assert relerr(nchw(dsrc), src.grad) <= 1e-6


def test_copy_channels():
    from footprints_amd import ops
    a = torch.rand(2, 3, 5, 16, device="cuda")
    b = torch.rand(2, 3, 5, 40, device="cuda")
    ref = b.clone()
    ops.copy_channels(a, b, 8, src_off=4, dst_off=12)
    ref[..., 12:20] = a[..., 4:12]
    assert torch.equal(b, ref)
    ops.copy_channels(a, b, 8, src_off=4, dst_off=12, accumulate=True)
    ref[..., 12:20] += a[..., 4:12]
    assert torch.equal(b, ref)


def _seg_model(P, Bf, psp):
    from footprints_amd.preprocessing.segmentation.network import Segmentor
    m = Segmentor(pretrained=False, use_PSP=psp)
    m.load_state_dict({**P, **Bf})
    return m.cuda()


@pytest.mark.parametrize("psp", [False, True])
def test_g9_segmentor_against_reference_fixture(psp):
    from oracle import filler, restatement as R
    from tests.golden.digest import compare, load
    gold = load("g9_segmentor")
    tag = "psp" if psp else "plain"
    B, H, W = 2, 64, 96
    image = torch.from_numpy(filler.uniform("g9:image", (B, 3, H, W))).cuda()
    gmask = torch.from_numpy(filler.bernoulli("g9:gmask", (B, H, W), 0.4)).cuda()
    lmask = torch.from_numpy(filler.bernoulli("g9:lmask", (B, H, W), 0.7)).cuda()
    P, Bf = R.make_seg_state(psp, tag="g9." + tag)
    m = _seg_model(P, Bf, psp)
    m.train()
    outs = m(image)
    assert [tuple(o.shape) for o in outs] == [(B, 1, H // s, W // s) for s in (8, 4, 2, 1)]
    for i, o in enumerate(outs):
        compare(gold, "seg.%s.out%d" % (tag, i), o)
    loss = R.seg_loss(outs, gmask, lmask, H, W)          # the trainer's torch ops (bilinear up-sizing + masked BCE) on the device tensors
    loss.backward()
    assert abs(float(loss) - float(gold["seg.%s.loss" % tag])) <= 1e-5 * abs(float(gold["seg.%s.loss" % tag]))
    g = dict(m.named_parameters())
    names = [str(n) for n in gold["seg.%s.param_names" % tag]]
    assert [k for k in names if g[k].grad is None] == [str(n) for n in gold["seg.%s.dead" % tag]]
    # 2x64x96 is fp32-ill-conditioned in the encoder (12 BatchNorm samples per channel at layer4, see test_gpu_parity_fullsize):
    # digests of the decoder-side tensors at 1e-3, the full gradient set is held to the fp64-anchored rule below at 2x192x640
    for k in [f[len("seg.%s.grad." % tag):].split("#")[0] for f in gold.files if f.startswith("seg.%s.grad." % tag)]:
        compare(gold, "seg.%s.grad.%s" % (tag, k), g[k].grad, rtol=1e-3, atol_scale=1e-3)


def test_segmentor_psp_train_step_fp64_anchored_at_kitti_resolution():
    """fwd + masked BCE + bwd of the PSP Segmentor at 2x192x640 against the oracle in fp32 and fp64 (tests/parity.py)"""
    from oracle import filler, restatement as R
    from tests.parity import anchored_report, chan_relerr
    B, H, W = 2, 192, 640
    image = torch.from_numpy(filler.uniform("segk:image", (B, 3, H, W)))
    gmask = torch.from_numpy(filler.bernoulli("segk:gmask", (B, H, W), 0.4))
    lmask = torch.from_numpy(filler.bernoulli("segk:lmask", (B, H, W), 0.7))
    P, Bf = R.make_seg_state(True, tag="segk")
    ref = {}
    rec64 = []
    for dt in (torch.float32, torch.float64):
        Pd = OrderedDict((k, v.detach().clone().to(dt).requires_grad_(True)) for k, v in P.items())
        Bd = OrderedDict((k, v.to(dt) if v.is_floating_point() else v.clone()) for k, v in Bf.items())
        outs = R.segmentor(image.to(dt), Pd, Bd, True, True, record=rec64 if dt == torch.float64 else None)
        loss = R.seg_loss(outs, gmask.to(dt), lmask.to(dt), H, W)
        loss.backward()
        ref[dt] = ([o.detach() for o in outs], float(loss), OrderedDict((k, p.grad) for k, p in Pd.items()))
    m = _seg_model(P, Bf, True)
    m.train()
    outs = m(image.cuda())
    loss = R.seg_loss(outs, gmask.cuda(), lmask.cuda(), H, W)
    loss.backward()
    for i, o in enumerate(outs):
        assert max(chan_relerr(o, ref[torch.float32][0][i])) <= 1e-4 and max(chan_relerr(o, ref[torch.float64][0][i])) <= 1e-4, i
    assert abs(float(loss) - ref[torch.float64][1]) <= 1e-5 * abs(ref[torch.float64][1])
    g_gpu = OrderedDict((n, p.grad) for n, p in m.named_parameters())
    g32, g64 = ref[torch.float32][2], ref[torch.float64][2]
    # two images = 240 BatchNorm samples per channel at layer4: one activation within fp32 round-off of 0 that an fp32 implementation
    # resolves differently from the float64 truth moves every gradient upstream by ~1e-3 (the CPU's own fp32 run shows errors of that
    # size here).  As in tests/test_gpu_network.py the encoder part of the rule applies when the engine's ReLU masks equal the
    # oracle's; the twelve-image Footprints tests (tests/test_gpu_parity_fullsize.py) cover the encoder without this caveat.
    flips = [int(((blk["out"].permute(0, 3, 1, 2).cpu() > 0) != (r.detach() > 0)).sum()) for blk, r in zip(m.engine().saved["blocks"], rec64)]
    if sum(flips):
        print("ReLU mask differences against the float64 oracle per encoder block: %s -> encoder gradients not compared" % flips)
        g_gpu, g32, g64 = (OrderedDict((n, g) for n, g in d.items() if "decoder" in n) for d in (g_gpu, g32, g64))
    bad, rows = anchored_report(g_gpu, g32, g64)
    print("\nsegmentor worst GPU/CPU32 ratios:", ["%s %.2f (gpu %.1e cpu %.1e)" % (n, r, eg, ec) for r, n, eg, ec in rows[:5]],
          "median %.2f" % float(np.median([r for r, *_ in rows])))
    assert not bad, bad[:10]
    # inference path (eval mode, folded BatchNorm, no_grad) == the oracle's eval forward
    m = _seg_model(P, Bf, True)           # fresh running statistics (the training forward above moved the first model's)
    m.eval()
    with torch.no_grad():
        ev = m(image.cuda())
    ref_ev = R.segmentor(image, P, OrderedDict((k, v.clone()) for k, v in Bf.items()), False, True)
    for a, b in zip(ev, ref_ev):
        assert max(chan_relerr(a, b)) <= 1e-4


def test_segmentation_inference_dropin():
    """segmentation/inference.py:74-77 counterpart against the oracle's restatement (the segmentation trainer's loss bookkeeping --
    segmentation/evaluation.py, train.py:184-193 -- is host plumbing that runs unchanged on Segmentor's outputs: INTEGRATION.md)"""
    from footprints_amd.preprocessing.segmentation.inference import InferenceManager
    from oracle import filler, restatement as R
    B, H, W = 2, 64, 96
    image = torch.from_numpy(filler.uniform("g9:image", (B, 3, H, W)))
    P, Bf = R.make_seg_state(True, tag="g9.psp")
    im = InferenceManager(model=_seg_model(P, Bf, True))
    got = im.test_batch({"image": image})
    ref = torch.sigmoid(R.segmentor(image, P, OrderedDict((k, v.clone()) for k, v in Bf.items()), False, True)[3]).numpy()
    assert got.shape == (B, 1, H, W) and np.abs(got - ref).max() <= 1e-5


@pytest.mark.parametrize("B,H,W", [(2, 64, 96), (3, 192, 640), (1, 32, 32)])
def test_segmentation_loss_kernel_against_oracle(B, H, W):
    """fp_seg_loss_fwd_bwd (csrc/seg_loss.hip) through SegmentationLoss: value, per-scale tracked means and the gradient with respect
    to the four low-resolution logit maps against the oracle's restatement of segmentation/train.py:184-193 + evaluation.py:39-58 (torch
    float64 autograd): 1e-6; on channel slices of wider buffers (how Segmentor hands its outputs out) and on dense tensors alike"""
    from footprints_amd.preprocessing.segmentation.losses import SegmentationLoss
    from oracle import restatement as R
    g = torch.Generator().manual_seed(B * 100 + H)
    outs = [(torch.rand(B, 1, H // s, W // s, generator=g) * 8 - 4).double().requires_grad_(True) for s in (8, 4, 2, 1)]
    gm = (torch.rand(B, H, W, generator=g) < 0.4).float()
    lm = (torch.rand(B, H, W, generator=g) < 0.7).float()
    lm[0, : H // 2] = 0.0                                    # an image with a large unlabelled region
    ref = R.seg_loss(outs, gm.double(), lm.double(), H, W)
    ref.backward()
    with torch.no_grad():       # the per-scale means of the per-image losses: what the Evaluator tracks under ground_loss_<scale>
        per = [(F.binary_cross_entropy_with_logits(F.interpolate(o, size=(H, W), mode="bilinear", align_corners=False).squeeze(1), gm.double(),
                                                   reduction="none") * lm.double()).sum(dim=[1, 2]) / (lm.double().sum(dim=[1, 2]) + 1e-7) for o in outs]
    want = {"ground_loss_%d" % s: float(per[s].mean()) for s in range(4)}
    assert abs(sum(want.values()) / 4 - float(ref.detach())) <= 1e-12
    for sliced in (False, True):
        if sliced:      # [B,2,h,w] buffers, channel 0 handed out
            bufs = [torch.zeros(B, 2, o.shape[2], o.shape[3], device="cuda") for o in outs]
            for bf, o in zip(bufs, outs):
                bf[:, 0] = o.detach().float().cuda()[:, 0]
            gp = [bf[:, :1].detach().requires_grad_(True) for bf in bufs]
        else:
            gp = [o.detach().float().cuda().requires_grad_(True) for o in outs]
        sl = SegmentationLoss()
        loss = sl(gp, gm.cuda(), lm.cuda())
        loss.backward()
        assert abs(float(loss) - float(ref)) <= 1e-6 * abs(float(ref))
        for p, o in zip(gp, outs):
            err = ((p.grad.double().cpu() - o.grad).norm() / o.grad.norm()).item()
            assert err <= 2e-6, err
        tr = sl.tracked()
        assert set(tr) == {"loss"} | {"ground_loss_%d" % s for s in range(4)} and abs(float(tr["loss"]) - float(ref)) <= 1e-6 * abs(float(ref))
        for key, w in want.items():
            assert abs(float(tr[key]) - w) <= 1e-6 * abs(w), (key, float(tr[key]), w)
        assert sl.tracked() == {}
