"""GPU: the segmentation network's inference mode -- fp_seg_pack (csrc/seg_infer.hip) against the float64 sigmoid and the NumPy
restatement of matplotlib's picture (tests/seg_infer_restatement.py, itself pinned to the reference by fixture G17), Segmentor's
`inference_scales`, and the Tester pipeline end to end against the plain network, the CPU oracle and the reference's file layout."""
import os
from collections import OrderedDict

import numpy as np
import pytest
import torch

from tests import seg_infer_restatement as SR

pytestmark = pytest.mark.gpu

# float16 subnormals come from logits of about -17.3 .. -9.7; -17.4 rounds to 0; +-40 and +-100 saturate
PLANTED = [-17.3, -17.4, -17.0, -16.0, -14.5, -12.0, -10.5, -9.7, 0.0, 17.3, 9.7, 40.0, -40.0, 100.0, -100.0]
GUARD = 64


def _image_pool(n, seed):
    """every k / 255, its float32 neighbours on both sides, and plain random floats, shuffled; the first n of them"""
    rng = np.random.default_rng(seed)
    k = np.arange(256, dtype=np.float32) / np.float32(255)
    up, down = np.nextafter(k[:-1], np.float32(2)), np.nextafter(k[1:], np.float32(-1))
    pool = np.concatenate([k, up, down, rng.random(max(n - 766, 64), dtype=np.float32)]).astype(np.float32)
    return rng.permutation(pool)[:n] if n < pool.size else rng.permutation(pool)


def _guarded(n, dtype, fill, offset):
    """a flat device buffer of n elements behind `offset` elements and in front of a guard, all filled with `fill`"""
    flat = torch.full((offset + n + GUARD,), fill, dtype=dtype, device="cuda")
    assert flat.data_ptr() % 16 == 0          # the offsets of the cases are taken from the 16-byte grid
    return flat, flat[offset:offset + n]


def _guards_intact(flat, n, fill, offset):
    host = flat.cpu()
    return bool((host[:offset] == fill).all() and (host[offset + n:] == fill).all())


CASES = {
    # B, H, W, layout of the logits, element offset of every base pointer
    "odd_stride": (2, 3, 37, "stride+1", 0),          # sample 1 and the odd rows are misaligned for every vector width
    "small": (1, 5, 8, "dense", 0),
    "small_offset_bases": (1, 5, 8, "dense", 1),      # W % 4 == 0 but every base pointer is one element off: scalar path per operand
    "head_buffer": (3, 64, 96, "channel0", 0),        # the engine's case: [:, 0:1] of [B, 2, H, W]
    # the choice of a wide access is per operand: W % 4 == 0 everywhere below, and only the named operands leave the 16-byte grid
    "mixed_odd_stride": (2, 4, 8, "stride+1", 0),                                              # logits scalar, everything else wide
    "mixed_logits_off": (2, 4, 8, "dense", dict(logits=1)),
    "mixed_half_picture_off": (2, 4, 8, "dense", dict(half=1, picture=1)),
    "mixed_f32_image_off": (2, 4, 8, "channel0", dict(f32=1, image=1)),
    # element-aligned but short of the wide access: half at 4 of 8 bytes, float32 / image / logits at 8 of 16, picture at 2 of 4
    "mixed_partly_aligned": (2, 4, 8, "dense", dict(logits=2, half=2, f32=2, image=2, picture=2)),
}
OPERANDS = ("logits", "image", "half", "f32", "picture")


def _make_logits(B, H, W, layout, offset, seed):
    rng = np.random.default_rng(seed)
    vals = rng.uniform(-30.0, 30.0, (B, H, W)).astype(np.float32)
    flatv = vals.reshape(-1)
    pos = rng.permutation(flatv.size)[:len(PLANTED)]
    flatv[pos] = np.array(PLANTED, np.float32)[:pos.size]
    hw = H * W
    stride = {"stride+1": 2 * hw + 1, "dense": hw, "channel0": 2 * hw}[layout]
    buf = torch.full((offset + B * stride + 8,), 1e30, dtype=torch.float32, device="cuda")
    if layout == "channel0":
        full = buf[offset:offset + B * stride].view(B, 2, H, W)
        view = full[:, 0:1]
    else:
        view = torch.as_strided(buf, (B, 1, H, W), (stride, hw, W, 1), storage_offset=offset)
    view.copy_(torch.from_numpy(vals).view(B, 1, H, W).cuda())
    assert view.stride(0) == stride or B == 1
    return view, vals.reshape(B, 1, H, W)


@pytest.mark.parametrize("case", list(CASES))
def test_seg_pack_against_float64_and_restatement(case):
    from footprints_amd import ops
    B, H, W, layout, offset = CASES[case]
    off = {k: (offset.get(k, 0) if isinstance(offset, dict) else offset) for k in OPERANDS}
    n = B * H * W
    logits, host_logits = _make_logits(B, H, W, layout, off["logits"], seed=len(case))
    image_host = _image_pool(B * 3 * H * W, seed=n).reshape(B, 3, H, W)
    offset = off["image"]
    image_flat, image = _guarded(B * 3 * H * W, torch.float32, -3.0, offset)
    image.copy_(torch.from_numpy(image_host).reshape(-1).cuda())
    image = image.view(B, 3, H, W)
    lut = ops.vis_colour_table()

    def run(want_f32, want_picture):
        bufs = (_guarded(n, torch.float16, -7.0, off["half"]), _guarded(n, torch.float32, -7.0, off["f32"]),
                _guarded(6 * n, torch.uint8, 0xA5, off["picture"]))
        half, f32, pic = ops.seg_pack(logits, image if want_picture else None, want_f32=want_f32, want_picture=want_picture,
                                      out=(bufs[0][1], bufs[1][1], bufs[2][1]))
        torch.cuda.synchronize()
        # what was asked for lies between intact guards; what was not asked for is untouched altogether
        assert half.data_ptr() == bufs[0][1].data_ptr() and _guards_intact(bufs[0][0], n, -7.0, off["half"])
        assert (f32 is not None) == want_f32 and (pic is not None) == want_picture
        assert _guards_intact(bufs[1][0], n if want_f32 else 0, -7.0, off["f32"])
        assert _guards_intact(bufs[2][0], 6 * n if want_picture else 0, 0xA5, off["picture"])
        assert bool((image_flat.cpu()[:offset] == -3.0).all() and (image_flat.cpu()[offset + B * 3 * H * W:] == -3.0).all())
        return (half.cpu().numpy().reshape(B, 1, H, W), f32.cpu().numpy().reshape(B, 1, H, W) if want_f32 else None,
                pic.cpu().numpy().reshape(B, H, 2 * W, 3) if want_picture else None)

    half, p32, pic = run(True, True)
    assert np.array_equal(logits.cpu().numpy(), host_logits)                       # the input is only read
    # (1) float32 sigmoid: 4 ulp of the float64 one on [-30, 30] (expf <= 1 ulp attenuated by e / (1 + e) <= 1, + 0.5 for the sum, + 0.5
    #     for the division, doubled for a binade edge between relative error and the ulp of the result)
    p64 = SR.sigmoid64(host_logits)
    inside = np.abs(host_logits) <= 30
    ulp = np.spacing(p64.astype(np.float32)).astype(np.float64)
    err = np.abs(p32.astype(np.float64) - p64) / ulp
    print("%s: max error of prob_f32 on [-30, 30] = %.3f ulp" % (case, err[inside].max()))
    assert err[inside].max() <= 4
    # (2) half = round to nearest even of the kernel's own float32, bit for bit, the planted subnormals included
    want_half = SR.to_half(p32)
    assert np.array_equal(half.view(np.uint16), want_half.view(np.uint16))
    sub = (want_half > 0) & (want_half < np.float16(6.104e-5))
    assert sub.sum() >= 5
    assert want_half[host_logits == np.float32(-17.3)][0] == np.float16(5.96e-8) and want_half[host_logits == np.float32(-17.4)][0] == 0
    # (3) saturation
    for v, h in ((40.0, 1.0), (100.0, 1.0), (-40.0, 0.0), (-100.0, 0.0)):
        at = host_logits == np.float32(v)
        assert at.sum() >= 1 and np.isfinite(p32[at]).all() and (p32[at] >= 0).all() and (p32[at] <= 1).all() and (half[at] == np.float16(h)).all()
    assert np.isfinite(p32).all() and p32.min() >= 0 and p32.max() <= 1
    # (4) the picture: the restatement on the device's own float32 sigmoid, byte for byte
    assert np.array_equal(pic, SR.picture(p32, image_host, lut))
    # (5) the optional outputs do not change the others
    for want_f32, want_picture in ((False, False), (True, False), (False, True)):
        h2, f2, p2 = run(want_f32, want_picture)
        assert np.array_equal(h2.view(np.uint16), half.view(np.uint16))
        assert f2 is None or np.array_equal(f2.view(np.uint32), p32.view(np.uint32))
        assert p2 is None or np.array_equal(p2, pic)


def test_seg_pack_clamps_image_and_rejects_other_layouts():
    from footprints_amd import ops
    B, H, W = 1, 2, 4
    logits = torch.zeros((B, 1, H, W), device="cuda")
    image = torch.tensor([-0.5, 0.0, 1.0, 1.5, float("nan"), 0.5, 2.0, -1e30], device="cuda").view(1, 1, 2, 4).repeat(1, 3, 1, 1).contiguous()
    half, f32, pic = ops.seg_pack(logits, image, want_f32=True, want_picture=True)
    assert (f32 == 0.5).all() and (half == 0.5).all()
    assert pic[0, :, :W, 0].cpu().reshape(-1).tolist() == [0, 0, 255, 255, 0, 127, 255, 0]
    assert (pic[0, :, W:].cpu().numpy() == ops.vis_colour_table()[128]).all()
    wide = torch.zeros((2, 1, 4, 8), device="cuda")
    with pytest.raises(RuntimeError):
        ops.seg_pack(wide[:, :, :, ::2])                       # columns with a stride
    with pytest.raises(RuntimeError):
        ops.seg_pack(wide[:, :, ::2])                          # rows with a stride
    with pytest.raises(RuntimeError):
        ops.seg_pack(wide, want_picture=True)                  # the picture needs the image
    with pytest.raises(RuntimeError):
        ops.seg_pack(wide.double())


def _seg_model(psp):
    from footprints_amd.preprocessing.segmentation.network import Segmentor
    from oracle import restatement as R
    P, Bf = R.make_seg_state(psp, tag="g9.psp" if psp else "g9.plain")
    m = Segmentor(pretrained=False, use_PSP=psp)
    m.load_state_dict({**P, **Bf})
    return m.cuda(), P, Bf


@pytest.mark.parametrize("psp", [False, True])
def test_segmentor_inference_scales(psp):
    from oracle import filler
    m, _, _ = _seg_model(psp)
    m.eval()
    image = torch.from_numpy(filler.uniform("g9:image", (2, 3, 64, 96))).cuda()
    assert m.inference_scales is None
    with torch.no_grad():
        full = [o.clone() for o in m(image)]
        m.inference_scales = ("1/1",)
        only = m(image)
        assert len(only) == 4 and only[0] is None and only[1] is None and only[2] is None
        assert only[3].shape == (2, 1, 64, 96) and torch.equal(only[3], full[3])
        m.inference_scales = ("1/4", "1/1")
        two = m(image)
        assert two[0] is None and two[2] is None and torch.equal(two[1], full[1]) and torch.equal(two[3], full[3])
    with pytest.raises(ValueError):
        m(image)                                               # grad enabled
    m.inference_scales = None
    with torch.no_grad():
        assert all(o is not None for o in m(image))


def test_tester_end_to_end(tmp_path):
    """7 frames of two native sizes in batches of 3 through 2 slots, pictures on: every file of the reference's layout, float16
    [1, H, W], bit-equal to seg_pack of the plain all-heads network on the Pillow-resized frame, and at the oracle's sigmoid"""
    from PIL import Image
    from footprints_amd import ops
    from footprints_amd.preprocessing.segmentation.datasets.inference import KITTIInferenceDataset
    from footprints_amd.preprocessing.segmentation.inference import Tester
    from footprints_amd.preprocessing.segmentation.options import SegmentationOptions
    from oracle import restatement as R
    H, W, BS = 64, 96, 3
    rng = np.random.default_rng(5)
    frames = [rng.integers(0, 256, ((70, 231) if i % 2 == 0 else (75, 248)) + (3,), dtype=np.uint8) for i in range(7)]
    names = ["2011_09_26/drive_%d %d %s" % (i // 4, 10 * i + 3, "l" if i % 3 else "r") for i in range(7)]

    class MemoryKITTI(KITTIInferenceDataset):
        def _load_image(self, index):
            return frames[index]

    model, P, Bf = _seg_model(True)
    opt = SegmentationOptions().parse(["--mode", "inference", "--height", str(H), "--width", str(W), "--batch_size", str(BS),
                                       "--save_test_visualisations", "--num_workers", "2"])
    dataset = MemoryKITTI("", names, H, W)
    tester = Tester(opt, model=model, dataset=dataset, save_path=str(tmp_path), slots=2)
    tester.test()

    # the reference's input: Pillow's LANCZOS resize and ToTensor on the host
    resized = np.stack([np.asarray(Image.fromarray(f).resize((W, H), Image.LANCZOS)) for f in frames])
    image = torch.from_numpy(resized).permute(0, 3, 1, 2).contiguous().float().div(255)
    oracle = torch.sigmoid(R.segmentor(image, P, OrderedDict((k, v.clone()) for k, v in Bf.items()), False, True)[3]).numpy()
    assert model.inference_scales is None                      # the Tester hands the caller's model back as it was
    model.eval()
    lut = ops.vis_colour_table()
    for k in range(0, 7, BS):                                  # the plain all-heads call, in the Tester's batches
        with torch.no_grad():
            x = image[k:k + BS].cuda()
            half, p32, _ = ops.seg_pack(model(x)[3], want_f32=True)
        half, p32 = half.cpu().numpy(), p32.cpu().numpy()
        for j in range(half.shape[0]):
            seq, frame, side = dataset._parse_index(k + j)
            path = os.path.join(str(tmp_path), seq, side, "data", "%010d.npy" % int(frame))
            assert os.path.exists(path)
            got = np.load(path)
            assert got.dtype == np.float16 and got.shape == (1, H, W) and np.load(path)[0].shape == (H, W)
            assert np.array_equal(got.view(np.uint16), half[j].view(np.uint16))
            # 1e-5 of the oracle's sigmoid, the bound of test_segmentation_inference_dropin, holds for the float32 sigmoid the file
            # was rounded from; the file itself is float16 (half an ulp is 2.4e-4 below 1), so for it the same bound reads: it is the
            # float16 rounding of SOME value within 1e-5 of the oracle -- rounding is monotonic, so that is an interval of halves
            assert np.abs(p32[j] - oracle[k + j]).max() <= 1e-5 and np.array_equal(got, SR.to_half(p32[j]))
            lo, hi = (oracle[k + j] - np.float32(1e-5)).astype(np.float16), (oracle[k + j] + np.float32(1e-5)).astype(np.float16)
            assert ((got >= lo) & (got <= hi)).all()
            jpg = os.path.join(str(tmp_path), seq, side, "visualisations", "%010d.jpg" % int(frame))
            with Image.open(jpg) as im:
                assert im.size == (2 * W, H) and im.mode == "RGB"
    # test_batch alone: the same bytes as the files of the first batch, and the picture the restatement draws from them
    half, pics = tester.test_batch(frames[:BS])
    with torch.no_grad():
        _, p32, _ = ops.seg_pack(model(image[:BS].cuda())[3], want_f32=True)
    assert half.dtype == np.float16 and half.shape == (BS, 1, H, W) and pics.shape == (BS, H, 2 * W, 3)
    assert np.array_equal(pics, SR.picture(p32.cpu().numpy(), image[:BS].numpy(), lut))
    for j in range(BS):
        seq, frame, side = dataset._parse_index(j)
        assert np.array_equal(half[j], np.load(os.path.join(str(tmp_path), seq, side, "data", "%010d.npy" % int(frame))))
