"""GPU: the reader kernels -- Pillow's 8-bit resize (csrc/resample_u8.hip) and the depth-mask filter (csrc/reader.hip) -- bit for bit against the restatement
(tests/reader_restatement.py, pinned to the installed Pillow and to scipy + the reference's loop by tests/test_reader_cpu.py) and against
the fixture g14_reader (the real Pillow's and the reference class's outputs); then the assembler and predict_simple options built on them.
Needs neither Pillow nor scipy nor the reference.  No tolerance anywhere: every comparison is np.array_equal."""
import functools
import random

import numpy as np
import pytest
import torch

from tests import reader_restatement as RR
from tests.golden import digest, reader_inputs as RI

pytestmark = pytest.mark.gpu


@functools.lru_cache(None)
def gold():
    return digest.load("g14_reader")


@functools.lru_cache(None)
def kitti_batch():
    """the mixed-size KITTI frames and their restated resize, computed once"""
    H, W = RI.KITTI_TARGET
    frames = [RI.image(h, w, 3, 30 + i) for i, (h, w) in enumerate(RI.KITTI_SIZES)]
    ref = np.stack([RR.resize(f, H, W) for f in frames])
    ref.setflags(write=False)
    return frames, ref


def gpu_resize(images, H, W, filt="lanczos"):
    from footprints_amd import ops
    out = ops.resize_u8(images, H, W, filt)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def digest_equal(g, name, arr):
    d = digest.digest(name, torch.from_numpy(np.ascontiguousarray(arr)), full_limit=1 << 10)
    return len(d) == 4 and all(np.array_equal(g[k], v) for k, v in d.items())


@pytest.mark.parametrize("case", RI.SMALL_CASES, ids=[c[0] for c in RI.SMALL_CASES])
def test_resize_small_cases_equal_restatement_and_pillow_fixture(case):
    name, (h, w), (H, W), c = case                    # down (ksize 15), mode "L", up, tiny (window clamped at both borders), ragged 17 x 23
    img = RI.image(h, w, c, [k[0] for k in RI.SMALL_CASES].index(name))
    got = gpu_resize([img], H, W)
    assert got.shape == (1, H, W, c) and got.dtype == np.uint8
    assert np.array_equal(got[0], RR.resize(img, H, W))
    assert np.array_equal(got[0], gold()["rs.%s.out" % name])
    if c == 1:                                        # [h, w] is accepted like [h, w, 1]
        assert np.array_equal(gpu_resize([img[:, :, 0]], H, W)[0], got[0])


def test_tiny_case_window_is_wider_than_the_input():
    bounds, kk = RR.coeffs(5, 2)
    assert kk.shape[1] > 5 and (bounds[:, 0] == 0).all() and (bounds[:, 1] == 5).all()


@pytest.mark.parametrize("case", RI.SKIP_CASES, ids=[c[0] for c in RI.SKIP_CASES])
def test_resize_with_one_pass_skipped(case):
    name, (h, w), (H, W), c = case
    img = RI.image(h, w, c, 20 + [k[0] for k in RI.SKIP_CASES].index(name))
    got = gpu_resize([img], H, W)[0]
    assert np.array_equal(got, RR.resize(img, H, W))
    assert digest_equal(gold(), "rs.%s.out" % name, got)


def test_resize_same_size_is_a_copy():
    img = RI.image(16, 24, 3, 9)
    assert np.array_equal(gpu_resize([img], 16, 24)[0], img)


def test_resize_half_image_clips_on_both_sides():
    name, (h, w), (H, W), c = RI.HALF_CASE
    img = RR.half_image(h, w, c)
    lo, hi = RR.pre_clip_range(img, H, W)
    assert lo < 0 and hi > 255
    got = gpu_resize([img], H, W)[0]
    assert np.array_equal(got, RR.resize(img, H, W)) and np.array_equal(got, gold()["rs.%s.out" % name])
    assert got.min() == 0 and got.max() == 255


@pytest.mark.parametrize("fname", sorted(RR.FILTERS))
def test_resize_every_filter(fname):
    name, (h, w), (H, W), c = RI.SMALL_CASES[0]
    img = RI.image(h, w, c, 0)
    got = gpu_resize([img], H, W, fname)[0]
    assert np.array_equal(got, RR.resize(img, H, W, RR.FILTERS[fname]))
    assert np.array_equal(got, gold()["rs.%s.%s.out" % (name, fname)])


def test_resize_mixed_kitti_sizes_in_one_call(monkeypatch):
    from footprints_amd import ops
    frames, ref = kitti_batch()
    H, W = RI.KITTI_TARGET
    calls = []
    packed_call = ops.resize_u8_packed                # the one place that calls fp_resize_u8: once per packed batch

    def counting(src, src_bytes, samples, B, *a, **kw):
        calls.append(B)
        return packed_call(src, src_bytes, samples, B, *a, **kw)
    monkeypatch.setattr(ops, "resize_u8_packed", counting)
    got = gpu_resize(frames, H, W)
    assert calls == [len(frames)]
    assert np.array_equal(got, ref)
    assert digest_equal(gold(), "rs.kitti.out", got)


def test_resize_ragged_batch_mixed_passes():
    """output sizes that are no multiple of the vertical tile (8 rows) or the 1024-byte strip, unaligned sample offsets, and in one
    batch: both passes, horizontal only, vertical only, neither"""
    H, W = 17, 23
    shapes = [(37, 53), (17, 53), (37, 23), (17, 23), (5, 7), (41, 23)]
    imgs = [RI.image(h, w, 3, 40 + i) for i, (h, w) in enumerate(shapes)]
    got = gpu_resize(imgs, H, W)
    for i, im in enumerate(imgs):
        assert np.array_equal(got[i], RR.resize(im, H, W)), shapes[i]
    wide = [RI.image(9, 700, 1, 50), RI.image(12, 350, 1, 51)]          # two strips of the vertical pass, the second one partial: 345 * 3 bytes
    got = gpu_resize([np.repeat(w, 3, axis=2) for w in wide], 11, 345)
    for i, im in enumerate(wide):
        assert np.array_equal(got[i], np.repeat(RR.resize(im, 11, 345), 3, axis=2))


def test_resize_rejects_what_it_cannot_do():
    from footprints_amd import ops
    with pytest.raises(ValueError):
        ops.resize_u8([np.zeros((4, 4, 2), np.uint8)], 2, 2)
    with pytest.raises(ValueError):
        ops.resize_u8([np.zeros((4, 4, 3), np.float32)], 2, 2)
    with pytest.raises(ValueError):
        ops.resize_u8([np.zeros((4, 4, 3), np.uint8)], 2, 2, "nearest")


def test_resize_reports_a_record_it_turned_down():
    """a record that points past the source buffer, or names a table of other sizes, is not followed: its sample stays unwritten, the
    other one is resized, and check=True raises"""
    from footprints_amd import _lib, ops
    H, W = 16, 24
    imgs = [RI.image(37, 53, 3, 60), RI.image(37, 53, 3, 61)]
    tables = ops.resize_table_set("cuda")
    packed, records, total, Cn, max_h, max_w = ops.resize_pack(imgs, H, W, tables)
    other = tables.index(50, W)                                        # a (50 -> 24) table: does not fit w = 53
    src = torch.from_numpy(packed).cuda()
    ref = np.stack([RR.resize(im, H, W) for im in imgs])

    def run(change):
        rec = (_lib.ResizeSample * 2).from_buffer_copy(records.tobytes())
        change(rec[1])
        d_rec = torch.from_numpy(np.frombuffer(bytes(rec), dtype=np.uint8).copy()).cuda()
        out = torch.full((2, H, W, 3), 7, dtype=torch.uint8, device="cuda")
        try:
            ops.resize_u8_packed(src, total, d_rec, 2, H, W, 3, max_h, max_w, tables, out=out, check=True)
            raised = False
        except ValueError:
            raised = True
        return raised, out.cpu().numpy()
    raised, out = run(lambda r: None)
    assert not raised and np.array_equal(out, ref)
    for change in (lambda r: setattr(r, "offset", total - 8), lambda r: setattr(r, "table_h", other), lambda r: setattr(r, "table_v", 1 << 20),
                   lambda r: setattr(r, "h", max_h + 1)):
        raised, out = run(change)
        assert raised and np.array_equal(out[0], ref[0]) and (out[1] == 7).all()
    raised, out = run(lambda r: None)                                  # the status word is cleared by the next call
    assert not raised and np.array_equal(out, ref)


# ---- depth-mask filter ---------------------------------------------------------------------------------------------------------------------
def gpu_filter(masks, dtype=np.float64, in_place=False):
    from footprints_amd import ops
    m = torch.from_numpy(np.ascontiguousarray(masks, dtype=dtype)).cuda()
    out = ops.filter_depth_mask(m, out=m if in_place else None)
    torch.cuda.synchronize()
    assert out.dtype == m.dtype and out.shape == m.shape
    return out.cpu().numpy()


@pytest.mark.parametrize("H,W", RI.MASK_SIZES)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_filter_cases_equal_restatement_and_reference_fixture(H, W, dtype):
    cases = dict(RR.mask_cases(H, W))                 # empty, full, checkerboard, diagonal touches (also across the 32 x 8 tile corner),
    for d in (10, 30, 55):                            # serpentine, sizes 5 / 6 / 7, every border; plus random densities
        cases["random%d" % d] = RI.random_mask(H, W, d, d)
    if W > RR.TILE_W:
        assert "diagonal_tile_corner" in cases
    for name, m in cases.items():
        got = gpu_filter(m[None], dtype)[0]
        assert np.array_equal(got, RR.filter_depth_mask(m).astype(dtype)), name
        ref = np.unpackbits(gold()["dm.%dx%d.%s" % (H, W, name)])[:H * W].reshape(H, W)
        assert np.array_equal(got, ref.astype(dtype)), name
    k = gpu_filter(cases["sizes_5_6_7"][None], dtype)[0]
    assert k.sum() == (10 if (H, W) == (20, 30) else 23)              # limit 6.0: the 5s stay, 6 and 7 go; limit 8.64: all stay


def test_filter_batch_keeps_images_apart_and_repeats_exactly():
    H, W = 24, 36
    c = RR.mask_cases(H, W)
    masks = np.stack([c["serpentine"], c["sizes_5_6_7"], RI.random_mask(H, W, 30, 3)])
    ref = np.stack([RR.filter_depth_mask(m) for m in masks])
    a = gpu_filter(masks)
    b = gpu_filter(masks)
    assert np.array_equal(a, ref) and a.tobytes() == b.tobytes()
    assert np.array_equal(gpu_filter(masks, in_place=True), ref)
    assert np.array_equal(gpu_filter(masks[::-1].copy()), ref[::-1])
    assert np.array_equal(gpu_filter(masks[1]), ref[1])              # [H, W] without a batch axis


def test_filter_tile_corner_touch_at_a_size_with_many_tiles():
    """two arms of 14 pixels that touch only diagonally, across a corner shared by four 32 x 8 tiles: each alone is below the limit of
    24 pixels and would stay, together they are 28 and go -- a missed merge shows"""
    H, W = 24, 100
    for y, x in ((8, 32), (16, 64), (16, 32)):
        for anti in (False, True):
            m = np.zeros((H, W))
            if anti:
                m[y - 1, x:x + 14] = 1
                m[y, x - 14:x] = 1
            else:
                m[y - 1, x - 14:x] = 1
                m[y, x:x + 14] = 1
            m[2, 2:16] = 1                                             # an arm of 14 on its own stays
            ref = RR.filter_depth_mask(m)
            assert ref.sum() == 14
            assert np.array_equal(gpu_filter(m[None])[0], ref), (y, x, anti)


def test_filter_kitti_size_masks():
    H, W = RI.KITTI_TARGET
    masks = RI.kitti_masks()
    names = sorted(masks)
    got = gpu_filter(np.stack([masks[n] for n in names]), np.float32)
    for i, n in enumerate(names):
        ref = np.unpackbits(gold()["dm.%dx%d.%s" % (H, W, n)])[:H * W].reshape(H, W)
        assert np.array_equal(got[i], ref.astype(np.float32)), n
    assert got[names.index("random10")].sum() == masks["random10"].sum()
    assert 0 < got[names.index("random10_block")].sum() < masks["random10_block"].sum() - 1600


# ---- assembler, predict_simple, inference --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W,raw_hw", [(3, 192, 640, RI.KITTI_SIZES), (2, 16, 24, [(37, 53), (41, 50), (16, 61)])])
def test_assembler_raw_images_and_mask_filter_equal_the_host_fed_path(B, H, W, raw_hw):
    from footprints_amd.datasets import DeviceBatchAssembler, SyntheticSampleSource, draw_augmentation
    src = SyntheticSampleSource(B, H, W, steps=2, seed=21, pool=2 * B, raw_hw=raw_hw)
    assert sorted({s[0].shape[:2] for s in src.pool}) == sorted(set(map(tuple, raw_hw)))
    for j, (img, maps) in enumerate(src.pool):                        # depth masks with components on both sides of the limit
        maps["depth_mask"] = RI.random_mask(H, W, 10 + 25 * (j % 2), j)
        if H >= 100:
            maps["depth_mask"][20:60, 100 + 10 * j:140 + 10 * j] = 1
    max_hw = (max(h for h, _ in raw_hw), max(w for _, w in raw_hw))
    dev = DeviceBatchAssembler(B, H, W, dataset="kitti", raw_images=True, max_src_hw=max_hw, filter_depth_mask=True)
    host = DeviceBatchAssembler(B, H, W, dataset="kitti")
    rng = random.Random(4)
    dropped = 0
    for samples in src:
        params = [draw_augmentation(True, rng) for _ in samples]
        fed = []
        for img, maps in samples:
            m = dict(maps)
            m["depth_mask"] = RR.filter_depth_mask(maps["depth_mask"])
            dropped += int(maps["depth_mask"].sum() - m["depth_mask"].sum())
            fed.append((RR.resize(img, H, W), m))
        a = dev.collect(dev.submit(samples, params))
        b = host.collect(host.submit(fed, params))
        torch.cuda.synchronize()
        assert set(a) == set(b)
        for k in a:
            assert torch.equal(a[k], b[k]), k
    assert dropped > 0
    with pytest.raises(ValueError):
        DeviceBatchAssembler(B, H, W, raw_images=True)


def test_predict_simple_device_resize_gives_the_same_input_tensor():
    from footprints_amd import predict_simple
    frames, ref = kitti_batch()
    H, W = RI.KITTI_TARGET
    x = predict_simple.preprocess(frames[0], (H, W), device_resize=True)
    assert x.is_cuda and x.dtype == torch.float32 and tuple(x.shape) == (1, 3, H, W)
    host = torch.from_numpy(ref[0].astype(np.float32) / 255.0).permute(2, 0, 1)[None].contiguous()       # preprocess() after the resize
    assert torch.equal(x.cpu(), host)
    from PIL import Image                             # predict_simple's own dependency
    assert torch.equal(x.cpu(), predict_simple.preprocess(Image.fromarray(frames[0]), (H, W)))
    assert torch.equal(predict_simple.preprocess(Image.fromarray(frames[0]), (H, W), device_resize=True).cpu(), x.cpu())


def test_inference_manager_device_resize_gives_the_same_input_tensor():
    from footprints_amd.evaluation.inference import InferenceManager
    frames, ref = kitti_batch()
    H, W = RI.KITTI_TARGET
    man = object.__new__(InferenceManager)                            # only the input path: no network needed
    man.device_resize, man.height_width = True, (H, W)
    x = man.input_tensor({"raw_image": frames})
    host = torch.from_numpy(ref.astype(np.float32) / 255.0).permute(0, 3, 1, 2).contiguous()
    assert torch.equal(x.cpu(), host)
    man.device_resize = False
    assert torch.equal(man.input_tensor({"image": host}).cpu(), host)
