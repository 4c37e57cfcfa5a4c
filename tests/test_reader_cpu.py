"""CPU: the restatement of the reader operations (tests/reader_restatement.py) against the installed Pillow byte for byte, against
scipy.ndimage.label + the reference's loop, and against the fixture g14_reader (the real Pillow and the reference class's own
filter_depth_mask); and the library's host coefficient tables against the restatement's.  No GPU."""
import numpy as np
import pytest
from PIL import Image

from tests import reader_restatement as RR
from tests.golden import digest, reader_inputs as RI

# the nine cases of the issue plus the mode-"L" one: (h, w) -> (H, W)
PIL_CASES = [((375, 1242), (192, 640)), ((370, 1224), (192, 640)), ((1024, 1280), (512, 640)), ((480, 640), (256, 448)), ((37, 53), (16, 24)),
             ((16, 24), (37, 53)), ((7, 5), (3, 2)), ((192, 1242), (192, 640)), ((375, 640), (192, 640))]


def _pil(img, H, W, filt):
    return np.asarray(Image.fromarray(img).resize((W, H), filt))


@pytest.mark.parametrize("src,dst", PIL_CASES)
def test_restatement_equals_pillow_lanczos(src, dst):
    img = RI.image(src[0], src[1], 3, 3)
    assert np.array_equal(RR.resize(img, dst[0], dst[1]), _pil(img, dst[0], dst[1], RR.LANCZOS))


@pytest.mark.parametrize("fname", sorted(RR.FILTERS))
def test_restatement_equals_pillow_small_cases_every_filter(fname):
    filt = RR.FILTERS[fname]
    for src, dst in PIL_CASES[4:7]:
        img = RI.image(src[0], src[1], 3, 4)
        assert np.array_equal(RR.resize(img, dst[0], dst[1], filt), _pil(img, dst[0], dst[1], filt)), (fname, src, dst)
    grey = RI.image(37, 53, 1, 5)[:, :, 0]                       # mode "L"
    assert np.array_equal(RR.resize(grey, 16, 24, filt), _pil(grey, 16, 24, filt))


@pytest.mark.parametrize("fname", sorted(RR.FILTERS))
def test_restatement_equals_pillow_1d_sweep(fname):
    filt = RR.FILTERS[fname]
    sizes = [1, 2, 3, 5, 8, 13, 16, 23, 37, 64, 100, 191, 192, 193, 255, 256, 257, 375, 448, 512, 639, 640, 641, 777, 1024, 1242, 1300]
    for n_in in sizes:
        row = RI.image(1, n_in, 1, n_in)[:, :, 0]                 # [1, in]: Pillow's size is (in, 1)
        for n_out in (2, 16, 192, 256, 448, 512, 640):
            assert np.array_equal(RR.resize(row, 1, n_out, filt), _pil(row, 1, n_out, filt)), (fname, n_in, n_out)
            if n_in in (1, 37, 640, 1300):                        # and the same sizes down the other axis
                assert np.array_equal(RR.resize(row.T.copy(), n_out, 1, filt), _pil(row.T.copy(), n_out, 1, filt)), (fname, n_in, n_out)


def test_library_host_tables_equal_the_restatement():
    from footprints_amd import _lib, ops
    lib = _lib.load()
    pairs = [(1242, 640), (375, 192), (1224, 640), (53, 24), (24, 53), (5, 2), (7, 3), (1, 16), (1300, 2), (640, 641), (3, 640)]
    for fname, filt in RR.FILTERS.items():
        for n_in, n_out in pairs:
            bounds, kk = ops.resize_tables(n_in, n_out, fname)
            rb, rk = RR.coeffs(n_in, n_out, filt)
            assert lib.fp_resize_ksize(n_in, n_out, filt) == RR.ksize(n_in, n_out, filt) == kk.shape[1]
            assert bounds.dtype == np.int32 and kk.dtype == np.int32
            assert np.array_equal(bounds, rb) and np.array_equal(kk, rk), (fname, n_in, n_out)
    assert ops.resize_tables(53, 24, "lanczos")[1] is ops.resize_tables(53, 24, RR.LANCZOS)[1]          # cached per (in, out, filter)
    assert lib.fp_resize_ksize(0, 4, RR.LANCZOS) == -1 and lib.fp_resize_ksize(4, 4, 0) == -1
    with pytest.raises(ValueError):
        ops.resize_tables(4, 4, "nearest")


def test_half_image_exercises_the_clip_on_both_sides():
    name, (h, w), (H, W), c = RI.HALF_CASE
    img = RR.half_image(h, w, c)
    lo, hi = RR.pre_clip_range(img, H, W)
    assert lo < 0 and hi > 255, (lo, hi)
    assert np.array_equal(RR.resize(img, H, W), _pil(img, H, W, RR.LANCZOS))


def test_resize_fixture_equals_restatement():
    g = digest.load("g14_reader")
    for seed, (name, (h, w), (H, W), c) in enumerate(RI.SMALL_CASES):
        img = RI.image(h, w, c, seed)
        assert np.array_equal(g["rs.%s.in" % name], img)
        assert np.array_equal(g["rs.%s.out" % name], RR.resize(img, H, W)), name
    name, (h, w), (H, W), c = RI.SMALL_CASES[0]
    for fname, filt in RR.FILTERS.items():
        assert np.array_equal(g["rs.%s.%s.out" % (name, fname)], RR.resize(RI.image(h, w, c, 0), H, W, filt)), fname
    name, (h, w), (H, W), c = RI.HALF_CASE
    assert np.array_equal(g["rs.%s.out" % name], RR.resize(RR.half_image(h, w, c), H, W))
    for seed, (name, (h, w), (H, W), c) in enumerate(RI.SKIP_CASES):
        assert fixture_digest_equal(g, "rs.%s.out" % name, RR.resize(RI.image(h, w, c, 20 + seed), H, W))
    H, W = RI.KITTI_TARGET
    batch = np.stack([RR.resize(RI.image(h, w, 3, 30 + i), H, W) for i, (h, w) in enumerate(RI.KITTI_SIZES)])
    assert fixture_digest_equal(g, "rs.kitti.out", batch)


def fixture_digest_equal(g, name, arr):
    """exact comparison with a digest entry of the fixture (shape, strided sample, sum, sum of magnitudes)"""
    import torch
    d = digest.digest(name, torch.from_numpy(np.ascontiguousarray(arr)), full_limit=1 << 10)
    return all(np.array_equal(g[k], v) for k, v in d.items()) and len(d) == 4


def test_filter_restatement_equals_scipy_label_and_reference_loop():
    ndimage = pytest.importorskip("scipy.ndimage")
    for H, W in RI.MASK_SIZES + [(64, 96)]:
        cases = dict(RR.mask_cases(H, W))
        for d in (5, 10, 20, 30, 45, 60):
            cases["random%d" % d] = RI.random_mask(H, W, d, 100 + d)
        for name, m in cases.items():
            connected = ndimage.label(m, structure=np.ones((3, 3)))[0]
            processed = np.zeros_like(m)
            for index in range(1, connected.max() + 1):           # footprint_dataset.py:100-103
                size = (connected == index).sum()
                if size < W * H / 100:
                    processed[connected == index] = 1
            assert np.array_equal(RR.filter_depth_mask(m), processed), (H, W, name)
            assert RR.components(m).max() == connected.max()


def test_filter_fixture_equals_restatement():
    g = digest.load("g14_reader")
    seen = 0
    for H, W in RI.MASK_SIZES:
        cases = dict(RR.mask_cases(H, W))
        for d in (10, 30, 55):
            cases["random%d" % d] = RI.random_mask(H, W, d, d)
        for name, m in cases.items():
            ref = np.unpackbits(g["dm.%dx%d.%s" % (H, W, name)])[:H * W].reshape(H, W)
            assert np.array_equal(RR.filter_depth_mask(m), ref.astype(m.dtype)), (H, W, name)
            seen += 1
    assert seen >= 20
    H, W = RI.KITTI_TARGET
    for name, m in RI.kitti_masks().items():
        ref = np.unpackbits(g["dm.%dx%d.%s" % (H, W, name)])[:H * W].reshape(H, W)
        got = RR.filter_depth_mask(m)
        assert np.array_equal(got, ref.astype(got.dtype)), name
        assert (got.sum() == m.sum()) == (name == "random10") and got.sum() > 0       # only the block case loses a component


def test_size_threshold_cases_are_what_they_claim():
    m = RR.mask_cases(20, 30)["sizes_5_6_7"]
    sizes = sorted(np.bincount(RR.components(m).reshape(-1))[1:])
    assert sizes == [5, 5, 6, 7] and 20 * 30 / 100 == 6.0
    kept = RR.filter_depth_mask(m)
    assert kept.sum() == 10                                       # the two components of 5; 6 and 7 are not < 6.0
    assert RR.filter_depth_mask(RR.mask_cases(24, 36)["sizes_5_6_7"]).sum() == 5 + 5 + 6 + 7          # limit 8.64
    for H, W in RI.MASK_SIZES:
        c = RR.mask_cases(H, W)
        assert RR.components(c["checkerboard"]).max() == 1 and RR.components(c["serpentine"]).max() == 1
        assert RR.components(c["diagonal"]).max() == 2
    c = RR.mask_cases(24, 36)
    assert RR.components(c["diagonal_tile_corner"]).max() == 1 and RR.components(c["antidiagonal_tile_corner"]).max() == 1
