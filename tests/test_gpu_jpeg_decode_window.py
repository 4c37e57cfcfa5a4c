"""GPU: fp_jpeg_decode_window (csrc/jpeg_decode.hip) -- one rectangle per sample, byte for byte the crop of Pillow's picture and the crop of
fp_jpeg_decode's: the rectangles that stress the blocks it chooses (MCU boundaries, the chroma neighbour in an MCU the window does not touch,
the picture's edge clamps), one call that mixes samplings and window sizes over a sentinel-filled output, per-sample refusals, the launch
budget's status, and the waiting convenience form."""
import ctypes as C
import functools
import io

import numpy as np
import pytest
import torch

from tests.golden import make_golden_jpeg_decode as G

pytestmark = pytest.mark.gpu

SIZES = ((8, 8), (16, 16), (33, 45), (70, 150))                 # (h, w); 16 x 16 is exactly one 4:2:0 MCU, 33 x 45 is odd both ways
SAMPLINGS = (0, 1, 2, "grey")                                   # Pillow's subsampling: 4:4:4, 4:2:2, 4:2:0; grey
SENTINEL = 0xA7


@functools.lru_cache(None)
def picture_file(size, sampling):
    h, w = size
    a = G.photo(h, w, 1000 + 7 * h + w)
    if sampling == "grey":
        return G.write(a[:, :, 1].copy(), 90)
    return G.write(a, 90, sampling)


@functools.lru_cache(None)
def noise_frame():
    """tests/test_gpu_jpeg_decode.py's: noise at quality 100 does not resynchronise, so a small launch budget does not settle it"""
    rng = np.random.default_rng(96128)
    return G.write(rng.integers(0, 256, (96, 128, 3), dtype=np.uint8), 100)


def rectangles(h, w):
    """(y0, x0, rh, rw) of the issue's list for a picture of h x w, without repeats"""
    odd = lambda n: max(1, n - (1 - n % 2))
    base = 16 if min(h, w) >= 32 else 0                         # an MCU boundary of every sampling (4:2:0's MCU is 16 x 16)
    span = 16 if min(h, w) >= 16 else 8
    rects = [(0, 0, h, w),                                      # the whole picture
             (0, 0, 1, 1), (0, w - 1, 1, 1), (h - 1, 0, 1, 1), (h - 1, w - 1, 1, 1),        # the corners
             (3, 5, odd(min(h - 3, 11)), odd(min(w - 5, 21))),  # odd origin, odd size
             (base, base, span, span),                          # from one MCU boundary to the next
             (base + 1, base + 1, span - 2, span - 2),          # one pixel inside both: the chroma neighbours lie in the MCUs around
             (h - 1, 0, 1, w), (0, w - 1, h, 1),                # the last row and the last column: the picture's edge clamps
             (h // 2, 0, 1, w), (0, w // 2, h, 1)]              # a full-width row and a full-height column inside
    assert all(rh >= 1 and rw >= 1 and y0 >= 0 and x0 >= 0 and y0 + rh <= h and x0 + rw <= w for y0, x0, rh, rw in rects), (h, w)
    return list(dict.fromkeys(rects))


def _rounds(files):
    """the launch budget that settles any content (tests/test_gpu_jpeg_decode.py::_decode_all)"""
    from footprints_amd import ops
    return max(-(-(-(-ops.jpeg_parse(f)["scan_bytes"] * 8 // ops.JPEG_DECODE_SUBSEQ_BITS)) // 64) for f in files) + 1


def _crop(a, r):
    y0, x0, rh, rw = r
    return a[y0:y0 + rh, x0:x0 + rw]


def _call(files, rects, gap=0, max_rounds=None):
    """jpeg_decode_window_packed into a sentinel-filled buffer with `gap` bytes in front of every window and behind the last ->
    (status list [B + 1], the buffer as numpy, offsets)"""
    from footprints_amd import ops
    offsets, at = [], 0
    for _, _, rh, rw in rects:
        at += gap
        offsets.append(at)
        at += max(rh, 0) * max(rw, 0) * 3
    at += gap
    pack = ops.jpeg_decode_pack(files)
    out = torch.full((at,), SENTINEL, dtype=torch.uint8, device="cuda")
    got, windows, status = ops.jpeg_decode_window_packed(pack, rects, out=out, out_offsets=offsets,
                                                         max_rounds=_rounds(files) if max_rounds is None else max_rounds)
    assert got is out and windows == [(r[2], r[3]) for r in rects]
    return status.cpu().tolist(), out.cpu().numpy(), offsets


def _expected(want, rects, offsets, total, bad=()):
    """the buffer a correct call leaves: sentinels, and the crop of every sample not in `bad` at its offset"""
    buf = np.full(total, SENTINEL, np.uint8)
    for n, (a, r, off) in enumerate(zip(want, rects, offsets)):
        if n not in bad:
            c = _crop(a, r)
            buf[off:off + c.size] = c.reshape(-1)
    return buf


def test_the_record_and_the_binding():
    from footprints_amd import _lib
    assert C.sizeof(_lib.JpegDecodeWindowSample) == _lib.load().fp_jpeg_decode_window_sample_bytes() == 64
    assert _lib.JpegDecodeWindowSample.y0.offset == C.sizeof(_lib.JpegDecodeSample) == 48


def test_every_rectangle_is_pillows_crop_and_the_whole_frame_decoders_crop():
    from footprints_amd import ops
    pictures = [picture_file(size, s) for size in SIZES for s in SAMPLINGS]
    assert sorted({(ops.jpeg_parse(f)["ncomp"], ops.jpeg_parse(f)["hs"], ops.jpeg_parse(f)["vs"]) for f in pictures}) == [
        (1, 1, 1), (3, 1, 1), (3, 2, 1), (3, 2, 2)]
    pillow = [G.pillow_decode(f) for f in pictures]
    whole, shapes, status = ops.jpeg_decode_packed(ops.jpeg_decode_pack(pictures), max_rounds=_rounds(pictures))
    assert status.cpu().tolist() == [0] * (len(pictures) + 1)
    whole, frames, at = whole.cpu().numpy(), [], 0
    for (h, w), p in zip(shapes, pillow):
        frames.append(whole[at:at + h * w * 3].reshape(h, w, 3))
        at += h * w * 3
        assert np.array_equal(frames[-1], p)
    files, rects, want, device = [], [], [], []
    for f, p, d in zip(pictures, pillow, frames):
        for r in rectangles(*p.shape[:2]):
            files.append(f), rects.append(r), want.append(p), device.append(d)
    status, out, offsets = _call(files, rects, gap=16)
    assert status == [0] * (len(files) + 1)
    for n, (r, off) in enumerate(zip(rects, offsets)):
        got = out[off:off + r[2] * r[3] * 3].reshape(r[2], r[3], 3)
        assert np.array_equal(got, _crop(want[n], r)), (n, want[n].shape, r)
        assert np.array_equal(got, _crop(device[n], r)), (n, want[n].shape, r)
    assert np.array_equal(out, _expected(want, rects, offsets, out.size))         # and not a byte outside the windows


def test_one_call_mixes_samplings_and_window_sizes_and_writes_nothing_outside_a_window():
    files = [picture_file((70, 150), 2), picture_file((33, 45), 0), picture_file((70, 150), 1), picture_file((16, 16), "grey"),
             picture_file((33, 45), 2), picture_file((8, 8), 1)]
    # max_win_h is the first sample's and max_win_w the third's: every other sample leaves most of both grids idle
    rects = [(1, 140, 69, 3), (30, 40, 1, 1), (65, 0, 2, 150), (5, 3, 9, 11), (17, 17, 14, 14), (0, 0, 8, 8)]
    want = [G.pillow_decode(f) for f in files]
    status, out, offsets = _call(files, rects, gap=64)
    assert status == [0] * 7
    assert np.array_equal(out, _expected(want, rects, offsets, out.size))


def test_a_bad_rectangle_is_refused_per_sample():
    files = [picture_file((33, 45), 2), picture_file((70, 150), 1), picture_file((33, 45), 0), picture_file((16, 16), 2)]
    want = [G.pillow_decode(f) for f in files]
    good = [(10, 10, 20, 30), (0, 0, 70, 150), (32, 44, 1, 1), (0, 0, 16, 16)]
    for bad, rect in ((2, (30, 40, 4, 5)), (2, (0, 40, 5, 6)), (0, (10, 10, 0, 30)), (0, (10, 10, 20, 0)), (3, (-1, 0, 4, 4)), (1, (69, 0, 2, 150)),
                      (3, (0, 0, 17, 16))):
        rects = list(good)
        rects[bad] = rect
        status, out, offsets = _call(files, rects, gap=32)
        assert [s != 0 for s in status[:4]] == [n == bad for n in range(4)] and status[4] == status[bad] == 1, (rect, status)
        assert np.array_equal(out, _expected(want, rects, offsets, out.size, bad=(bad,))), rect


def test_a_sample_that_does_not_settle_reports_what_fp_jpeg_decode_reports():
    from footprints_amd import ops
    # the neighbours are one workgroup of subsequences each: settled by the first launch, found settled by the second
    files = [picture_file((16, 16), 2), noise_frame(), picture_file((16, 16), 0)]
    assert all(-(-ops.jpeg_parse(f)["scan_bytes"] * 8 // ops.JPEG_DECODE_SUBSEQ_BITS) <= 64 for f in (files[0], files[2]))
    want = [G.pillow_decode(f) for f in files]
    rects = [(3, 5, 11, 11), (10, 20, 50, 60), (1, 1, 14, 14)]
    pack = ops.jpeg_decode_pack(files)
    _, _, whole = ops.jpeg_decode_packed(pack, max_rounds=2)
    whole = whole.cpu().tolist()
    assert whole == [0, 2, 0, 2]
    status, out, offsets = _call(files, rects, gap=32, max_rounds=2)
    assert status == whole
    assert np.array_equal(out, _expected(want, rects, offsets, out.size, bad=(1,)))
    status, out, offsets = _call(files, rects, gap=32)                 # with the budget that settles anything, the noise decodes too
    assert status == [0] * 4 and np.array_equal(out, _expected(want, rects, offsets, out.size))


def test_the_waiting_form_returns_pillows_crops_whatever_the_file():
    from PIL import Image
    from footprints_amd import ops
    buf = io.BytesIO()
    Image.fromarray(G.photo(40, 56, 7)).save(buf, format="JPEG", progressive=True)
    files = [picture_file((70, 150), 2), buf.getvalue(), noise_frame(), picture_file((33, 45), "grey"), picture_file((33, 45), 1)]
    rects = [(17, 33, 40, 100), (5, 7, 30, 41), (1, 1, 94, 126), (32, 0, 1, 45), (0, 44, 33, 1)]
    arrays, statuses = ops.jpeg_decode_window(files, rects, return_status=True)
    assert statuses == [0, -1, 2, 0, 0]                                 # the parser's refusal, the default budget's, and three from the device
    for a, f, r in zip(arrays, files, rects):
        assert a.dtype == np.uint8 and np.array_equal(a, _crop(G.pillow_decode(f), r)), r
    assert all(np.array_equal(a, b) for a, b in zip(ops.jpeg_decode_window(files, rects), arrays))
    with pytest.raises(ValueError):
        ops.jpeg_decode_window(files[:1], [(0, 0, 71, 150)])
    with pytest.raises(ValueError):
        ops.jpeg_decode_window(files[1:2], [(0, 0, 40, 57)])
