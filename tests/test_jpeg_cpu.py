"""The baseline JPEG encoder without a GPU: the NumPy restatement of csrc/jpeg.hip (tests/jpeg_restatement.py) against Pillow's bytes
as recorded (tests/golden/g18_jpeg.npz) and against the installed Pillow where it is built on libjpeg-turbo; the header rule; what the
case list covers; the host side of the library and the command-line flags."""
import io

import numpy as np
import pytest

from tests import jpeg_restatement as JR
from tests.golden import make_golden_jpeg as G

GOLD = G.load()
CASES = list(G.cases())
_counters = {}


def restated(name, size, content):
    out, counters = JR.encode(G.picture(size, content), JR.parse_header(GOLD[name]))
    _counters[name] = counters
    return out


def test_fixture_holds_every_case():
    assert sorted(GOLD) == sorted(c[0] for c in CASES) and len(CASES) == len(G.SIZES) * len(G.CONTENTS) * len(G.QUALITIES) == 192


@pytest.mark.parametrize("quality", G.QUALITIES)
def test_restatement_equals_the_recorded_bytes(quality):
    for name, size, content, q in CASES:
        if q == quality:
            assert restated(name, size, content) == GOLD[name], name


def test_the_cases_cover_run_codes_stuffing_and_dummy_blocks():
    """counted by the restatement itself, so the list cannot silently stop covering them"""
    for name, size, content, _ in CASES:
        if name not in _counters:
            restated(name, size, content)
    assert any(c["zrl"] > 0 for c in _counters.values())
    assert any(c["stuffed"] > 0 for c in _counters.values())
    assert any(c["dummy_right"] > 0 and c["dummy_bottom"] > 0 for c in _counters.values())
    # and a last byte that is itself stuffed: the scan ends FF 00 before the EOI marker
    assert any(GOLD[name].endswith(b"\xff\x00\xff\xd9") for name in GOLD)


def _pillow(a, quality):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(a).save(buf, format="JPEG", quality=quality)
    return buf.getvalue()


def test_restatement_equals_the_installed_pillow():
    from PIL import features
    if not features.check_feature("libjpeg_turbo"):
        print("the installed Pillow is not built on libjpeg-turbo: the recorded bytes are the reference")
        return
    from footprints_amd import ops
    for name, size, content, quality in CASES:
        if size in ((9, 25), (37, 50), (75, 122)):
            a = G.picture(size, content)
            t = ops.jpeg_tables(quality)
            out, _ = JR.encode(a, dict(header=t.header, size_at=t.size_at, quant=t.quant, huff=t.huff))
            assert out == _pillow(a, quality), name


@pytest.mark.parametrize("quality", G.QUALITIES)
def test_patched_header_equals_pillows(quality):
    """ops.jpeg_tables parses a dummy of the installed Pillow; the header of a real picture is those bytes with four bytes patched"""
    from footprints_amd import ops
    t = ops.jpeg_tables(quality)
    assert ops.jpeg_tables(quality) is t                                          # once per quality
    for h, w in ((1, 1), (37, 50), (375, 1242), (300, 70000 % 65536)):
        ref = _pillow(np.zeros((h, w, 3), dtype=np.uint8), quality)
        parsed = JR.parse_header(ref)
        assert t.file_header(h, w) == parsed["header"] and t.size_at == parsed["size_at"]
        assert {k: list(v) for k, v in t.quant.items()} == parsed["quant"] and t.huff == parsed["huff"]
    # the code table of the library: quantisation values, then code | length << 16 per symbol
    from footprints_amd import _lib
    assert t.words.shape == (_lib.JPEG_TABLE_WORDS,) and list(t.words[:64]) == list(t.quant[0]) and list(t.words[64:128]) == list(t.quant[1])
    code, n = t.huff[0x11][0xF0]
    assert t.words[160 + 256 + 0xF0] == code | n << 16 and t.words[128 + 16 + 3] == t.huff[0x01][3][0] | t.huff[0x01][3][1] << 16


def test_host_side_of_the_library():
    import ctypes as C
    from footprints_amd import _lib, ops
    lib = _lib.load()
    assert lib.fp_jpeg_sample_bytes() == C.sizeof(_lib.JpegSample) == 16 and lib.fp_jpeg_table_words() == _lib.JPEG_TABLE_WORDS
    # the stated worst case of a block: 20 DC bits and 63 AC terms of 26 bits; doubled for stuffing in the output
    blocks = 78 * 24 * 6
    per_block = 20 + 63 * 26
    assert lib.fp_jpeg_max_scan_bytes(12, 375, 1242) == 12 * 2 * ((blocks * per_block + 7) // 8)
    assert lib.fp_jpeg_workspace_bytes(12, 375, 1242) >= 12 * (blocks * 132 + (blocks * per_block + 7) // 8)
    for bad in ((0, 8, 8), (1, 0, 8), (1, 8, 0), (1, 65536, 8), (70000, 8, 8), (1, 65535, 65535)):
        assert lib.fp_jpeg_workspace_bytes(*bad) == -1 and lib.fp_jpeg_max_scan_bytes(*bad) == -1
    rec, total, max_h, max_w = ops.jpeg_records([(2, 3), (5, 1)])
    assert total == 33 and (max_h, max_w) == (5, 3) and rec.view(np.int64)[2] == 18 and list(rec.view(np.int32)[6:8]) == [5, 1]
    assert lib.fp_jpeg_encode(None, 0, None, None, None, 0, None, 1, 8, 8, None, 0, None) == -1


def test_jpeg_files_puts_header_and_eoi_around_the_scans():
    from footprints_amd import ops
    table = np.array([[0, 3], [3, 2], [5, 0]], dtype=np.int64)
    files = ops.jpeg_files(b"abcde", table, [(4, 5), (6, 7)], 75)
    t = ops.jpeg_tables(75)
    assert files == [t.file_header(4, 5) + b"abc\xff\xd9", t.file_header(6, 7) + b"de\xff\xd9"]
    table[2, 1] = 1
    with pytest.raises(ValueError):
        ops.jpeg_files(b"abcde", table, [(4, 5), (6, 7)], 75)


def test_the_parsers_accept_device_jpeg():
    from footprints_amd import predict_simple
    from footprints_amd.preprocessing.segmentation.options import SegmentationOptions
    args = predict_simple.parse_args(["--image", "x", "--model", "kitti", "--device_vis", "--device_jpeg"])
    assert args.device_jpeg and args.device_vis
    assert not predict_simple.parse_args(["--image", "x", "--model", "kitti", "--device_vis"]).device_jpeg
    with pytest.raises(SystemExit):
        predict_simple.parse_args(["--image", "x", "--model", "kitti", "--device_jpeg"])              # not without --device_vis
    opt = SegmentationOptions().parse(["--mode", "inference", "--save_test_visualisations", "--device_jpeg"])
    assert opt.device_jpeg and not SegmentationOptions().parse(["--mode", "inference"]).device_jpeg


def test_save_result_takes_the_files_bytes(tmp_path):
    """the array path is unchanged; bytes are written as they are"""
    from footprints_amd.preprocessing.segmentation.datasets.inference import InferenceDataset
    ds = InferenceDataset("", [], 8, 8)
    pred = np.zeros((1, 8, 8), dtype=np.float16)
    pic = G.picture((8, 16), "ramp")
    ds.save_result(str(tmp_path / "a"), 7, pred, pic)
    ds.save_result(str(tmp_path / "b"), 7, pred, _pillow(pic, 95))
    ds.save_result(str(tmp_path / "c"), 7, pred)
    name = "visualisations/0000000007.jpg"
    assert (tmp_path / "a" / name).read_bytes() == (tmp_path / "b" / name).read_bytes() == _pillow(pic, 95)
    assert not (tmp_path / "c" / "visualisations").exists() and (tmp_path / "b" / "data" / "0000000007.npy").exists()
