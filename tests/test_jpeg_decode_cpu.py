"""CPU: the host half of the device JPEG decoder (footprints_amd.ops.jpeg_parse / jpeg_decode_pack) and its NumPy restatement
(tests/jpeg_decode_restatement.py): the restatement against the recorded fixture G19 and against the installed Pillow, the parser's
verdicts, and the model of the subsequence scheme that the GPU tests' demands rest on.  No kernel is launched here."""
import functools
import io

import numpy as np
import pytest

from tests import jpeg_decode_restatement as JD
from tests.golden import make_golden_jpeg_decode as G


@functools.lru_cache(None)
def gold():
    return G.load()


def test_restatement_equals_the_fixture():
    assert len(gold()) == len(list(G.cases())) <= 100
    for name, (data, rgb) in gold().items():
        assert rgb.shape[0] <= 48 and rgb.shape[1] <= 64
        assert np.array_equal(JD.decode(data), rgb), name


@pytest.mark.parametrize("size", G.SIZES + G.MORE_SIZES, ids=lambda s: "%dx%d" % s)
def test_restatement_equals_the_installed_pillow(size):
    for name, size_, content, quality, sampling in G.grid((size,)):
        data = G.write(G.picture(size_, content), quality, sampling)
        assert np.array_equal(JD.decode(data), G.pillow_decode(data)), name
    data = G.write(G.picture(size, "noise"), 75, 2, optimize=True)
    assert np.array_equal(JD.decode(data), G.pillow_decode(data)), "optimised tables"
    data = G.write(G.picture(size, "noise", grey=True), 90)
    assert np.array_equal(JD.decode(data), G.pillow_decode(data)), "grey"


def test_the_fixture_files_are_what_the_installed_pillow_decodes_alike():
    """the recorded arrays are Pillow's where they were recorded; the installed one must agree or nothing here is byte-equal to it"""
    for name, (data, rgb) in gold().items():
        assert np.array_equal(G.pillow_decode(data), rgb), name


def _parsers():
    from footprints_amd import ops
    return (("ops", ops.jpeg_parse), ("restatement", JD.parse))


def test_parser_accepts_every_fixture_file_and_agrees_with_the_restatement():
    from footprints_amd import ops
    for name, (data, rgb) in gold().items():
        a, b = ops.jpeg_parse(data), JD.parse(data)
        assert a["device"] and b["device"], name
        for key in ("h", "w", "ncomp", "hs", "vs", "scan_offset", "scan_bytes"):
            assert a[key] == b[key], (name, key)
        assert (a["h"], a["w"]) == rgb.shape[:2] and tuple(a["td"]) == tuple(b["td"]) and tuple(a["tq"]) == tuple(b["tq"])
        assert data[a["scan_offset"] + a["scan_bytes"]:a["scan_offset"] + a["scan_bytes"] + 2] == b"\xff\xd9"


def test_parser_sends_what_it_does_not_take_to_the_host():
    from PIL import Image
    a = G.picture((37, 53), "ramp")

    def saved(image, **kw):
        buf = io.BytesIO()
        image.save(buf, format="JPEG", **kw)
        return buf.getvalue()
    good = saved(Image.fromarray(a))
    host = {"progressive": saved(Image.fromarray(a), progressive=True),
            "restart markers": saved(Image.fromarray(a), restart_marker_blocks=4),
            "CMYK": saved(Image.fromarray(np.dstack([a, a[:, :, :1]]), mode="CMYK")),
            "cut inside the header": good[:100],
            "cut behind the marker": good[:3],
            "empty": b"",
            "zero-length segment": good[:20] + b"\xff\xe1\x00\x00" + good[20:],
            "no end-of-image marker": good[:-2],
            "not a JPEG": b"\x89PNG\r\n\x1a\n" + bytes(64)}
    for _, parse in _parsers():
        assert parse(good)["device"]
    for what, data in host.items():
        for who, parse in _parsers():
            verdict = parse(data)
            assert verdict["device"] is False and isinstance(verdict["reason"], str) and verdict["reason"], (what, who)


def test_pack_shares_the_table_blocks_of_files_with_the_same_tables():
    from footprints_amd import _lib, ops
    by_quality = {}
    for name in gold():
        if name.startswith("48x64_s2") and not name.endswith("opt"):
            by_quality.setdefault(name.split("_")[2], name)
    files = [gold()[n][0] for n in by_quality.values()] * 2 + [gold()["48x64_s2_q75_noise_opt"][0]]
    pack = ops.jpeg_decode_pack(files)
    assert pack["B"] == len(files) and pack["n_sets"] == len(by_quality) + 1
    assert pack["tables"].size == pack["n_sets"] * _lib.JPEG_DECODE_TABLE_WORDS and pack["scan_bytes"] == pack["scans"].size
    rec = np.frombuffer(pack["records"].tobytes(), dtype=np.int32).reshape(len(files), 12)
    assert list(rec[:, 10]) == list(range(len(by_quality))) * 2 + [len(by_quality)]
    assert pack["out_bytes"] == len(files) * 48 * 64 * 3 and pack["max_scan"] == max(rec[:, 4])
    with pytest.raises(ValueError):
        ops.jpeg_decode_pack([b"\xff\xd8\xff"])


# ---- the model of the subsequence scheme ---------------------------------------------------------------------------------------------------
def test_settled_entry_states_are_symbol_boundaries_of_the_serial_decode():
    for name, (data, _) in gold().items():
        info = JD.parse(data)
        marks = set()
        JD.serial_coefficients(info, data, marks)
        total = JD.Stream(info, data).total
        for bits in (32, 128):
            m = JD.model(data, bits)
            # behind the last block only padding follows: a state there is no symbol's start
            last = max(p for p, _, _ in marks)
            for e in m["entries"]:
                assert e in marks or e[0] > last, (name, bits, e)
            assert m["entries"][0] == (0, 0, 0) and m["nsub"] == max(1, -(-total // bits))


@functools.lru_cache(None)
def noise_frame():
    rng = np.random.default_rng(96128)
    return G.write(rng.integers(0, 256, (96, 128, 3), dtype=np.uint8), 100)


def test_pictures_settle_within_half_the_default_budget_and_noise_does_not():
    """the condition under which the GPU tests may demand that no picture falls back -- and the case that keeps the fallback honest:
    blocks of noise at quality 100 have no end-of-block symbol, so a wrong zigzag phase never corrects"""
    from footprints_amd import ops
    bits, budget = ops.JPEG_DECODE_SUBSEQ_BITS, ops.JPEG_DECODE_MAX_ROUNDS
    assert 128 <= bits <= 2048 and budget >= 2
    spans = []
    for quality, sampling in ((90, 2), (75, 2), (95, 0)):
        data = G.write(G.photo(192, 256, 7), quality, sampling)
        m = JD.model(data, bits)
        assert m["launches"] <= budget // 2 and m["hops"] < JD.GROUP, (quality, sampling, m["launches"], m["hops"])
        spans.append(m["nsub"])
    assert max(spans) > 2 * JD.GROUP            # several workgroups: an entry state crossed a launch boundary
    m = JD.model(noise_frame(), bits)
    assert m["launches"] > budget, (m["launches"], m["hops"], m["nsub"])
