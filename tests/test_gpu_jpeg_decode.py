"""GPU: the device JPEG decoder (csrc/jpeg_decode.hip) against Pillow, byte for byte -- the fixture G19 and the same grid written afresh
by the installed Pillow, a mixed batch, subsequence boundaries, the launch budget and its host fallback, guarded inputs, and
predict_simple's --device_decode."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from tests.golden import make_golden_jpeg_decode as G

pytestmark = pytest.mark.gpu


@functools.lru_cache(None)
def gold():
    return G.load()


def _gold(prefix, suffix=""):
    """the file of the first fixture case whose name begins and ends so"""
    return gold()[next(k for k in sorted(gold()) if k.startswith(prefix) and k.endswith(suffix))][0]


def _nsub(data, bits):
    from footprints_amd import ops
    return -(-ops.jpeg_parse(data)["scan_bytes"] * 8 // bits)


def _decode_all(files, want, default_budget=False):
    """ops.jpeg_decode in batches: every file decoded on the device (status 0), equal to `want`.  Noise at quality 100 does not
    resynchronise (tests/test_jpeg_decode_cpu.py), so unless default_budget is set the launch budget is the one that settles any
    content: a launch settles at least one more workgroup of 64 subsequences."""
    from footprints_amd import ops
    for at in range(0, len(files), 48):
        kw = {} if default_budget else {"max_rounds": max(-(-_nsub(f, ops.JPEG_DECODE_SUBSEQ_BITS) // 64) for f in files[at:at + 48]) + 1}
        arrays, statuses = ops.jpeg_decode(files[at:at + 48], return_status=True, **kw)
        assert statuses == [0] * len(arrays), (at, statuses)
        for n, (a, w) in enumerate(zip(arrays, want[at:at + 48])):
            assert a.dtype == np.uint8 and a.shape == w.shape and np.array_equal(a, w), at + n


def test_every_fixture_case():
    names = sorted(gold())
    _decode_all([gold()[n][0] for n in names], [gold()[n][1] for n in names])


def test_pictures_settle_within_the_default_budget():
    """what tests/test_jpeg_decode_cpu.py shows on the model: nothing picture-like falls back"""
    files = [G.write(G.photo(192, 256, 7), quality, sampling) for quality, sampling in ((90, 2), (75, 2), (95, 0), (95, 1))]
    files += [G.write(G.photo(375, 621, 8), 95, 2), G.write(G.photo(75, 122, 9)[:, :, 1].copy(), 85)]
    _decode_all(files, [G.pillow_decode(f) for f in files], default_budget=True)


@pytest.mark.parametrize("sizes", (G.SIZES[:5], G.SIZES[5:], G.MORE_SIZES), ids=("small", "medium", "large"))
def test_the_grid_written_afresh(sizes):
    files = [G.write(G.picture(size, content), quality, sampling) for _, size, content, quality, sampling in G.grid(sizes)]
    files += [G.write(G.picture(size, "noise"), 75, 2, optimize=True) for size in sizes] + [G.write(G.picture(size, "ramp", grey=True), 90) for size in sizes]
    _decode_all(files, [G.pillow_decode(f) for f in files])


def test_mixed_batch_equals_single_calls():
    from PIL import Image
    import io
    from footprints_amd import ops
    buf = io.BytesIO()
    Image.fromarray(G.picture((33, 15), "ramp")).save(buf, format="JPEG", progressive=True)
    files = [_gold("48x64_s0", "noise"), _gold("7x9_s1"), _gold("37x53_s2"), _gold("1x1_s0"), _gold("37x53_grey"), _gold("15x33_s2", "opt"),
             _gold("33x15_s2"), _gold("17x17_s0"), _gold("48x64_s2", "opt"), _gold("16x16_s1")]
    files.insert(4, buf.getvalue())
    assert len({ops.jpeg_parse(f).get("hs", 0) * 2 + ops.jpeg_parse(f).get("vs", 0) for f in files}) == 4       # host, 1x1, 2x1, 2x2
    batch, statuses = ops.jpeg_decode(files, return_status=True)
    assert statuses == [0] * 4 + [-1] + [0] * 6
    for n, f in enumerate(files):
        single = ops.jpeg_decode([f])[0]
        assert np.array_equal(batch[n], single) and np.array_equal(single, G.pillow_decode(f)), n


def test_symbols_and_stuffing_across_subsequence_boundaries():
    from footprints_amd import ops
    files = [G.write(G.picture((48, 64), "noise"), 95), G.write(G.picture((100, 75), "noise"), 95), G.write(G.picture((100, 75), "sat"), 100)]
    assert files[2][ops.jpeg_parse(files[2])["scan_offset"]:].count(b"\xff\x00") > 40
    for f in files:
        n = _nsub(f, 128)
        assert n > 2 * 64                           # several workgroups
        arrays, statuses = ops.jpeg_decode([f], subseq_bits=128, max_rounds=n, return_status=True)
        assert statuses == [0] and np.array_equal(arrays[0], G.pillow_decode(f))
    arrays, statuses = ops.jpeg_decode(files, subseq_bits=128, max_rounds=max(_nsub(f, 128) for f in files), return_status=True)
    assert statuses == [0, 0, 0] and all(np.array_equal(a, G.pillow_decode(f)) for a, f in zip(arrays, files))


@functools.lru_cache(None)
def noise_frame():
    rng = np.random.default_rng(96128)
    return G.write(rng.integers(0, 256, (96, 128, 3), dtype=np.uint8), 100)


def test_the_budget_and_the_host_fallback():
    from footprints_amd import ops
    f = noise_frame()
    want = G.pillow_decode(f)
    pack = ops.jpeg_decode_pack([f])
    out = torch.full((pack["out_bytes"],), 0x5A, dtype=torch.uint8, device="cuda")
    _, _, status = ops.jpeg_decode_packed(pack, out=out, max_rounds=1)
    assert status.cpu().tolist() == [2, 2] and bool((out == 0x5A).all())
    arrays, statuses = ops.jpeg_decode([f], max_rounds=1, return_status=True)
    assert statuses == [2] and np.array_equal(arrays[0], want)
    n = _nsub(f, ops.JPEG_DECODE_SUBSEQ_BITS)
    _, _, status, info = ops.jpeg_decode_packed(pack, out=out, max_rounds=n, want_info=True)
    assert status.cpu().tolist() == [0, 0] and np.array_equal(out.cpu().numpy().reshape(want.shape), want)
    assert 1 < int(info[0, 1]) + 1 <= n             # the launches it needed: more than one, the serial bound at most


def _raw_call(pack, records, scans, out_room, max_rounds, subseq_bits=256):
    """fp_jpeg_decode with sentinel bytes around the output and the workspace -> (status, the output's part, all sentinels intact)"""
    from footprints_amd import _lib, ops
    lib = _lib.load()
    B = pack["B"]
    need = lib.fp_jpeg_decode_workspace_bytes(B, pack["max_h"], pack["max_w"], pack["max_scan"], subseq_bits)
    assert need > 0
    ws = torch.full((need + 512,), 0xC3, dtype=torch.uint8, device="cuda")
    out = torch.full((out_room + 512,), 0xA7, dtype=torch.uint8, device="cuda")
    status = torch.full((B + 1 + 8,), 0x77777777, dtype=torch.int32, device="cuda")
    d_scans, d_rec = torch.from_numpy(scans).cuda(), torch.from_numpy(records).cuda()
    d_tab = torch.from_numpy(pack["tables"].view("int32")).cuda()
    _lib.check(lib.fp_jpeg_decode(d_scans.data_ptr(), d_scans.numel(), d_rec.data_ptr(), d_tab.data_ptr(), pack["n_sets"], out.data_ptr() + 256,
                                  out_room, status.data_ptr(), B, pack["max_h"], pack["max_w"], pack["max_scan"], subseq_bits, max_rounds,
                                  ws.data_ptr() + 256, need, ops.stream()), "fp_jpeg_decode")
    torch.cuda.synchronize()
    ws, out, status = ws.cpu().numpy(), out.cpu().numpy(), status.cpu().numpy()
    intact = bool((ws[:256] == 0xC3).all() and (ws[256 + need:] == 0xC3).all() and (out[:256] == 0xA7).all() and (out[256 + out_room:] == 0xA7).all()
                  and (status[B + 1:] == 0x77777777).all())
    return status[:B + 1].tolist(), out[256:256 + out_room], intact


def test_guarded_inputs_write_nothing():
    from footprints_amd import _lib, ops
    files = [_gold("37x53_s2"), _gold("48x64_s0", "noise"), _gold("33x15_s1")]
    want = [G.pillow_decode(f) for f in files]
    pack = ops.jpeg_decode_pack(files)
    sizes = [w.size for w in want]
    rounds = max(_nsub(f, 256) for f in files)
    rec = lambda: np.frombuffer(pack["records"].tobytes(), dtype=np.uint8).copy()
    fields = lambda r: r.view(np.int32).reshape(3, 12)          # scan_offset, out_offset (two words each), scan_bytes, h, w, ...

    def check(status, out, intact, bad, code):
        assert intact
        assert [status[n] for n in range(3)] == [code if n == bad else 0 for n in range(3)] and status[3] == code
        at = 0
        for n in range(3):
            part = out[at:at + sizes[n]]
            at += sizes[n]
            if at > out.size:
                break
            if n == bad:
                assert (part == 0xA7).all(), "a sample with a non-zero status wrote into out"
            else:
                assert np.array_equal(part.reshape(want[n].shape), want[n])
    check(*_raw_call(pack, rec(), pack["scans"], pack["out_bytes"], rounds), bad=-1, code=0)
    # a record pointing outside the scans
    r = rec()
    fields(r)[1, 0] = pack["scan_bytes"] - 10
    check(*_raw_call(pack, r, pack["scans"], pack["out_bytes"], rounds), bad=1, code=1)
    # an output one byte too small for the last sample
    status, out, intact = _raw_call(pack, rec(), pack["scans"], pack["out_bytes"] - 1, rounds)
    assert intact and status == [0, 0, 1, 1] and (out[sizes[0] + sizes[1]:] == 0xA7).all()
    assert np.array_equal(out[:sizes[0]].reshape(want[0].shape), want[0])
    # a scan cut to half its length
    r = rec()
    fields(r)[1, 4] //= 2
    status, out, intact = _raw_call(pack, r, pack["scans"], pack["out_bytes"], rounds)
    assert status[1] in (1, 3)
    check(status, out, intact, bad=1, code=status[1])
    # random bytes under a valid header
    scans = pack["scans"].copy()
    at, n = int(fields(rec())[1, 0]), int(fields(rec())[1, 4])
    scans[at:at + n] = np.random.default_rng(4).integers(0, 256, n, dtype=np.uint8)
    status, out, intact = _raw_call(pack, rec(), scans, pack["out_bytes"], rounds)
    assert status[1] in (1, 3)
    check(status, out, intact, bad=1, code=status[1])
    # the public call hands such a file to Pillow: whatever it returns or raises is the result
    info = ops.jpeg_parse(files[1])
    cut = files[1][:info["scan_offset"] + info["scan_bytes"] // 2].rstrip(b"\xff") + b"\xff\xd9"
    try:
        expected = G.pillow_decode(cut)
    except Exception as e:                              # noqa: BLE001 -- Pillow's verdict, whatever it is
        with pytest.raises(type(e)):
            ops.jpeg_decode([cut])
    else:
        arrays, statuses = ops.jpeg_decode([cut], return_status=True)
        assert statuses == [3] and np.array_equal(arrays[0], expected)
    assert C.sizeof(_lib.JpegDecodeSample) == _lib.load().fp_jpeg_decode_sample_bytes() == 48
    assert _lib.load().fp_jpeg_decode_table_words() == _lib.JPEG_DECODE_TABLE_WORDS


# ---- predict_simple --------------------------------------------------------------------------------------------------------------------------
def _files_below(root):
    return {os.path.relpath(os.path.join(d, f), root): open(os.path.join(d, f), "rb").read() for d, _, fs in os.walk(root) for f in fs}


@functools.lru_cache(None)
def model_manager():
    from footprints_amd.model_manager import ModelManager
    torch.manual_seed(5)
    return ModelManager(is_inference=True)


@pytest.mark.parametrize("device_vis", (False, True), ids=("host_vis", "device_vis"))
def test_predict_simple_writes_the_same_files(tmp_path, device_vis):
    from PIL import Image
    from footprints_amd.predict_simple import InferenceManager, parse_args
    folder = tmp_path / "photos"
    folder.mkdir()
    for i, (stem, (h, w)) in enumerate({"a": (120, 400), "b": (97, 311), "c": (75, 122)}.items()):
        Image.fromarray(G.photo(h, w, 300 + i)).save(folder / (stem + ".jpg"), quality=(95, 80, 90)[i], subsampling=(2, 0, 1)[i])
    Image.fromarray(G.photo(60, 200, 9)).save(folder / "d.png")
    with pytest.raises(ValueError):
        InferenceManager("kitti", str(tmp_path / "x"), model_manager=model_manager(), device_decode=True)
    with pytest.raises(SystemExit):
        parse_args(["--image", str(folder), "--model", "kitti", "--device_decode"])
    assert parse_args(["--image", str(folder), "--model", "kitti", "--device_decode", "--device_resize"]).device_decode
    written, inputs, managers = {}, {}, {}
    for flag in (False, True):
        im = InferenceManager("kitti", str(tmp_path / str(flag)), model_manager=model_manager(), device_resize=True, device_vis=device_vis,
                              batch_size=3, device_decode=flag)
        managers[flag] = im
        seen = inputs.setdefault(flag, [])
        hook = model_manager().model.register_forward_pre_hook(lambda m, args, seen=seen: seen.append(args[0].detach().cpu().numpy().copy()))
        try:
            assert im.predict(str(folder)) == 4
        finally:
            hook.remove()
        written[flag] = _files_below(tmp_path / str(flag))
    assert sorted(written[True]) == sorted("%s/%s.%s" % (d, s, e) for d, e in (("outputs", "npy"), ("visualisations", "jpg")) for s in "abcd")
    assert [x.shape for x in inputs[True]] == [(3, 3, 192, 640), (1, 3, 192, 640)]
    assert all(np.array_equal(a, b) for a, b in zip(inputs[True], inputs[False])) and len(inputs[False]) == 2
    assert written[True] == written[False]
    # one file alone goes the same way
    for flag in (False, True):
        assert managers[flag].predict(str(folder / "b.jpg")) == 1
    assert _files_below(tmp_path / "True") == _files_below(tmp_path / "False")
