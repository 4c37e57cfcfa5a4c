"""GPU: the baseline JPEG encoder (csrc/jpeg.hip) byte for byte against Pillow's bytes as recorded (tests/golden/g18_jpeg.npz) and the
NumPy restatement (tests/jpeg_restatement.py, pinned to both by tests/test_jpeg_cpu.py); then the three routes built on it, each run
with and without the flag into two folders that must hold identical files.  No tolerance anywhere."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import jpeg_restatement as JR
from tests.golden import make_golden_jpeg as G

pytestmark = pytest.mark.gpu

GOLD = G.load()
CASES = list(G.cases())


def restated(a, quality):
    from footprints_amd import ops
    t = ops.jpeg_tables(quality)
    return JR.encode(a, dict(header=t.header, size_at=t.size_at, quant=t.quant, huff=t.huff))[0]


def recorded_tables_are_installed(quality):
    """the recorded files carry their own tables; the encoder uses the installed Pillow's.  They are the standard ones in both."""
    from footprints_amd import ops
    name = "8x8_noise_q%d" % quality
    parsed = JR.parse_header(GOLD[name])
    return parsed["header"] == ops.jpeg_tables(quality).file_header(8, 8)


@pytest.mark.parametrize("quality", G.QUALITIES)
def test_every_fixture_case(quality):
    from footprints_amd import ops
    assert recorded_tables_are_installed(quality)
    for name, size, content, q in CASES:
        if q == quality:
            got = ops.jpeg_encode([G.picture(size, content)], quality=quality)
            assert len(got) == 1 and got[0] == GOLD[name], name


def test_mixed_batch_equals_single_calls():
    from footprints_amd import ops
    pictures = [G.picture(size, content) for size, content in (((1, 1), "noise"), ((9, 25), "ramp"), ((37, 50), "bw"), ((75, 122), "noise"))]
    batch = ops.jpeg_encode(pictures, quality=95)
    assert batch == [ops.jpeg_encode([p], quality=95)[0] for p in pictures]
    assert batch == [GOLD["1x1_noise_q95"], GOLD["9x25_ramp_q95"], GOLD["37x50_bw_q95"], GOLD["75x122_noise_q95"]]
    # a dense device tensor is the equal-size case of the same path
    same = np.stack([G.picture((33, 47), c) for c in G.CONTENTS])
    assert ops.jpeg_encode(torch.from_numpy(same).cuda(), quality=75) == [GOLD["33x47_%s_q75" % c] for c in G.CONTENTS]


def test_scan_carries_across_chunks():
    """192 x 320: 1 440 blocks, more than the 1 024 one pass of the per-sample prefix sum covers; noise at quality 100 also makes the
    unstuffed stream longer than one 4 KiB chunk of the stuffing kernels"""
    from footprints_amd import ops
    rng = np.random.default_rng(192320)
    yy, xx = np.mgrid[0:192, 0:320]
    ramp = np.clip(np.stack([xx // 2 + yy // 3, 255 - yy, (xx + yy) // 2], -1) + rng.integers(-6, 6, (192, 320, 3)), 0, 255).astype(np.uint8)
    noise = rng.integers(0, 256, (192, 320, 3), dtype=np.uint8)
    got = ops.jpeg_encode([ramp, noise], quality=95) + ops.jpeg_encode([noise], quality=100)
    assert got[0] == restated(ramp, 95) and got[1] == restated(noise, 95) and got[2] == restated(noise, 100)
    assert len(got[2]) > 3 * 4096


def _packed(pictures):
    from footprints_amd import ops
    shapes = [p.shape[:2] for p in pictures]
    records, total, max_h, max_w = ops.jpeg_records(shapes)
    src = torch.from_numpy(np.concatenate([p.reshape(-1) for p in pictures])).cuda()
    return src, records, total, max_h, max_w, shapes


def test_guard_bytes_and_an_output_that_is_too_small():
    from footprints_amd import ops
    pictures = [G.picture((37, 50), "noise"), G.picture((16, 17), "bw"), G.picture((41, 57), "ramp")]
    names = ["37x50_noise_q95", "16x17_bw_q95", "41x57_ramp_q95"]
    src, records, total, max_h, max_w, shapes = _packed(pictures)
    rec = torch.from_numpy(records).cuda()
    scans = [len(GOLD[n]) - len(ops.jpeg_tables(95).header) - 2 for n in names]
    need = sum(scans)
    for room in (need, need - 1):                           # exactly enough; one byte short for the last sample
        buf = torch.full((need + 128,), 0xCD, dtype=torch.uint8, device="cuda")
        out, table = ops.jpeg_encode_packed(src, total, rec, 3, 95, out=buf[64:64 + room], max_h=max_h, max_w=max_w)
        table, host = table.cpu().numpy(), buf.cpu().numpy()
        fits = 3 if room == need else 2
        assert (host[:64] == 0xCD).all() and (host[64 + sum(scans[:fits]):] == 0xCD).all()
        assert [int(v) for v in table[:3, 1]] == scans[:fits] + [0] * (3 - fits) and int(table[3, 0]) == sum(scans[:fits])
        assert int(table[3, 1]) == (0 if fits == 3 else 1)
        if fits == 3:
            assert ops.jpeg_files(host[64:64 + need], table, shapes, 95) == [GOLD[n] for n in names]
        else:
            with pytest.raises(ValueError):
                ops.jpeg_files(host[64:64 + need], table, shapes, 95)
            table[3, 1] = 0
            assert ops.jpeg_files(host[64:64 + need], table, shapes[:2], 95) == [GOLD[n] for n in names[:2]]


def test_a_turned_down_record_sets_the_status_and_writes_nothing():
    from footprints_amd import _lib, ops
    pictures = [G.picture((24, 40), "ramp"), G.picture((9, 25), "noise")]
    src, records, total, max_h, max_w, shapes = _packed(pictures)
    good = [GOLD["24x40_ramp_q95"], GOLD["9x25_noise_q95"]]
    assert ops.jpeg_encode(pictures, quality=95) == good
    bad_records = {"zero height": _lib.JpegSample(0, 0, 40), "negative width": _lib.JpegSample(0, 24, -1), "too wide": _lib.JpegSample(0, 1, 65536),
                   "beyond max_w": _lib.JpegSample(0, 9, 41), "offset beyond the buffer": _lib.JpegSample(total - 10, 9, 25),
                   "negative offset": _lib.JpegSample(-1, 9, 25)}
    for what, bad in bad_records.items():
        rec = np.concatenate([records[:16], np.frombuffer(bytes(bad), dtype=np.uint8), records[16:]])
        out = torch.full((ops.jpeg_max_scan_bytes(3, max_h, max_w),), 0xAB, dtype=torch.uint8, device="cuda")
        _, table = ops.jpeg_encode_packed(src, total, torch.from_numpy(rec).cuda(), 3, 95, out=out, max_h=max_h, max_w=max_w)
        table, host = table.cpu().numpy(), out.cpu().numpy()
        assert int(table[3, 1]) == 1 and int(table[1, 1]) == 0, what
        used = int(table[3, 0])
        assert used == int(table[0, 1]) + int(table[2, 1]) and int(table[2, 0]) == int(table[0, 1]) and (host[used:] == 0xAB).all(), what
        table[3, 1] = 0
        files = ops.jpeg_files(host, table[[0, 2, 3]], shapes, 95)
        assert files == good, what


# ---- the three routes ----------------------------------------------------------------------------------------------------------------------
def _files_below(root):
    return {os.path.relpath(os.path.join(d, f), root): open(os.path.join(d, f), "rb").read() for d, _, fs in os.walk(root) for f in fs}


@functools.lru_cache(None)
def model_manager():
    from footprints_amd.model_manager import ModelManager
    torch.manual_seed(5)
    return ModelManager(is_inference=True)


def _photo(h, w, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    ramp = np.stack([(xx * 255) // w, (yy * 255) // h, ((xx + yy) * 255) // (h + w)], -1)
    return np.clip(ramp + rng.integers(-12, 12, ramp.shape), 0, 255).astype(np.uint8)


def test_predict_simple_writes_the_same_files(tmp_path):
    from PIL import Image
    from footprints_amd.predict_simple import InferenceManager
    folder = tmp_path / "photos"
    folder.mkdir()
    for i, (stem, (h, w)) in enumerate({"a": (120, 400), "b": (97, 311), "c": (75, 122)}.items()):
        Image.fromarray(_photo(h, w, 300 + i)).save(folder / (stem + ".png"))
    with pytest.raises(ValueError):
        InferenceManager("kitti", str(tmp_path / "x"), model_manager=model_manager(), device_jpeg=True)
    written = {}
    for flag in (False, True):
        im = InferenceManager("kitti", str(tmp_path / str(flag)), model_manager=model_manager(), device_resize=True, device_vis=True,
                              batch_size=3, device_jpeg=flag)
        assert im.predict(str(folder)) == 3
        written[flag] = _files_below(tmp_path / str(flag))
    assert sorted(written[True]) == sorted("%s/%s.%s" % (d, s, e) for d, e in (("outputs", "npy"), ("visualisations", "jpg")) for s in "abc")
    assert written[True] == written[False]
    # the hook still sees the raw overlay
    seen = {}
    im.overlay_hook = lambda stem, vis: seen.__setitem__(stem, vis.copy())
    im.predict(str(folder))
    assert sorted(seen) == ["a", "b", "c"] and seen["c"].shape == (75, 122, 3) and _files_below(tmp_path / "True") == written[False]
    assert restated(seen["b"], 95) == written[True]["visualisations/b.jpg"]


def test_test_set_inference_writes_the_same_files(tmp_path):
    from footprints_amd.evaluation.inference import InferenceManager
    from footprints_amd.training.train import synthetic_batch
    img = synthetic_batch(2, 64, 96, "cuda")["image"]
    written = {}
    for flag in (False, True):
        im = InferenceManager(model_manager=model_manager(), save_path=str(tmp_path / str(flag)), save_test_visualisations=True, device_jpeg=flag)
        im.run([{"image": img.cpu(), "idx": ["f0", "f1"]}])
        written[flag] = _files_below(tmp_path / str(flag))
    assert sorted(written[True]) == ["f0.jpg", "f0.npy", "f1.jpg", "f1.npy"] and written[True] == written[False]


def test_tester_writes_the_same_files(tmp_path):
    """7 frames of two native sizes in batches of 3 (the last one short) through 2 slots"""
    from footprints_amd.preprocessing.segmentation.datasets.inference import KITTIInferenceDataset
    from footprints_amd.preprocessing.segmentation.inference import Tester
    from footprints_amd.preprocessing.segmentation.network import Segmentor
    from footprints_amd.preprocessing.segmentation.options import SegmentationOptions
    from oracle import restatement as R
    H, W = 64, 96
    frames = [_photo(*((70, 231) if i % 2 == 0 else (75, 248)), 400 + i) for i in range(7)]
    names = ["2011_09_26/drive_%d %d %s" % (i // 4, 10 * i + 3, "l" if i % 3 else "r") for i in range(7)]

    class MemoryKITTI(KITTIInferenceDataset):
        def _load_image(self, index):
            return frames[index]

    P, Bf = R.make_seg_state(True, tag="g9.psp")
    model = Segmentor(pretrained=False, use_PSP=True)
    model.load_state_dict({**P, **Bf})
    model.cuda()
    written = {}
    for flag in (False, True):
        opt = SegmentationOptions().parse(["--mode", "inference", "--height", str(H), "--width", str(W), "--batch_size", "3",
                                           "--save_test_visualisations", "--num_workers", "2"] + (["--device_jpeg"] if flag else []))
        tester = Tester(opt, model=model, dataset=MemoryKITTI("", names, H, W), save_path=str(tmp_path / str(flag)), slots=2)
        tester.test()
        written[flag] = _files_below(tmp_path / str(flag))
    assert len(written[True]) == 14 and sum(k.endswith(".jpg") for k in written[True]) == 7
    assert written[True] == written[False]
    # the blocking call hands out the files' bytes
    half, files = tester.test_batch(frames[:3])
    assert half.shape == (3, 1, H, W) and files == [written[True][os.path.join("2011_09_26/drive_0", "image_02" if n.endswith("l") else "image_03",
                                                                              "visualisations", "%010d.jpg" % int(n.split(" ")[1]))] for n in names[:3]]
    # without --save_test_visualisations the flag asks for nothing
    opt = SegmentationOptions().parse(["--mode", "inference", "--height", str(H), "--width", str(W), "--batch_size", "3", "--device_jpeg"])
    assert not Tester(opt, model=model, dataset=MemoryKITTI("", names, H, W), save_path=str(tmp_path / "none")).device_jpeg
