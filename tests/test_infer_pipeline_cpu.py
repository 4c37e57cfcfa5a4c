"""CPU: the host side of test-set inference from the command line -- the main network's test-set readers and
their file layout, the new flags of both parsers, the host half of the decode stage with a fake "device", and the restatement of
fp_infer_pack against the restatements it is built from.  No kernel is launched here."""
import io
import os

import numpy as np
import pytest
import torch

from tests import infer_pack_restatement as IR
from tests import seg_infer_restatement as SR
from tests import vis_restatement as VR
from tests.golden import make_golden_jpeg_decode as G


# ---- the dataset classes ---------------------------------------------------------------------------------------------------------------
def test_kitti_names_and_files(tmp_path):
    from footprints_amd.datasets.inference import KITTIInferenceDataset, get_inference_dataset_class
    names = ["2011_09_26/2011_09_26_drive_0001_sync %d %s" % (i, "l" if i != 6 else "r") for i in range(8)]
    ds = KITTIInferenceDataset("/data/kitti", names, 192, 640)
    assert len(ds) == 8 and (ds.height, ds.width) == (192, 640) and ds.image_ext == "jpg"
    assert ds.image_path(5) == "/data/kitti/2011_09_26/2011_09_26_drive_0001_sync/image_02/data/0000000005.jpg"
    assert ds.image_path(6) == "/data/kitti/2011_09_26/2011_09_26_drive_0001_sync/image_03/data/0000000006.jpg"
    assert KITTIInferenceDataset("/d", names, 1, 1, image_ext="png").image_path(0).endswith("image_02/data/0000000000.png")
    pred = (np.arange(4 * 3 * 5, dtype=np.float32).reshape(4, 3, 5) / 7).astype(np.float16)
    pic = np.arange(3 * 10 * 3, dtype=np.uint8).reshape(3, 10, 3)
    ds.save_result(7, pred, str(tmp_path / "out"), pic)
    ds.save_result(np.int64(12), pred, str(tmp_path / "out"))
    ds.save_result(3, pred, str(tmp_path / "out"), b"\xff\xd8 bytes as the device encoded them \xff\xd9")
    assert sorted(os.listdir(tmp_path / "out")) == ["003.jpg", "003.npy", "007.jpg", "007.npy", "012.npy"]
    got = np.load(tmp_path / "out" / "007.npy")
    assert got.dtype == np.float16 and got.shape == (4, 3, 5) and np.array_equal(got.view(np.uint16), pred.view(np.uint16))
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(pic).save(buf, format="JPEG", quality=95)
    assert (tmp_path / "out" / "007.jpg").read_bytes() == buf.getvalue()                 # what InferenceManager.run writes
    assert (tmp_path / "out" / "003.jpg").read_bytes() == b"\xff\xd8 bytes as the device encoded them \xff\xd9"
    assert get_inference_dataset_class("kitti") is KITTIInferenceDataset


def test_matterport_names_and_files(tmp_path):
    from footprints_amd.datasets.inference import MatterportInferenceDataset, get_inference_dataset_class
    ds = MatterportInferenceDataset("/data/mp", ["17DRP5sb8fy 0f37bd0737e349de9d536263a4bdd60d 1 2"], 512, 640)
    assert ds.image_path(0) == "/data/mp/17DRP5sb8fy/17DRP5sb8fy/matterport_color_images/0f37bd0737e349de9d536263a4bdd60d_i1_2.jpg"
    assert "sample_dataset" not in ds.image_path(0)                   # that prefix belongs to the segmentation network's reader
    pred = np.full((4, 2, 2), 0.25, np.float16)
    ds.save_result(0, pred, str(tmp_path), np.zeros((2, 4, 3), np.uint8))
    assert sorted(os.listdir(tmp_path / "17DRP5sb8fy")) == ["0f37bd0737e349de9d536263a4bdd60d_1_2.jpg", "0f37bd0737e349de9d536263a4bdd60d_1_2.npy"]
    assert np.array_equal(np.load(tmp_path / "17DRP5sb8fy" / "0f37bd0737e349de9d536263a4bdd60d_1_2.npy"), pred)
    assert get_inference_dataset_class("matterport") is MatterportInferenceDataset
    with pytest.raises(NotImplementedError):
        get_inference_dataset_class("handheld")


def test_samples_are_frames_or_bytes(tmp_path):
    from PIL import Image
    from footprints_amd.datasets.inference import KITTIInferenceDataset
    folder = tmp_path / "seq" / "image_02" / "data"
    folder.mkdir(parents=True)
    frame = G.photo(40, 56, 3)
    (folder / "0000000001.jpg").write_bytes(G.write(frame, 95, 2))
    Image.fromarray(frame).convert("L").save(folder / "0000000002.jpg", quality=90)
    buf = io.BytesIO()
    Image.fromarray(frame).save(buf, format="JPEG", progressive=True)
    (folder / "0000000003.jpg").write_bytes(buf.getvalue())
    ds = KITTIInferenceDataset(str(tmp_path), ["seq 1 l", "seq 2 l", "seq 3 l", "seq 4 l"], 32, 48)
    for i in range(3):
        smp = ds[i]                                                   # host decoding: the frame at its native size, RGB
        data = (folder / ("%010d.jpg" % (i + 1))).read_bytes()
        assert smp["idx"] == i and smp["image"].shape == (40, 56, 3) and np.array_equal(smp["image"], G.pillow_decode(data))
        assert "bytes" not in smp and "refused" not in smp
    a, b, c = (ds.read(i, device_decode=True) for i in range(3))
    assert "image" not in a and a["bytes"] == (folder / "0000000001.jpg").read_bytes() and (a["info"]["h"], a["info"]["w"]) == (40, 56)
    assert "image" not in b and b["info"]["ncomp"] == 1
    assert "bytes" not in c and c["refused"] and np.array_equal(c["image"], G.pillow_decode(buf.getvalue()))
    with pytest.raises(FileNotFoundError):
        ds[3]


# ---- the flags -------------------------------------------------------------------------------------------------------------------------
def test_both_parsers_take_the_new_flags():
    from footprints_amd.options import Options
    from footprints_amd.preprocessing.segmentation.options import SegmentationOptions
    opt = Options().parse(["--mode", "inference", "--device_decode", "--device_jpeg", "--save_test_visualisations"])
    assert opt.device_decode is True and opt.device_jpeg is True and opt.mode == "inference"
    off = Options().parse(["--mode", "inference"])
    assert getattr(off, "device_decode", False) is False and getattr(off, "device_jpeg", False) is False
    seg = SegmentationOptions().parse(["--mode", "inference", "--device_decode"])
    assert seg.device_decode is True and seg.device_jpeg is False
    assert SegmentationOptions().parse(["--mode", "inference"]).device_decode is False


def test_inference_mode_reads_config_and_split(tmp_path, monkeypatch):
    """`main --mode inference` no longer exits: it gets as far as the files the reference reads, relative to the working directory"""
    from footprints_amd.main import main
    monkeypatch.chdir(tmp_path)
    with pytest.raises(FileNotFoundError, match="paths.yaml"):
        main(["--mode", "inference", "--load_path", str(tmp_path)])
    (tmp_path / "paths.yaml").write_text("kitti:\n  dataset: %s\n" % (tmp_path / "raw"))
    with pytest.raises(FileNotFoundError, match="test.txt"):
        main(["--mode", "inference", "--load_path", str(tmp_path)])


# ---- the decode stage's host half ------------------------------------------------------------------------------------------------------
class _Event:
    def record(self):
        pass

    def query(self):
        return True


def _fake_stage(B, H, W, decode, status):
    """a DecodeStage whose "device" is host memory: uploads are copies, the decode launch is recorded, the status is injected"""
    from footprints_amd import ops
    from footprints_amd.datasets.decode_stage import DecodeStage

    class Fake(DecodeStage):
        def __init__(self):
            super().__init__(B, H, W, ops.ResizeTableSet("cpu"), "cpu", decode=decode)
            self.uploads, self.launches = [], []

        def _pinned(self, n, dtype):
            return torch.zeros(n, dtype=dtype)

        def _event(self):
            return _Event()

        def _upload(self, s, off, nbytes):
            self.uploads.append((off, nbytes))
            super()._upload(s, off, nbytes)

        def _decode(self, s, pack, batch):
            self.launches.append(pack)

        def _status(self, s, nd):
            return np.asarray(status[:nd])

    return Fake()


def _batch_files():
    from PIL import Image
    photo, grey = G.photo(70, 231, 1), np.asarray(Image.fromarray(G.photo(75, 248, 2)).convert("L"))
    buf, png = io.BytesIO(), io.BytesIO()
    Image.fromarray(G.photo(33, 45, 3)).save(buf, format="JPEG", progressive=True)
    Image.fromarray(G.photo(21, 17, 4)).save(png, format="PNG")
    return [G.write(photo, 95, 2), G.write(grey, 90), buf.getvalue(), png.getvalue()]


def test_decode_stage_host_half(tmp_path):
    from footprints_amd import _lib, ops
    from footprints_amd.datasets.decode_stage import host_decode, read_sample
    H, W = 64, 96
    files = _batch_files()
    paths = []
    for i, f in enumerate(files):
        paths.append(str(tmp_path / ("%d.%s" % (i, "png" if i == 3 else "jpg"))))
        with open(paths[-1], "wb") as fh:
            fh.write(f)
    frames = [G.pillow_decode(f) for f in files]
    calls = []

    def decode(data):
        calls.append(data)
        return host_decode(data)

    samples = [read_sample(p, True, decode) for p in paths]
    assert ["image" in s for s in samples] == [False, False, True, True] and calls == files[2:]            # parser's verdicts; Pillow at once
    assert "refused" in samples[2] and "refused" in samples[3]
    stage = _fake_stage(4, H, W, decode, status=[0, 2])
    s = stage.new_slot()
    stage.queue(s, samples)
    # the layout: ops.resize_pack of the Pillow-decoded frames -- offsets, records, sizes
    packed, records, total, Cn, max_h, max_w = ops.resize_pack(frames, H, W, stage.tables)
    batch = s["batch"]
    assert (batch["total"], batch["max_h"], batch["max_w"], Cn) == (total, max_h, max_w, 3)
    assert np.array_equal(s["h_rec"].numpy()[:records.size], records)
    rec = (_lib.ResizeSample * 4).from_buffer_copy(records.tobytes())
    assert batch["offsets"] == [r.offset for r in rec] and batch["shapes"] == [f.shape[:2] for f in frames]
    # which file goes where: the two host frames lie in the pinned buffer and are uploaded; the two others are one decode launch
    assert batch["on_device"] == [0, 1] and batch["on_host"] == [2, 3]
    for b in (2, 3):
        off = batch["offsets"][b]
        assert np.array_equal(s["h_src"].numpy()[off:off + frames[b].size], frames[b].reshape(-1))
        assert np.array_equal(s["d_src"].numpy()[off:off + frames[b].size], frames[b].reshape(-1))
    assert stage.uploads == [(batch["offsets"][2], 33 * 45 * 3), (batch["offsets"][3], 21 * 17 * 3)]
    assert len(stage.launches) == 1
    pack = stage.launches[0]
    assert pack["B"] == 2 and pack["shapes"] == [(70, 231), (75, 248)]
    drec = (_lib.JpegDecodeSample * 2).from_buffer_copy(pack["records"].numpy().tobytes())
    assert [r.out_offset for r in drec] == batch["offsets"][:2]          # out_offsets = the layout's
    assert stage.counters == dict(device=0, host_parser=2, host_status=0) and len(calls) == 2
    # finish with the injected status [0, 2]: exactly the flagged sample is decoded by Pillow and uploaded to its offset
    d = stage.finish(s)
    assert d["status"] == [0, 2, -1, -1] and calls[2:] == [files[1]]
    assert stage.counters == dict(device=1, host_parser=2, host_status=1)
    assert stage.uploads[2:] == [(batch["offsets"][1], 75 * 248 * 3)]
    off = batch["offsets"][1]
    assert np.array_equal(s["d_src"].numpy()[off:off + frames[1].size], frames[1].reshape(-1))
    assert (d["total"], d["n"], d["max_h"], d["max_w"]) == (total, 4, max_h, max_w) and d["src"] is s["d_src"] and d["records"] is s["d_rec"]
    assert d["shapes"] == [f.shape[:2] for f in frames]
    with pytest.raises(RuntimeError):
        stage.finish(s)                                               # nothing queued
    # every status 0: the host decodes nothing more
    stage2 = _fake_stage(4, H, W, decode, status=[0, 0])
    s2 = stage2.new_slot()
    stage2.queue(s2, samples[:2])
    before = len(calls)
    assert stage2.finish(s2)["status"] == [0, 0] and len(calls) == before and stage2.counters == dict(device=2, host_parser=0, host_status=0)
    # every frame decoded by the host, as without --device_decode: ONE upload of the bytes in use, no launch, nothing counted
    stage3 = _fake_stage(4, H, W, decode, status=[])
    s3 = stage3.new_slot()
    stage3.queue(s3, [{"image": f} for f in frames])
    assert stage3.uploads == [(0, total)] and stage3.launches == [] and s3["batch"]["on_device"] == []
    assert np.array_equal(s3["h_rec"].numpy()[:records.size], records)
    for f, off in zip(frames, s3["batch"]["offsets"]):
        assert np.array_equal(s3["d_src"].numpy()[off:off + f.size], f.reshape(-1))
    assert np.array_equal(s3["d_src"].numpy()[:total], packed[:total])
    d3 = stage3.finish(s3)
    assert d3["status"] == [-1] * 4 and (d3["total"], d3["n"], d3["max_h"], d3["max_w"]) == (total, 4, max_h, max_w)
    assert stage3.uploads == [(0, total)] and len(calls) == before and stage3.counters == dict(device=0, host_parser=0, host_status=0)


def test_decode_stage_limits_and_errors(tmp_path):
    from footprints_amd.datasets.decode_stage import host_decode, read_sample
    stage = _fake_stage(2, 8, 8, host_decode, status=[3])
    s = stage.new_slot()
    with pytest.raises(ValueError, match="1 to 2"):
        stage.queue(s, [])
    wide = {"path": "wide.jpg", "image": np.zeros((1, 21843, 3), np.uint8)}                  # 21843 * 3 = 65529 > 65528
    with pytest.raises(ValueError, match="wide.jpg"):
        stage.queue(s, [wide])
    stage.queue(s, [{"path": "fits.jpg", "image": np.zeros((1, 21842, 3), np.uint8)}])
    assert stage.finish(s)["status"] == [-1]
    # a file the device turns down (status 3) and the host decoder cannot read either: its exception, with the path in the message
    good = G.write(G.photo(16, 16, 1), 90, 2)
    path = tmp_path / "cut.jpg"
    path.write_bytes(good)
    def refuse(data):
        raise OSError("image file is truncated")

    stage.decode = refuse
    stage.queue(s, [read_sample(str(path), True)])
    with pytest.raises(OSError, match="cut.jpg: image file is truncated"):
        stage.finish(s)
    bad = tmp_path / "bad.png"
    bad.write_bytes(b"not a picture")
    with pytest.raises(Exception, match="bad.png"):
        read_sample(str(bad), True)


# ---- the restatement of fp_infer_pack --------------------------------------------------------------------------------------------------
def test_infer_pack_restatement_is_made_of_the_existing_ones():
    pred, image = IR.inputs(2, 6, 8, seed=1)
    c0, c1 = np.array([13, 8, 135], np.uint8), np.array([240, 249, 33], np.uint8)
    half, pic = IR.pack(pred, image, c0, c1)
    assert half.dtype == np.float16 and half.shape == (2, 4, 6, 8) and pic.shape == (2, 6, 16, 3)
    assert np.array_equal(half[:, :2], SR.to_half(SR.sigmoid64(pred[:, :2]).astype(np.float32)))
    assert np.array_equal(half[:, 2:], pred[:, 2:].astype(np.float16))
    assert np.array_equal(pic, VR.side_by_side(image, pred, c0, c1))
    assert IR.pack(pred, None, c0, c1)[1] is None
    # the planted values are there, and do what they are planted for
    flat = pred[:, 1].reshape(-1)
    right = pic[:, :, 8:].reshape(-1, 3)
    for v, colour in ((1e-8, c1), (-1e-8, c0), (0.0, c0)):
        at = np.flatnonzero(flat == np.float32(v))
        assert at.size >= 1 and (right[at] == colour).all()
        assert (half[:, 1].reshape(-1)[at] == np.float16(0.5)).all()
    assert np.signbit(pred[:, :2]).sum() > 0 and (pred[:, :2] == 0).sum() >= 4              # both zeros in both channels
    sub = half[:, :2][(half[:, :2] > 0) & (half[:, :2] < np.float16(6.104e-5))]
    assert sub.size >= 5                                                                   # float16 subnormals
    for v, h in ((20.0, 1.0), (88.0, 1.0), (104.0, 1.0), (-20.0, 0.0), (-88.0, 0.0), (-104.0, 0.0)):
        assert (half[:, :2][pred[:, :2] == np.float32(v)] == np.float16(h)).all() and (pred[:, :2] == np.float32(v)).sum() >= 2
    # exact float16 ties among the depth channels: the float32 value lies exactly between two float16 neighbours
    d = pred[:, 2:].astype(np.float64)
    lo = d.astype(np.float16)
    other = np.where(lo.astype(np.float64) < d, np.nextafter(lo, np.float16(2)), np.nextafter(lo, np.float16(-2))).astype(np.float64)
    ties = (lo.astype(np.float64) != d) & (np.abs(d - lo.astype(np.float64)) == np.abs(d - other))
    assert ties.sum() >= 20 and d.min() >= 0 and d.max() <= 1
