"""CPU: the training readers under device_decode, the content of every JPEG the GPU tests expect the device to decode (so that "all decoded
on the device" there is a statement about the feature, not about the content), the order in which DeviceLoader and the decode stage queue
decodes and read their status -- with the device half stubbed at DecodeStage's seams, as tests/test_infer_pipeline_cpu.py does -- and the
flip rule of Pillow's NEAREST.  tests/test_gpu_train_decode.py imports the frame catalogue and the tree helpers from here."""
import functools
import io
import os

import numpy as np
import pytest
import torch

from tests import jpeg_decode_restatement as JR
from tests.golden import make_golden_jpeg_decode as G
from tests.test_label_resize_cpu import write_kitti_tree

# every JPEG the GPU tests expect the device to decode: name -> (h, w, quality, Pillow's subsampling, grey); content G.photo(h, w, 100 + h)
FRAMES = {"48x160": (48, 160, 90, 2, False), "50x168": (50, 168, 92, 2, False), "56x176": (56, 176, 95, 0, False),
          "52x164": (52, 164, 75, 1, False), "52x164 grey": (52, 164, 90, None, True), "70x150": (70, 150, 90, 2, False),
          "96x200": (96, 200, 95, 2, False), "128x256": (128, 256, 85, 0, False), "80x100": (80, 100, 90, 2, False),
          "80x100 b": (80, 100, 85, 0, False)}
KITTI_BATCH = ("48x160", "50x168", "56x176", "52x164 grey")


@functools.lru_cache(None)
def frame_file(name):
    """the JPEG file (bytes) of a catalogue frame"""
    from PIL import Image
    h, w, quality, sampling, grey = FRAMES[name]
    a = G.photo(h, w, 100 + h + (1 if name.endswith(" b") else 0))
    if grey:
        a = np.asarray(Image.fromarray(a).convert("L"))
    return G.write(a, quality, sampling)


def progressive_file(h=40, w=56, seed=7):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(G.photo(h, w, seed)).save(buf, format="JPEG", progressive=True)
    return buf.getvalue()


def write_photo_kitti_tree(root, frames, seed=0, skip_mask=()):
    """write_kitti_tree with picture-like frames: frames = [(seq, frame number, side, catalogue name or file bytes, (h, w) of the maps)]
    -> (raw path, training-data path, split lines, [path of every JPEG])"""
    files = [frame_file(f[3]) if isinstance(f[3], str) else f[3] for f in frames]
    shapes = [G.pillow_decode(f).shape[:2] for f in files]
    raw, train, lines = write_kitti_tree(root, [(seq, n, side, hw, mhw) for (seq, n, side, _, mhw), hw in zip(frames, shapes)], seed, skip_mask)
    paths = []
    for (seq, n, side, _, _), data in zip(frames, files):
        paths.append(os.path.join(raw, seq, "image_02" if side == "l" else "image_03", "data", str(n).zfill(10) + ".jpg"))
        with open(paths[-1], "wb") as fh:                                # over the helper's uniform noise
            fh.write(data)
    return raw, train, lines, paths


def write_matterport_tree(root, frames, seed=0):
    """a small Matterport tree: frames = [(scan, pos, height, direction, catalogue name, (h, w) of the depth PNG and the maps)], the depth a
    16-bit PNG that holds 0 and 65535 -> (raw path, training-data path, split lines)"""
    from PIL import Image
    rng = np.random.default_rng(seed)
    raw, train = os.path.join(root, "raw"), os.path.join(root, "training_data")
    lines = []
    for scan, pos, height, direction, name, (mh, mw) in frames:
        for sub in ("matterport_color_images", "matterport_depth_images"):
            os.makedirs(os.path.join(raw, scan, scan, sub), exist_ok=True)
        with open(os.path.join(raw, scan, scan, "matterport_color_images", "%s_i%s_%s.jpg" % (pos, height, direction)), "wb") as fh:
            fh.write(frame_file(name))
        depth = rng.integers(0, 65536, (mh, mw)).astype(np.uint16)
        depth[0, 0], depth[-1, -1] = 0, 65535
        Image.fromarray(depth).save(os.path.join(raw, scan, scan, "matterport_depth_images", "%s_d%s_%s.png" % (pos, height, direction)))
        maps = {"ground_seg": rng.random((mh, mw)).astype(np.float16),
                "hidden_depth": (rng.random((mh, mw)) * 30 * (rng.random((mh, mw)) < 0.5)).astype(np.float32),
                "depth_masks": (rng.random((mh, mw)) < 0.1).astype(np.uint8)}
        for kind, arr in maps.items():
            os.makedirs(os.path.join(train, kind, scan, "data"), exist_ok=True)
            np.save(os.path.join(train, kind, scan, "data", "%s_%s_%s.npy" % (pos, height, direction)), arr)
        lines.append("%s %s %s %s" % (scan, pos, height, direction))
    return raw, train, lines


def pil_nearest_statement(m, H, W, flip):
    """numpy: Image.fromarray(m).resize((W, H), NEAREST), then transpose(FLIP_LEFT_RIGHT) when flip (footprint_dataset.py:73-80): the
    resize comes FIRST, so final column x holds source column index[W - 1 - x]"""
    h, w = m.shape
    iy = np.minimum(np.floor((np.arange(H) + 0.5) * h / H).astype(np.int64), h - 1)
    ix = np.minimum(np.floor((np.arange(W) + 0.5) * w / W).astype(np.int64), w - 1)
    if flip:
        ix = ix[W - 1 - np.arange(W)]
    return m[iy][:, ix]


# ---- readers --------------------------------------------------------------------------------------------------------------------------------
def _same_maps(a, b):
    assert set(a) == set(b)
    for k in a:
        assert (a[k] is None and b[k] is None) or (a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k])), k


def test_kitti_reader_hands_over_bytes_or_a_refused_frame(tmp_path):
    from footprints_amd.datasets.training import KITTIReader
    seq = "2011_09_26/drive_0001_sync"
    frames = [(seq, 3, "l", "48x160", (70, 150)), (seq, 12, "r", "56x176", (96, 200)), (seq, 13, "r", progressive_file(), (64, 128))]
    raw, train, lines, paths = write_photo_kitti_tree(str(tmp_path), frames, skip_mask=(1,))
    plain = KITTIReader(raw, train, lines, 64, 128, is_train=True)
    dev = KITTIReader(raw, train, lines, 64, 128, is_train=True, device_decode=True)
    assert plain.device_decode is False and dev.device_decode is True
    for i, (h, w) in enumerate(((48, 160), (56, 176))):
        smp, maps = dev[i]
        img, ref_maps = plain[i]
        assert set(smp) == {"path", "bytes", "info"} and smp["path"] == paths[i] == dev.paths(i)["image"]
        assert smp["bytes"] == frame_file(frames[i][3]) and smp["info"]["device"] and (smp["info"]["h"], smp["info"]["w"]) == (h, w) == img.shape[:2]
        _same_maps(maps, ref_maps)
        assert dev.paths(i) == plain.paths(i)
    smp, maps = dev[2]                                                   # progressive: Pillow at once, on the reader thread
    assert set(smp) == {"path", "image", "refused"} and smp["refused"] and np.array_equal(smp["image"], plain[2][0])
    _same_maps(maps, plain[2][1])
    assert dev[1][1]["depth_mask"] is None


def test_matterport_reader_hands_over_the_depth_png_as_stored(tmp_path):
    from PIL import Image
    from footprints_amd.datasets.training import MatterportReader
    frames = [("scanA", "p0", "1", "2", "80x100", (80, 100)), ("scanA", "p1", "0", "5", "80x100 b", (80, 100))]
    raw, train, lines = write_matterport_tree(str(tmp_path), frames)
    plain = MatterportReader(raw, train, lines, 64, 96)
    dev = MatterportReader(raw, train, lines, 64, 96, device_decode=True)
    for i in range(2):
        smp, maps = dev[i]
        img, ref_maps = plain[i]
        assert set(smp) == {"path", "bytes", "info"} and (smp["info"]["h"], smp["info"]["w"]) == (80, 100) == img.shape[:2]
        stored = np.asarray(Image.open(dev.paths(i)["depth_raw"]))
        assert stored.dtype == np.uint16 and stored.min() == 0 and stored.max() == 65535
        assert maps["depth_raw"].dtype == np.uint16 and maps["depth_raw"].shape == (80, 100) and np.array_equal(maps["depth_raw"], stored)
        assert ref_maps["depth_raw"].dtype == np.float32 and ref_maps["depth_raw"].shape == (64, 96)
        # ... and the device's rule applied to it is what the reader thread computes without the flag
        assert np.array_equal(pil_nearest_statement(stored, 64, 96, False).astype(np.float32), ref_maps["depth_raw"])
        _same_maps({k: v for k, v in maps.items() if k != "depth_raw"}, {k: v for k, v in ref_maps.items() if k != "depth_raw"})
        assert dev.paths(i) == plain.paths(i)


# ---- content guard --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(FRAMES))
def test_catalogue_frames_settle_well_inside_the_decoders_budget(name):
    from footprints_amd import ops
    data = frame_file(name)
    info = ops.jpeg_parse(data)
    assert info["device"] and (info["h"], info["w"]) == FRAMES[name][:2]
    m = JR.model(data, ops.JPEG_DECODE_SUBSEQ_BITS)
    print(name, "launches", m["launches"], "hops", m["hops"], "nsub", m["nsub"])
    assert m["launches"] <= ops.JPEG_DECODE_MAX_ROUNDS / 2 and m["hops"] < JR.GROUP


def test_some_catalogue_frames_span_more_than_one_workgroup():
    from footprints_amd import ops
    assert sum(JR.model(frame_file(n), ops.JPEG_DECODE_SUBSEQ_BITS)["nsub"] > JR.GROUP for n in ("96x200", "128x256", "56x176", "70x150")) >= 2


# ---- ordering -------------------------------------------------------------------------------------------------------------------------------
class _Event:
    def record(self):
        pass

    def query(self):
        return True


def _fake_stage(B, H, W, decode, statuses, log):
    """a DecodeStage whose "device" is host memory; statuses: {batch number: [status per device sample]} (default: all 0); every queued
    decode, status read, upload and pinned allocation goes into `log` with the batch number its slot carries (s['k'])"""
    from footprints_amd import ops
    from footprints_amd.datasets.decode_stage import DecodeStage

    class Fake(DecodeStage):
        def __init__(self):
            super().__init__(B, H, W, ops.ResizeTableSet("cpu"), "cpu", decode=decode)

        def _pinned(self, n, dtype):
            log.append(("pinned", n))
            return torch.zeros(n, dtype=dtype)

        def _event(self):
            return _Event()

        def _upload(self, s, off, nbytes):
            log.append(("upload", s["k"], off, nbytes))
            super()._upload(s, off, nbytes)

        def _decode(self, s, pack, batch):
            log.append(("decode", s["k"], pack["B"]))

        def _status(self, s, nd):
            log.append(("status", s["k"]))
            return np.asarray(statuses.get(s["k"], [0] * nd)[:nd])

    return Fake()


class _FakeAssembler:
    """the three calls DeviceBatchAssembler makes into its decode stage (prepare in fill, launch in _launch, collect in collect), around
    slots that hold nothing else; the rest of a slot's chain is a log entry"""
    device_decode = True

    def __init__(self, stage, slots, log):
        self.stage, self.log, self.slots, self.filled = stage, log, [stage.new_slot() for _ in range(slots)], 0

    def fill(self, samples, params):
        i = self.filled % len(self.slots)
        self.slots[i]["k"] = self.filled
        self.log.append(("fill", self.filled))
        self.filled += 1
        self.stage.prepare(self.slots[i], samples)
        return i

    def launch(self, i):
        s = self.slots[i]
        self.stage.launch(s)
        self.log.append(("chain", s["k"]))

    def collect(self, i):
        s = self.slots[i]
        self.stage.collect(s, lambda: self.log.append(("chain again", s["k"])))
        self.log.append(("collected", s["k"]))
        return s["k"]

    def release(self, i):
        pass


def _samples(tmp_path, names):
    from footprints_amd.datasets.decode_stage import read_sample
    out = []
    for j, name in enumerate(names):
        p = tmp_path / ("%d.jpg" % j)
        p.write_bytes(frame_file(name))
        out.append(read_sample(str(p), True))
    return out


def test_no_status_is_read_before_the_next_decode_is_queued_and_the_ring_stops_allocating(tmp_path):
    from footprints_amd.datasets.decode_stage import host_decode
    from footprints_amd.datasets.device_path import DeviceLoader
    log, calls = [], []
    stage = _fake_stage(2, 64, 128, lambda data: calls.append(data) or host_decode(data), {}, log)
    asm = _FakeAssembler(stage, 2, log)
    batch = _samples(tmp_path, ("48x160", "50x168"))
    got = list(DeviceLoader([batch] * 5, asm, is_train=False))
    assert got == [0, 1, 2, 3, 4] and calls == []
    at = {e: n for n, e in enumerate(log) if e[0] in ("status", "collected", "fill")}
    queued = {e[1]: n for n, e in enumerate(log) if e[0] == "decode"}
    assert sorted(queued) == [0, 1, 2, 3, 4]
    for k in range(5):
        assert queued[k] < at[("status", k)] < at[("collected", k)]
        if k < 4:
            assert queued[k + 1] < at[("status", k)], (k, log)          # batch k + 1's decode is in the queue before k's status is looked at
    assert not [e for e in log if e[0] == "chain again"]
    assert stage.counters == dict(device=10, host_parser=0, host_status=0)
    second_turn = at[("fill", 2)]                                       # two slots: the ring's first turn ends where batch 2 is filled
    assert [e for e in log[:second_turn] if e[0] == "pinned"] and not [e for e in log[second_turn:] if e[0] == "pinned"]


def test_a_non_zero_status_sends_that_frame_to_the_host_decoder_before_the_batch_is_returned(tmp_path):
    from footprints_amd.datasets.decode_stage import host_decode
    from footprints_amd.datasets.device_path import DeviceLoader
    log, calls = [], []
    stage = _fake_stage(2, 64, 128, lambda data: calls.append(data) or host_decode(data), {2: [0, 2]}, log)
    asm = _FakeAssembler(stage, 2, log)
    batch = _samples(tmp_path, ("48x160", "50x168"))
    assert list(DeviceLoader([batch] * 4, asm, is_train=False)) == [0, 1, 2, 3]
    assert calls == [frame_file("50x168")]                              # exactly that frame, once
    off = 48 * 160 * 3
    n = [e for e in log if e[0] in ("status", "upload", "chain again", "collected") and e[1] == 2]
    assert n == [("status", 2), ("upload", 2, off, 50 * 168 * 3), ("chain again", 2), ("collected", 2)]
    assert np.array_equal(asm.slots[0]["d_src"].numpy()[off:off + 50 * 168 * 3], G.pillow_decode(frame_file("50x168")).reshape(-1))
    assert [e for e in log if e[0] == "chain again"] == [("chain again", 2)]
    assert stage.counters == dict(device=7, host_parser=0, host_status=1)


def test_a_frame_over_max_src_hw_is_refused_by_name(tmp_path):
    from footprints_amd import ops
    from footprints_amd.datasets.decode_stage import DecodeStage
    batch = _samples(tmp_path, ("48x160", "50x168"))
    stage = DecodeStage(2, 64, 128, ops.ResizeTableSet("cpu"), "cpu", max_hw=(48, 168))
    with pytest.raises(ValueError, match=r"1\.jpg: a frame of 50 x 168 is larger than max_src_hw"):
        stage.layout(batch)
    assert DecodeStage(2, 64, 128, ops.ResizeTableSet("cpu"), "cpu", max_hw=(50, 168)).layout(batch)[2] == (48 * 160 + 50 * 168) * 3


# ---- flip rule and pack ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,W,differ", [(53, 32, False), (64, 32, True), (1280, 640, True), (96, 32, False), (12, 8, False), (12, 6, True)])
def test_flipped_pil_nearest_is_resized_first_and_flipped_then(w, W, differ):
    """The numpy statement of the flipped resize against Pillow (resize, then transpose), and which sizes can tell "resize, then flip"
    (index[W - 1 - x]) from "flip, then resize" (w - 1 - index[x]).  floor(w - t) = w - 1 - floor(t) unless t is whole, so the two orders
    differ exactly at the columns where (x + 0.5) * w / W is a whole number: none at 53 -> 32 (53 * (2 x + 1) is odd, 64 is not), every
    one at an even ratio such as 64 -> 32 or Matterport's 1280 -> 640.  The sizes that differ are the ones that pin the order; 53 -> 32 is
    kept and pins the statement alone."""
    from PIL import Image
    from footprints_amd import ops
    h, H = 37, 32
    index = np.minimum(np.floor((np.arange(W) + 0.5) * w / W).astype(np.int64), w - 1)
    assert np.array_equal(index, ops.pil_nearest_axis(w, W)) and np.array_equal(index, ops.nearest_index(w, W))
    x = np.arange(W)
    whole = ((2 * x + 1) * w) % (2 * W) == 0
    assert np.array_equal(index[W - 1 - x] != w - 1 - index[x], whole) and bool(whole.any()) == differ
    m = np.random.default_rng(5).integers(0, 65536, (h, w)).astype(np.uint16)
    pil = Image.fromarray(m).resize((W, H), Image.NEAREST)
    assert np.array_equal(pil_nearest_statement(m, H, W, False), np.asarray(pil))
    assert np.array_equal(pil_nearest_statement(m, H, W, True), np.asarray(pil.transpose(Image.FLIP_LEFT_RIGHT)))
    other_order = np.asarray(Image.fromarray(m[:, ::-1].copy()).resize((W, H), Image.NEAREST))
    assert np.array_equal(pil_nearest_statement(m, H, W, True), other_order) == (not differ)


@pytest.mark.parametrize("src,dst", [((1024, 1280), (512, 640)), ((37, 53), (32, 64)), ((70, 45), (64, 32)), ((33, 47), (64, 96)), ((5, 7), (32, 32)),
                                     ((80, 100), (64, 96))])
def test_the_closed_form_equals_pillow_on_uint16(src, dst):
    from PIL import Image
    from footprints_amd import ops
    m = np.random.default_rng(src[0]).integers(0, 65536, src).astype(np.uint16)
    assert np.array_equal(pil_nearest_statement(m, dst[0], dst[1], False), np.asarray(Image.fromarray(m).resize((dst[1], dst[0]), Image.NEAREST)))
    for a, b in zip(src, dst):
        assert np.array_equal(ops.pil_nearest_axis(a, b), ops.nearest_index(a, b))


def test_pack_takes_uint16_maps_and_the_method_name():
    from footprints_amd import _lib, ops
    tables = ops.LabelTableSet("cuda:0")                                 # host work only
    m = np.arange(5 * 7, dtype=np.uint16).reshape(5, 7) * 1000
    packed, records, used, _ = ops.label_resize_pack([m, m.astype(np.float32)], 32, 32, ["pil_nearest", "nearest"], [True, False], [0.25e-3, 1.0],
                                                     tables=tables)
    rec = (_lib.LabelSample * 2).from_buffer_copy(records.tobytes())
    assert (rec[0].h, rec[0].w, rec[0].dtype, rec[0].method, rec[0].flip) == (5, 7, _lib.LABEL_U16, _lib.LABEL_PIL_NEAREST, 1)
    assert (_lib.LABEL_U16, _lib.LABEL_PIL_NEAREST) == (4, 3) and rec[0].multiplier == 0.25e-3 and rec[1].offset == 72 and used == 72 + 144
    assert np.array_equal(packed[:70].view(np.uint16).reshape(5, 7), m)
    assert ops.label_pack_bytes([m]) == 72 and ops.label_source_itemsize(m) == 2
    assert len(tables.records) == 0                                      # a gather: no table
