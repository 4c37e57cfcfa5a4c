"""GPU: training with --device_decode.  fp_label_resize's uint16 / pil_nearest records against the numpy gather, the batch assembler fed
JPEG files against the same batches fed Pillow-decoded frames (KITTI, Matterport, the fallback, the ring of a DeviceLoader), and
`--mode train` with and without the flag.  No tolerance anywhere: np.array_equal / torch.equal on the bits.  The JPEG content is the
catalogue of tests/test_train_decode_cpu.py, which checks on the decoder's CPU model that every frame settles well inside the budget."""
import os
import random

import numpy as np
import pytest
import torch

from tests import label_resize_restatement as LR
from tests.golden import make_golden_jpeg_decode as G
from tests.test_gpu_jpeg_decode import noise_frame
from tests.test_gpu_label_resize import bits_equal
from tests.test_train_decode_cpu import (KITTI_BATCH, frame_file, pil_nearest_statement, progressive_file, write_matterport_tree,
                                         write_photo_kitti_tree)

pytestmark = pytest.mark.gpu

SCALE = 0.25e-3


# ---- fp_label_resize: FP_LABEL_U16, FP_LABEL_PIL_NEAREST --------------------------------------------------------------------------------------
def _depth(rng, h, w):
    m = rng.integers(0, 65536, (h, w)).astype(np.uint16)
    m[0, 0], m[-1, -1], m[0, -1] = 0, 65535, 65535
    return m


@pytest.mark.parametrize("src,dst,flip", [((5, 7), (32, 32), False), ((70, 45), (64, 32), False), ((37, 53), (32, 64), True),
                                          ((1024, 1280), (512, 640), False)])
def test_uint16_pil_nearest_records_in_a_mixed_launch_equal_the_numpy_gather(src, dst, flip):
    """A launch has ONE target size, so each of the four records gets a launch of its own at its target, mixed with: the same map with the
    other flip, a flipped uint16 map at twice the target (an even ratio: the only kind at which "resize, then flip" and "flip, then resize"
    differ -- tests/test_train_decode_cpu.py), a uint8 / area record and a float32 / nearest record against the cv2 restatement."""
    from footprints_amd import ops
    (h, w), (H, W) = src, dst
    rng = np.random.default_rng(h * 7 + w)
    m, twice = _depth(rng, h, w), _depth(rng, 2 * H, 2 * W)
    area = rng.integers(0, 256, (2 * H, 3 * W), dtype=np.uint8)
    near = rng.random((H + 5, W + 3)).astype(np.float32)
    maps = [m, m, twice, area, near]
    methods = ["pil_nearest", "pil_nearest", "pil_nearest", "area", "nearest"]
    flips = [flip, not flip, True, True, False]
    mults = [SCALE, SCALE, SCALE, 1.0, 2.5]
    got = ops.label_resize(maps, H, W, methods, flips, mults)
    torch.cuda.synchronize()
    assert got.dtype == torch.float64 and tuple(got.shape) == (5, H, W)
    got = got.cpu().numpy()
    for j in range(3):
        final = pil_nearest_statement(maps[j], H, W, flips[j]).astype(np.float64) * SCALE       # what the batch holds after the flip ...
        assert bits_equal(got[j], final[:, ::-1] if flips[j] else final), (j, src, dst, flips[j])          # ... the kernel stores mirrored
    other = pil_nearest_statement(twice[:, ::-1], H, W, False).astype(np.float64) * SCALE                 # flip first, resize then: not this
    assert not np.array_equal(got[2][:, ::-1], other)
    assert got[0].min() == 0.0 and got[0].max() == 65535 * SCALE
    ref = LR.label_resize(area, H, W, "area", True, 1.0)
    assert bits_equal(got[3], ref[:, ::-1]) and bits_equal(got[4], LR.label_resize(near, H, W, "nearest", False, 2.5))


def test_a_uint16_record_outside_the_buffer_is_turned_down_and_its_neighbours_are_written():
    from footprints_amd import _lib, ops
    H, W = 32, 64
    rng = np.random.default_rng(3)
    maps = [_depth(rng, 37, 53), _depth(rng, 37, 53), _depth(rng, 16, 20)]
    ref = np.stack([pil_nearest_statement(m, H, W, False).astype(np.float64) * SCALE for m in maps])
    tables = ops.label_table_set("cuda")
    packed, records, total, _ = ops.label_resize_pack(maps, H, W, "pil_nearest", False, SCALE, tables=tables)
    src = torch.from_numpy(packed).cuda()

    def run(change):
        rec = (_lib.LabelSample * 3).from_buffer_copy(records.tobytes())
        change(rec[1])
        d_rec = torch.from_numpy(np.frombuffer(bytes(rec), dtype=np.uint8).copy()).cuda()
        out = torch.full((3, H, W), -7.0, dtype=torch.float64, device="cuda")
        try:
            ops.label_resize_packed(src, total, d_rec, 3, H, W, tables, out=out, check=True)
            raised = False
        except ValueError:
            raised = True
        return raised, out.cpu().numpy()
    raised, out = run(lambda r: None)
    assert not raised and bits_equal(out, ref)
    for change in (lambda r: setattr(r, "offset", total - 8), lambda r: setattr(r, "offset", 2), lambda r: setattr(r, "h", 38 + 16),
                   lambda r: setattr(r, "dtype", 5), lambda r: setattr(r, "method", 4)):
        raised, out = run(change)
        assert raised and bits_equal(out[0], ref[0]) and bits_equal(out[2], ref[2]) and (out[1] == -7.0).all()
    raised, out = run(lambda r: None)
    assert not raised and bits_equal(out, ref)


# ---- the assembler ----------------------------------------------------------------------------------------------------------------------------
def _kitti_maps(rng, mh, mw, mask=True):
    return {"visible_ground": rng.random((mh, mw)).astype(np.float16),
            "ground_depth": (rng.random((mh, mw)) * 30 * (rng.random((mh, mw)) < 0.5)).astype(np.float32),
            "depth_mask": (rng.random((mh, mw)) < 0.3).astype(np.uint8) if mask else None,
            "disparity": (rng.random((mh, mw)) * 60).astype(np.float32), "moving_objects": rng.random((mh, mw)) < 0.2}


def _files(tmp_path, files, decode=None):
    """the files on disk, read the way a reader thread under device_decode reads them"""
    from footprints_amd.datasets.decode_stage import host_decode, read_sample
    out = []
    for j, data in enumerate(files):
        p = tmp_path / ("%d_%d.jpg" % (len(os.listdir(tmp_path)), j))
        p.write_bytes(data)
        out.append(read_sample(str(p), True, decode or host_decode))
    return out


def _assemblers(B, H, W, max_src_hw, max_map_hw, dataset="kitti", slots=3, decode=None):
    from footprints_amd.datasets import DeviceBatchAssembler
    kw = dict(dataset=dataset, raw_images=True, max_src_hw=max_src_hw, filter_depth_mask=True, raw_maps=True, max_map_hw=max_map_hw, check=True,
              slots=slots)
    return DeviceBatchAssembler(B, H, W, device_decode=True, decode=decode, **kw), DeviceBatchAssembler(B, H, W, **kw)


def _params(n, seed, flips):
    from footprints_amd.datasets.device_path import draw_augmentation, draw_jitter
    rng = random.Random(seed)
    params = [draw_augmentation(True, rng) for _ in range(n)]
    for p, f in zip(params, flips):
        p.flip = f
    draw_jitter(params[1], rng=rng)                                      # at least one colour jitter, whatever the draws said
    return params


def _batch(asm, samples, params):
    out = asm.collect(asm.submit(samples, params))
    torch.cuda.synchronize()
    return {k: v.clone() for k, v in out.items()}


def _equal(a, b, what):
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]), (what, k)


def test_kitti_batch_from_files_equals_the_batch_from_decoded_frames(tmp_path):
    B, H, W = 4, 64, 128
    rng = np.random.default_rng(31)
    files = [frame_file(n) for n in KITTI_BATCH]
    maps = [_kitti_maps(rng, 70, 150), _kitti_maps(rng, 96, 200, mask=False), _kitti_maps(rng, 128, 256), _kitti_maps(rng, 64, 128)]
    dev, plain = _assemblers(B, H, W, (56, 176), (128, 256))
    params = _params(B, 4, (1, 0, 0, 1))
    assert any(p.flip for p in params) and any(p.n_ops for p in params)
    got = _batch(dev, list(zip(_files(tmp_path, files), maps)), params)
    decoded = [G.pillow_decode(f) for f in files]
    assert [d.shape[:2] for d in decoded] == [(48, 160), (50, 168), (56, 176), (52, 164)]
    _equal(got, _batch(plain, list(zip(decoded, maps)), params), "against today's path")
    assert dev.counters == dict(device=4, host_parser=0, host_status=0)
    _equal(got, _batch(dev, list(zip(decoded, maps)), params), "the same assembler, fed decoded frames")
    assert dev.counters == dict(device=4, host_parser=0, host_status=0) and plain.counters == dict(device=0, host_parser=0, host_status=0)
    assert float(got["image"].std()) > 0.05
    with pytest.raises(ValueError, match="larger than max_src_hw"):      # by the header's size, by name, at fill time
        small = _assemblers(B, H, W, (55, 176), (128, 256), slots=1)[0]
        small.fill(list(zip(_files(tmp_path, files), maps)), params)
    with pytest.raises(ValueError, match="raw_images"):
        from footprints_amd.datasets import DeviceBatchAssembler
        DeviceBatchAssembler(B, H, W, device_decode=True)


def test_what_the_device_turns_down_goes_through_the_host_decoder_and_the_slot_works_on(tmp_path):
    from footprints_amd.datasets.decode_stage import host_decode
    B, H, W = 4, 64, 128
    rng = np.random.default_rng(37)
    seen = []

    def decode(data):
        seen.append(data)
        return host_decode(data)

    files = [progressive_file(), frame_file("48x160"), noise_frame(), frame_file("70x150")]
    maps = [_kitti_maps(rng, 70, 150) for _ in files]
    dev, plain = _assemblers(B, H, W, (96, 176), (70, 150), slots=1, decode=decode)
    params = _params(B, 9, (0, 1, 1, 0))
    got = _batch(dev, list(zip(_files(tmp_path, files, decode), maps)), params)
    _equal(got, _batch(plain, list(zip([G.pillow_decode(f) for f in files], maps)), params), "fallback")
    assert dev.counters == dict(device=2, host_parser=1, host_status=1)
    assert seen == [files[0], files[2]]                                  # the progressive file on the reader, the noise after its status 2
    files2 = [frame_file(n) for n in KITTI_BATCH]                        # the next batch through the same slot
    got2 = _batch(dev, list(zip(_files(tmp_path, files2), maps)), params)
    _equal(got2, _batch(plain, list(zip([G.pillow_decode(f) for f in files2], maps)), params), "after the fallback")
    assert dev.counters == dict(device=6, host_parser=1, host_status=1) and len(seen) == 2


def test_the_ring_of_a_loader_equals_its_host_fed_twin_and_stops_allocating_pinned_memory(tmp_path):
    from footprints_amd.datasets.device_path import DeviceLoader
    B, H, W, slots = 2, 64, 128, 2
    rng = np.random.default_rng(41)
    names = [("48x160", "50x168"), ("52x164", "70x150"), ("56x176", "48x160"), ("96x200", "128x256"), ("50x168", "52x164 grey")]
    assert len(names) == 2 * slots + 1
    maps = [[_kitti_maps(rng, 70, 150), _kitti_maps(rng, 64, 128, mask=False)] for _ in names]
    from_files = [list(zip(_files(tmp_path, [frame_file(n) for n in pair]), m)) for pair, m in zip(names, maps)]
    decoded = [list(zip([G.pillow_decode(frame_file(n)) for n in pair], m)) for pair, m in zip(names, maps)]
    dev, plain = _assemblers(B, H, W, (128, 256), (70, 150), slots=slots)
    pinned, packed = [], []
    pin, pack_into = dev.stage._pinned, dev.stage.pack_into
    dev.stage._pinned = lambda n, dtype: pinned.append(len(packed) - 1) or pin(n, dtype)
    dev.stage.pack_into = lambda s, batch: packed.append(1) or pack_into(s, batch)
    got = [{k: v.clone() for k, v in b.items()} for b in DeviceLoader(from_files, dev, is_train=True, rng=random.Random(7))]
    want = [{k: v.clone() for k, v in b.items()} for b in DeviceLoader(decoded, plain, is_train=True, rng=random.Random(7))]
    torch.cuda.synchronize()
    assert len(got) == len(want) == 5
    for k, (a, b) in enumerate(zip(got, want)):
        _equal(a, b, "batch %d" % k)
    assert dev.counters == dict(device=10, host_parser=0, host_status=0)
    # every slot allocates with its first batch, batch 3 (the large frames) makes its slot's scan buffer grow, and nothing allocates after it
    assert {0, 1} <= set(pinned) and 3 in pinned and max(pinned) == 3, pinned


def test_matterport_batch_from_files_equals_todays_path(tmp_path):
    from footprints_amd.datasets.training import MatterportReader
    B, H, W = 2, 64, 96
    frames = [("scanA", "p0", "1", "2", "80x100", (80, 100)), ("scanA", "p1", "0", "5", "80x100 b", (80, 100))]
    raw, train, lines = write_matterport_tree(str(tmp_path), frames, seed=43)
    today = MatterportReader(raw, train, lines, H, W)                    # Pillow decodes the frame and resizes the depth: float32 at 64 x 96
    flagged = MatterportReader(raw, train, lines, H, W, device_decode=True)
    dev, plain = _assemblers(B, H, W, (80, 100), (80, 100), dataset="matterport")
    params = _params(B, 11, (1, 0))
    a, b = [flagged[0], flagged[1]], [today[0], today[1]]
    assert a[0][1]["depth_raw"].dtype == np.uint16 and b[0][1]["depth_raw"].dtype == np.float32 and "bytes" in a[0][0]
    got = _batch(dev, a, params)
    _equal(got, _batch(plain, b, params), "matterport")
    assert dev.counters == dict(device=2, host_parser=0, host_status=0) and float(got["depth"].max()) > 0.0


# ---- the trainer ------------------------------------------------------------------------------------------------------------------------------
def test_main_trains_the_same_weights_with_and_without_device_decode(tmp_path, monkeypatch, capsys):
    from footprints_amd.main import main
    from footprints_amd.training import train as T
    seq = "2011_09_26/2011_09_26_drive_0001_sync"
    frames = [(seq, 3, "l", "48x160", (70, 150)), (seq, 4, "r", "50x168", (96, 200)), (seq, 17, "l", "56x176", (128, 256)),
              (seq, 18, "l", "52x164", (64, 128))]
    raw, train, lines, _ = write_photo_kitti_tree(str(tmp_path), frames, seed=3, skip_mask=(2,))
    os.makedirs(tmp_path / "splits" / "kitti")
    (tmp_path / "splits" / "kitti" / "train.txt").write_text("\n".join(lines) + "\n")
    (tmp_path / "splits" / "kitti" / "val.txt").write_text("\n".join(lines[:2]) + "\n")
    (tmp_path / "paths.yaml").write_text("kitti:\n  dataset: %s\n  training_data: %s\n" % (raw, train))
    monkeypatch.chdir(tmp_path)
    made = []
    orig = T.TrainManager.__init__

    def spy(self, *a, **k):
        orig(self, *a, **k)
        made.append(self)
    monkeypatch.setattr(T.TrainManager, "__init__", spy)
    for name, flag in (("plain", []), ("flagged", ["--device_decode"])):
        random.seed(5)
        main(["--mode", "train", "--epochs", "1", "--batch_size", "2", "--height", "64", "--width", "128", "--val_batches", "1", "--num_workers", "2",
              "--config_path", str(tmp_path / "paths.yaml"), "--log_path", str(tmp_path / "logs"), "--model_name", name, "--no_summaries"] + flag)
        torch.cuda.synchronize()
    plain, flagged = made
    said = [line for line in capsys.readouterr().out.splitlines() if "frames decoded so far" in line]
    assert said == ["Epoch 0 -- train frames decoded so far: device 4, host (parser) 0, host (status) 0",
                    "Epoch 0 -- val frames decoded so far: device 2, host (parser) 0, host (status) 0"]      # the flagged run's epoch, once
    assert plain.step == flagged.step == 2 and len(plain.history["train"]) == 1 and len(plain.history["val"]) == 1
    assert plain.history == flagged.history
    a, b = (torch.load(tmp_path / "logs" / name / "models" / "weights_0" / "model.pth", map_location="cpu") for name in ("plain", "flagged"))
    assert set(a) == set(b) and len(a) > 10
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert flagged.train_loader.counters == dict(device=4, host_parser=0, host_status=0)
    assert flagged.val_loader.counters == dict(device=2, host_parser=0, host_status=0)
    # the decoding loaders work on the engine's decoder weight-gradient stream, not on a fifth stream of their own
    dwg0 = flagged.train_step.eng.dwg[0].cuda_stream
    assert flagged.train_loader.asm.stream.cuda_stream == dwg0 == flagged.val_loader.asm.stream.cuda_stream
    eng = plain.train_step.eng
    assert plain.train_loader.asm.stream.cuda_stream not in [s.cuda_stream for s in (eng.aux, eng.wg, eng.dwg[0], eng.dwg[1])]
    assert plain.train_loader.counters == plain.val_loader.counters == dict(device=0, host_parser=0, host_status=0)
