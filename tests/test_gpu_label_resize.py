"""GPU: fp_label_resize (csrc/label_resize.hip) bit for bit against the numpy restatement of OpenCV's resize
(tests/label_resize_restatement.py, pinned by tests/test_label_resize_cpu.py), the assembler's raw_maps path against the host-fed path, and
`--mode train` from a folder.  No tolerance anywhere: every comparison is np.array_equal / torch.equal on the float64 bits."""
import functools
import os
import random

import numpy as np
import pytest
import torch

from tests import label_resize_restatement as LR
from tests.test_label_resize_cpu import write_kitti_tree

pytestmark = pytest.mark.gpu


def bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))


def gpu_label_resize(maps, H, W, method, flip=False, multiplier=1.0):
    from footprints_amd import ops
    out = ops.label_resize(maps, H, W, method, flip, multiplier)
    torch.cuda.synchronize()
    assert out.dtype == torch.float64 and tuple(out.shape) == (len(maps), H, W)
    return out.cpu().numpy()


@functools.lru_cache(None)
def mixed_call():
    """one call at H, W = 8, 16 with B = 3 'samples' of 5 maps: general 37 x 61, integer 2 x 3 from 16 x 48, copy 8 x 16, all four stored
    dtypes, both methods, flip on and off, the disparity multiplier, a zero record -> (maps, methods, flips, multipliers, reference)"""
    H, W = 8, 16
    rng = np.random.default_rng(11)
    sizes = [(37, 61), (16, 48), (8, 16)]
    maps, methods, flips, mults = [], [], [], []
    for k, (method, dtypes) in enumerate((("area", (np.float16, np.float32, np.float64)), ("area", (np.float64, np.float16, np.float32)),
                                          ("nearest", (np.uint8, np.bool_, np.uint8)), ("area", (np.float32, np.float64, np.float16)),
                                          ("nearest", (np.uint8, np.float32, np.float64)))):
        for b, dt in enumerate(dtypes):
            h, w = sizes[(b + k) % 3]
            m = rng.random((h, w)) * (60.0 if k == 3 else 1.0)
            m = (m < 0.3) if dt == np.bool_ else (m < 0.3).astype(dt) if method == "nearest" else m.astype(dt)
            maps.append(None if (k, b) == (2, 2) else m)
            methods.append("zero" if (k, b) == (4, 0) else method)
            flips.append(b == 1 or (k, b) == (0, 2))
            mults.append(W / w if k == 3 else 1.0)
    ref = np.stack([LR.label_resize(m, H, W, me, f, mu) for m, me, f, mu in zip(maps, methods, flips, mults)])
    for j, f in enumerate(flips):                                        # a flipped record stores mirrored
        if f:
            ref[j] = ref[j][:, ::-1]
    ref.setflags(write=False)
    return maps, methods, flips, mults, ref


def test_one_mixed_call_equals_the_restatement_bit_for_bit():
    maps, methods, flips, mults, ref = mixed_call()
    assert {None if m is None else m.dtype.name for m in maps} == {None, "bool", "uint8", "float16", "float32", "float64"}
    assert {(m.shape, me) for m, me in zip(maps, methods) if m is not None} >= {((37, 61), "area"), ((16, 48), "area"), ((8, 16), "area"),
                                                                                ((37, 61), "nearest")}
    got = gpu_label_resize(maps, 8, 16, methods, flips, mults)
    for j in range(len(maps)):
        assert bits_equal(got[j], ref[j]), (j, methods[j], flips[j], None if maps[j] is None else (maps[j].shape, maps[j].dtype))
    assert maps[8] is None and methods[12] == "zero" and not got[8].any() and not got[12].any()                        # the None map and the 'zero' record
    assert bits_equal(gpu_label_resize(maps, 8, 16, methods, flips, mults), got)


@pytest.mark.parametrize("src,dst", [((7, 11), (3, 4)), ((13, 29), (5, 8)), ((9, 10), (8, 9))])
def test_small_targets_with_one_to_three_entries_per_output(src, dst):
    """targets narrower than a wave, 1 - 5 entries per output index"""
    (h, w), (H, W) = src, dst
    rng = np.random.default_rng(h + w)
    maps = [rng.random((h, w)) * 80.0, rng.standard_normal((h, w)).astype(np.float32), rng.random((h, w)).astype(np.float16),
            rng.integers(0, 256, (h, w), dtype=np.uint8)]
    for flip in (False, True):
        for method in ("area", "nearest"):
            got = gpu_label_resize(maps, H, W, method, flip)
            for j, m in enumerate(maps):
                ref = LR.label_resize(m, H, W, method, flip)
                assert bits_equal(got[j], ref[:, ::-1] if flip else ref), (j, method, flip)


def test_kitti_size_float16_map_equals_the_restatement():
    rng = np.random.default_rng(17)
    m = (rng.random((375, 1242)) * 60.0).astype(np.float16)
    got = gpu_label_resize([m, m], 192, 640, "area", [False, True], 640 / 1242)
    ref = LR.label_resize(m, 192, 640, "area", False, 640 / 1242)
    assert bits_equal(got[0], ref)
    assert bits_equal(got[1], LR.label_resize(m, 192, 640, "area", True, 640 / 1242)[:, ::-1])
    assert np.abs(got[1] - got[0]).max() < 60.0 * 2.0 ** -21             # the two differ in rounding only


def test_a_record_outside_the_buffer_is_turned_down_and_its_neighbours_are_not():
    from footprints_amd import _lib, ops
    H, W = 8, 16
    rng = np.random.default_rng(19)
    maps = [rng.random((37, 61)), rng.random((37, 61)).astype(np.float32), rng.random((16, 48))]
    ref = np.stack([LR.label_resize(m, H, W, "area") for m in maps])
    tables = ops.label_table_set("cuda")
    packed, records, total, _ = ops.label_resize_pack(maps, H, W, "area", tables=tables)
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
    for change in (lambda r: setattr(r, "offset", total - 8), lambda r: setattr(r, "offset", 4), lambda r: setattr(r, "table_x", r.table_y),
                   lambda r: setattr(r, "table_y", 1 << 20), lambda r: setattr(r, "h", 38), lambda r: setattr(r, "dtype", 9),
                   lambda r: (setattr(r, "h", 7), setattr(r, "w", 61))):
        raised, out = run(change)
        assert raised and bits_equal(out[0], ref[0]) and bits_equal(out[2], ref[2]) and (out[1] == -7.0).all()
    raised, out = run(lambda r: None)                                    # the status word is cleared by the next call
    assert not raised and bits_equal(out, ref)


# ---- assembler ------------------------------------------------------------------------------------------------------------------------------
def _raw_samples(dataset, H, W, sizes, seed):
    """samples as the training readers deliver them: native-size frames, maps at native size in their stored dtypes"""
    rng = np.random.default_rng(seed)
    samples = []
    for j, ((ih, iw), (mh, mw)) in enumerate(sizes):
        maps = {"visible_ground": rng.random((mh, mw)).astype(np.float16),
                "ground_depth": (rng.random((mh, mw)) * 30 * (rng.random((mh, mw)) < 0.5)).astype(np.float32),
                "depth_mask": None if j == 1 else (rng.random((mh, mw)) < 0.3).astype(np.uint8)}
        if dataset == "kitti":
            maps["disparity"] = (rng.random((mh, mw)) * 60).astype(np.float32)
            maps["moving_objects"] = rng.random((mh, mw)) < 0.2
        else:
            maps["depth_raw"] = rng.integers(0, 65536, (H, W)).astype(np.float32)        # at the target size: Pillow's NEAREST ran on the reader
            maps["ground_depth"][::3, ::5] = np.float32(0.1)
        samples.append((rng.integers(0, 256, (ih, iw, 3), dtype=np.uint8), maps))
    return samples


@pytest.mark.parametrize("dataset", ["kitti", "matterport"])
def test_assembler_raw_maps_equal_the_host_fed_path(dataset):
    from footprints_amd.datasets import DeviceBatchAssembler, draw_augmentation
    from footprints_amd.datasets.device_path import MAP_KEYS, MAP_METHODS
    B, H, W = 2, 16, 24
    sizes = [((37, 53), (37, 61)), ((41, 50), (32, 48))]                 # different native sizes; the second one's maps take the integer path
    samples = _raw_samples(dataset, H, W, sizes, seed=23)
    dev = DeviceBatchAssembler(B, H, W, dataset=dataset, raw_images=True, max_src_hw=(41, 53), filter_depth_mask=True, raw_maps=True,
                               max_map_hw=(37, 61), check=True)
    host = DeviceBatchAssembler(B, H, W, dataset=dataset, raw_images=True, max_src_hw=(41, 53), filter_depth_mask=True)
    rng = random.Random(4)
    for it in range(2):                                                  # one sample flipped, one not, and the other way round
        params = [draw_augmentation(True, rng) for _ in samples]
        params[0].flip, params[1].flip = it, 1 - it
        fed = []
        for (img, maps), p in zip(samples, params):
            m = {}
            for key in MAP_KEYS[dataset]:
                mult = W / maps[key].shape[1] if key == "disparity" else 1.0
                r = LR.label_resize(maps[key], H, W, MAP_METHODS[key], bool(p.flip), mult)
                m[key] = r[:, ::-1] if p.flip else r                     # the host-fed path takes maps NOT flipped: undo the mirroring
            fed.append((img, m))
        a = dev.collect(dev.submit(samples, params))
        b = host.collect(host.submit(fed, params))
        torch.cuda.synchronize()
        assert set(a) == set(b)
        for k in a:
            assert torch.equal(a[k], b[k]), (dataset, k)
        assert float(a["depth_mask"][1].abs().sum()) == 0.0 and float(a["ground_depth"].sum()) > 0.0
    # staging buffers sized for one byte per element grow when the batch holds float16 / float32 maps, and the batch is the same
    tight = DeviceBatchAssembler(B, H, W, dataset=dataset, raw_images=True, max_src_hw=(41, 53), filter_depth_mask=True, raw_maps=True,
                                 max_map_hw=(37, 61), max_map_itemsize=1, slots=1, check=True)
    before = tight.slots[0]["h_msrc"].numel()
    c = tight.collect(tight.submit(samples, params))
    torch.cuda.synchronize()
    assert tight.slots[0]["h_msrc"].numel() > before and tight.slots[0]["d_msrc"].numel() == tight.slots[0]["h_msrc"].numel()
    for k in a:
        assert torch.equal(c[k], a[k]), (dataset, k)
    # a map that only the depth mask (and the moving objects) may lack is an error, not a map of zeros
    for broken in ({k: v for k, v in samples[0][1].items() if k != "visible_ground"}, dict(samples[0][1], ground_depth=None)):
        with pytest.raises((KeyError, ValueError), match="visible_ground|ground_depth"):
            tight.fill([(samples[0][0], broken), samples[1]], params)
    with pytest.raises(ValueError):
        DeviceBatchAssembler(B, H, W, raw_maps=True)
    with pytest.raises(ValueError):
        DeviceBatchAssembler(B, H, W, raw_maps=True, max_map_hw=(37, 61), map_dtype=np.float32)
    with pytest.raises(ValueError, match="larger than max_map_hw"):
        small = DeviceBatchAssembler(B, H, W, dataset=dataset, raw_images=True, max_src_hw=(41, 53), raw_maps=True, max_map_hw=(36, 61), slots=1)
        small.fill(samples, params)


# ---- command line ---------------------------------------------------------------------------------------------------------------------------
def test_main_trains_from_a_kitti_folder(tmp_path, monkeypatch):
    """`--mode train` without --synthetic_steps reads the folders the config file names: 4 frames, batch 2, one epoch at 64 x 128"""
    from footprints_amd.main import main
    from footprints_amd.training import train as T
    frames = [("2011_09_26/2011_09_26_drive_0001_sync", 3, "l", (48, 160), (70, 150)),
              ("2011_09_26/2011_09_26_drive_0001_sync", 4, "r", (50, 168), (96, 200)),
              ("2011_09_26/2011_09_26_drive_0002_sync", 17, "l", (56, 176), (128, 256)),
              ("2011_09_26/2011_09_26_drive_0002_sync", 18, "l", (52, 164), (64, 128))]
    raw, train, lines = write_kitti_tree(str(tmp_path), frames, seed=3, skip_mask=(2,))
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
    random.seed(5)
    main(["--mode", "train", "--epochs", "1", "--batch_size", "2", "--height", "64", "--width", "128", "--val_batches", "1", "--num_workers", "2",
          "--config_path", str(tmp_path / "paths.yaml"), "--log_path", str(tmp_path / "logs"), "--model_name", "folder"])
    tm = made[0]
    torch.cuda.synchronize()
    assert tm.step == 2 and len(tm.train_loader) == 2 and len(tm.train_loader.dataset) == 4
    assert os.path.exists(tmp_path / "logs" / "folder" / "models" / "weights_0" / "model.pth")
    assert len(tm.history["train"]) == 1 and len(tm.history["val"]) == 1
    assert all(np.isfinite(v) for v in tm.history["train"][0][1].values()) and all(np.isfinite(v) for v in tm.history["val"][0][1].values())
