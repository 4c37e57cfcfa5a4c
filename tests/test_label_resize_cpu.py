"""CPU: the host half of the label-map resize and the training-set file readers.

No cv2 is installed where this was written, so the resize is pinned in two steps: the library's INTER_AREA tables equal the numpy
restatement of OpenCV's algorithm (tests/label_resize_restatement.py) entry for entry, and the restatement lies within a DERIVED bound of
the exact rational area average.  Where cv2 imports, one more test compares the restatement with cv2.resize bit for bit.  The device side is
tests/test_gpu_label_resize.py.  Inputs are drawn from seeded generators; nothing comes from the reference."""
import os
import random
from fractions import Fraction

import numpy as np
import pytest

from tests import label_resize_restatement as LR

TABLE_CASES = [(375, 192), (1242, 640), (370, 192), (1226, 640), (11, 4), (29, 8), (10, 9), (12, 4), (8, 8)]
EXACT_CASES = [((7, 11), (3, 4)), ((13, 29), (5, 8)), ((9, 10), (8, 9)), ((17, 33), (16, 32))]


@pytest.mark.parametrize("S,D", TABLE_CASES)
def test_area_table_equals_the_restatement_entry_for_entry(S, D):
    from footprints_amd import ops
    bounds, index, weight = ops.area_table(S, D)
    rb, ri, rw = LR.area_table(S, D)
    assert bounds.dtype == np.int32 and index.dtype == np.int32 and weight.dtype == np.float32
    assert np.array_equal(bounds, rb) and np.array_equal(index, ri) and np.array_equal(weight.view(np.int32), rw.view(np.int32))
    # every output index has entries, they tile the table, stay inside the source, and their weights sum to one within float rounding
    assert bounds[0, 0] == 0 and (bounds[:, 1] >= 1).all() and np.array_equal(bounds[1:, 0], (bounds[:, 0] + bounds[:, 1])[:-1])
    assert bounds[-1].sum() == index.size and index.min() >= 0 and index.max() < S
    sums = np.add.reduceat(weight.astype(np.float64), bounds[:, 0])
    assert np.abs(sums - 1.0).max() < bounds[:, 1].max() * 2.0 ** -23
    if S % D == 0:                                                      # integer factor: whole cells only
        assert (bounds[:, 1] == S // D).all() and (weight == np.float32(D / S)).all()


def test_area_table_refuses_enlarging_and_bad_sizes():
    from footprints_amd import ops
    for S, D in ((4, 5), (0, 1), (3, 0)):
        with pytest.raises(ValueError):
            ops.area_table(S, D)


@pytest.mark.parametrize("src,dst", EXACT_CASES)
def test_restatement_lies_within_the_derived_bound_of_the_exact_area_average(src, dst):
    """Bound: every term of the exact average is S * wy * wx with rational weights; the restatement uses two float weights per term, each
    within 2^-24 relative of its rational (round to nearest), so a term is off by at most (2 * 2^-24 + 2^-48) |S| wy wx, and the weights sum
    to one: 2^-23 * max|S| plus the double roundings of the sums (below 2^-50 relative) -- 2^-22 * max|S| holds with a factor of two to
    spare.  The 1e-3 cut drops no true sliver here: for D < 1000 every overlap is a multiple of 1 / D > 1e-3.
    Measured when written: at most 5.5e-8 * max|S| against the bound of 2.4e-7."""
    (h, w), (H, W) = src, dst
    rng = np.random.default_rng(h * 100 + w)
    for m in (rng.random((h, w)) * 80.0, rng.standard_normal((h, w)), (rng.random((h, w)) < 0.4).astype(np.float64)):
        got = LR.restate(m, H, W, "area")
        exact = LR.exact_area(m, H, W)
        dev = max(abs(Fraction(float(got[y, x])) - exact[y][x]) for y in range(H) for x in range(W))
        print("area %dx%d -> %dx%d: max deviation %.3e * max|src| (bound %.3e)" % (h, w, H, W, float(dev) / np.abs(m).max(), 2.0 ** -22))
        assert dev <= Fraction(2) ** -22 * Fraction(float(np.abs(m).max()))


def test_restatement_fast_path_copy_and_nearest():
    rng = np.random.default_rng(3)
    m = rng.random((16, 48))
    fast = LR.restate(m, 8, 16, "area")                                 # 2 x 3 blocks: row-major sum, times float 1 / 6
    assert LR.is_fast(16, 48, 8, 16) and not LR.is_fast(37, 61, 8, 16)
    blk = m.reshape(8, 2, 16, 3)
    ref = ((((blk[:, 0, :, 0] + blk[:, 0, :, 1]) + blk[:, 0, :, 2]) + blk[:, 1, :, 0]) + blk[:, 1, :, 1]) + blk[:, 1, :, 2]
    assert np.array_equal(fast, ref * float(np.float32(1.0) / np.float32(6.0)))
    assert np.array_equal(LR.restate(m, 16, 48, "area"), m) and np.array_equal(LR.restate(m, 16, 48, "nearest"), m)
    near = LR.restate(m, 5, 7, "nearest")
    assert np.array_equal(near, m[[0, 3, 6, 9, 12]][:, [0, 6, 13, 20, 27, 34, 41]])      # floor(d * scale), scale = 1 / (out / in)
    up = LR.restate(m[:3, :4], 7, 9, "nearest")                          # NEAREST may enlarge
    assert up.shape == (7, 9) and up[6, 8] == m[2, 3] and up[0, 0] == m[0, 0]
    with pytest.raises(ValueError):
        LR.restate(m, 17, 48, "area")


def test_a_flipped_record_is_the_resize_of_the_mirrored_map():
    """the record layout's flip: read mirrored, store mirrored = restate(fliplr(m))[:, ::-1]; INTER_AREA's general tables are not
    symmetric (the 1e-3 cut and the float weights), so this differs from restate(m) in bits"""
    rng = np.random.default_rng(5)
    m = rng.random((37, 61)).astype(np.float32)
    plain, flipped = LR.label_resize(m, 8, 16, "area"), LR.label_resize(m, 8, 16, "area", flip=True)
    assert np.array_equal(flipped, LR.restate(np.fliplr(m), 8, 16, "area"))
    assert np.abs(flipped[:, ::-1] - plain).max() < 2.0 ** -22 and flipped.shape == plain.shape
    assert np.array_equal(LR.label_resize(m, 8, 16, "area", multiplier=16 / 61), plain * (16 / 61))
    assert np.array_equal(LR.label_resize(None, 8, 16, "nearest"), np.zeros((8, 16)))


def test_cv2_equals_the_restatement_bit_for_bit():
    cv2 = pytest.importorskip("cv2")
    if not all(hasattr(cv2, name) for name in ("resize", "INTER_AREA", "INTER_NEAREST")):
        pytest.skip("the module named cv2 is a stand-in another test put into sys.modules, not OpenCV")
    rng = np.random.default_rng(7)
    for (h, w), (H, W) in EXACT_CASES + [((37, 61), (8, 16)), ((16, 48), (8, 16)), ((8, 16), (8, 16)), ((375, 1242), (192, 640))]:
        m = rng.random((h, w)) * 80.0
        for name, flag in (("area", cv2.INTER_AREA), ("nearest", cv2.INTER_NEAREST)):
            assert np.array_equal(cv2.resize(m, (W, H), interpolation=flag), LR.restate(m, H, W, name)), (h, w, H, W, name)


# ---- host pack ------------------------------------------------------------------------------------------------------------------------------
def test_pack_lays_out_records_and_refuses_what_the_kernel_does_not_provide():
    import ctypes as C
    from footprints_amd import _lib, ops
    lib = _lib.load()
    assert lib.fp_label_sample_bytes() == C.sizeof(_lib.LabelSample) == 48 and lib.fp_label_table_bytes() == C.sizeof(_lib.LabelTable) == 24
    assert lib.fp_label_max_entries() == _lib.LABEL_MAX_ENTRIES
    rng = np.random.default_rng(9)
    tables = ops.LabelTableSet("cuda:0")                                 # host work only: nothing is uploaded here
    maps = [rng.random((37, 61)).astype(np.float16), rng.random((16, 48)).astype(np.float32), None, rng.random((8, 16)) < 0.5,
            rng.integers(0, 9, (9, 17))]
    packed, records, used, _ = ops.label_resize_pack(maps, 8, 16, ["area", "area", "nearest", "nearest", "nearest"], [False, True] * 2 + [False],
                                                     [1.0, 16 / 48, 1.0, 1.0, 1.0], tables=tables, max_map_hw=(37, 61))
    rec = (_lib.LabelSample * 5).from_buffer_copy(records.tobytes())
    assert [(r.h, r.w, r.dtype, r.method, r.flip) for r in rec] == [(37, 61, 1, 2, 0), (16, 48, 2, 2, 1), (0, 0, 0, 0, 0), (8, 16, 0, 1, 1),
                                                                   (9, 17, 3, 1, 0)]
    assert all(r.offset % 8 == 0 for r in rec) and rec[1].multiplier == 16 / 48 and used == 4520 + 3072 + 128 + 9 * 17 * 8
    assert (rec[0].table_x, rec[0].table_y) == (0, 1) and (rec[1].table_x, rec[1].table_y) == (-1, -1)          # general / integer path
    assert np.array_equal(packed[rec[0].offset:rec[0].offset + 37 * 61 * 2].view(np.float16).reshape(37, 61), maps[0])
    assert np.array_equal(packed[rec[4].offset:rec[4].offset + 9 * 17 * 8].view(np.float64).reshape(9, 17), maps[4].astype(np.float64))
    assert len(tables.records) == 2 and tables.records[0].in_size == 61 and tables.records[1].out_size == 8
    with pytest.raises(ValueError, match="7 x 61 up to 8 x 16"):        # INTER_AREA would enlarge: cv2 goes linear there
        ops.label_resize_pack([rng.random((7, 61))], 8, 16, "area", tables=tables)
    with pytest.raises(ValueError, match="38 x 61, larger than max_map_hw"):
        ops.label_resize_pack([rng.random((38, 61))], 8, 16, "nearest", tables=tables, max_map_hw=(37, 61))
    with pytest.raises(ValueError, match="the buffer holds"):
        ops.label_resize_pack(maps, 8, 16, "nearest", tables=tables, packed=np.empty(64, np.uint8))
    with pytest.raises(ValueError, match="entries per output"):         # a non-integer factor beyond what a thread stages
        ops.label_resize_pack([rng.random((8, 16 * 13 + 1))], 8, 16, "area", tables=tables)
    ops.label_resize_pack([rng.random((7, 9))], 8, 16, "nearest", tables=tables)          # NEAREST may enlarge


# ---- readers --------------------------------------------------------------------------------------------------------------------------------
def test_readers_build_the_reference_paths():
    from footprints_amd.datasets.training import KITTIReader, MatterportReader, get_dataset_class
    assert get_dataset_class("kitti") is KITTIReader and get_dataset_class("matterport") is MatterportReader
    with pytest.raises(NotImplementedError):
        get_dataset_class("nyu")
    k = KITTIReader("/raw", "/train", ["2011_09_26/2011_09_26_drive_0022_sync 473 r", "2011_09_26/2011_09_26_drive_0001_sync 5 l"], 192, 640)
    assert k.paths(0) == {
        "image": "/raw/2011_09_26/2011_09_26_drive_0022_sync/image_03/data/0000000473.jpg",
        "visible_ground": "/train/ground_seg/2011_09_26/2011_09_26_drive_0022_sync/image_03/data/0000000473.npy",
        "ground_depth": "/train/hidden_depths/2011_09_26/2011_09_26_drive_0022_sync/image_03/data/0000000473.npy",
        "depth_mask": "/train/depth_masks/2011_09_26/2011_09_26_drive_0022_sync/image_03/data/0000000473.npy",
        "disparity": "/train/stereo_matching_disps/2011_09_26/2011_09_26_drive_0022_sync/image_03/0000000473.npy",
        "moving_objects": "/train/moving_objects/2011_09_26/2011_09_26_drive_0022_sync/image_03/data/0000000473.npy"}
    assert k.paths(1)["image"] == "/raw/2011_09_26/2011_09_26_drive_0001_sync/image_02/data/0000000005.jpg" and len(k) == 2
    m = MatterportReader("/raw", "/train", ["17DRP5sb8fy 0f37bd0737e349de9d536263a4bdd60d 1 3"], 512, 640, no_depth_mask=False)
    assert m.paths(0) == {
        "image": "/raw/17DRP5sb8fy/17DRP5sb8fy/matterport_color_images/0f37bd0737e349de9d536263a4bdd60d_i1_3.jpg",
        "depth_raw": "/raw/17DRP5sb8fy/17DRP5sb8fy/matterport_depth_images/0f37bd0737e349de9d536263a4bdd60d_d1_3.png",
        "visible_ground": "/train/ground_seg/17DRP5sb8fy/data/0f37bd0737e349de9d536263a4bdd60d_1_3.npy",
        "ground_depth": "/train/hidden_depth/17DRP5sb8fy/data/0f37bd0737e349de9d536263a4bdd60d_1_3.npy",
        "depth_mask": "/train/depth_masks/17DRP5sb8fy/data/0f37bd0737e349de9d536263a4bdd60d_1_3.npy"}
    with pytest.raises(AssertionError):
        KITTIReader("/raw", "/train", [], 192, 640, project_down_baseline=True, moving_objects_method="ours")


def write_kitti_tree(root, frames, seed=0, skip_mask=()):
    """a small KITTI tree as this package's label generation leaves it: frames = [(seq, frame number, side, (h, w) of the JPEG, (h, w) of
    the maps)], maps in float16 / float32 / uint8 -> (raw path, training-data path, split lines)"""
    from PIL import Image
    rng = np.random.default_rng(seed)
    raw, train = os.path.join(root, "raw"), os.path.join(root, "training_data")
    lines = []
    for j, (seq, frame, side, (ih, iw), (mh, mw)) in enumerate(frames):
        folder, name = "image_02" if side == "l" else "image_03", str(frame).zfill(10)
        os.makedirs(os.path.join(raw, seq, folder, "data"), exist_ok=True)
        Image.fromarray(rng.integers(0, 256, (ih, iw, 3), dtype=np.uint8)).save(os.path.join(raw, seq, folder, "data", name + ".jpg"), quality=90)
        maps = {"ground_seg": rng.random((1, mh, mw)).astype(np.float16),                       # 3-D: the reader takes npy[0]
                "hidden_depths": (rng.random((mh, mw)) * 30 * (rng.random((mh, mw)) < 0.5)).astype(np.float32),
                "depth_masks": (rng.random((mh, mw)) < 0.1).astype(np.uint8),
                "stereo_matching_disps": (rng.random((mh, mw)) * 60).astype(np.float32),
                "moving_objects": (rng.random((mh, mw)) < 0.05).astype(np.uint8)}
        for kind, arr in maps.items():
            if kind == "depth_masks" and j in skip_mask:
                continue
            sub = os.path.join(train, kind, seq, folder) if kind == "stereo_matching_disps" else os.path.join(train, kind, seq, folder, "data")
            os.makedirs(sub, exist_ok=True)
            np.save(os.path.join(sub, name + ".npy"), arr)
        lines.append("%s %d %s" % (seq, frame, side))
    return raw, train, lines


def test_kitti_reader_delivers_the_files_as_stored_and_none_for_a_missing_mask(tmp_path):
    from footprints_amd.datasets.training import KITTIReader
    frames = [("2011_09_26/drive_0001_sync", 3, "l", (48, 160), (70, 150)), ("2011_09_26/drive_0001_sync", 12, "r", (56, 176), (96, 200))]
    raw, train, lines = write_kitti_tree(str(tmp_path), frames, skip_mask=(1,))
    r = KITTIReader(raw, train, lines, 64, 128, no_depth_mask=False, moving_objects_method="ours", project_down_baseline=False, is_train=True)
    img, maps = r[0]
    assert img.shape == (48, 160, 3) and img.dtype == np.uint8 and set(maps) == {"visible_ground", "ground_depth", "depth_mask", "disparity",
                                                                                  "moving_objects"}
    assert maps["visible_ground"].shape == (70, 150) and maps["visible_ground"].dtype == np.float16          # npy[0] of the 3-D file
    assert maps["ground_depth"].dtype == np.float32 and maps["depth_mask"].dtype == np.uint8 and maps["disparity"].shape == (70, 150)
    assert np.array_equal(maps["moving_objects"], np.load(r.paths(0)["moving_objects"]))
    img, maps = r[1]
    assert img.shape == (56, 176, 3) and maps["depth_mask"] is None and maps["ground_depth"].shape == (96, 200)
    none = KITTIReader(raw, train, lines, 64, 128, moving_objects_method="none")
    assert none[0][1]["moving_objects"] is None


class _CountingReader:
    def __init__(self, n, tag):
        self.n, self.tag = n, tag

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        return (self.tag, i)


def test_threaded_batch_source_keeps_batch_source_order_and_sharding():
    from footprints_amd.datasets.training import ThreadedBatchSource
    from footprints_amd.preprocessing.segmentation.datasets import BatchSource
    readers = [_CountingReader(23, "a"), _CountingReader(14, "b")]
    for shuffle in (True, False):
        plain = BatchSource(readers, 4, shuffle=shuffle, rng=random.Random(6))
        threaded = ThreadedBatchSource(readers, 4, shuffle=shuffle, rng=random.Random(6), num_workers=40, ahead=2)
        assert threaded.num_workers == 16 and len(threaded) == len(plain) == 9 and threaded.dataset == plain.dataset
        ref = list(plain)
        assert list(threaded) == ref and len(ref) == 9
        shards = [ThreadedBatchSource(readers, 4, shuffle=shuffle, rng=random.Random(6), num_workers=3).shard(r, 2) for r in range(2)]
        assert [len(s) for s in shards] == [len(plain.shard(r, 2)) for r in range(2)] == [5, 4]
        assert list(shards[0]) == ref[0::2] and list(shards[1]) == ref[1::2]
    it = iter(ThreadedBatchSource(readers, 4, shuffle=False, num_workers=2))           # a consumer that stops early leaves nothing running
    assert next(it) == [("a", 0), ("a", 1), ("a", 2), ("a", 3)]
    it.close()
