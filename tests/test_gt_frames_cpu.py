"""CPU: the host half of the label generators' loader (csrc/gt_frames.hip, ops.gt_frame_pack, data_loader.py, the command line) against the
numpy restatement (tests/gt_frames_restatement.py), and the restatement's INTER_LINEAR against what bilinear interpolation must give.
No cv2 exists here: the restatement is a reading of OpenCV's portable path and has not been compared with a cv2 binary."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import gt_frames_restatement as GR
from tests import label_resize_restatement as LR

KITTI_WIDTHS, KITTI_HEIGHTS = (1242, 1241, 1238, 1226, 1224), (376, 375, 374, 370)
# (native, target) of the GPU test's mixed launch, per axis, and the two enlarging pairs
SMALL_PAIRS = [(6, 4), (10, 6), (8, 4), (12, 6), (4, 4), (6, 6), (3, 4), (5, 6), (1, 4), (1, 6), (40, 33), (70, 64), (24, 12), (80, 40)]
TABLE_PAIRS = [(w, 640) for w in KITTI_WIDTHS] + [(h, 192) for h in KITTI_HEIGHTS] + [(1280, 640), (1024, 480)] + SMALL_PAIRS


# ---- synthetic dataset folders (shared with tests/test_gpu_gt_frames.py) --------------------------------------------------------------------
def write_kitti_gt_tree(root, sequence, frames, native=(24, 80), seed=0, missing=()):
    """the label generators' KITTI inputs under <root>/training: disparities (float32, strictly positive), ground segmentations (float16
    [1, h, w], ground in the lower half), ORB-SLAM poses (a camera moving forward) and optical flow (float32 [2, h, w]) for both cameras of
    every frame; `missing` = (frame, side, folder) files left out -> the training_data path"""
    rng = np.random.default_rng(seed)
    t = os.path.join(str(root), "training")
    h, w = native
    for f in frames:
        name = "{}.npy".format(str(f).zfill(10))
        pose = np.eye(4)[:3].copy()
        pose[:, 3] = (0.01 * f, 0.0, 0.4 * f)
        files = {os.path.join("poses", sequence, "orbslam_poses"): pose.reshape(-1)}
        for side in ("image_02", "image_03"):
            seg = rng.random((1, h, w)) * 0.5
            seg[:, h // 2:] = 0.72 + 0.28 * rng.random((1, h - h // 2, w))
            rows = np.linspace(0.0, 1.0, h)[:, None]
            files[os.path.join("stereo_matching_disps", sequence, side)] = (1.0 + 3.0 * rows + 0.2 * rng.random((h, w))).astype(np.float32) * (w / 40.0)
            files[os.path.join("ground_seg", sequence, side, "data")] = seg.astype(np.float16)
            files[os.path.join("optical_flow", sequence, side, "data")] = (rng.standard_normal((2, h, w)) * 4).astype(np.float32)
            for folder, arr in list(files.items()):
                if (f, side, folder.split(os.sep)[0]) in missing:
                    continue
                os.makedirs(os.path.join(t, folder), exist_ok=True)
                np.save(os.path.join(t, folder, name), arr)
            files = {}
    return t


def write_matterport_gt_tree(root, scan, names, native=(24, 32), depth_native=(32, 40), seed=0):
    """a Matterport scan's inputs: <root>/raw/<scan>/<scan>/matterport_{depth_images,camera_poses,camera_intrinsics} and
    <root>/training/ground_seg/<scan>/data; names = (pos, height, direction) -> (raw path, training_data path).  The last camera is 2 m
    higher than the others, so it is not `close` to them."""
    from PIL import Image
    rng = np.random.default_rng(seed)
    raw, t = os.path.join(str(root), "raw"), os.path.join(str(root), "training")
    base = os.path.join(raw, scan, scan)
    for d in ("matterport_depth_images", "matterport_camera_poses", "matterport_camera_intrinsics"):
        os.makedirs(os.path.join(base, d), exist_ok=True)
    os.makedirs(os.path.join(t, "ground_seg", scan, "data"), exist_ok=True)
    h, w = native
    for j, (pos, height, direction) in enumerate(names):
        seg = rng.random((1, h, w)) * 0.5
        seg[:, h // 2:] = 0.72 + 0.28 * rng.random((1, h - h // 2, w))
        np.save(os.path.join(t, "ground_seg", scan, "data", "{}_{}_{}.npy".format(pos, height, direction)), seg.astype(np.float16))
        depth = (4000.0 + 8000.0 * np.linspace(1.0, 0.2, depth_native[0])[:, None] + rng.integers(0, 400, depth_native)).astype(np.uint16)
        Image.fromarray(depth).save(os.path.join(base, "matterport_depth_images", "{}_d{}_{}.png".format(pos, height, direction)))
        pose = np.eye(4)
        pose[:3, 3] = (0.3 * j, 0.1 * j, 2.0 if j == len(names) - 1 else 0.0)
        with open(os.path.join(base, "matterport_camera_poses", "{}_pose_{}_{}.txt".format(pos, height, direction)), "w") as fh:
            fh.write(" ".join(repr(float(v)) for v in pose.reshape(-1)))
        with open(os.path.join(base, "matterport_camera_intrinsics", "{}_intrinsics_{}.txt".format(pos, height)), "w") as fh:
            fh.write("1280 1024 1075.5 1076.25 629.75 {} 0 0 0 0 0".format(521.5 + int(height)))
    return raw, t


class RecordingCache:
    """stands where data_loader.FrameCache stands and records what a loader asks of the device"""

    def __init__(self):
        self.used, self.resets, self.uploads, self.gathers = 0, 0, [], []

    def alloc(self, n):
        first, self.used = self.used, self.used + n
        return list(range(first, self.used))

    def reset(self):
        self.used, self.resets = 0, self.resets + 1

    def view(self, slot, n=None):
        return ("view", slot, n)

    def resize_into(self, maps, slots, method="linear", pre=1.0, post=1.0, threshold=None):
        self.uploads.append({"maps": maps, "slots": list(slots), "method": method, "pre": pre, "post": post, "threshold": threshold})

    def gather(self, depth_slots, seg_slots, fb=None):
        self.gathers.append((list(depth_slots), list(seg_slots), fb))
        return ("depths", len(depth_slots)), ("ground_segs", len(seg_slots))


# ---- tables ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clamp", [True, False])
def test_linear_tables_equal_the_restatement_bit_for_bit(clamp):
    from footprints_amd import ops
    for S, D in TABLE_PAIRS:
        offsets, coeffs = ops.linear_table(S, D, clamp)
        ref_o, ref_c = GR.linear_table(S, D, clamp)
        assert offsets.dtype == np.int32 and coeffs.dtype == np.float32 and coeffs.shape == (D, 2)
        assert np.array_equal(offsets, ref_o), (S, D)
        assert np.array_equal(coeffs.view(np.int32), ref_c.view(np.int32)), (S, D)
        if clamp:
            assert offsets.min() >= 0 and offsets.max() <= S - 1 and (coeffs[offsets == S - 1, 1] == 0).all()
    # enlarging reaches both clamps; the unclamped form keeps the negative offset and its fraction
    o, c = ops.linear_table(3, 4, False)
    assert o[0] == -1 and c[0, 1] == np.float32(0.875) and ops.linear_table(3, 4, True)[0][0] == 0
    with pytest.raises(ValueError):
        ops.linear_table(0, 4, True)


# ---- what `linear` must be, whatever cv2 does with the last bits ---------------------------------------------------------------------------
def test_linear_at_equal_sizes_is_the_source():
    rng = np.random.default_rng(3)
    m = rng.standard_normal((7, 9)) * 50
    sy, cy = GR.linear_table(7, 7, False)
    assert np.array_equal(sy, np.arange(7)) and (cy[:, 1] == 0).all()              # f = 0: the vertical form is r * 1 + r' * 0
    assert np.array_equal(GR.linear(m, 7, 9), m)


@pytest.mark.parametrize("src,dst", [((6, 10), (4, 6)), ((8, 10), (4, 6)), ((3, 5), (4, 6)), ((1, 1), (4, 6)), ((40, 70), (33, 64)),
                                     ((375, 1242), (192, 640)), ((370, 1224), (192, 640))])
def test_linear_lies_within_float_coefficient_error_of_exact_bilinear(src, dst):
    """Two references, both bilinear interpolation in float64.
    (a) With exact coefficients 1 - f and f at the positions OpenCV samples: the float coefficient 1.f - f is off by at most 2^-24 and there
        are a few double roundings, so 2^-22 * max|src| bounds the difference (the bound the label resize uses for its float weights).
    (b) On the exact rational grid (d + 1/2) * S / D - 1/2.  OpenCV rounds that position to float BEFORE it takes the fraction, so f is off
        by up to 2^-24 * position -- 2^-21 at position 8.67 of the 10 -> 6 axis, 6e-5 at column 1241 -- and the 2^-22 bound does not hold
        against this grid: random 6 x 10 -> 4 x 6 data differs by 3.3e-5 where 2^-22 * max|src| is 3.1e-5, random 375 x 1242 -> 192 x 640 data by 1.4e-2 where it is 6.7e-5.
        Bilinear interpolation is continuous and piecewise linear with slope at most 2 * max|src| per axis, so a position error of
        2^-24 * w and 2^-24 * h moves it by at most 2 * max|src| * 2^-24 * (w + h); with (a)'s share on top that is the bound here."""
    rng = np.random.default_rng(src[0] + src[1])
    m = rng.standard_normal(src) * 60.0
    top = np.abs(m).max()
    got = GR.linear(m, *dst)
    err_a, err_b = np.abs(got - GR.exact_coefficient_bilinear(m, *dst)).max(), np.abs(got - GR.exact_bilinear(m, *dst)).max()
    print("linear %r -> %r: max|src| %.3f, against exact coefficients %.3e (bound %.3e), against the rational grid %.3e (bound %.3e)"
          % (src, dst, top, err_a, 2.0 ** -22 * top, err_b, top * (2.0 ** -22 + 2.0 ** -23 * (src[0] + src[1]))))
    assert got.shape == dst and err_a <= 2.0 ** -22 * top
    assert err_b <= top * (2.0 ** -22 + 2.0 ** -23 * (src[0] + src[1]))
    assert got.min() >= m.min() - 1e-9 and got.max() <= m.max() + 1e-9


def test_exact_two_times_is_dispatched_to_area2_and_one_axis_is_not():
    from footprints_amd import _lib, ops
    rng = np.random.default_rng(5)
    tables = ops.LinearTableSet("cpu")
    both, one = rng.random((8, 12)) * 9, rng.random((8, 10)) * 9
    pack = ops.gt_frame_pack([both, one], 4, 6, [0, 24], 48, "linear", tables=tables)
    assert pack.records[0].method == _lib.GT_AREA2 and (pack.records[0].table_x, pack.records[0].table_y) == (-1, -1)
    assert pack.records[1].method == _lib.GT_LINEAR and pack.records[1].table_x >= 0 and pack.records[1].table_y >= 0
    assert GR.is_area2(8, 12, 4, 6) and not GR.is_area2(8, 10, 4, 6) and not GR.is_area2(12, 18, 4, 6)
    assert np.array_equal(GR.resize(both, 4, 6, "linear"), LR.restate(both, 4, 6, "area"))
    assert np.array_equal(GR.resize(one, 4, 6, "linear"), GR.linear(one, 4, 6))
    assert not np.array_equal(GR.linear(both, 4, 6), LR.restate(both, 4, 6, "area"))      # the dispatch matters: the two differ


# ---- records --------------------------------------------------------------------------------------------------------------------------------
def _small_pack(tables=None, **kw):
    from footprints_amd import ops
    rng = np.random.default_rng(7)
    maps = [rng.random((6, 10)).astype(np.float16), rng.random((3, 5)).astype(np.float32), rng.random((8, 12)),
            rng.integers(0, 65536, (4, 6)).astype(np.uint16)]
    tables = ops.LinearTableSet("cpu") if tables is None else tables
    args = dict(dst=[72, 0, 24, 48], cache_elems=96, method=["linear", "linear", "linear", "nearest"], pre=[0.6, 1.0, 1.0, 1.0],
                post=[1.0, (6.0, 5.0), 1.0, 0.00025], threshold=[0.75, None, None, None])
    args.update(kw)
    return maps, tables, ops.gt_frame_pack(maps, 4, 6, tables=tables, **args)


def test_record_layout_equals_the_library():
    from footprints_amd import _lib
    lib = _lib.load()
    assert lib.fp_gt_frame_bytes() == C.sizeof(_lib.GtFrame) == 80 and lib.fp_gt_table_bytes() == C.sizeof(_lib.GtTable) == 16
    maps, tables, pack = _small_pack()
    assert pack.n == 4 and pack.src_bytes == pack.records_offset == 6 * 10 * 2 + 3 * 5 * 4 + 4 + 8 * 12 * 8 + 4 * 6 * 2
    assert pack.total == pack.src_bytes + 4 * 80 and pack.packed.dtype == np.uint8 and pack.packed.size >= pack.total
    rec = (_lib.GtFrame * 4).from_buffer_copy(pack.packed[pack.records_offset:pack.total].tobytes())
    for r, m, dst in zip(rec, maps, (72, 0, 24, 48)):
        assert r.offset % 8 == 0 and (r.h, r.w) == m.shape and r.dst == dst
        assert np.array_equal(pack.packed[r.offset:r.offset + m.nbytes].view(m.dtype).reshape(m.shape), m)
    assert [r.dtype for r in rec] == [_lib.GT_F16, _lib.GT_F32, _lib.GT_F64, _lib.GT_U16]
    assert [r.method for r in rec] == [_lib.GT_LINEAR, _lib.GT_LINEAR, _lib.GT_AREA2, _lib.GT_NEAREST]
    assert rec[0].pre == float(np.float16(0.6)) and rec[0].threshold == 1 and rec[0].thr == 0.75 and rec[1].threshold == 0
    assert (rec[1].post_num, rec[1].post_den) == (6.0, 5.0) and (rec[3].post_num, rec[3].post_den) == (0.00025, 1.0)
    t_rec, n_tables, words = tables.host_records()
    assert n_tables == 4 and words == 3 * 6 + 3 * 4 + 3 * 6 + 3 * 4
    assert [(t.in_size, t.out_size, t.clamp) for t in t_rec] == [(10, 6, 1), (6, 4, 0), (5, 6, 1), (3, 4, 0)]


def test_records_outside_their_buffers_are_refused_on_the_host():
    from footprints_amd import _lib, ops
    lib = _lib.load()
    maps, tables, pack = _small_pack()
    t_rec, n_tables, words = tables.host_records()

    def check(change, src_bytes=pack.src_bytes, cache_elems=96, words_len=words, n_tab=n_tables):
        rec = (_lib.GtFrame * 4).from_buffer_copy(bytes(pack.records))
        change(rec)
        return lib.fp_gt_frame_check(C.addressof(rec), 4, src_bytes, C.addressof(t_rec), n_tab, words_len, cache_elems, 4, 6)
    assert check(lambda r: None) == 0
    for change in (lambda r: setattr(r[0], "offset", 4), lambda r: setattr(r[2], "offset", pack.src_bytes - 8), lambda r: setattr(r[1], "h", 400),
                   lambda r: setattr(r[0], "offset", -8), lambda r: setattr(r[1], "dst", 73), lambda r: setattr(r[1], "dst", -1),
                   lambda r: setattr(r[3], "dst", 1 << 40), lambda r: setattr(r[0], "dtype", 4), lambda r: setattr(r[0], "method", 3),
                   lambda r: setattr(r[0], "table_x", r[0].table_y), lambda r: setattr(r[0], "table_y", 99), lambda r: setattr(r[1], "table_x", -1),
                   lambda r: setattr(r[2], "h", 9), lambda r: setattr(r[3], "pre", 2.0), lambda r: setattr(r[1], "post_den", 0.0),
                   lambda r: setattr(r[1], "pre", 0.1)):
        assert check(change) != 0
        assert b"record" in lib.fp_last_error_string()
    assert check(lambda r: None, src_bytes=pack.src_bytes - 8) != 0 and check(lambda r: None, cache_elems=95) != 0
    assert check(lambda r: None, words_len=words - 1) != 0 and check(lambda r: None, n_tab=3) != 0
    # Python sees ValueError, before anything is launched
    with pytest.raises(ValueError, match="destination"):
        _small_pack(dst=[72, 0, 24, 73])
    with pytest.raises(ValueError, match="destination"):
        _small_pack(cache_elems=95)
    with pytest.raises(ValueError, match="pre-scale"):
        _small_pack(pre=[1.0, 1.0, 1.0, 2.0])
    with pytest.raises(ValueError, match="area2"):
        _small_pack(method=["linear", "area2", "linear", "nearest"])
    with pytest.raises(ValueError, match="bytes"):
        _small_pack(packed=np.empty(64, np.uint8))
    with pytest.raises(ValueError):
        ops.gt_frame_pack([np.zeros((2, 3, 4))], 4, 6, [0], 24, tables=tables)
    cache = torch.zeros((3, 4, 6))
    for d, s in (([0, 3], [1, 2]), ([0, 1], [-1, 2]), ([], [])):
        with pytest.raises(ValueError, match="slots"):
            ops.gt_gather_frames(cache, d, s, 1.0)


# ---- the loaders' plans ---------------------------------------------------------------------------------------------------------------------
SEQ = "2011_09_26/2011_09_26_drive_0001_sync"


def test_kitti_loader_plans_the_reference_window_and_uploads_each_frame_once(tmp_path):
    from footprints_amd.preprocessing.ground_truth_generation import KITTILoader
    t = write_kitti_gt_tree(tmp_path, SEQ, range(8), missing={(5, "image_03", "ground_seg")})
    cache = RecordingCache()
    loader = KITTILoader("unused", t, 12, 40, frame_cache=cache)
    assert (loader.num_frames_bwd, loader.num_frames_fwd, loader.stereo_baseline) == (25, 50, 0.54) and loader.buffer == {}
    assert loader.K.dtype == np.float32 and loader.K[0, 0] == np.float32(0.58) * 40 and np.allclose(loader.invK @ loader.K, np.eye(4), atol=1e-6)
    assert loader.window(30) == [(f, s) for f in range(5, 80, 2) for s in ("image_02", "image_03")] and len(loader.window(30)) == 76
    data = loader.load_data(SEQ, 3)                                  # range(-22, 53, 2): the even frames; negative and missing ones are skipped
    keys = [(SEQ, f, s) for f in (0, 2, 4, 6) for s in ("image_02", "image_03")]
    assert list(loader.buffer) == keys and data["sides"] == [k[2] for k in keys]
    assert len(cache.uploads) == 1 and len(cache.uploads[0]["maps"]) == 16 and cache.uploads[0]["slots"] == list(range(16))
    up = cache.uploads[0]
    assert up["method"] == "linear" and up["pre"] == [40 / 80, 1.0] * 8 and up["threshold"] == [None, 0.75] * 8 and up["post"] == [1.0] * 16
    assert [m.shape for m in up["maps"]] == [(24, 80)] * 16 and up["maps"][0].dtype == np.float32 and up["maps"][1].dtype == np.float16
    d, s, fb = cache.gathers[0]
    assert d == list(range(0, 16, 2)) and s == list(range(1, 16, 2)) and fb == float(np.float32(float(loader.K[0, 0]) * 0.54))
    assert data["depths"] == ("depths", 8) and tuple(data["poses"].shape) == (8, 4, 4) and data["poses"].dtype == torch.float32
    assert tuple(data["intrinsics"].shape) == (8, 4, 4) and float(data["poses"][2, 2, 3]) == np.float32(0.4 * 2)
    loader.load_data(SEQ, 5)                                         # the same existing frames: nothing goes up
    assert len(cache.uploads) == 1 and cache.gathers[1][0] == d
    # the generator asks for the base pose with the frame as a string: the same buffer entry
    assert loader.load_frame_data(SEQ, "4", "image_02")["pose"] is loader.buffer[(SEQ, 4, "image_02")]["pose"] and len(cache.uploads) == 1
    loader.load_data(SEQ, 4)                                         # the odd frames; frame 5's right camera lacks a file and is absent
    assert len(cache.uploads) == 2 and len(cache.uploads[1]["maps"]) == 14 and len(loader.buffer) == 15 and (SEQ, 5, "image_03") not in loader.buffer
    assert cache.gathers[2][0] == list(range(16, 30, 2))
    loader.purge_buffer()
    assert loader.buffer == {} and cache.resets == 1 and cache.used == 0
    # a short window: the next target frame of the same parity uploads only the frames that entered the window
    short = KITTILoader("unused", t, 12, 40, num_frames_bwd=2, num_frames_fwd=3, frame_cache=RecordingCache())
    short.load_data(SEQ, 3)
    short.load_data(SEQ, 5)
    assert [len(u["maps"]) for u in short.frame_cache.uploads] == [5 * 2, 2 * 2] and len(short.buffer) == 7
    with pytest.raises(ValueError):
        short.load_data(SEQ, 200)


def test_kitti_loader_frame_data_flow_and_unbuffered_loads(tmp_path):
    from footprints_amd.preprocessing.ground_truth_generation import KITTILoader
    t = write_kitti_gt_tree(tmp_path, SEQ, range(3), native=(20, 60), missing={(2, "image_02", "optical_flow")})
    cache = RecordingCache()
    loader = KITTILoader("unused", t, 12, 40, frame_cache=cache)
    assert loader.load_frame_data(SEQ, 7, "image_02") is None and loader.load_frame_data(SEQ, -1, "image_02") is None and not cache.uploads
    plain = loader.load_frame_data(SEQ, 1, "image_02")
    assert set(plain) == {"pose", "disparity", "ground_seg"} and plain["disparity"] == ("view", 0, None) and plain["ground_seg"] == ("view", 1, None)
    with_flow = loader.load_frame_data(SEQ, 1, "image_02", load_flow=True)             # buffered without flow: only the flow goes up
    assert with_flow["flow"] == ("view", 2, 2) and len(cache.uploads) == 2 and len(loader.buffer) == 1
    assert cache.uploads[1]["post"] == [(40.0, 60.0), (12.0, 20.0)] and cache.uploads[1]["slots"] == [2, 3]
    assert [m.shape for m in cache.uploads[1]["maps"]] == [(20, 60)] * 2
    fresh = loader.load_frame_data(SEQ, 0, "image_03", load_flow=True)                 # a miss with flow: four maps in one upload
    assert len(cache.uploads[2]["maps"]) == 4 and fresh["flow"] == ("view", 6, 2)
    assert loader.load_frame_data(SEQ, 2, "image_02", load_flow=True) is None and len(loader.buffer) == 2
    raw = loader.load_frame_data(SEQ, 1, "image_02", use_buffer=False, threshold_ground=False)
    assert cache.uploads[-1]["threshold"] == [None, None] and len(loader.buffer) == 2 and raw["disparity"] == ("view", 8, None)
    loader.load_frame_data(SEQ, 0, "image_02", use_buffer=False, threshold_ground=False)
    assert cache.uploads[-1]["slots"] == [8, 9] and cache.used == 12                   # unbuffered loads share their slots


def test_matterport_loader_lists_and_parses_a_scan(tmp_path):
    from footprints_amd.preprocessing.ground_truth_generation import MatterportLoader
    names = [("aa11", "0", "3"), ("aa11", "1", "0"), ("bb22", "2", "5")]
    raw, t = write_matterport_gt_tree(tmp_path, "scanA", names)
    open(os.path.join(t, "ground_seg", "scanA", "data", ".hidden_0_1.npy"), "w").close()
    open(os.path.join(t, "ground_seg", "scanA", "data", "notes.txt"), "w").close()
    cache = RecordingCache()
    loader = MatterportLoader(raw, t, 12, 16, footprint_threshold=0.7, frame_cache=cache)
    assert (loader.full_size_width, loader.full_size_height, loader.pose_tracker, loader.scan_data) == (1280.0, 1024.0, {}, None)
    data = loader.load_data("scanA", *names[1])
    host = GR.HostMatterportLoader(raw, t, 12, 16, footprint_threshold=0.7)
    ref = host.load_data("scanA", *names[1])
    assert list(loader.pose_tracker) == names == list(host.pose_tracker)
    for k in ("poses", "intrinsics", "inv_intrinsics"):
        assert torch.equal(data[k], ref[k]), k
    assert float(data["intrinsics"][2, 1, 2]) == np.float32(523.5 * 12 / 1024.0) and float(data["poses"][2, 2, 3]) == 2.0
    up = cache.uploads[0]
    assert len(cache.uploads) == 1 and up["method"] == "nearest" and up["slots"] == [2, 3, 4, 5, 6, 7] and up["post"] == [0.00025] * 3 + [1.0] * 3
    assert [m.dtype for m in up["maps"]] == [np.uint16] * 3 + [np.float16] * 3 and [m.shape for m in up["maps"]] == [(12, 16)] * 3 + [(24, 32)] * 3
    assert up["threshold"] == [None] * 3 + [float(np.float16(0.7))] * 3                  # the reference compares in the stored dtype
    from PIL import Image
    with Image.open(os.path.join(raw, "scanA", "scanA", "matterport_depth_images", "aa11_d1_0.png")) as im:
        assert np.array_equal(up["maps"][1], np.array(im.resize((16, 12), Image.NEAREST)))
    assert data["depths"] == ("view", 2, 3) and data["ground_segs"] == ("view", 5, 3)
    loader.load_data("scanA", *names[0])                                                # the same scan: nothing is read again
    assert len(cache.uploads) == 1
    loader.gather_frames([2, 0])
    assert cache.gathers[-1] == ([4, 2], [7, 5], None)
    with pytest.raises(ValueError):
        loader.gather_frames([3])
    seg, depth, pose, K = loader.load_frame_data("scanA", *names[2])
    assert (seg, depth) == (("view", 1, None), ("view", 0, None)) and cache.uploads[-1]["slots"] == [0, 1] and pose[2, 3] == 2.0
    assert np.array_equal(K, host.load_frame_data("scanA", *names[2])[3])


# ---- command line ---------------------------------------------------------------------------------------------------------------------------
def test_command_line_dispatches_to_the_five_generators(tmp_path, monkeypatch):
    from footprints_amd.preprocessing.ground_truth_generation import ground_truth_generator as G
    expected = {("kitti", "hidden_depths"): G.KITTIGroundTruthGenerator, ("kitti", "moving_objects"): G.KITTIMovingObjectDetector,
                ("kitti", "depth_masks"): G.KITTIDepthMaskingGenerator, ("matterport", "hidden_depths"): G.MatterportGroundTruthGenerator,
                ("matterport", "depth_masks"): G.MatterportDepthMaskingGenerator}
    (tmp_path / "paths.yaml").write_text("kitti:\n  dataset: /k/raw\n  training_data: /k/train\nmatterport:\n  dataset: /m/raw\n  training_data: /m/train\n")
    (tmp_path / "files.txt").write_text("b 2 l\na 1 r\nc 3 l\n")
    ran = []
    monkeypatch.setattr(G.GroundTruthGenerator, "run", lambda self: ran.append(self))
    for (data_type, kind), cls in expected.items():
        gen = G.main(["--data_type", data_type, "--type", kind, "--config_path", str(tmp_path / "paths.yaml"), "--textfile", str(tmp_path / "files.txt"),
                      "--footprint_threshold", "0.6", "--idx_start", "1"])
        assert type(gen) is cls and ran[-1] is gen and type(gen.loader) is cls.loader_class
        root = "/k" if data_type == "kitti" else "/m"
        assert (gen.loader.raw_data_path, gen.loader.training_data_path, gen.training_datapath) == (root + "/raw", root + "/train", root + "/train")
        assert (gen.loader.height, gen.loader.width) == (cls.height, cls.width) and gen.loader.footprint_threshold == 0.6
        assert gen.filenames == ["b 2 l", "c 3 l"]
    with pytest.raises(NotImplementedError):
        G.main(["--data_type", "matterport", "--type", "moving_objects", "--config_path", str(tmp_path / "paths.yaml")])
    for data_type, kind in ((None, "hidden_depths"), ("kitti", None)):
        with pytest.raises(NotImplementedError):
            G.generator_class(data_type, kind)
    assert len(ran) == 5


def test_run_prints_the_progress_lines(tmp_path, capsys):
    from footprints_amd.preprocessing.ground_truth_generation import ground_truth_generator as G
    (tmp_path / "files.txt").write_text("\n".join("s %d l" % i for i in range(27)) + "\n")

    class Gen(G.GroundTruthGenerator):
        height, width = 2, 3
        robust_aggregation = True

        def load_data(self, idx, filename):
            return filename

        def process_data(self, data, robust_aggregation=True):
            return data

        def save_result(self, result, filename, save_viz=False):
            saved.append((result, save_viz))
    saved = []
    import types
    Gen(G.get_options(["--textfile", str(tmp_path / "files.txt"), "--save_visualisations"]), types.SimpleNamespace(buffer={1: 2})).run()
    out = capsys.readouterr().out.splitlines()
    assert out[0] == "running ground truth generation on 27 files..." and out[1] == "computing image 0 of 27" and out[2] == "computing image 25 of 27"
    assert out[3].startswith("average time per image: ") and out[4] == "buffer size 1" and len(out) == 5
    assert len(saved) == 27 and saved[0] == ("s 0 l", True)
