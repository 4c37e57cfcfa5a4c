"""GPU: fp_gt_frame_resize and fp_gt_gather_frames (csrc/gt_frames.hip) bit for bit against the numpy restatement
(tests/gt_frames_restatement.py, pinned by tests/test_gt_frames_cpu.py), and the five label generators from dataset folders -- through
`from_options` and data_loader.py's loaders -- against the same generators over the restated reference loaders.  No tolerance anywhere:
every comparison is on the float32 bits or on the saved files' bytes."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import gt_frames_restatement as GR
from tests.test_gt_frames_cpu import SEQ, write_kitti_gt_tree, write_matterport_gt_tree

pytestmark = pytest.mark.gpu

DTYPES = (np.float16, np.float32, np.float64, np.uint16)


def bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.int32), b.view(np.int32))


def random_map(rng, shape, dtype):
    if dtype == np.uint16:
        return rng.integers(0, 65536, shape).astype(np.uint16)
    return (rng.random(shape) * 60.0 - 6.0).astype(dtype)


def run_launch(maps, H, W, slots, n_slots, method, pre, post, threshold):
    """one fp_gt_frame_resize launch into a cache of n_slots slots filled with -7 -> the cache as an array"""
    from footprints_amd import ops
    tables = ops.linear_table_set("cuda")
    cache = torch.full((n_slots, H, W), -7.0, dtype=torch.float32, device="cuda")
    pack = ops.gt_frame_pack(maps, H, W, [s * H * W for s in slots], cache.numel(), method, pre, post, threshold, tables)
    ops.gt_frame_resize(pack, torch.from_numpy(pack.packed[:pack.total]).cuda(), cache)
    torch.cuda.synchronize()
    return cache.cpu().numpy()


@functools.lru_cache(None)
def mixed_launch():
    """the 4 x 6 launch: six native sizes x four stored dtypes, threshold on and off, pre and post other than 1, slots out of order"""
    rng = np.random.default_rng(29)
    sizes = [(6, 10), (8, 12), (8, 10), (4, 6), (3, 5), (1, 1)]
    maps, pre, post, thr = [], [], [], []
    for k, size in enumerate(sizes):
        for j, dt in enumerate(DTYPES):
            maps.append(random_map(rng, size, dt))
            pre.append(1.0 if dt == np.uint16 or (k + j) % 3 == 0 else 6 / size[1])
            post.append([1.0, (6.0, float(size[1])), 0.00025, (4.0, float(size[0]))][(k + j) % 4])
            thr.append(None if (k + 2 * j) % 3 else 24.0 * (post[-1][0] / post[-1][1] if isinstance(post[-1], tuple) else post[-1]))
    slots = list(rng.permutation(len(maps) + 3))[:len(maps)]
    ref = [GR.frame(m, 4, 6, "linear", p, q, t) for m, p, q, t in zip(maps, pre, post, thr)]
    return maps, pre, post, thr, [int(s) for s in slots], ref


def test_one_launch_of_mixed_records_equals_the_restatement_bit_for_bit():
    from footprints_amd import _lib, ops
    maps, pre, post, thr, slots, ref = mixed_launch()
    got = run_launch(maps, 4, 6, slots, len(maps) + 3, "linear", pre, post, thr)
    for j, s in enumerate(slots):
        assert bits_equal(got[s], ref[j]), (j, maps[j].shape, maps[j].dtype, pre[j], post[j], thr[j])
    assert all((got[s] == -7.0).all() for s in set(range(len(maps) + 3)) - set(slots))           # every other slot is untouched
    # the records took the three paths, and thresholds gave both values
    pack = ops.gt_frame_pack(maps, 4, 6, [0] * len(maps), 24, "linear", pre, post, thr, ops.linear_table_set("cuda"))
    assert [r.method for r in pack.records] == [_lib.GT_LINEAR] * 4 + [_lib.GT_AREA2] * 4 + [_lib.GT_LINEAR] * 16
    on = np.stack([ref[j] for j in range(len(maps)) if thr[j] is not None])
    assert set(np.unique(on)) == {0.0, 1.0} and 0.1 < on.mean() < 0.9
    # nearest: resized, and the same-size copy
    near = run_launch(maps, 4, 6, list(range(len(maps))), len(maps), "nearest", pre, post, thr)
    for j in range(len(maps)):
        assert bits_equal(near[j], GR.frame(maps[j], 4, 6, "nearest", pre[j], post[j], thr[j])), j
    assert maps[13].shape == (4, 6) and (pre[13], post[13], thr[13]) == (1.0, 1.0, None) and np.array_equal(near[13], maps[13])


@pytest.mark.parametrize("dtype", DTYPES)
def test_more_than_one_block_per_record(dtype):
    rng = np.random.default_rng(31)
    maps = [random_map(rng, (40, 70), dtype), random_map(rng, (66, 128), dtype), random_map(rng, (33, 64), dtype)]
    pre = 1.0 if dtype == np.uint16 else 64 / 70
    got = run_launch(maps, 33, 64, [2, 0, 1], 3, "linear", pre, (64.0, 70.0), [None, None, 11.0])
    for j, s in enumerate([2, 0, 1]):
        assert bits_equal(got[s], GR.frame(maps[j], 33, 64, "linear", pre, (64.0, 70.0), [None, None, 11.0][j])), j


def test_one_kitti_sized_disparity_and_its_segmentation():
    rng = np.random.default_rng(37)
    disp = (rng.random((375, 1242)) * 90.0 + 0.5).astype(np.float32)
    seg = rng.random((375, 1242)).astype(np.float16)
    got = run_launch([disp, seg], 192, 640, [0, 1], 2, "linear", [640 / 1242, 1.0], 1.0, [None, 0.75])
    assert bits_equal(got[0], GR.frame(disp, 192, 640, "linear", 640 / 1242))
    assert bits_equal(got[1], GR.frame(seg, 192, 640, "linear", threshold=0.75)) and 0.05 < got[1].mean() < 0.5


@pytest.mark.parametrize("B", [1, 3, 76])
@pytest.mark.parametrize("hw", [(5, 7), (12, 40)])
def test_gather_frames_equals_numpy(B, hw):
    """(5, 7): H * W is no multiple of 4, one float per thread; (12, 40): four"""
    from footprints_amd import ops
    rng = np.random.default_rng(41 + B)
    cache = (rng.random((9,) + hw) * 50.0 + 0.01).astype(np.float32)                   # strictly positive disparities
    d_idx, s_idx = rng.integers(0, 9, B), rng.integers(0, 9, B)
    fb = np.float32(float(np.float32(0.58 * 640)) * 0.54)
    dev = torch.from_numpy(cache).cuda()
    depths, segs = ops.gt_gather_frames(dev, d_idx, s_idx, float(fb))
    plain, _ = ops.gt_gather_frames(dev, d_idx, s_idx, None)
    torch.cuda.synchronize()
    assert tuple(depths.shape) == tuple(segs.shape) == (B,) + hw
    assert bits_equal(depths.cpu().numpy(), fb / cache[d_idx]) and bits_equal(segs.cpu().numpy(), cache[s_idx])
    assert bits_equal(plain.cpu().numpy(), cache[d_idx])


# ---- end to end: the five generators from folders -------------------------------------------------------------------------------------------
def _saved(folder):
    out = {}
    for root, _, files in os.walk(folder):
        for f in files:
            with open(os.path.join(root, f), "rb") as fh:
                out[os.path.relpath(os.path.join(root, f), folder)] = fh.read()
    return out


def _both_ways(tmp_path, cls, data_type, host_loader, lines, extra=()):
    """run `cls` over the textfile through from_options and over the restated reference loader -> (generator, files, files)"""
    from footprints_amd.preprocessing.ground_truth_generation import get_options
    (tmp_path / "files.txt").write_text("\n".join(lines) + "\n")
    argv = ["--config_path", str(tmp_path / "paths.yaml"), "--textfile", str(tmp_path / "files.txt"), "--data_type", data_type] + list(extra)
    np.random.seed(123)
    gen = cls.from_options(get_options(argv + ["--save_folder_name", "out_device"]))
    gen.run()
    torch.cuda.synchronize()
    np.random.seed(123)
    cls(get_options(argv + ["--save_folder_name", "out_host"]), host_loader, training_datapath=gen.training_datapath).run()
    a, b = _saved(os.path.join(gen.training_datapath, "out_device")), _saved(os.path.join(gen.training_datapath, "out_host"))
    assert len(a) == len(lines) and set(a) == set(b)
    for name in a:
        assert a[name] == b[name], name
    return gen, a


@pytest.mark.parametrize("kind", ["hidden_depths", "moving_objects", "depth_masks"])
@pytest.mark.parametrize("native", [(24, 80), (26, 90)])
def test_kitti_generators_from_folders_equal_the_reference_loader(tmp_path, kind, native):
    """native 24 x 80 is exactly twice the 12 x 40 target (the area path); 26 x 90 takes the linear tables"""
    from footprints_amd.preprocessing.ground_truth_generation import ground_truth_generator as G

    class Small(G.generator_class("kitti", kind)):
        height, width = 12, 40
    t = write_kitti_gt_tree(tmp_path, SEQ, range(8), native=native, seed=native[0])
    (tmp_path / "paths.yaml").write_text("kitti:\n  dataset: %s\n  training_data: %s\n" % (tmp_path / "raw", t))
    lines = ["%s 3 l" % SEQ, "%s 4 r" % SEQ, "%s 5 l" % SEQ]
    gen, files = _both_ways(tmp_path, Small, "kitti", GR.HostKITTILoader(str(tmp_path / "raw"), t, 12, 40), lines)
    results = [np.load(os.path.join(gen.training_datapath, "out_device", name)) for name in files]
    assert all(r.shape == (12, 40) for r in results) and sum(int(np.count_nonzero(r)) for r in results) > 0
    loader = gen.loader
    assert all(isinstance(k[1], int) for k in loader.buffer)                             # each frame once: no second entry under a string
    if kind == "hidden_depths":
        assert len(loader.buffer) == 16 and sum(n for n, _ in loader.frame_cache.uploads) == 32 and loader.frame_cache.used == 32
    elif kind == "moving_objects":
        assert sorted(k[1:] for k in loader.buffer) == [(2, "image_02"), (3, "image_02"), (3, "image_03"), (4, "image_02"), (4, "image_03"),
                                                        (5, "image_02")]
        assert loader.frame_cache.used == 24
    else:
        assert loader.buffer == {} and loader.frame_cache.used == 4


@pytest.mark.parametrize("kind", ["hidden_depths", "depth_masks"])
@pytest.mark.parametrize("threshold", [0.75, 0.7])
def test_matterport_generators_from_folders_equal_the_reference_loader(tmp_path, kind, threshold):
    """threshold 0.7 is no float16 value: the reference compares the stored float16 map with float16(0.7) = 0.7002, and a block of every
    segmentation holds exactly that value -- ground under a comparison in double, not ground under the reference's"""
    from footprints_amd.preprocessing.ground_truth_generation import ground_truth_generator as G

    class Small(G.generator_class("matterport", kind)):
        height, width = 12, 40
    names = [("aa11", "0", "3"), ("aa11", "1", "0"), ("bb22", "0", "1"), ("bb22", "2", "5"), ("cc33", "1", "2")]
    raw, t = write_matterport_gt_tree(tmp_path, "scanA", names, native=(24, 80), depth_native=(30, 100), seed=7)
    (tmp_path / "paths.yaml").write_text("matterport:\n  dataset: %s\n  training_data: %s\n" % (raw, t))
    for n in names:
        path = os.path.join(t, "ground_seg", "scanA", "data", "%s_%s_%s.npy" % n)
        seg = np.load(path)
        seg[0, 14:20, 10:50] = np.float16(0.7)
        assert seg.dtype == np.float16 and float(seg[0, 14, 10]) > 0.7 and not (seg[0, 14, 10] > 0.7)
        np.save(path, seg)
    lines = ["scanA %s %s %s" % n for n in (names[0], names[2], names[4])]
    gen, files = _both_ways(tmp_path, Small, "matterport", GR.HostMatterportLoader(raw, t, 12, 40, footprint_threshold=threshold), lines,
                            ["--footprint_threshold", str(threshold)])
    assert gen.loader.footprint_threshold == threshold
    results = [np.load(os.path.join(gen.training_datapath, "out_device", name)) for name in files]
    assert all(r.shape == (12, 40) for r in results) and sum(int(np.count_nonzero(r)) for r in results) > 0
    if kind == "hidden_depths":
        assert len(gen.loader.pose_tracker) == 5 and gen.loader.frame_cache.used == 12 and len(gen.loader.frame_cache.uploads) == 1
        assert tuple(gen.loader.scan_data["depths"].shape) == (5, 12, 40) and gen.loader.scan_data["depths"].is_cuda


def test_linear_equals_cv2_where_cv2_exists():
    """skips wherever cv2 is missing -- which includes the machines this suite was written on: `linear` is a reading of OpenCV's portable
    path that no cv2 binary has confirmed yet"""
    cv2 = pytest.importorskip("cv2")
    cv2.ipp.setUseIPP(False)
    cv2.setNumThreads(0)
    rng = np.random.default_rng(43)
    for src, dst in (((6, 10), (4, 6)), ((8, 12), (4, 6)), ((8, 10), (4, 6)), ((3, 5), (4, 6)), ((1, 1), (4, 6)), ((40, 70), (33, 64)),
                     ((375, 1242), (192, 640))):
        m = rng.random(src) * 60.0
        ref = cv2.resize(m, (dst[1], dst[0])).astype(np.float32)
        assert bits_equal(run_launch([m], dst[0], dst[1], [0], 1, "linear", 1.0, 1.0, None)[0], ref), (src, dst)
