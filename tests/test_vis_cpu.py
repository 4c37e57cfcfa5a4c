"""CPU: the NumPy restatement of the visualisation kernels (tests/vis_restatement.py) against the libraries it restates -- the installed
Pillow's mode-"F" BILINEAR resize, matplotlib's plasma map, and predict_simple.InferenceManager.visualise built on both -- and against the
fixture g15_vis those libraries wrote; then the library's double coefficient tables against the restatement's, bit for bit, and the int32
tables of fp_resize_coeffs against the restatement that pinned them before.  No tolerance anywhere."""
import functools

import numpy as np
import pytest
import torch

from tests import reader_restatement as RR
from tests import vis_restatement as VR
from tests.golden import digest

LIMIT = 1 << 10
SIZES = [(192, 640, 375, 1242), (192, 640, 100, 333), (192, 640, 480, 640), (32, 64, 37, 124), (32, 64, 13, 29), (32, 64, 61, 50),
         (32, 64, 1, 3), (32, 64, 32, 64)]


@functools.lru_cache(None)
def gold():
    return digest.load("g15_vis")


@functools.lru_cache(None)
def lut():
    t = gold()["lut"]
    t.setflags(write=False)
    return t


def matches(name, arr):
    g = gold()
    d = digest.digest(name, torch.from_numpy(np.array(arr)), full_limit=LIMIT)
    return all(k in g.files and np.array_equal(g[k], v) for k, v in d.items())


def test_colour_table_is_matplotlibs_and_the_blend_is_a_selection():
    plt = pytest.importorskip("matplotlib.pyplot")
    cmap = plt.get_cmap("plasma", 256)
    assert np.array_equal(lut(), (cmap(np.arange(256))[:, :3] * 255).astype(np.uint8))
    # the index rule on a float32 array, every representable kind of input: grid points, their neighbours, the ends
    x = np.concatenate([np.arange(257, dtype=np.float32) / np.float32(256), np.nextafter(np.arange(1, 257, dtype=np.float32) / np.float32(256), np.float32(0)),
                        VR._hash((4096,), 1).astype(np.float32)])
    x = np.clip(x, 0, 1)
    assert np.array_equal((cmap(x)[:, :3] * 255).astype(np.uint8), lut()[VR.colour_index(x)])
    b = np.arange(256, dtype=np.uint8)
    assert np.array_equal(((b / 255.0) * 255).astype(np.uint8), b)                                   # the photo's bytes survive the float64 blend
    assert np.array_equal(((b.astype(np.float32) / np.float32(255)) * np.float32(255)).astype(np.uint8), b)    # and ToTensor's floats the side-by-side


@pytest.mark.parametrize("H,W,h,w", SIZES)
def test_float_resample_equals_pillow(H, W, h, w):
    Image = pytest.importorskip("PIL.Image")
    a = VR.prediction(H, W, 3)[1] if H < 100 else (VR._hash((H, W), 5) * 6 - 3).astype(np.float32)
    ref = np.asarray(Image.fromarray(a, "F").resize((w, h), Image.BILINEAR))
    got = VR.resize_f32(a, h, w)
    assert got.dtype == np.float32 and got.tobytes() == ref.tobytes()


@pytest.mark.parametrize("name", [c[0] for c in VR.SIZE_CASES])
def test_overlay_equals_visualise_and_fixture(name):
    Image = pytest.importorskip("PIL.Image")
    pytest.importorskip("matplotlib")
    from footprints_amd.predict_simple import InferenceManager
    pred, orig = VR.size_case_inputs(name)
    got = VR.overlay(pred, orig, lut())
    assert np.array_equal(got, InferenceManager.visualise(pred, Image.fromarray(orig)))
    assert matches("vis.%s" % name, got)
    assert matches("rf.%s" % name, VR.resize_f32(pred[1], *orig.shape[:2]).view(np.uint8))      # the fixture holds the floats' bytes
    assert (got != orig).any() and (got == orig).all(axis=2).any()        # both sides of the mask are present


def test_overlay_value_cases_equal_visualise_and_fixture():
    Image = pytest.importorskip("PIL.Image")
    pytest.importorskip("matplotlib")
    from footprints_amd.predict_simple import InferenceManager
    cases = VR.value_cases()
    for name, pred in cases.items():
        for h, w in VR.VALUE_SIZES:
            orig = VR.original(h, w, 60)
            got = VR.overlay(pred, orig, lut())
            assert np.array_equal(got, InferenceManager.visualise(pred, Image.fromarray(orig))), (name, h, w)
            assert matches("vis.%s.%dx%d" % (name, h, w), got), (name, h, w)
    assert not (VR.overlay_maps(cases["empty_mask"], 37, 124)[0] > 0.5).any()
    assert (VR.overlay_maps(cases["one_pixel"], 32, 64)[0] > 0.5).sum() == 1
    lg, dp = VR.overlay_maps(cases["constant_depth"], 37, 124)
    assert dp[lg > 0.5].max() == dp[lg > 0.5].min()
    lg = VR.overlay_maps(cases["logit_half"], 37, 124)[0]
    assert (lg == np.float32(0.5)).sum() > 0                              # exactly at the threshold: outside the mask


def test_side_by_side_equals_fixture_and_its_inputs_keep_the_condition():
    image, pred = VR.side_by_side_inputs()
    lg = pred[:, 1].astype(np.float64)
    assert not ((lg > 0) & (lg < 1e-6)).any()                             # where `logit > 0` and the fp32 `sigmoid > 0.5` could differ
    assert (lg == 0).sum() >= 8 and np.signbit(pred[:, 1][lg == 0]).any() and not np.signbit(pred[:, 1][lg == 0]).all()
    got = VR.side_by_side(image, pred, lut()[0], lut()[255])
    assert got.shape == (2, 32, 128, 3) and matches("sbs", got)
    sig = torch.sigmoid(torch.from_numpy(pred[:, 1])).numpy()            # the reference's own predicate, in fp32
    assert np.array_equal((got[:, :, 64:] == lut()[255]).all(axis=3), sig > 0.5)


# ---- the library's host functions (no GPU needed) --------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_size,out_size", [(640, 1242), (192, 375), (640, 333), (64, 29), (64, 3), (32, 1), (5, 2), (1242, 640)])
@pytest.mark.parametrize("fname", sorted(RR.FILTERS))
def test_double_tables_equal_the_restatement_bit_for_bit(in_size, out_size, fname):
    from footprints_amd import ops
    bounds, kk = ops.vis_tables(in_size, out_size, fname)
    rb, rk = VR.coeffs_f64(in_size, out_size, RR.FILTERS[fname])
    assert kk.dtype == np.float64 and kk.shape == rk.shape
    assert np.array_equal(bounds, rb) and kk.tobytes() == rk.tobytes()
    assert ops.vis_tables(in_size, out_size, fname)[1] is kk              # cached


@pytest.mark.parametrize("in_size,out_size", [(1242, 640), (375, 192), (53, 24), (24, 53), (5, 2), (7, 3), (640, 640)])
@pytest.mark.parametrize("fname", sorted(RR.FILTERS))
def test_quantised_tables_are_unchanged(in_size, out_size, fname):
    """fp_resize_coeffs now shares its double stage with fp_resize_coeffs_f64: same int32 bytes as the restatement that pinned it"""
    import ctypes as C
    from footprints_amd import _lib
    lib = _lib.load()
    f = RR.FILTERS[fname]
    ks = lib.fp_resize_ksize(in_size, out_size, f)
    rb, rk = RR.coeffs(in_size, out_size, f)
    assert ks == rk.shape[1]
    bounds, kk = np.full((out_size, 2), -7, np.int32), np.full((out_size, ks), -7, np.int32)
    assert lib.fp_resize_coeffs(in_size, out_size, f, bounds.ctypes.data, kk.ctypes.data, ks) == 0
    assert bounds.tobytes() == rb.tobytes() and kk.tobytes() == rk.tobytes()
    assert lib.fp_resize_coeffs_f64(in_size, out_size, f, bounds.ctypes.data, None, ks) == -1
    assert lib.fp_resize_coeffs_f64(in_size, out_size, 9, bounds.ctypes.data, kk.ctypes.data, ks) == -1


def test_overlay_workspace_query_refuses_what_is_too_large():
    from footprints_amd import _lib
    lib = _lib.load()
    assert lib.fp_vis_overlay_workspace(12, 192, 640, 376, 1242) > 12 * 376 * 1242 * 5
    off = lib.fp_vis_overlay_status_offset(12, 192, 640, 376, 1242)
    assert 0 < off == lib.fp_vis_overlay_workspace(12, 192, 640, 376, 1242) - 16
    for bad in ((0, 192, 640, 376, 1242), (1, 192, 640, 0, 1242), (1, 192, 640, 40000, 40000), (70000, 4, 4, 4, 4)):
        assert lib.fp_vis_overlay_workspace(*bad) == -1 and lib.fp_vis_overlay_status_offset(*bad) == -1


def test_predict_simple_new_flags_default_to_the_old_behaviour():
    from footprints_amd.predict_simple import parse_args
    a = parse_args(["--image", "x", "--model", "kitti"])
    assert a.device_vis is False and a.batch_size == 1
    a = parse_args(["--image", "x", "--model", "kitti", "--device_vis", "--batch_size", "12"])
    assert a.device_vis is True and a.batch_size == 12


def test_size_cases_have_seven_taps_and_a_window_wider_than_the_input():
    """properties of the GPU tests' inputs (tests/test_gpu_vis.py): the down-scale case has 7 taps in both axes and leaves the next sample's
    base unaligned; the 1 x 3 case asks for a source window wider than the prediction"""
    assert VR.coeffs_f64(64, 29)[1].shape[1] == 7 and VR.coeffs_f64(32, 13)[1].shape[1] == 7
    bounds, kk = VR.coeffs_f64(32, 1)
    assert kk.shape[1] > 32 and tuple(bounds[0]) == (0, 32)
    assert (13 * 29 * 3) % 2 == 1


def test_evaluation_manager_reads_save_test_visualisations_from_the_options():
    from types import SimpleNamespace
    from footprints_amd.evaluation.inference import InferenceManager
    mm = SimpleNamespace(model=torch.nn.Identity())
    for flag in (False, True):
        opt = SimpleNamespace(load_path=None, inference_save_path="somewhere", save_test_visualisations=flag)
        im = InferenceManager.from_options(opt, model_manager=mm)
        assert im.save_test_visualisations is flag and im.savepath == "somewhere" and im.model is mm.model
