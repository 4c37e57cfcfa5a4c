"""CPU: the host half of the segmentation reader -- the restatement (tests/seg_reader_restatement.py) against the installed Pillow and
against what the reference's own dataset code wrote (tests/golden/g16_seg_reader.npz), the library's host functions
(fp_nearest_index, fp_resize_coeffs_range) and the plan (footprints_amd/preprocessing/segmentation/datasets/plan.py)."""
import os
import random
import re

import numpy as np
import pytest

from tests import reader_restatement as RR
from tests import seg_reader_restatement as SR
from tests.golden import digest, seg_reader_inputs as SI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_WINDOW_CASES = SI.WINDOW_CASES + SI.GREY_CASES


def _pil():
    return pytest.importorskip("PIL.Image")


def _dedupe(sizes):
    """the sizes of a chain without the resizes that change nothing (the reference asks Pillow for those too)"""
    out = [tuple(sizes[0])]
    for s in sizes[1:]:
        if tuple(s) != out[-1]:
            out.append(tuple(s))
    return out


@pytest.fixture(scope="module")
def gold():
    return digest.load("g16_seg_reader")


@pytest.mark.parametrize("case", ALL_WINDOW_CASES, ids=[c[0] for c in ALL_WINDOW_CASES])
def test_restatement_window_equals_pillow(case):
    Image = _pil()
    name, (h, w), (th, tw), (top, left, wh, ww), c = case
    img = SI.image(h, w, c, 3)
    src = img[:, :, 0] if c == 1 else img
    ref = np.asarray(Image.fromarray(src).resize((tw, th), Image.LANCZOS).crop((left, top, left + ww, top + wh))).reshape(wh, ww, c)
    assert np.array_equal(SR.resize_window(img, th, tw, (top, left, wh, ww)), ref)


def test_restatement_chain_equals_pillow():
    Image = _pil()
    name, (h, w), s1, s2, (top, left, wh, ww), c = SI.CHAIN_CASE
    img = SI.image(h, w, c, 5)
    ref = Image.fromarray(img).resize(s1[::-1], Image.LANCZOS).resize(s2[::-1], Image.LANCZOS).crop((left, top, left + ww, top + wh))
    assert np.array_equal(SR.image_u8(img, h, [(h, w), s1, s2], (top, left, wh, ww)), np.asarray(ref))


def test_nearest_index_equals_pillow():
    Image = _pil()
    from footprints_amd import ops
    rng = np.random.default_rng(7)
    pairs = [(1, 1), (1, 9), (9, 1), (795, 318), (2048, 819), (5, 16), (18, 57)] + [tuple(int(v) for v in rng.integers(1, 2101, 2)) for _ in range(300)]
    for n_in, n_out in pairs:
        ramp = np.arange(n_in, dtype=np.int32).reshape(1, n_in)
        ref = np.asarray(Image.fromarray(ramp, mode="I").resize((n_out, 1), Image.NEAREST))[0]
        got = ops.nearest_index(n_in, n_out)
        assert got.dtype == np.int32 and np.array_equal(got, ref), (n_in, n_out)
        assert np.array_equal(SR.nearest_index(n_in, n_out), ref), (n_in, n_out)
    img = SI.labels("ADE20K", 37, 53, 2)                  # both axes at once, RGB and L
    for mode_img in (img, img[..., 1]):
        ref = np.asarray(Image.fromarray(mode_img).resize((44, 30), Image.NEAREST))
        assert np.array_equal(SR.nearest_resize(mode_img, 30, 44), ref)


def test_nearest_index_without_pillow():
    from footprints_amd import ops
    for n_in, n_out in [(1, 1), (7, 3), (3, 7), (795, 318), (2048, 819), (1024, 1024)]:
        got = ops.nearest_index(n_in, n_out)
        assert np.array_equal(got, SR.nearest_index(n_in, n_out))
        assert got.min() >= 0 and got.max() < n_in and np.all(np.diff(got) >= 0)
    assert np.array_equal(ops.nearest_index(9, 9), np.arange(9))
    with pytest.raises(Exception):
        ops.nearest_index(0, 4)


@pytest.mark.parametrize("sizes", [(260, 104), (53, 44), (12, 24), (2048, 1111), (37, 37 * 3)])
def test_coeffs_range_equals_rows_of_whole_table(sizes):
    from footprints_amd import ops
    n_in, n_out = sizes
    bounds, kk = ops.resize_tables(n_in, n_out)
    for first, count in [(0, n_out), (0, 1), (n_out - 1, 1), (n_out // 3, n_out // 2), (n_out - 5, 5)]:
        b, k = ops.resize_tables_range(n_in, n_out, first, count)
        assert np.array_equal(b, bounds[first:first + count]) and np.array_equal(k, kk[first:first + count])
    b, k = SR.coeffs_range(n_in, n_out, n_out // 3, 7)
    rb, rk = ops.resize_tables_range(n_in, n_out, n_out // 3, 7)
    assert np.array_equal(b, rb) and np.array_equal(k, rk)
    for first, count in [(-1, 2), (0, 0), (n_out - 1, 2)]:
        with pytest.raises(Exception):
            ops.resize_tables_range(n_in, n_out, first, count)


def test_window_axis_spans_are_the_union_of_the_bounds():
    from footprints_amd import ops
    bounds, _ = RR.coeffs(260, 104)
    t, lo, hi = ops.resize_window_axis(260, 104, 40, 24)
    assert t[0] == 40 and np.array_equal(t[1], bounds[40:64])
    assert lo == bounds[40:64, 0].min() and hi == (bounds[40:64, 0] + bounds[40:64, 1]).max()
    assert ops.resize_window_axis(50, 50, 7, 16) == (None, 7, 23)
    with pytest.raises(ValueError):
        ops.resize_window_axis(260, 104, 90, 24)


@pytest.mark.parametrize("case", SI.SAMPLES + SI.BIG, ids=[c[0] for c in SI.SAMPLES + SI.BIG])
def test_plan_reproduces_the_reference_sizes_and_windows(gold, case):
    """the sizes of every LANCZOS resize Pillow was asked for and crop_all's box, from the seeded stream and from the stored draws"""
    from footprints_amd.preprocessing.segmentation.datasets import plan as P
    name, dataset, hw, is_train, seed = case
    feed = SI.BIG_FEED if case in SI.BIG else SI.FEED
    rng = random.Random(seed)
    plan = P.draw_seg_plan(dataset, hw, feed, is_train, rng)
    ref_sizes = _dedupe([P.plan_sizes(plan)[0]] + [tuple(int(v) for v in s) for s in gold[name + ".resizes"]])
    assert P.plan_sizes(plan) == ref_sizes
    assert plan.window == tuple(int(v) for v in gold[name + ".window"])
    draws = gold[name + ".draws"]
    again = random.Random(seed)
    n_uniform = len(draws)
    assert [again.random() for _ in range(n_uniform)] == list(draws)          # the plan drew what the reference drew, in its order
    r = SR.plan_from_draws(dataset, hw, feed, is_train, draws)
    assert _dedupe(r["sizes"]) == ref_sizes and r["window"] == plan.window
    assert r["used"] + (2 if is_train else 0) == n_uniform
    if is_train:
        assert plan.aug.flip == int(draws[r["used"] + 1] > 0.5) and (plan.aug.n_ops == 4) == bool(draws[r["used"]] > 0.5)
    else:
        assert plan.aug.flip == 0 and plan.aug.n_ops == 0


def test_plan_branches_are_all_in_the_fixture(gold):
    sizes = {c[0]: _dedupe([c[2]] + [tuple(int(v) for v in s) for s in gold[c[0] + ".resizes"]]) for c in SI.SAMPLES if c[1] != "cityscapes"}
    assert sizes["ade_equal_ratio"] == [(8, 12), (24, 24)]                    # (feed_width, feed_width)
    assert sizes["ade_height"] == [(10, 40), (16, 64)] and sizes["ade_width"] == [(30, 20), (36, 24)]
    assert sizes["ade_exact"] == [(16, 24)] and sizes["ade_crop"] == [(40, 50)]
    assert len(sizes["mp_two_stage"]) == 3 and len(sizes["mp_two_stage_b"]) == 3 and len(sizes["mp_one_stage"]) == 2
    flips = [int(gold[c[0] + ".draws"][-1] > 0.5) for c in SI.SAMPLES if c[3]]
    jitters = [int(gold[c[0] + ".draws"][-2] > 0.5) for c in SI.SAMPLES if c[3]]
    assert 0 in flips and 1 in flips and 0 in jitters and 1 in jitters


def test_plan_draws_nothing_but_the_crop_in_validation():
    from footprints_amd.preprocessing.segmentation.datasets import plan as P

    class Counting(random.Random):
        n = 0

        def random(self):
            self.n += 1
            return super().random()
    rng = Counting(1)
    P.draw_seg_plan("cityscapes", (1024, 2048), (192, 640), False, rng)
    assert rng.n == 2
    rng = Counting(1)
    p = P.draw_seg_plan("ADE20K", (16, 24), (16, 24), False, rng)
    assert rng.n == 0 and p.window == (0, 0, 16, 24) and p.stage1 is None and p.stage2 is None
    with pytest.raises(ValueError):
        P.draw_seg_plan("kitti", (16, 24), (16, 24), False, rng)


@pytest.mark.parametrize("case", SI.SAMPLES, ids=[c[0] for c in SI.SAMPLES])
def test_restatement_equals_the_reference_written_sample(gold, case):
    from footprints_amd.preprocessing.segmentation.datasets import plan as P
    name, dataset, hw, is_train, seed = case
    _, image, labels = SI.sample_inputs(case)
    plan = P.draw_seg_plan(dataset, hw, SI.FEED, is_train, random.Random(seed))
    a = plan.aug
    img, ground, labelled = SR.sample(dataset, image, labels, plan.rows, P.plan_sizes(plan), plan.window, a.flip, a.n_ops, list(a.ops),
                                      list(a.factor), a.hue_shift)
    assert np.array_equal(img, gold[name + ".image"])
    assert np.array_equal(ground, gold[name + ".ground_mask"]) and np.array_equal(labelled, gold[name + ".labelled_pix"])


@pytest.mark.parametrize("case", SI.SAMPLES, ids=[c[0] for c in SI.SAMPLES])
def test_composed_label_tables_equal_the_chain(case):
    from footprints_amd import ops
    from footprints_amd.preprocessing.segmentation.datasets import plan as P
    name, dataset, hw, is_train, seed = case
    _, image, labels = SI.sample_inputs(case)
    plan = P.draw_seg_plan(dataset, hw, SI.FEED, is_train, random.Random(seed))
    rows, cols = P.label_tables(plan, ops.nearest_index)
    assert rows.dtype == np.int32 and rows.shape == (SI.FEED[0],) and cols.shape == (SI.FEED[1],)
    picked = labels[rows][:, cols]
    ids = picked[..., 0].astype(np.int64) // 10 * 256 + picked[..., 1] if dataset == "ADE20K" else (picked[..., 0] if picked.ndim == 3 else picked)
    ref = SR.label_ids(dataset, labels, plan.rows, P.plan_sizes(plan), plan.window)
    assert np.array_equal(ids, ref[:, ::-1] if plan.aug.flip else ref)


def test_image_stages_cover_exactly_what_the_taps_reach():
    from footprints_amd import ops
    from footprints_amd.preprocessing.segmentation.datasets import plan as P
    plan = P.draw_seg_plan("matterport", (20, 70), SI.FEED, True, random.Random(31))
    stages, rect = P.image_stages(plan, ops.resize_window_axis)
    assert [s["out_hw"] for s in stages] == [(5, 18), (16, 57)] and stages[1]["window"] == plan.window
    b_v, _ = RR.coeffs(5, 16)
    b_h, _ = RR.coeffs(18, 57)
    top, left, H, W = plan.window
    want = (b_v[top:top + H, 0].min(), b_h[left:left + W, 0].min())
    assert stages[0]["window"][:2] == want                                   # the first resize produces what the second one's taps reach
    assert rect[0] >= 0 and rect[0] + rect[2] <= 20 and rect[1] + rect[3] <= 70
    plan = P.draw_seg_plan("ADE20K", (40, 50), SI.FEED, False, random.Random(1))
    stages, rect = P.image_stages(plan, ops.resize_window_axis)
    assert len(stages) == 1 and stages[0]["table_h"] is None and stages[0]["table_v"] is None and rect == plan.window


def test_header_lists_the_new_entry_points():
    hdr = open(os.path.join(ROOT, "include", "footprints_hip.h")).read()
    from footprints_amd import _lib
    for name in ("fp_resize_window_u8", "fp_resize_window_workspace", "fp_resize_window_status_offset", "fp_resize_coeffs_range", "fp_nearest_index",
                 "fp_seg_labels", "fp_resize_window_sample_bytes", "fp_resize_window_table_bytes", "fp_seg_label_sample_bytes"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.SIGNATURES and hasattr(_lib.load(), name)
    lib = _lib.load()
    import ctypes as C
    assert lib.fp_resize_window_sample_bytes() == C.sizeof(_lib.ResizeWindowSample)
    assert lib.fp_resize_window_table_bytes() == C.sizeof(_lib.ResizeWindowTable)
    assert lib.fp_seg_label_sample_bytes() == C.sizeof(_lib.SegLabelSample)
    assert lib.fp_resize_window_workspace(2, 40, 24, 3) == ((2 * 40 * 24 * 3 + 15) & ~15) + 16
    assert lib.fp_resize_window_status_offset(2, 40, 24, 3) == lib.fp_resize_window_workspace(2, 40, 24, 3) - 16
    assert lib.fp_resize_window_workspace(2, 40, 24, 2) == -1 and lib.fp_resize_window_workspace(0, 40, 24, 3) == -1
