"""Host plan of one segmentation training sample: every size, crop offset and augmentation decision the reference's dataset classes
make, taken before any pixel is touched.

Reference: footprints/preprocessing/segmentation/datasets/base_dataset.py:62-102 (`__getitem__`, `_augment_data`),
dataset_utils.py:24-91 (`prepare_size`, `crop_all`, `resize_all`), cityscapes_dataset.py:46-59 and matterport_dataset.py:44-53
(`_preprocess`).  The crop offsets depend only on the image sizes and the random draws, so the device resizes nothing but the window
that `crop_all` keeps (csrc/seg_reader.hip).

All size arithmetic is written as the reference writes it (Python floats, `int()` truncation, the same order of operations), quirks
included: when the aspect ratios of the image and the feed size agree exactly, `prepare_size` resizes to (feed_width, feed_width).

Random draws: the reference splits them between Python's `random` (resize factor, crop offsets, ColorJitter.get_params) and
`torch.rand(2)` (colour augmentation, flip).  Here ALL of them come from the one `rng`, in the reference's order: resize factor, top,
left, colour-augmentation draw, flip draw, then ColorJitter's own draws -- a seeded run makes the reference's decisions when the
reference's two torch draws are fed from the same stream.
"""
import random
from collections import namedtuple

import numpy as np

from ....datasets.device_path import AugParams, draw_jitter

DATASETS = ("ADE20K", "cityscapes", "matterport")
SEG_JITTER_RANGES = ((0.7, 1.3), (0.8, 1.2), (0.7, 1.3), (-0.1, 0.1))      # base_dataset.py:21-24: ColorJitter(0.3, 0.2, 0.3, 0.1)
CITYSCAPES_ROWS = 795                                                      # cityscapes_dataset.py:48: the ego car is cropped away
# (offset, scale) of `resize_factor = offset + scale * random.random()`; None: no resize in _preprocess
RESIZE_FACTOR = {"ADE20K": None, "cityscapes": (0.4, 0.6), "matterport": (0.25, 0.75)}
# ground ids: ade20k_dataset.py:16-31, cityscapes_dataset.py:18-23, matterport_dataset.py:18-21
GROUND_IDS = {"ADE20K": (976, 2131, 1125, 2377, 838, 913, 2212, 1788, 2530, 2185, 2531, 738, 1401, 1494),
              "cityscapes": (6, 7, 8, 9, 22),
              "matterport": (1,)}

# src_hw: the decoded frame; rows: the source rows that take part (Cityscapes' crop); stage1 / stage2: (height, width) targets of the
# _preprocess resize and of prepare_size's resize, None where that resize does not change the size; window = (top, left, H, W) in
# the last target; factor: the resize factor drawn (None without one)
SegPlan = namedtuple("SegPlan", "dataset src_hw rows stage1 stage2 window aug factor")


def prepare_size_target(height, width, feed_height, feed_width):
    """dataset_utils.py:28-52 with keep_aspect_ratio=True -> (target_height, target_width)"""
    if feed_height <= height and feed_width <= width:
        return height, width
    current_ratio = height / width
    target_ratio = feed_height / feed_width
    if current_ratio < target_ratio:
        return feed_height, int(feed_height / height * width)
    if current_ratio > target_ratio:
        return int(feed_width / width * height), feed_width
    return feed_width, feed_width               # "ratio is the same - just resize": the reference's bug, reproduced


def draw_seg_plan(dataset, src_hw, feed_hw, is_train, rng=random):
    """the plan of one sample of `dataset` whose decoded frame is src_hw = (h, w), for the feed size feed_hw = (H, W)"""
    if dataset not in DATASETS:
        raise ValueError("dataset must be one of %r" % (DATASETS,))
    h, w = int(src_hw[0]), int(src_hw[1])
    H, W = int(feed_hw[0]), int(feed_hw[1])
    rows = h
    if dataset == "cityscapes":
        if h < CITYSCAPES_ROWS:
            raise ValueError("a Cityscapes frame has at least %d rows (PIL's crop would pad a shorter one)" % CITYSCAPES_ROWS)
        rows = CITYSCAPES_ROWS
    height, width = rows, w
    factor, stage1 = None, None
    if is_train and RESIZE_FACTOR[dataset] is not None:
        offset, scale = RESIZE_FACTOR[dataset]
        factor = offset + scale * rng.random()
        stage1 = (int(height * factor), int(width * factor))
        height, width = stage1
    target = prepare_size_target(height, width, H, W)
    stage2 = target if target != (height, width) else None
    top = left = 0
    if target != (H, W):                        # crop_all
        top = int(rng.random() * (target[0] - H))
        left = int(rng.random() * (target[1] - W))
    if min(target) <= 0 or top < 0 or left < 0 or top + H > target[0] or left + W > target[1]:
        raise ValueError("the feed size %r does not fit the resized image %r" % ((H, W), target))
    aug = AugParams()
    if is_train:                                # _augment_data: rands[0] colour, rands[1] flip, both drawn first
        colour, flip = rng.random(), rng.random()
        if colour > 0.5:
            draw_jitter(aug, SEG_JITTER_RANGES, rng)
        aug.flip = int(flip > 0.5)
    if stage1 == (rows, w):
        stage1 = None
    return SegPlan(dataset, (h, w), rows, stage1, stage2, (top, left, H, W), aug, factor)


def plan_sizes(plan):
    """[(height, width)] of the image before the first resize and after every resize that happens"""
    sizes = [(plan.rows, plan.src_hw[1])]
    for s in (plan.stage1, plan.stage2):
        if s is not None:
            sizes.append(s)
    return sizes


def label_tables(plan, nearest_index):
    """row crop o NEAREST resizes o crop window o flip composed into (rows int32 [H], cols int32 [W]): the source row / column of
    every output row / column in the decoded label image.  nearest_index(in_size, out_size) -> int32 [out_size] (ops.nearest_index)"""
    top, left, H, W = plan.window
    rows = np.arange(top, top + H, dtype=np.int64)
    cols = np.arange(left, left + W, dtype=np.int64)
    if plan.aug.flip:
        cols = cols[::-1]
    sizes = plan_sizes(plan)
    for (ih, iw), (oh, ow) in reversed(list(zip(sizes[:-1], sizes[1:]))):
        if ih != oh:
            rows = nearest_index(ih, oh)[rows]
        if iw != ow:
            cols = nearest_index(iw, ow)[cols]
    return np.ascontiguousarray(rows, dtype=np.int32), np.ascontiguousarray(cols, dtype=np.int32)


def image_stages(plan, window_axis, whole_tables=False):
    """the chain of windowed resizes that produces the plan's window, worked out backwards from it.
    window_axis(in_size, out_size, first, count, whole_table=...) -> (table, lo, hi) (ops.resize_window_axis).
    -> (stages, rect): stages, first resize first, are dicts(in_hw, out_hw, window, table_h, table_v) whose window is what that resize
    has to produce -- for the last one the plan's window, for an earlier one the rectangle the next one's taps reach; rect = (y0, x0, h,
    w) of the decoded frame that the first stage's taps reach.  Without any resize there is one stage that copies the window."""
    sizes = plan_sizes(plan)
    need = plan.window
    stages = []
    pairs = list(zip(sizes[:-1], sizes[1:])) or [(sizes[0], sizes[0])]
    for (ih, iw), (oh, ow) in reversed(pairs):
        top, left, wh, ww = need
        tv, y_lo, y_hi = window_axis(ih, oh, top, wh, whole_table=whole_tables)
        th, x_lo, x_hi = window_axis(iw, ow, left, ww, whole_table=whole_tables)
        stages.append(dict(in_hw=(ih, iw), out_hw=(oh, ow), window=need, table_h=th, table_v=tv))
        need = (y_lo, x_lo, y_hi - y_lo, x_hi - x_lo)
    return stages[::-1], need
