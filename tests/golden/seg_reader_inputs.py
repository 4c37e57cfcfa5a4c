"""Inputs of the segmentation-reader fixture (tests/golden/g16_seg_reader.npz) and of its tests, as pure functions of their arguments
(the integer hash of reader_inputs.py): decoded frames and label images of the three segmentation datasets at small native sizes."""
import numpy as np

from tests.golden.reader_inputs import image

FEED = (16, 24)
# (name, dataset, native (h, w), is_train, seed of Python's RNG).  Cityscapes frames need the 795 rows its _preprocess crops to.
SAMPLES = [
    ("cs_train_a", "cityscapes", (800, 90), True, 11),
    ("cs_train_b", "cityscapes", (810, 100), True, 12),
    ("cs_train_c", "cityscapes", (795, 64), True, 13),
    ("cs_val", "cityscapes", (800, 90), False, 14),
    ("ade_crop", "ADE20K", (40, 50), True, 21),                 # the feed size fits: crop only
    ("ade_exact", "ADE20K", (16, 24), True, 22),                # nothing at all
    ("ade_equal_ratio", "ADE20K", (8, 12), True, 23),           # the (feed_width, feed_width) quirk: 24 x 24, rows cropped
    ("ade_height", "ADE20K", (10, 40), True, 24),               # height is the constraint: 16 x 64
    ("ade_width", "ADE20K", (30, 20), True, 25),                # width is the constraint: 36 x 24
    ("ade_val", "ADE20K", (37, 53), False, 26),
    ("mp_two_stage", "matterport", (20, 70), True, 31),         # factor < 0.8: 20 rows shrink below 16, prepare_size resizes again
    ("mp_two_stage_b", "matterport", (64, 40), True, 36),        # width is the constraint of the second resize
    ("mp_one_stage", "matterport", (64, 80), True, 33),
    ("mp_val", "matterport", (20, 30), False, 34),
]
# the realistic size: two Cityscapes frames at 1024 x 2048, feed 192 x 640, resize factors near 0.7 (seeds chosen for that)
BIG_FEED = (192, 640)
BIG = [("big_a", "cityscapes", (1024, 2048), True, 50), ("big_b", "cityscapes", (1024, 2048), True, 61)]

_CS_IDS = np.array([0, 6, 7, 8, 9, 22, 5, 10, 21, 23, 1, 33])                       # ground ids, their neighbours, unlabelled
_ADE_IDS = np.array([0, 6655, 976, 975, 977, 2131, 2531, 2532, 737, 738, 1494, 1495, 3000, 838, 913])      # both ends of the range


def _hash(h, w, seed):
    y, x = np.meshgrid(np.arange(h, dtype=np.uint64), np.arange(w, dtype=np.uint64), indexing="ij")
    v = (y * np.uint64(104729) + x * np.uint64(7919) + np.uint64(seed) * np.uint64(15485863) + np.uint64(977)) * np.uint64(2654435761)
    v = (v ^ (v >> np.uint64(15))) * np.uint64(2246822519)
    return (v >> np.uint64(16)).astype(np.int64)


def labels(dataset, h, w, seed):
    """the decoded label image: uint8 [h, w, 3] (Cityscapes: three equal channels; ADE20K: R = id / 256 * 10 + class remainder, G = id % 256,
    B = instance noise) or uint8 [h, w] of zeros and ones (Matterport).  Ids change every 3 rows / 5 columns, and per pixel on every
    seventh row"""
    fine = _hash(h, w, seed)
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    coarse = _hash(h, w, seed + 1000)[(y // 3) * 3, (x // 5) * 5]
    pick = np.where(y % 7 == 0, fine, coarse)
    if dataset == "cityscapes":
        return np.repeat(_CS_IDS[pick % len(_CS_IDS)][..., None], 3, -1).astype(np.uint8)
    if dataset == "ADE20K":
        ids = _ADE_IDS[pick % len(_ADE_IDS)]
        r = ids // 256 * 10 + (fine >> 8) % np.where(ids // 256 == 25, 6, 10)
        return np.stack([r, ids % 256, (fine >> 4) % 256], -1).astype(np.uint8)
    return (pick % 3 == 0).astype(np.uint8)


def sample_inputs(case):
    """(dataset, image uint8 [h, w, 3], labels) of one entry of SAMPLES / BIG"""
    name, dataset, (h, w), is_train, seed = case
    return dataset, image(h, w, 3, seed), labels(dataset, h, w, seed)


# the windowed-resize cases of the GPU tests: (name, source (h, w), target (th, tw), window (top, left, h, w), channels)
WINDOW_CASES = [
    ("corner_top_left", (37, 53), (30, 44), (0, 0, 16, 24), 3),             # taps clamped at the borders
    ("corner_bottom_right", (37, 53), (30, 44), (14, 20, 16, 24), 3),
    ("interior_strong", (150, 260), (60, 104), (22, 40, 16, 24), 3),        # 17-tap rows
    ("horizontal_only", (30, 53), (30, 44), (7, 11, 16, 24), 3),            # table_v = -1
    ("vertical_only", (37, 44), (30, 44), (7, 11, 16, 24), 3),              # table_h = -1
    ("crop_only", (40, 50), (40, 50), (7, 11, 16, 24), 3),
    ("exact", (16, 24), (16, 24), (0, 0, 16, 24), 3),
    ("equal_ratio", (8, 12), (24, 24), (4, 0, 16, 24), 3),                  # the reference's quirk: rows cropped
    ("ragged", (37, 53), (31, 47), (3, 5, 17, 23), 3),                      # nothing a multiple of anything
]
GREY_CASES = [("grey", (37, 53), (30, 44), (5, 9, 16, 24), 1), ("grey_crop", (40, 50), (40, 50), (7, 11, 16, 24), 1)]
# a chain of two resizes: source (h, w), first target, second target, window of the second
CHAIN_CASE = ("chain", (20, 70), (10, 35), (16, 56), (0, 13, 16, 24), 3)
