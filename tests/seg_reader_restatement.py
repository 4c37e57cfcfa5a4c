"""NumPy restatement of what csrc/resample_u8.hip, csrc/seg_reader.hip and footprints_amd/preprocessing/segmentation/datasets/plan.py do for a sample of the
ground-segmentation trainer (no Pillow needed), built on tests/reader_restatement.py (Pillow's 8-bit resample) and on
oracle/data_path.jitter_np (torchvision 0.4.2's ColorJitter in Pillow's byte arithmetic):

* the windowed resize: `Image.resize((tw, th), LANCZOS).crop(window)` -- here literally the whole resize, then the crop;
* Pillow's NEAREST resize (libImaging Geometry.c: the source coordinate starts at half a step and is accumulated in double);
* the composed label path of the three datasets (footprints/preprocessing/segmentation/datasets/*_dataset.py): row crop, NEAREST
  resizes, crop window, flip, id decode, np.in1d against the ground ids, `labelled_pix`;
* the plan arithmetic of `prepare_size` / `crop_all` / `_preprocess` (dataset_utils.py:24-81), written a second time.

tests/test_seg_reader_cpu.py pins all of it to the installed Pillow and to the reference's own code (tests/golden/g16_seg_reader.npz).
"""
import numpy as np

from oracle import data_path as D
from tests import reader_restatement as RR

GROUND_IDS = {"ADE20K": (976, 2131, 1125, 2377, 838, 913, 2212, 1788, 2530, 2185, 2531, 738, 1401, 1494),
              "cityscapes": (6, 7, 8, 9, 22), "matterport": (1,)}
FACTOR = {"ADE20K": None, "cityscapes": (0.4, 0.6), "matterport": (0.25, 0.75)}
JITTER_RANGES = ((0.7, 1.3), (0.8, 1.2), (0.7, 1.3), (-0.1, 0.1))


# ---- resizes --------------------------------------------------------------------------------------------------------------------------
def coeffs_range(in_size, out_size, first, count, filt=RR.LANCZOS):
    bounds, kk = RR.coeffs(in_size, out_size, filt)
    return bounds[first:first + count], kk[first:first + count]


def resize_window(img, th, tw, window, filt=RR.LANCZOS):
    """Image.fromarray(img).resize((tw, th), filt).crop((left, top, left + w, top + h)) for uint8 [h, w] or [h, w, C]"""
    top, left, h, w = window
    assert 0 <= top and top + h <= th and 0 <= left and left + w <= tw
    return np.ascontiguousarray(RR.resize(img, th, tw, filt)[top:top + h, left:left + w])


def nearest_index(in_size, out_size):
    step = in_size / out_size
    o = step * 0.5
    idx = np.empty(out_size, np.int32)
    for x in range(out_size):
        idx[x] = int(o)
        o += step
    return idx


def nearest_resize(img, th, tw):
    h, w = img.shape[:2]
    return np.ascontiguousarray(img[nearest_index(h, th)][:, nearest_index(w, tw)])


# ---- plan -----------------------------------------------------------------------------------------------------------------------------
def target_size(height, width, feed_h, feed_w):
    """prepare_size(keep_aspect_ratio=True): the size resize_all is called with"""
    if feed_h <= height and feed_w <= width:
        return height, width
    cur, tgt = height / width, feed_h / feed_w
    if cur < tgt:
        return feed_h, int(feed_h / height * width)
    if cur > tgt:
        return int(feed_w / width * height), feed_w
    return feed_w, feed_w


def plan_from_draws(dataset, src_hw, feed_hw, is_train, draws):
    """sizes and window from the uniform draws in the reference's order (resize factor, top, left); -> dict(rows, sizes = the image's
    size before and after each resize_all / resize call, window, used = number of draws consumed)"""
    draws = list(draws)
    h, w = src_hw
    H, W = feed_hw
    rows = 795 if dataset == "cityscapes" else h
    sizes = [(rows, w)]
    k = 0
    if is_train and FACTOR[dataset] is not None:
        f = FACTOR[dataset][0] + FACTOR[dataset][1] * draws[k]
        k += 1
        sizes.append((int(rows * f), int(w * f)))
    sizes.append(target_size(sizes[-1][0], sizes[-1][1], H, W))
    top = left = 0
    if sizes[-1] != (H, W):
        top = int(draws[k] * (sizes[-1][0] - H))
        left = int(draws[k + 1] * (sizes[-1][1] - W))
        k += 2
    return dict(rows=rows, sizes=sizes, window=(top, left, H, W), used=k)


# ---- one sample -----------------------------------------------------------------------------------------------------------------------
def image_u8(image, rows, sizes, window):
    """the uint8 image after the row crop, every resize of `sizes[1:]` and the crop"""
    img = image[:rows]
    for th, tw in sizes[1:]:
        img = RR.resize(img, th, tw)                      # a resize to the same size is the identity, as in Pillow
    top, left, H, W = window
    return np.ascontiguousarray(img[top:top + H, left:left + W])


def label_ids(dataset, labels, rows, sizes, window):
    """the label ids after the same chain with NEAREST"""
    lab = labels[:rows]
    for th, tw in sizes[1:]:
        if (th, tw) != lab.shape[:2]:
            lab = nearest_resize(lab, th, tw)
    top, left, H, W = window
    lab = lab[top:top + H, left:left + W]
    if dataset == "ADE20K":
        return lab[..., 0].astype(np.int64) // 10 * 256 + lab[..., 1].astype(np.int64)
    return (lab[..., 0] if lab.ndim == 3 else lab).astype(np.int64)


def _hue_factor_of_byte(shift):
    """a hue factor whose np.uint8(factor * 255) is `shift` (the record the device gets holds the byte, not the factor)"""
    v = shift if shift < 128 else shift - 256
    return (v + 0.5) / 255 if v >= 0 else (v - 0.5) / 255


def jitter(rgb, n_ops, ops, factors, hue_shift):
    """the jitter of an fp_aug_params record on uint8 [H, W, 3]"""
    if not n_ops:
        return rgb
    f = [float(np.float32(v)) for v in factors]
    f[D.HUE] = _hue_factor_of_byte(int(hue_shift))
    return D.jitter_np(rgb, [int(o) for o in ops[:n_ops]], f)


def sample(dataset, image, labels, rows, sizes, window, flip, n_ops=0, ops=(), factors=(), hue_shift=0):
    """-> (image float32 [3, H, W], ground_mask float32 [H, W], labelled_pix float32 [H, W]) as BaseDataset.__getitem__ returns them"""
    img = jitter(image_u8(image, rows, sizes, window), n_ops, ops, factors, hue_shift)
    ids = label_ids(dataset, labels, rows, sizes, window)
    if flip:
        img, ids = img[:, ::-1], ids[:, ::-1]
    ground = np.isin(ids, GROUND_IDS[dataset]).astype(np.float32)
    labelled = (ids != 0).astype(np.float32) if dataset == "cityscapes" else np.ones(ids.shape, np.float32)
    return np.ascontiguousarray(img.transpose(2, 0, 1)).astype(np.float32) / np.float32(255), ground, labelled
