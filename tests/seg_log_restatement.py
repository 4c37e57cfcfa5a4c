"""The picture of the segmentation trainer's log event (reference preprocessing/segmentation/logger.py:14-42, then tensorboardX's
`(x.astype(float32) * 255).astype(uint8)`), restated in numpy: in float32, operation by operation as the reference's arrays go, and with
dtype=float64 from the same float32 inputs.  The float32 form is held against the reference's own `log` by tests/golden/g_seg_log.npz
(tests/golden/make_golden_seg_log.py); the device kernel (csrc/stretch_map.hip, fp_seg_log_panels) against both
(tests/test_gpu_stretch_map.py).  Also here: the inputs of those tests and the host stand-in for ops.seg_log_panels.

The reference's trainer hands `log` the sigmoid of the full-resolution logits; here the logits go in and the sigmoid is part of the
restatement, as it is part of the kernel."""
import numpy as np


def tags(n):
    return ["Image/%d" % i for i in range(n)]


def sigmoid(x, dtype=np.float32):
    x = np.asarray(x).astype(dtype)
    one = dtype(1)
    return one / (one + np.exp(-x))


def normalize_image(img):
    """logger.py:14-19: Python floats (float64) for the range, the array's own dtype for the arithmetic"""
    img_max = float(img.max())
    img_min = float(img.min())
    denom = img_max - img_min if img_max != img_min else 1e5
    return (img - img.dtype.type(img_min)) / img.dtype.type(denom)


def plasma_floats():
    """matplotlib's plasma with 256 entries, float64 [256, 3]: what `COLORMAP(x)[:, :, :3]` reads"""
    import matplotlib
    return matplotlib.colormaps["plasma"].resampled(256)(np.arange(256))[:, :3]


def byte_table():
    """tensorboardX's rule on those colours: uint8 [256, 3]"""
    return (plasma_floats().astype(np.float32) * np.float32(255)).astype(np.uint8)


def float_parts(inputs, logits, n=10, dtype=np.float32):
    """per logged sample (image stretched [3, H, W], ground-truth red plane [H, W], probability [H, W]) in `dtype`"""
    image = np.asarray(inputs["image"]).astype(dtype)
    B, _, H, W = image.shape
    mask = np.asarray(inputs["ground_mask"]).reshape(B, H, W)
    logits = np.asarray(logits).reshape(B, H, W)
    out = []
    for i in range(min(n, B)):
        out.append((normalize_image(image[i]), (mask[i] == 1).astype(dtype), sigmoid(logits[i], dtype)))
    return out


def index_scaled(p):
    """the number whose integer part is the colour-table index, in p's dtype (matplotlib scales a float array in its own dtype)"""
    return p * p.dtype.type(256)


def to_bytes(parts, table=None):
    """-> uint8 [n, H, 3 W, 3]"""
    table = byte_table() if table is None else table
    out = []
    for image, red, p in parts:
        left = (image.astype(np.float32) * np.float32(255)).astype(np.uint8).transpose(1, 2, 0)
        mid = np.zeros_like(left)
        mid[..., 0] = (red.astype(np.float32) * np.float32(255)).astype(np.uint8)
        right = table[np.minimum(index_scaled(p).astype(np.int64), 255)]
        out.append(np.concatenate([left, mid, right], axis=1))
    return np.stack(out)


def render(inputs, logits, n=10, out=None):
    """ops.seg_log_panels' signature on the host: torch or numpy in -> (uint8 torch tensor [n, H, 3 W, 3], tags)"""
    import torch
    host = lambda v: v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)
    by = to_bytes(float_parts({k: host(v) for k, v in inputs.items()}, host(logits), n=n))
    return torch.from_numpy(by), tags(by.shape[0])


def make_inputs(B, H, W, seed, constant=False):
    """a batch with the segmentation loader's schema and full-resolution logits [B, 1, H, W]; the image is NOT confined to [0, 1] (the
    loader's colour augmentation leaves it so, which is why the reference stretches it); constant=True makes sample 0's image constant"""
    rng = np.random.default_rng(seed)
    image = (rng.random((B, 3, H, W)) * 1.5 - 0.2).astype(np.float32)
    if constant:
        image[0] = np.float32(0.375)
    inputs = {"image": image, "ground_mask": (rng.random((B, H, W)) < 0.4).astype(np.float32),
              "labelled_pix": (rng.random((B, H, W)) < 0.9).astype(np.float32)}
    logits = (rng.random((B, 1, H, W)) * 12.0 - 6.0).astype(np.float32)
    return inputs, logits
