"""The pictures of the trainer's log event (reference training/logger.py:19-67 over training/losses.py:54-78 and utils.py:36-66), restated
twice on the host: in torch float32 on the CPU, operation by operation as the reference's tensors go, and in float64 from the same float32
inputs.  The float32 form is held against the reference's own `log` by tests/golden/g21_log.npz (tests/golden/make_golden_log.py); the
device kernel (csrc/log_panels.hip) is held against both (tests/test_gpu_log_panels.py).  Also here: the inputs of those tests, and the
renderer the CPU trainer test hands to TrainManager in place of ops.log_panels."""
import numpy as np
import torch

TAGS = ("image", "target_disp", "target_visible_ground", "target_all_ground", "target_ground_depth", "depth_mask", "moving_pixels",
        "pred_disp_1", "pred_ground_visible_1", "pred_ground_all_1", "pred_ground_disp_1", "pred_ground_disp_masked_1")
TARGET_PANELS = TAGS[:7]
PRED_PANELS = TAGS[7:]
LABELS = ("visible_ground", "depth", "ground_depth", "moving_object_mask", "depth_mask", "all_ground")


def tags(n, moving=True):
    return ["%s/%d" % (t, i) for i in range(n) for t in TAGS if moving or t != "moving_pixels"]


# ---- the reference's helpers, dtype-generic (utils.py:36-66) --------------------------------------------------------------------------------
def sigmoid_to_depth(disp, min_depth, max_depth):
    min_disp = 1 / max_depth
    max_disp = 1 / min_depth
    scaled_disp = min_disp + (max_disp - min_disp) * disp
    return 1 / scaled_disp


def depth_to_disp(depth):
    mask = (depth > 0).to(depth.dtype)
    return 1 / (depth + 1e-7) * mask


def normalise_image(img):
    img_max = float(img.max())
    img_min = float(img.min())
    denom = img_max - img_min if img_max != img_min else 1e5
    return (img - img_min) / denom


def viz_predictions(pred, depth_range):
    """what LossManager adds to `predictions` for one scale (losses.py:54-78) from the raw [B, 4, H, W] output, in pred's dtype"""
    vis = torch.sigmoid(pred[:, 0])
    allg = torch.sigmoid(pred[:, 1])
    depth = sigmoid_to_depth(pred[:, 2], depth_range[0], depth_range[1])
    gd = sigmoid_to_depth(pred[:, 3], depth_range[0], depth_range[1])
    return {"visible_ground": vis, "all_ground": allg, "depth": depth, "ground_depth": gd, "ground_depth_masked": gd * (allg > 0.5).to(pred.dtype)}


def float_panels(inputs, pred, depth_range, n=4, dtype=torch.float32):
    """-> list of (tag, tensor) in the reference's order: the image [3, H, W] and the normalised maps [H, W] in `dtype`, before the colour
    map and the byte rule.  Inputs are float32 CPU tensors; dtype=float64 converts them first and follows the same formulas."""
    image = inputs["image"].to(dtype)
    B, _, H, W = image.shape
    lab = {k: (inputs[k].reshape(B, H, W).to(dtype) if inputs.get(k) is not None else None) for k in LABELS}
    viz = viz_predictions(pred.to(dtype), depth_range)
    out = []
    for i in range(min(n, B)):
        out.append(("image/%d" % i, image[i]))
        out.append(("target_disp/%d" % i, normalise_image(depth_to_disp(lab["depth"][i]))))
        out.append(("target_visible_ground/%d" % i, normalise_image(lab["visible_ground"][i])))
        out.append(("target_all_ground/%d" % i, normalise_image(lab["all_ground"][i])))
        out.append(("target_ground_depth/%d" % i, normalise_image(lab["ground_depth"][i])))
        out.append(("depth_mask/%d" % i, normalise_image(lab["depth_mask"][i])))
        if lab["moving_object_mask"] is not None:
            out.append(("moving_pixels/%d" % i, normalise_image(lab["moving_object_mask"][i])))
        out.append(("pred_disp_1/%d" % i, normalise_image(depth_to_disp(viz["depth"][i]))))
        out.append(("pred_ground_visible_1/%d" % i, normalise_image(viz["visible_ground"][i])))
        out.append(("pred_ground_all_1/%d" % i, normalise_image(viz["all_ground"][i])))
        out.append(("pred_ground_disp_1/%d" % i, normalise_image(depth_to_disp(viz["ground_depth"][i]))))
        out.append(("pred_ground_disp_masked_1/%d" % i, normalise_image(depth_to_disp(viz["ground_depth_masked"][i]))))
    return out


def scaled(tag, x):
    """the number whose integer part is the byte (x * 255) or, for the colour-mapped panel, the table index (x * 256), in x's dtype"""
    return x * (256.0 if tag.startswith("pred_disp_1/") else 255.0)


def lut():
    from footprints_amd import ops
    return ops.vis_colour_table()


def to_bytes(panels, table=None):
    """the byte rule: uint8(float32(x) * 255) truncating, grey replicated to three channels (tensorboardX's add_image of a [1, H, W]
    tensor); the colour-mapped panel reads table[min(int(x * 256), 255)] -> uint8 [len(panels), H, W, 3]"""
    table = lut() if table is None else table
    out = []
    for tag, x in panels:
        v = scaled(tag, x.to(torch.float32)).numpy()
        if tag.startswith("pred_disp_1/"):
            out.append(table[np.minimum(v.astype(np.int64), 255)])
        elif x.dim() == 3:
            out.append(v.astype(np.uint8).transpose(1, 2, 0))
        else:
            out.append(np.repeat(v.astype(np.uint8)[:, :, None], 3, axis=2))
    return np.stack(out)


def render(inputs, pred, depth_range, n=4, out=None):
    """ops.log_panels' signature on the host: -> (uint8 tensor [n, P, H, W, 3], tags)"""
    cpu = {k: (v.detach().cpu() if torch.is_tensor(v) else v) for k, v in inputs.items()}
    panels = float_panels(cpu, pred.detach().cpu(), depth_range, n=n)
    n = min(n, pred.shape[0])
    by = to_bytes(panels)
    return torch.from_numpy(by.reshape((n, len(panels) // n) + by.shape[1:])), [t for t, _ in panels]


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------
def make_inputs(B, H, W, seed, moving=True, constant=False, channel_dim=False):
    """a batch with the reference's schema and a raw prediction built the way the trainer's outputs are: logits on channels 0 and 1,
    sigmoid disparities on 2 and 3.  depth and ground_depth hold exact zeros (the `d > 0` mask); the all-ground logit stays 1e-3 and more
    away from 0, its sigmoid from the 0.5 decision by 2.5e-4 and more.  constant=True makes one target (depth_mask) and one prediction
    channel (0) constant."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g)
    t = {"image": r(B, 3, H, W)}
    t["visible_ground"] = (r(B, H, W) < 0.4).float()
    t["depth"] = r(B, H, W) * 80.0 * (r(B, H, W) < 0.8).float()
    t["ground_depth"] = r(B, H, W) * 30.0 * (r(B, H, W) < 0.5).float()
    t["moving_object_mask"] = (r(B, H, W) < 0.05).float()
    t["depth_mask"] = (r(B, H, W) < 0.1).float()
    t["all_ground"] = ((t["ground_depth"] + t["visible_ground"]) > 0).float()
    pred = r(B, 4, H, W) * 6.0 - 3.0
    pred[:, 1] = torch.where(pred[:, 1].abs() < 1e-3, torch.full_like(pred[:, 1], 0.25), pred[:, 1])
    pred[:, 2:] = torch.sigmoid(pred[:, 2:])
    if constant:
        t["depth_mask"] = torch.zeros(B, H, W)
        pred[:, 0] = 0.75
    if not moving:
        t["moving_object_mask"] = None
    if channel_dim:
        t = {k: (v.reshape(B, 1, H, W) if v is not None and k != "image" else v) for k, v in t.items()}
    return t, pred.contiguous()
