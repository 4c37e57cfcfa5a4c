"""numpy restatement of the label generators' loader work (csrc/gt_frames.hip): cv2.resize's default INTER_LINEAR on float64 data, written
out from a reading of OpenCV's portable C++ path (imgproc/src/resize.cpp, double data, no SIMD, IPP off) -- no cv2 is needed, and none
was at hand to pin it -- plus what data_loader.py of the reference wraps around it.  `nearest` and `area2` come from
label_resize_restatement.  numpy never fuses a product into a sum, so `a * b + c * d` below is three rounded operations, as in OpenCV's
scalar loops.

`HostKITTILoader` / `HostMatterportLoader` are the reference's loaders with this restatement in place of cv2: host arrays and host tensors,
one frame at a time, the schema ground_truth_generator's docstring promises."""
import os
from fractions import Fraction

import numpy as np
import torch

from tests import label_resize_restatement as LR


def linear_table(S, D, clamp):
    """offsets int32 [D] and float32 coefficients [D, 2] of one axis: f = (float)((d + 0.5) * scale - 0.5), s = floor(f), f -= s; with
    `clamp` (the horizontal pass) s < 0 -> (0, f = 0) and s >= S - 1 -> (S - 1, f = 0)"""
    scale = LR.scales(S, D)
    f = ((np.arange(D) + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int32)
    f = f - s.astype(np.float32)
    assert f.dtype == np.float32
    if clamp:
        lo = s < 0
        f[lo], s[lo] = 0, 0
        hi = s >= S - 1
        f[hi], s[hi] = 0, S - 1
    return s, np.stack([np.float32(1) - f, f], 1).astype(np.float32)


def linear(m, H, W):
    """the general INTER_LINEAR path on float64 [h, w] -> [H, W]: horizontal pass per source row (S[s] * c0 + S[s + 1] * c1; S[w - 1] * 1.0
    from the first output whose s reaches w - 1 on), then the vertical pass over rows s and s + 1 clipped into the map, f not clamped"""
    m = np.asarray(m, np.float64)
    h, w = m.shape
    sx, cx = linear_table(w, W, True)
    sy, cy = linear_table(h, H, False)
    cx, cy = cx.astype(np.float64), cy.astype(np.float64)            # float coefficients widened when used
    right = sx == w - 1
    with np.errstate(invalid="ignore"):
        hbuf = m[:, sx] * cx[:, 0] + m[:, np.minimum(sx + 1, w - 1)] * cx[:, 1]
        hbuf[:, right] = m[:, sx[right]] * 1.0
        r0, r1 = np.clip(sy, 0, h - 1), np.clip(sy + 1, 0, h - 1)
        return hbuf[r0] * cy[:, 0:1] + hbuf[r1] * cy[:, 1:2]


def is_area2(h, w, H, W):
    """cv::resize turns INTER_LINEAR into INTER_AREA when both scales are integers (within DBL_EPSILON) and equal 2"""
    return LR.is_fast(h, w, H, W) and int(round(LR.scales(w, W))) == 2 and int(round(LR.scales(h, H))) == 2


def resize(m, H, W, method):
    """cv2.resize(m.astype(float), (W, H)) for 'linear' (with its dispatch to the 2 x 2 area path), INTER_NEAREST for 'nearest'"""
    m = np.asarray(m).astype(np.float64)
    h, w = m.shape
    if method == "nearest":
        return LR.restate(m, H, W, "nearest")
    if method == "area2" or (method == "linear" and is_area2(h, w, H, W)):
        assert is_area2(h, w, H, W)
        return LR._area_fast(m, H, W)
    if method != "linear":
        raise ValueError(method)
    return linear(m, H, W)


def frame(m, H, W, method="linear", pre=1.0, post=1.0, threshold=None):
    """one record of fp_gt_frame_resize: `m *= pre` in the stored dtype, .astype(float), the resize, (v * num) / den in double, the
    threshold in double, .float() -> float32 [H, W]"""
    m = np.asarray(m)
    if m.dtype.kind == "f":
        stored = m.dtype
        m = m * stored.type(pre)                                     # numpy's in-place product: the scalar takes the array's dtype
        assert m.dtype == stored
    else:
        assert float(pre) == 1.0
    v = resize(m, H, W, method)
    num, den = post if isinstance(post, tuple) else (post, 1.0)
    v = (v * float(num)) / float(den)
    if threshold is not None:
        v = (v > float(threshold)).astype(np.float64)
    return v.astype(np.float32)


def exact_coefficient_bilinear(m, H, W):
    """bilinear interpolation at `linear`'s own sampling positions -- OpenCV rounds (d + 0.5) * scale - 0.5 to float before it splits it into
    s and f -- with the coefficients 1 - f and f taken exactly (float64 holds both) instead of the float 1.f - f"""
    m = np.asarray(m, np.float64)
    h, w = m.shape
    sx, cx = linear_table(w, W, True)
    sy, cy = linear_table(h, H, False)
    fx, fy = cx[:, 1].astype(np.float64), cy[:, 1].astype(np.float64)
    hbuf = m[:, sx] * (1.0 - fx) + m[:, np.minimum(sx + 1, w - 1)] * fx
    r0, r1 = np.clip(sy, 0, h - 1), np.clip(sy + 1, 0, h - 1)
    return hbuf[r0] * (1.0 - fy)[:, None] + hbuf[r1] * fy[:, None]


def exact_bilinear(m, H, W):
    """bilinear interpolation on the exact rational sampling grid (d + 1/2) * S / D - 1/2 with the same clamps, evaluated in float64"""
    m = np.asarray(m, np.float64)
    h, w = m.shape

    def axis(S, D):
        s, f = np.zeros(D, np.int64), np.zeros(D)
        for d in range(D):
            x = Fraction(2 * d + 1, 2) * Fraction(S, D) - Fraction(1, 2)
            s[d] = x.numerator // x.denominator
            f[d] = float(x - s[d])
        return s, f
    sx, fx = axis(w, W)
    sy, fy = axis(h, H)
    x0, x1 = np.clip(sx, 0, w - 1), np.clip(sx + 1, 0, w - 1)
    y0, y1 = np.clip(sy, 0, h - 1), np.clip(sy + 1, 0, h - 1)
    fx = np.where((sx < 0) | (sx >= w - 1), 0.0, fx)
    hbuf = m[:, x0] * (1.0 - fx) + m[:, x1] * fx
    return hbuf[y0] * (1.0 - fy)[:, None] + hbuf[y1] * fy[:, None]


# ---- the reference's loaders over the restatement ------------------------------------------------------------------------------------------
class HostKITTILoader:

    def __init__(self, raw_data_path, training_data_path, height, width, num_frames_bwd=25, num_frames_fwd=50, footprint_threshold=0.75):
        self.raw_data_path, self.training_data_path = raw_data_path, training_data_path
        self.height, self.width, self.footprint_threshold = height, width, footprint_threshold
        self.num_frames_bwd, self.num_frames_fwd = num_frames_bwd, num_frames_fwd
        self.buffer = {}
        self.K = np.array([[0.58, 0, 0.5, 0], [0, 1.92, 0.5, 0], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=np.float32)
        self.K[0] *= width
        self.K[1] *= height
        self.invK = np.linalg.pinv(self.K)
        self.stereo_baseline = 0.54

    def load_data(self, sequence, frame):
        frames, sides = [], []
        for f in range(frame - self.num_frames_bwd, frame + self.num_frames_fwd, 2):
            for side in ("image_02", "image_03"):
                data = self.load_frame_data(sequence, f, side)
                if data:
                    frames.append(data)
                    sides.append(side)
        disparities = torch.from_numpy(np.stack([d["disparity"] for d in frames])).float()
        fb = torch.tensor(np.float32(float(self.K[0, 0]) * self.stereo_baseline))
        return {"depths": fb / disparities, "ground_segs": torch.from_numpy(np.stack([d["ground_seg"] for d in frames])).float(),
                "poses": torch.from_numpy(np.stack([d["pose"] for d in frames])).float(), "sides": sides,
                "intrinsics": torch.from_numpy(np.stack([self.K] * len(frames))).float(),
                "inv_intrinsics": torch.from_numpy(np.stack([self.invK] * len(frames))).float()}

    def load_frame_data(self, sequence, frame, side, load_flow=False, use_buffer=True, threshold_ground=True):
        key = (sequence, int(frame), side)
        data = self.buffer.get(key) if use_buffer else None
        if data and (not load_flow or "flow" in data):
            return data
        name = "{}.npy".format(str(frame).zfill(10))
        t, H, W = self.training_data_path, self.height, self.width
        try:
            disp = np.load(os.path.join(t, "stereo_matching_disps", sequence, side, name))
            data = {"disparity": frame_f64(disp, H, W, pre=W / disp.shape[1])}
            seg = np.load(os.path.join(t, "ground_seg", sequence, side, "data", name))[0]
            data["ground_seg"] = frame_f64(seg, H, W, threshold=self.footprint_threshold if threshold_ground else None)
            pose = np.eye(4)
            pose[:3] = np.load(os.path.join(t, "poses", sequence, "orbslam_poses", name)).reshape(3, 4)
            data["pose"] = pose
            if load_flow:
                flow = np.load(os.path.join(t, "optical_flow", sequence, side, "data", name))
                data["flow"] = np.stack([frame_f64(flow[0], H, W, post=(float(W), float(flow.shape[2]))),
                                         frame_f64(flow[1], H, W, post=(float(H), float(flow.shape[1])))])
        except FileNotFoundError:
            return None
        if use_buffer:
            self.buffer[key] = data
        return data

    def purge_buffer(self):
        self.buffer = {}


def frame_f64(m, H, W, method="linear", pre=1.0, post=1.0, threshold=None):
    """`frame` as the reference holds it: float64 (the values are float32 values already, as after the generator's upload)"""
    return frame(m, H, W, method, pre, post, threshold).astype(np.float64)


class HostMatterportLoader:

    def __init__(self, raw_data_path, training_data_path, height, width, footprint_threshold=0.75):
        self.raw_data_path, self.training_data_path = raw_data_path, training_data_path
        self.height, self.width, self.footprint_threshold = height, width, footprint_threshold
        self.current_scan, self.scan_data, self.pose_tracker = None, None, {}
        self.full_size_width, self.full_size_height = 1280.0, 1024.0

    def load_data(self, scan, pos, height, direction):
        if self.current_scan != scan:
            self.pose_tracker, self.current_scan = {}, scan
            self.load_scan_data()
        return dict(self.scan_data)

    def load_frame_data(self, scan, pos, height, direction, threshold_ground=True):
        from PIL import Image
        scan_path = os.path.join(self.raw_data_path, scan, scan)
        seg = np.load(os.path.join(self.training_data_path, "ground_seg", scan, "data", "{}_{}_{}.npy".format(pos, height, direction)))[0]
        ground_seg = LR.restate((seg > self.footprint_threshold).astype(float), self.height, self.width, "nearest")
        depth = Image.open(os.path.join(scan_path, "matterport_depth_images", "{}_d{}_{}.png".format(pos, height, direction)))
        depth = np.array(depth.resize((self.width, self.height), resample=Image.NEAREST)).astype(float) * 0.00025
        with open(os.path.join(scan_path, "matterport_camera_poses", "{}_pose_{}_{}.txt".format(pos, height, direction))) as fh:
            pose = np.array(fh.read().split()).astype(float).reshape(4, 4)
        K = np.eye(4)
        with open(os.path.join(scan_path, "matterport_camera_intrinsics", "{}_intrinsics_{}.txt".format(pos, height))) as fh:
            words = fh.read().split()
        K[0, 0], K[0, 2], K[1, 1], K[1, 2] = float(words[2]), float(words[4]), float(words[3]), float(words[5])
        K[0] *= self.width / self.full_size_width
        K[1] *= self.height / self.full_size_height
        return ground_seg, depth, pose, K

    def load_scan_data(self):
        segs, depths, poses, Ks, invKs = [], [], [], [], []
        for file in sorted(os.listdir(os.path.join(self.training_data_path, "ground_seg", self.current_scan, "data"))):
            if file[-4:] == ".npy" and file[0] != ".":
                pos, height, direction = file.split("_")
                direction = direction[0]
                seg, depth, pose, K = self.load_frame_data(self.current_scan, pos, height, direction)
                segs.append(seg), depths.append(depth), poses.append(pose), Ks.append(K), invKs.append(np.linalg.pinv(K))
                self.pose_tracker[(pos, height, direction)] = pose
        f = lambda xs: torch.from_numpy(np.stack(xs)).float()
        self.scan_data = {"depths": f(depths), "ground_segs": f(segs), "poses": f(poses), "intrinsics": f(Ks), "inv_intrinsics": f(invKs)}
