"""Loaders of what the baselines read -- counterpart of the reference's footprints/baselines/prepare_test_data.py.

File names and the `predictions_rerun/<baseline>/<line>` layout of get_save_path are the reference's.  The folders come from
arguments instead of paths.yaml and a download:

    predictions       the folder that holds the network's predictions (the reference reads `<predictions>/ours` for KITTI and
                      `<predictions>/lambda_0.5` for Matterport; here the folder is given directly).  A file is looked up under the
                      reference's name first (`{:03d}_color.npy`, `{}_{}_{}_{}.npy`) and then under the name this package's own
                      `main.py --mode inference` writes (`{:03d}.npy`, `{}/{}_{}_{}.npy`)
    ground_truth_dir  the folder that holds `kitti_ground_truth/kitti_ground_truth` and `matterport_ground_truth/matterport_ground_truth`
    dataset           the Matterport dataset root (camera intrinsics)
    bounding_boxes    the folder of the 3D-detector footprints (`{:03d}_colorfootprint.png`)
    save_root         where `predictions_rerun/` is made; the parent of `predictions` when not given, as in the reference

The reference brings every input to W x H with cv2.resize(x, (W, H)), which copies an input that already has that size -- the case
for this package's own `*_predictions` and for the ground-truth masks; that case is taken as a copy here.  For any other size the cv2
call is NOT reproduced: the package's stated stand-in is used, Pillow's mode-"F" BILINEAR resize on the host (as predict_simple.py
does).  cv2.imread(...)[:, :, ::-1] is Pillow's RGB image."""
import os

import numpy as np

from ..utils import sigmoid_to_depth


def imread_strict(im_path):
    from PIL import Image
    if os.path.isfile(im_path):
        return np.asarray(Image.open(im_path).convert("RGB"))
    raise FileNotFoundError(im_path)


def resize(x, W, H):
    """cv2.resize(x, (W, H)) for an input that is already H x W (a copy); otherwise Pillow mode-"F" BILINEAR, channel by channel"""
    from PIL import Image
    x = np.asarray(x)
    if x.shape[:2] == (H, W):
        return x.copy()
    planes = x.reshape(x.shape[0], x.shape[1], -1)
    out = [np.asarray(Image.fromarray(planes[:, :, c].astype(np.float32)).resize((W, H), Image.BILINEAR)) for c in range(planes.shape[2])]
    return np.stack(out, -1).reshape((H, W) + x.shape[2:])


def scaled_intrinsics(calibration, H, W, shape):
    """calibration = one *_intrinsics_*.txt line (.., .., fx, fy, cx, cy) for an H x W image -> K for a depth map of `shape` (each row
    divided by the calibrated size, then multiplied by the map's, in that order) and its pseudo-inverse, float64 [3,3]"""
    fx, fy, cx, cy = (float(v) for v in np.asarray(calibration).ravel()[2:6])
    K = np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])
    K[0] = K[0] / W * shape[1]
    K[1] = K[1] / H * shape[0]
    return K, np.linalg.pinv(K)


def _first_existing(*candidates):
    for path in candidates:
        if os.path.isfile(path):
            return path
    raise FileNotFoundError(candidates[0])


class TestLoader:
    """what a baseline class asks its loader for, and where the files are"""
    __test__ = False            # not a test class, whatever its name says

    def __init__(self, load_bounding_box_predictions=False, load_visible_ground=False, baseline_type="", predictions=None,
                 ground_truth_dir=None, dataset=None, bounding_boxes=None, save_root=None):
        self.load_bounding_box_predictions = load_bounding_box_predictions
        self.load_visible_ground = load_visible_ground
        self.baseline_type = baseline_type
        self.predictions, self.ground_truth_dir, self.dataset, self.bounding_boxes = predictions, ground_truth_dir, dataset, bounding_boxes
        self.save_root = save_root if save_root is not None else (os.path.join(predictions, "..") if predictions is not None else None)

    def _need(self, name):
        value = getattr(self, name)
        if value is None:
            raise ValueError("the %s baseline needs the `%s` path" % (self.baseline_type, name))
        return value

    def _save_path(self, baseline_type, name):
        save_path = os.path.join(self._need("save_root"), "predictions_rerun", baseline_type, name)
        os.makedirs(os.path.dirname(save_path), exist_ok=True)
        return save_path


class KittiTestLoader(TestLoader):
    """KITTI: 192 x 640; visible ground and, for the bounding-box baseline, the detector's footprints"""
    W = 640
    H = 192

    def __call__(self, frame_num):
        inputs = {}
        if self.load_visible_ground == "pred":
            pred = self._need("predictions")
            path = _first_existing(os.path.join(pred, "{:03d}_color.npy".format(frame_num)), os.path.join(pred, "{:03d}.npy".format(frame_num)))
            inputs["visible_ground"] = np.load(path)[0]                      # channel 0: visible ground
        elif self.load_visible_ground == "ground_truth":
            gt = os.path.join(self._need("ground_truth_dir"), "kitti_ground_truth", "kitti_ground_truth")
            inputs["visible_ground"] = imread_strict(os.path.join(gt, "{:05d}_ground.png".format(frame_num)))
        if self.load_bounding_box_predictions:
            bounding_box_path = os.path.join(self._need("bounding_boxes"), "{:03d}_colorfootprint.png".format(frame_num))
            inputs["bounding_box_mask"] = imread_strict(bounding_box_path)[:, :, 0]
        for key in inputs:
            inputs[key] = resize(inputs[key], self.W, self.H)
        return inputs

    def get_save_path(self, baseline_type, test_file_line):
        return self._save_path(baseline_type, str(test_file_line))


class MatterportTestLoader(TestLoader):
    """Matterport: 512 x 640; depth and intrinsics for the RANSAC baselines"""
    H = 512
    W = 640
    bounding_box_training_data = None

    def load_intrinsics(self, frame_data, depth):
        int_path = os.path.join(self._need("dataset"), "{}/{}/matterport_camera_intrinsics/{}_intrinsics_{}.txt").format(frame_data[0], *frame_data)
        return scaled_intrinsics(np.loadtxt(int_path), self.H, self.W, depth.shape)

    def _load_pred(self, frame_data):
        pred = self._need("predictions")
        return np.load(_first_existing(os.path.join(pred, "{}_{}_{}_{}.npy".format(*frame_data)),
                                       os.path.join(pred, "{}".format(frame_data[0]), "{}_{}_{}.npy".format(*frame_data[1:]))))

    def __call__(self, test_file_line):
        frame_data = test_file_line.strip().split()
        if 'ransac_plane' in self.baseline_type:
            pred = self._load_pred(frame_data)
            # the kernels take float32 depths (cv2.resize, which the reference calls here, does not take float16 either)
            depth = resize(np.asarray(sigmoid_to_depth(pred[2]), np.float32), self.W, self.H)
            K, inv_K = self.load_intrinsics(frame_data, depth)
            inputs = {"depth": depth, "inv_K": inv_K, "K": K}
        else:
            inputs = {}
        if self.load_visible_ground == "pred":
            pred = self._load_pred(frame_data)
            inputs["visible_ground"] = resize(pred[0], self.W, self.H)
        elif self.load_visible_ground == "ground_truth":
            gt_dir = os.path.join(self._need("ground_truth_dir"), "matterport_ground_truth", "matterport_ground_truth")
            gt = np.load(os.path.join(gt_dir, "{}_{}_{}_{}_groundtruth.npy".format(*frame_data)))
            inputs["visible_ground"] = resize(gt, self.W, self.H)
        if self.load_bounding_box_predictions:
            bbox_mask_path = os.path.join(self._need("bounding_boxes"), str(self.bounding_box_training_data), "{}_{}_{}_{}.png".format(*frame_data))
            inputs["bounding_box_mask"] = resize(imread_strict(bbox_mask_path), self.W, self.H)[:, :, 0]
        return inputs

    def get_save_path(self, baseline_type, test_file_line):
        return self._save_path(baseline_type, str(test_file_line).replace(' ', '_'))
