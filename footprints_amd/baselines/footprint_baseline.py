"""The comparison rows of the paper's tables -- counterpart of the reference's footprints/baselines/footprint_baseline.py.

    visible_ground        the hidden ground is the empty set: the visible-ground prediction, thresholded
    convex_hull           the convex hull of the visible ground (skimage.morphology.convex_hull_image's semantics)
    bounding_box          the hull, minus the footprints of a 3D detector's boxes, plus the visible ground
    ransac_plane          a RANSAC plane through the visible ground's points (ransac.py), evaluated at every pixel
    ransac_plane_oracle   the same with the ground-truth visible ground

The reference works one frame at a time on the host (Qhull and a facet test per pixel; 100 SVDs and 100 passes over the points).  Here
run_all() stacks `batch_size` frames and each step is one call into csrc/baselines.hip (ops.convex_hull_mask, ops.baseline_mask_counts,
ops.baseline_plane_fit, ops.baseline_plane_depth); frame_predict(inputs) is the batch of one.  A writer thread saves
`<save_path>_ground_mask.png` (Pillow, single channel) and, where the reference does, `<save_path>_ground_depth.npy`.

The host draws the RANSAC sample ranks exactly as ransac.run_ransac does -- numpy.random.seed(random_seed), then one
numpy.random.randint(n, size=3) per iteration, 100 iterations, per frame with at least 20 masked pixels.  Stated deviation: a sample
that repeats a rank scores 0 here (the reference leaves it to LAPACK's choice within a two-dimensional null space).

    python -m footprints_amd.baselines.footprint_baseline --dataset {kitti,matterport} [--tiny] --predictions DIR
        [--ground_truth_dir DIR] [--dataset_path DIR] [--bounding_boxes DIR] [--save_root DIR]
"""
import argparse
import queue
import threading

import numpy as np
import torch

from .. import ops
from .prepare_test_data import KittiTestLoader, MatterportTestLoader

RANSAC_ITERATIONS = 100          # ransac.fit_plane's max_iterations
RANSAC_MIN_POINTS = 20           # RansacPlane.frame_predict


def draw_sample_ranks(n, random_seed=None, iterations=RANSAC_ITERATIONS):
    """the `iterations` rank triples ransac.run_ransac draws for n points: int32 [iterations, 3]"""
    np.random.seed(random_seed)
    return np.stack([np.random.randint(n, size=3) for _ in range(iterations)]).astype(np.int32)


def _device_mask(frames, threshold):
    """[B,H,W] host arrays -> (device tensor, threshold or None): float16 / float32 maps are compared on the device in their own dtype,
    anything else is compared by numpy and travels as uint8"""
    x = np.stack(frames)
    if x.dtype in (np.float16, np.float32):
        return torch.from_numpy(x).cuda(), threshold
    return torch.from_numpy((x > threshold).astype(np.uint8)).cuda(), None


def _save(job):
    from PIL import Image
    save_path, ground_mask, ground_depth = job
    Image.fromarray((ground_mask * 255).astype(np.uint8)).save(save_path + "_ground_mask.png")
    if ground_depth is not None:
        np.save(save_path + "_ground_depth.npy", ground_depth)


class BaselineParentClass:
    load_bounding_box_predictions = False

    def __init__(self, dataset_type, random_seed=None, **paths):
        self.filenames = []
        self.dataset_type = dataset_type
        self.random_seed = random_seed
        self.loader = {"kitti": KittiTestLoader, "matterport": MatterportTestLoader}[dataset_type](
            self.load_bounding_box_predictions, self.load_visible_ground, self.baseline_type, **paths)

    def run_all(self, batch_size=12):
        """every frame of `self.filenames`, `batch_size` frames per device call; the files are written by a thread of their own"""
        jobs = queue.Queue(maxsize=4 * batch_size)
        failure = []

        def writer():
            while True:
                job = jobs.get()
                if job is None:
                    return
                try:
                    if not failure:
                        _save(job)
                except Exception as e:          # reported by the caller's thread below
                    failure.append(e)

        thread = threading.Thread(target=writer, daemon=True)
        thread.start()
        try:
            for i in range(0, len(self.filenames), batch_size):
                lines = self.filenames[i:i + batch_size]
                results = self.batch_predict([self.loader(line) for line in lines])
                for line, (ground_mask, ground_depth) in zip(lines, results):
                    jobs.put((self.loader.get_save_path(self.get_baseline_type(), line), ground_mask, ground_depth))
        finally:
            jobs.put(None)
            thread.join()
        if failure:
            raise failure[0]

    def frame_predict(self, inputs):
        return self.batch_predict([inputs])[0]

    def batch_predict(self, batch):
        """list of the loader's dictionaries (one shape) -> list of (ground_mask, ground_depth or None)"""
        raise NotImplementedError

    def get_baseline_type(self):
        return self.baseline_type


class RansacPlane(BaselineParentClass):
    baseline_type = "ransac_plane"
    load_visible_ground = "pred"

    def batch_predict(self, batch):
        depth = torch.from_numpy(np.stack([np.asarray(b["depth"], np.float32) for b in batch])).cuda()
        inv_K = torch.from_numpy(np.stack([np.asarray(b["inv_K"], np.float64)[:3, :3] for b in batch])).cuda()
        mask, threshold = _device_mask([b["visible_ground"] for b in batch], 0.5)
        counts = ops.baseline_mask_counts(mask, threshold).cpu().numpy()              # the one small copy the draw needs
        passthrough = counts < RANSAC_MIN_POINTS
        samples = np.zeros((len(batch), RANSAC_ITERATIONS, 3), np.int32)
        for b in np.flatnonzero(~passthrough):
            samples[b] = draw_sample_ranks(int(counts[b]), self.random_seed)
        fit = ops.baseline_plane_fit(depth, inv_K, mask, torch.from_numpy(samples).cuda(), threshold)
        floor = ops.baseline_plane_depth(depth, inv_K, fit["best_plane"], torch.from_numpy(passthrough.astype(np.uint8)).cuda()).cpu().numpy()
        out = []
        for b, inputs in enumerate(batch):
            floor_depth = inputs["depth"] if passthrough[b] else floor[b]
            out.append((floor_depth, floor_depth))
        return out


class RansacPlaneOracle(RansacPlane):
    baseline_type = "ransac_plane_oracle"
    load_visible_ground = "ground_truth"


class VisibleGround(BaselineParentClass):
    """nothing is hidden: the thresholded visible-ground prediction itself"""
    baseline_type = "visible_ground"
    load_visible_ground = "pred"

    def batch_predict(self, batch):
        return [(b["visible_ground"] > 0.1, b.get("depth", None)) for b in batch]


class ConvexHull(BaselineParentClass):
    """the convex hull of the visible ground stands for all ground"""
    baseline_type = "convex_hull"
    load_visible_ground = "pred"

    def batch_predict(self, batch):
        mask, threshold = _device_mask([b["visible_ground"] for b in batch], 0.5)
        hull = ops.convex_hull_mask(mask, threshold).cpu().numpy().astype(bool)
        return [(hull[b], None) for b in range(len(batch))]


class BoundingBox(ConvexHull):
    """the hull without the floor footprints of a 3D detector's boxes, with the visible ground put back"""
    baseline_type = "bounding_box"
    load_visible_ground = "pred"
    load_bounding_box_predictions = True

    def __init__(self, dataset_type, bounding_box_training_data, **kwargs):
        super().__init__(dataset_type, **kwargs)
        self.bounding_box_training_data = bounding_box_training_data
        self.loader.bounding_box_training_data = bounding_box_training_data

    def batch_predict(self, batch):
        mask, threshold = _device_mask([b["visible_ground"] for b in batch], 0.5)
        boxes = np.stack([b["bounding_box_mask"] for b in batch])
        if boxes.dtype not in (np.uint8, np.float16, np.float32):
            boxes = boxes.astype(np.float32)
        hull = ops.convex_hull_mask(mask, threshold, remove=torch.from_numpy(boxes).cuda(), keep=mask).cpu().numpy().astype(bool)
        return [(hull[b], None) for b in range(len(batch))]

    def get_baseline_type(self):
        return self.baseline_type + "_" + self.bounding_box_training_data


def main(argv=None):
    parser = argparse.ArgumentParser(description="The baselines of the footprints evaluation, on the device.")
    parser.add_argument("--dataset", type=str, choices=["matterport", "kitti"], required=True, help="dataset to evaluate on")
    parser.add_argument("--tiny", action="store_true", help="only the first 20 frames; useful for debugging")
    parser.add_argument("--predictions", type=str, required=True, help="folder of the network's predictions")
    parser.add_argument("--ground_truth_dir", type=str, default=None, help="folder that holds <dataset>_ground_truth/<dataset>_ground_truth")
    parser.add_argument("--dataset_path", type=str, default=None, help="Matterport dataset root (camera intrinsics)")
    parser.add_argument("--bounding_boxes", type=str, default=None, help="folder of the 3D-detector footprints (KITTI)")
    parser.add_argument("--save_root", type=str, default=None, help="where predictions_rerun/ is made (default: the parent of --predictions)")
    parser.add_argument("--split_file", type=str, default="splits/matterport/test.txt", help="the Matterport test split")
    parser.add_argument("--batch_size", type=int, default=12)
    parser.add_argument("--random_seed", type=int, default=None)
    opts = parser.parse_args(argv)

    if opts.dataset == "matterport":
        with open(opts.split_file, "r") as fh:
            test_filenames = fh.read().splitlines()[:500]
    else:
        test_filenames = list(range(697))
    if opts.tiny:
        test_filenames = test_filenames[:20]
    print("Testing on {} images".format(len(test_filenames)))

    paths = {"predictions": opts.predictions, "ground_truth_dir": opts.ground_truth_dir, "dataset": opts.dataset_path,
             "bounding_boxes": opts.bounding_boxes, "save_root": opts.save_root}
    runs = [lambda: VisibleGround(opts.dataset, **paths), lambda: ConvexHull(opts.dataset, **paths)]
    if opts.dataset == "matterport":
        runs += [lambda: RansacPlaneOracle(opts.dataset, random_seed=opts.random_seed, **paths),
                 lambda: RansacPlane(opts.dataset, random_seed=opts.random_seed, **paths)]
    elif opts.bounding_boxes is not None:
        runs.append(lambda: BoundingBox(opts.dataset, "3d_boundingbox", **paths))
    for make in runs:
        predictor = make()
        predictor.filenames = test_filenames
        predictor.run_all(batch_size=opts.batch_size)
        print("{}: done".format(predictor.get_baseline_type()))


if __name__ == "__main__":
    main()
