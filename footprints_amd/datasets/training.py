"""Training-set readers of the main network: the reference's constructor arguments, folders, file names and `split(' ')` parsing
(footprints/datasets/{footprint,kitti,matterport}_dataset.py, TrainManager.create_dataloaders), with the file reading left on the host and
nothing else.

A sample is (image uint8 [h, w, 3] -- the decoded RGB frame at its NATIVE size, {map name: array or None}) with the map names of
device_path.MAP_KEYS.  A map is what `np.load` returns (`npy[0]` when the file holds a 3-D array): native size, stored dtype, not flipped,
the depth mask unfiltered; None stands for a missing depth-mask file (the reference's `except FileNotFoundError`) and for the moving-object
map when --moving_objects_method is not 'ours'.  Everything behind the files runs on the device for the whole batch --
DeviceBatchAssembler(raw_images=True, raw_maps=True, filter_depth_mask=True): Pillow's LANCZOS resize of the frame, cv2's INTER_AREA /
INTER_NEAREST resizes of the maps, filter_depth_mask, flip, colour jitter and the label algebra.  The reference opens the image without
`.convert("RGB")`; every reader of this package converts, and so does this one.

One exception: Matterport's 16-bit depth PNG keeps Pillow's `resize(NEAREST)` on the reader thread and is handed over at the target size
as float32 (exact for 16 bits).

device_decode=True (--device_decode) takes the remaining pixel work off the reader threads.  The image of a sample is then what
decode_stage.read_sample(path, True) returns: {'path', 'bytes', 'info'} -- the file's bytes and its parsed header -- for a baseline JPEG,
which the assembler decodes on the device (csrc/jpeg_decode.hip, byte-equal to Pillow), or {'path', 'image', 'refused'} for a file the
parser refuses (progressive, restart markers, CMYK, PNG, ...), which Pillow decodes at once on that thread.  Matterport's depth PNG is
handed over as the uint16 array at its native size and resized on the device (fp_label_resize: FP_LABEL_U16, FP_LABEL_PIL_NEAREST).  A
reader thread then reads files, parses headers and decodes PNG, and does no other pixel work.

ThreadedBatchSource is BatchSource (the segmentation trainer's shuffled sample lists, with its `shard(rank, world)`) reading the samples of
upcoming batches on a pool of threads: one thread cannot decode 12 JPEGs and load 60 .npy files inside one training step."""
import os
from collections import deque

import numpy as np

from ..preprocessing.segmentation.datasets.base import BatchSource, pil_loader

# the largest frame / label map the per-slot staging buffers are sized for: KITTI raw frames are at most 376 x 1242, Matterport's 1024 x 1280
MAX_SRC_HW = {"kitti": (384, 1248), "matterport": (1024, 1280)}


def load_npy(path):
    """load_and_resize_npy's file half (footprint_dataset.py:84-86): np.load, the first plane of a 3-D array"""
    npy = np.load(path)
    if npy.ndim == 3:
        npy = npy[0]
    return npy


def load_optional_npy(path):
    """a map that may not exist (the depth masks) -> array or None"""
    try:
        return load_npy(path)
    except FileNotFoundError:
        return None


class TrainingReader:
    dataset = None

    def __init__(self, raw_data_path, training_data_path, filenames, height, width, no_depth_mask=False, moving_objects_method="ours",
                 project_down_baseline=False, is_train=False, device_decode=False, **kwargs):
        self.raw_data_path, self.training_data_path = raw_data_path, training_data_path
        self.filenames = list(filenames)
        self.height, self.width, self.is_train = height, width, is_train
        self.no_depth_mask, self.moving_objects_method, self.project_down_baseline = no_depth_mask, moving_objects_method, project_down_baseline
        self.device_decode = bool(device_decode)

    def image(self, path):
        """the decoded frame, or under device_decode what decode_stage.read_sample returns"""
        if self.device_decode:
            from .decode_stage import read_sample
            return read_sample(path, True)
        return pil_loader(path)

    def __len__(self):
        return len(self.filenames)

    def paths(self, index):
        """{'image': path, map name: path, ...} of one line of the split file"""
        raise NotImplementedError

    def __getitem__(self, index):
        raise NotImplementedError


class KITTIReader(TrainingReader):
    """kitti_dataset.py:51-105"""
    dataset = "kitti"

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        if self.project_down_baseline:
            assert self.moving_objects_method == "none", "Error - can't use project down baseline with moving object masking"

    def paths(self, index):
        seq, frame, side = self.filenames[index].split(" ")
        side = "image_02" if side == "l" else "image_03"
        frame_string = str(frame).zfill(10)
        t = self.training_data_path
        return {"image": os.path.join(self.raw_data_path, seq, side, "data", frame_string + ".jpg"),
                "visible_ground": os.path.join(t, "ground_seg", seq, side, "data", frame_string + ".npy"),
                "ground_depth": os.path.join(t, "hidden_depths", seq, side, "data", frame_string + ".npy"),
                "depth_mask": os.path.join(t, "depth_masks", seq, side, "data", frame_string + ".npy"),
                "disparity": os.path.join(t, "stereo_matching_disps", seq, side, frame_string + ".npy"),
                "moving_objects": os.path.join(t, "moving_objects", seq, side, "data", frame_string + ".npy")}

    def __getitem__(self, index):
        p = self.paths(index)
        maps = {"visible_ground": load_npy(p["visible_ground"]), "ground_depth": load_npy(p["ground_depth"]),
                "depth_mask": load_optional_npy(p["depth_mask"]), "disparity": load_npy(p["disparity"]),
                "moving_objects": load_npy(p["moving_objects"]) if self.moving_objects_method == "ours" else None}
        return self.image(p["image"]), maps


class MatterportReader(TrainingReader):
    """matterport_dataset.py:43-89"""
    dataset = "matterport"

    def paths(self, index):
        scan, pos, height, direction = self.filenames[index].split(" ")
        t = self.training_data_path
        name = "{}_{}_{}.npy".format(pos, height, direction)
        return {"image": os.path.join(self.raw_data_path, scan, scan, "matterport_color_images", "{}_i{}_{}.jpg".format(pos, height, direction)),
                "depth_raw": os.path.join(self.raw_data_path, scan, scan, "matterport_depth_images", "{}_d{}_{}.png".format(pos, height, direction)),
                "visible_ground": os.path.join(t, "ground_seg", scan, "data", name),
                "ground_depth": os.path.join(t, "hidden_depth", scan, "data", name),
                "depth_mask": os.path.join(t, "depth_masks", scan, "data", name)}

    def __getitem__(self, index):
        from PIL import Image
        p = self.paths(index)
        with Image.open(p["depth_raw"]) as im:
            if self.device_decode:                                     # the 16-bit PNG as stored: the device resizes it
                depth = np.asarray(im)
            else:                                                      # Pillow's NEAREST, on this thread
                depth = np.array(im.resize((self.width, self.height), Image.NEAREST)).astype(np.float32)
        maps = {"visible_ground": load_npy(p["visible_ground"]), "ground_depth": load_npy(p["ground_depth"]),
                "depth_mask": load_optional_npy(p["depth_mask"]), "depth_raw": depth}
        return self.image(p["image"]), maps


def get_dataset_class(name):
    """the reference's footprints/datasets/__init__.py:get_dataset_class"""
    try:
        return {"kitti": KITTIReader, "matterport": MatterportReader}[name]
    except KeyError:
        raise NotImplementedError("no training dataset %r (kitti, matterport)" % (name,)) from None


class ThreadedBatchSource(BatchSource):
    """BatchSource whose samples are read on min(num_workers, 16) threads, `ahead` batches in front of the consumer and in order: the
    shuffle, the batch boundaries and `shard(rank, world)` are BatchSource's, sample for sample."""

    def __init__(self, readers, batch_size, shuffle=True, rng=None, num_workers=8, ahead=3):
        import random
        super().__init__(readers, batch_size, shuffle, rng if rng is not None else random)
        self.num_workers, self.ahead = max(1, min(int(num_workers), 16)), max(1, int(ahead))

    def __iter__(self):
        from concurrent.futures import ThreadPoolExecutor
        order = list(range(len(self.index)))
        if self.shuffle:
            self.rng.shuffle(order)
        batches = iter(range(self.first, len(order) // self.B, self.stride))
        with ThreadPoolExecutor(self.num_workers) as pool:
            def read(j):
                reader, i = self.index[j]
                return reader[i]

            def submit():
                b = next(batches, None)
                if b is not None:
                    queue.append([pool.submit(read, j) for j in order[b * self.B:(b + 1) * self.B]])

            queue = deque()
            try:
                for _ in range(self.ahead):
                    submit()
                while queue:
                    futures = queue.popleft()
                    samples = [f.result() for f in futures]
                    submit()
                    yield samples
            finally:
                for futures in queue:                                  # the consumer stopped early: drop what has not started
                    for f in futures:
                        f.cancel()


def create_dataloaders(opt, stream=None, max_src_hw=None, max_map_hw=None, max_map_itemsize=4, device_decode=False):
    """TrainManager.create_dataloaders of the reference (training/train.py:99-134) over the device path: the config file's
    [training_dataset]['dataset' | 'training_data'], splits/<dataset>/{train,val}.txt relative to the working directory, the options
    no_depth_mask, moving_objects_method and project_down_baseline handed on, val with is_train=False; both shuffled, as the reference's
    DataLoaders are -> (train DeviceLoader, val DeviceLoader).  Under a data-parallel launch TrainManager shards the train loader's source.
    No file is read here.  max_src_hw / max_map_hw: the largest frame / label map (a larger one is refused by name when its batch is
    filled); max_map_itemsize: the stored element the map staging buffers start with (4: float32 maps) -- a batch of wider maps makes them
    grow once.  device_decode: both readers hand over file bytes and both assemblers decode them on the device (see the top)."""
    import random
    import yaml
    from .device_path import DeviceBatchAssembler, DeviceLoader
    dataset = opt.training_dataset
    with open(opt.config_path) as fh:
        config = yaml.safe_load(fh)
    raw_data_path, training_data_path = config[dataset]["dataset"], config[dataset]["training_data"]
    dataset_class = get_dataset_class(dataset)
    max_src_hw = tuple(max_src_hw or MAX_SRC_HW[dataset])
    max_map_hw = tuple(max_map_hw or MAX_SRC_HW[dataset])
    loaders = []
    for split, is_train, workers, slots in (("train", True, opt.num_workers, 3), ("val", False, min(2, opt.num_workers), 2)):
        with open(os.path.join("splits", dataset, split + ".txt")) as fh:
            files = fh.read().splitlines()
        reader = dataset_class(raw_data_path, training_data_path, files, opt.height, opt.width, no_depth_mask=opt.no_depth_mask,
                               moving_objects_method=opt.moving_objects_method, project_down_baseline=opt.project_down_baseline, is_train=is_train,
                               device_decode=device_decode)
        source = ThreadedBatchSource([reader], opt.batch_size, shuffle=True, rng=random, num_workers=workers)
        asm = DeviceBatchAssembler(opt.batch_size, opt.height, opt.width, dataset=dataset, slots=slots, no_depth_mask=opt.no_depth_mask,
                                   project_down_baseline=opt.project_down_baseline, moving_objects_method=opt.moving_objects_method,
                                   stream=stream, raw_images=True, max_src_hw=max_src_hw, filter_depth_mask=True, raw_maps=True,
                                   max_map_hw=max_map_hw, max_map_itemsize=max_map_itemsize, device_decode=device_decode)
        loader = DeviceLoader(source, asm, is_train=is_train, rng=random)
        loader.dataset = source.dataset
        loaders.append(loader)
    return loaders[0], loaders[1]
