"""File readers of the segmentation trainer: what is left on the host of the reference's dataset classes
(footprints/preprocessing/segmentation/datasets/*_dataset.py) -- decoding.  A reader yields (dataset name, image uint8 [h, w, 3],
labels uint8) at the NATIVE size; every resize, crop, flip, jitter and label lookup happens on the device
(footprints_amd/datasets/device_path.SegBatchAssembler).  With device_decode the image is the file itself and baseline JPEGs are decoded
there too; footprints_amd/datasets/training.ThreadedBatchSource is BatchSource reading ahead on --num_workers threads."""
import random

import numpy as np


def pil_loader(path):
    """dataset_utils.py:14-21: RGB through Pillow"""
    from PIL import Image
    with open(path, "rb") as fh:
        with Image.open(fh) as img:
            return np.asarray(img.convert("RGB"))


class SegFileReader:
    name = None

    def __init__(self, datapath, filenames, device_decode=False):
        """device_decode (--device_decode): the image of a sample is what datasets/decode_stage.read_sample(path, True) returns --
        {'path', 'bytes', 'info'} for a baseline JPEG, which SegBatchAssembler(device_decode=True) decodes on the device, or
        {'path', 'image', 'refused'} for a file the parser refuses (every PNG of Cityscapes, progressive JPEGs, ...), decoded by Pillow on
        the reader's thread.  Labels are read as ever."""
        self.datapath, self.filenames, self.device_decode = datapath, list(filenames), bool(device_decode)

    def __len__(self):
        return len(self.filenames)

    def read_image(self, path):
        """the decoded frame, or under device_decode the file sample"""
        if self.device_decode:
            from ....datasets.decode_stage import read_sample
            return read_sample(path, True)
        return pil_loader(path)

    def load_image(self, index):
        raise NotImplementedError

    def load_labels(self, index):
        raise NotImplementedError

    def __getitem__(self, index):
        return self.name, self.load_image(index), self.load_labels(index)


class BatchSource:
    """The reference's ConcatDataset + DataLoader(shuffle=...) over file readers, as the iterable of sample lists a DeviceLoader takes:
    one batch mixes datasets.  The assembler's batch size is fixed, so an incomplete last batch is dropped (the reference's DataLoader
    delivers it smaller)."""

    def __init__(self, readers, batch_size, shuffle=True, rng=random):
        self.readers, self.B, self.shuffle, self.rng = list(readers), int(batch_size), shuffle, rng
        self.index = [(r, i) for r in self.readers for i in range(len(r))]
        self.dataset = self.index                      # len(loader.dataset), as the reference prints it
        self.first, self.stride = 0, 1

    def __len__(self):
        return len(range(self.first, len(self.index) // self.B, self.stride))

    def shard(self, rank, world):
        import copy
        v = copy.copy(self)
        v.first, v.stride = rank, world
        return v

    def __iter__(self):
        order = list(range(len(self.index)))
        if self.shuffle:
            self.rng.shuffle(order)
        for b in range(self.first, len(order) // self.B, self.stride):
            yield [self.index[j][0][self.index[j][1]] for j in order[b * self.B:(b + 1) * self.B]]
