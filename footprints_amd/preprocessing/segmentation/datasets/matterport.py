"""Matterport file reader (reference: segmentation/datasets/matterport_dataset.py:27-42)"""
import os

import numpy as np

from .base import SegFileReader


class MatterportReader(SegFileReader):
    name = "matterport"

    def _parts(self, index):
        return self.filenames[index].split(" ")

    def load_image(self, index):
        scan, pos, height, direction = self._parts(index)
        return self.read_image(os.path.join(self.datapath, "sample_dataset/v1/scans", scan, scan, "matterport_color_images",
                                            "{}_i{}_{}.jpg".format(pos, height, direction)))

    def load_labels(self, index):
        scan, pos, height, direction = self._parts(index)
        labels = np.load(os.path.join(self.datapath, "sample_dataset/v1/scans", scan, "nia_ground_masks",
                                      "out_{}_{}_{}_visibleground.npy".format(pos, height, direction)))
        return (labels > 0).astype(np.uint8)
