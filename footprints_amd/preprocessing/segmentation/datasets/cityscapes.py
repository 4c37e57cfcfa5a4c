"""Cityscapes file reader (reference: segmentation/datasets/cityscapes_dataset.py:30-44)"""
import os

from .base import SegFileReader, pil_loader


class CityscapesReader(SegFileReader):
    name = "cityscapes"

    def load_image(self, index):
        folder, city, frame = self.filenames[index].split()
        return self.read_image(os.path.join(self.datapath, "leftImg8bit", folder, city, frame + "_leftImg8bit.png"))

    def load_labels(self, index):                   # fine ground truth, else coarse; all channels are equal, the device reads one
        folder, city, frame = self.filenames[index].split()
        try:
            return pil_loader(os.path.join(self.datapath, "gtFine", folder, city, frame + "_gtFine_labelIds.png"))
        except FileNotFoundError:
            return pil_loader(os.path.join(self.datapath, "gtCoarse", folder + "_extra", city, frame + "_gtCoarse_labelIds.png"))
