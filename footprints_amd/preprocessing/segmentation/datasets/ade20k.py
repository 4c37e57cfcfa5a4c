"""ADE20K file reader (reference: segmentation/datasets/ade20k_dataset.py:38-44)"""
import os

from .base import SegFileReader, pil_loader


class ADE20KReader(SegFileReader):
    name = "ADE20K"

    def load_image(self, index):
        return self.read_image(os.path.join(self.datapath, os.path.splitext(self.filenames[index])[0] + ".jpg"))

    def load_labels(self, index):                   # the RGB segmentation image: the id is decoded on the device
        return pil_loader(os.path.join(self.datapath, os.path.splitext(self.filenames[index])[0] + "_seg.png"))
