from .ade20k import ADE20KReader
from .base import BatchSource, SegFileReader
from .cityscapes import CityscapesReader
from .matterport import MatterportReader

READERS = {"ADE20K": ADE20KReader, "cityscapes": CityscapesReader, "matterport": MatterportReader}
