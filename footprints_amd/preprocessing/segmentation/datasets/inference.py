"""Datasets of the segmentation network's inference mode: the reference's constructor arguments, file-name parsing and `save_result`
layout (footprints/preprocessing/segmentation/datasets/inference_dataset.py), with the decoding left on the host and nothing else.

A sample is {'image': the decoded RGB frame uint8 [h, w, 3] at its NATIVE size, 'idx': index}: the reference's
`Resize((height, width), ANTIALIAS)` + `ToTensor` run on the device for the whole batch (ops.resize_u8 + ops.to_tensor_u8, bit-equal).
`save_result` writes what the reference writes -- `<savepath>/.../data/<name>.npy`, float16 [1, H, W], and, when a picture is passed,
`<savepath>/.../visualisations/<name>.jpg` -- but takes the float16 array and the uint8 picture as the device produced them
(ops.seg_pack): no cast, no colour map, and Pillow encodes the bytes where the reference calls plt.imsave -- or, with --device_jpeg,
the file's bytes arrive encoded (ops.jpeg_encode_packed: what Pillow would write, byte for byte) and are written as they are.

The reference's MatterportInferenceDataset cannot be constructed: `__init__` reads an undefined name `image_ext`
(inference_dataset.py:101) and `_load_image` reads `self.datapath` where the attribute is `data_path` (:107).  It is built here as
evidently meant: `image_ext='jpg'` as a keyword like KITTI's, and `data_path`.  Its file name `<pos>_<height>_<direction>` goes through
the same `str(name).zfill(10)` as KITTI's frame number; Matterport's names are longer than that, so they are written as they are, which is
the name ground_truth_generation's loader reads."""
import os

import numpy as np

from .base import pil_loader


class InferenceDataset:

    def __init__(self, data_path, filenames, height, width):
        self.data_path = data_path
        self.filenames = filenames
        self.height = height
        self.width = width
        self.pil_loader = pil_loader

    def __len__(self):
        return len(self.filenames)

    def _load_image(self, index):
        raise NotImplementedError

    def save_result(self, savepath, filename, prediction, visualisation=None):
        """prediction: [1, H, W], written as float16; visualisation: uint8 [H, 2 W, 3], or the .jpg file's bytes as the device encoded
        them (ops.jpeg_encode), or None"""
        _savepath = os.path.join(savepath, "data")
        os.makedirs(_savepath, exist_ok=True)
        np.save(os.path.join(_savepath, "{}.npy".format(str(filename).zfill(10))), np.asarray(prediction, dtype=np.float16))
        if visualisation is not None:
            from PIL import Image
            _savepath = os.path.join(savepath, "visualisations")
            os.makedirs(_savepath, exist_ok=True)
            if isinstance(visualisation, (bytes, bytearray, memoryview)):
                with open(os.path.join(_savepath, "{}.jpg".format(str(filename).zfill(10))), "wb") as fh:
                    fh.write(visualisation)
                return
            Image.fromarray(np.asarray(visualisation, dtype=np.uint8)).save(
                os.path.join(_savepath, "{}.jpg".format(str(filename).zfill(10))), quality=95)

    def __getitem__(self, index):
        return {"image": np.asarray(self._load_image(index), dtype=np.uint8), "idx": index}


class KITTIInferenceDataset(InferenceDataset):

    def __init__(self, data_path, filenames, height, width, image_ext="jpg"):
        super().__init__(data_path, filenames, height, width)
        self.image_ext = image_ext

    def _parse_index(self, index):
        seq, frame, side = self.filenames[index].split(" ")
        side = "image_02" if side == "l" else "image_03"
        return seq, frame, side

    def image_path(self, index):
        seq, frame, side = self._parse_index(index)
        return os.path.join(self.data_path, seq, side, "data", "{}.{}".format(str(frame).zfill(10), self.image_ext))

    def _load_image(self, index):
        return self.pil_loader(self.image_path(index))

    def save_result(self, index, prediction, savepath, visualisation=None):
        seq, frame, side = self._parse_index(index)
        super().save_result(os.path.join(savepath, seq, side), frame, prediction, visualisation)


class MatterportInferenceDataset(InferenceDataset):

    def __init__(self, data_path, filenames, height, width, image_ext="jpg"):
        super().__init__(data_path, filenames, height, width)
        self.image_ext = image_ext

    def _parse_index(self, index):
        scan, pos, height, direction = self.filenames[index].split(" ")
        return scan, pos, height, direction

    def image_path(self, index):
        scan, pos, height, direction = self._parse_index(index)
        return os.path.join(self.data_path, "sample_dataset/v1/scans", scan, scan, "matterport_color_images",
                            "{}_i{}_{}.{}".format(pos, height, direction, self.image_ext))

    def _load_image(self, index):
        return self.pil_loader(self.image_path(index))

    def save_result(self, index, prediction, savepath, visualisation=None):
        scan, pos, height, direction = self._parse_index(index)
        super().save_result(os.path.join(savepath, scan), "{}_{}_{}".format(pos, height, direction), prediction, visualisation)


INFERENCE_DATASETS = {"kitti": KITTIInferenceDataset, "matterport": MatterportInferenceDataset}
