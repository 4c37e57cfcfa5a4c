"""Test-set readers of the main network: the reference's constructor arguments, file-name parsing and `save_result` layout
(footprints/datasets/inference_dataset.py), with the file reading left on the host and nothing else.

A sample is {'image': the decoded RGB frame uint8 [h, w, 3] at its NATIVE size, 'path', 'idx': index} -- or, with device_decode,
{'bytes', 'info', 'path', 'idx'}: the file's bytes and what ops.jpeg_parse found, for a file the device decoder accepts
(decode_stage.read_sample).  The reference's `Resize((height, width), ANTIALIAS)` + `ToTensor` (:26-27, :48-49) run on the device for the
whole batch (ops.resize_u8_packed + ops.to_tensor_u8, bit-equal).  The reference opens the image without `.convert("RGB")` (:77, :98);
every reader of this package converts, and so does this one.

`save_result` writes what the reference writes (:35-43, :82-86, :104-113) --
    KITTI        <savepath>/<index zero-filled to 3>.npy and .jpg
    Matterport   <savepath>/<scan>/<pos>_<height>_<direction>.npy and .jpg
-- but takes the float16 array [4, H, W] and the picture as the device produced them (ops.infer_pack): no cast, and the picture is either
the uint8 array [H, 2 W, 3], which Pillow encodes at quality 95 as InferenceManager.run does, or the .jpg file's bytes as the device
encoded them (--device_jpeg), which are written as they are."""
import os

import numpy as np

from .decode_stage import read_sample


class InferenceDataset:

    def __init__(self, data_path, filenames, height, width):
        self.data_path = data_path
        self.filenames = filenames
        self.height = height
        self.width = width

    def __len__(self):
        return len(self.filenames)

    def image_path(self, index):
        raise NotImplementedError

    def read(self, index, device_decode=False):
        """one sample; with device_decode a file the device decoder accepts stays undecoded"""
        sample = read_sample(self.image_path(index), device_decode)
        sample["idx"] = index
        return sample

    def __getitem__(self, index):
        return self.read(index)

    def save_result(self, savepath, filename, prediction, visualisation=None):
        """prediction: float16 [4, H, W], written as given; visualisation: uint8 [H, 2 W, 3], the .jpg file's bytes, or None"""
        os.makedirs(savepath, exist_ok=True)
        np.save(os.path.join(savepath, "{}.npy".format(filename)), np.asarray(prediction, dtype=np.float16))
        if visualisation is None:
            return
        jpg = os.path.join(savepath, "{}.jpg".format(filename))
        if isinstance(visualisation, (bytes, bytearray, memoryview)):
            with open(jpg, "wb") as fh:
                fh.write(visualisation)
            return
        from PIL import Image
        Image.fromarray(np.asarray(visualisation, dtype=np.uint8)).save(jpg, quality=95)


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

    def save_result(self, index, prediction, savepath, visualisation=None):
        super().save_result(savepath, str(int(index)).zfill(3), prediction, visualisation)


class MatterportInferenceDataset(InferenceDataset):

    def __init__(self, data_path, filenames, height, width, *args, **kwargs):
        super().__init__(data_path, filenames, height, width)

    def _parse_index(self, index):
        scan, pos, height, direction = self.filenames[index].split(" ")
        return scan, pos, height, direction

    def image_path(self, index):
        scan, pos, height, direction = self._parse_index(index)
        return os.path.join(self.data_path, scan, scan, "matterport_color_images", "{}_i{}_{}.jpg".format(pos, height, direction))

    def save_result(self, index, prediction, savepath, visualisation=None):
        scan, pos, height, direction = self._parse_index(index)
        super().save_result(os.path.join(savepath, scan), "{}_{}_{}".format(pos, height, direction), prediction, visualisation)


def get_inference_dataset_class(name):
    """the reference's footprints/datasets/__init__.py:get_inference_dataset_class"""
    try:
        return {"kitti": KITTIInferenceDataset, "matterport": MatterportInferenceDataset}[name]
    except KeyError:
        raise NotImplementedError("no inference dataset %r (kitti, matterport)" % (name,)) from None
