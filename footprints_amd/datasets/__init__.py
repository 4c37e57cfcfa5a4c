"""Device-side data path.  Of the KITTI / Matterport file readers, the image resize
(Pillow's LANCZOS, byte for byte) and the connected-components filter of the depth mask can run on the device (DeviceBatchAssembler's
`raw_images` / `filter_depth_mask` options; csrc/reader.hip), and so can the cv2 resizes of the label maps (`raw_maps`;
csrc/label_resize.hip); of the training readers (training.py) only file decoding stays on the host, and
with `device_decode` (--mode train --device_decode) only file reading, header parsing and PNG decoding do: the
baseline JPEG frames are decoded inside the batch assembly and Matterport's 16-bit depth PNG is resized there.  The test-set readers of the main network (inference.py) and the two inference pipelines decode
baseline JPEG frames on the device when asked to (decode_stage.py: one batch ahead of the network); ring.py is
what those pipelines share: the thread / slot / writer scaffolding and the device side of the ring."""
from .device_path import AugParams, DeviceBatchAssembler, DeviceLoader, SyntheticSampleSource, draw_augmentation  # noqa: F401
