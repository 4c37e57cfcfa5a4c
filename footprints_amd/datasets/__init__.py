"""Device-side data path.  Of the KITTI / Matterport file readers, the image resize
(Pillow's LANCZOS, byte for byte) and the connected-components filter of the depth mask can run on the device (DeviceBatchAssembler's
`raw_images` / `filter_depth_mask` options; csrc/reader.hip); file decoding and the cv2 resizes of the label maps stay host-side dataset
plumbing."""
from .device_path import AugParams, DeviceBatchAssembler, DeviceLoader, SyntheticSampleSource, draw_augmentation  # noqa: F401
