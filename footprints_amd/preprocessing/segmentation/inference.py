"""Ground-segmentation inference -- counterpart of footprints/preprocessing/segmentation/inference.py.  `InferenceManager.test_batch` is
the bare step (:60-84): an already resized tensor through the network, the full resolution logit map through a sigmoid, as a float32
numpy array [B,1,H,W].  `Tester` is the reference's program around it (`--mode inference`): the datasets of datasets/inference.py, the
resize, the network's full-resolution head alone and the output stage (csrc/seg_infer.hip) on the device, file writing on a thread --
a thin class over the ring of datasets/ring.py."""
import os

import numpy as np
import torch

from ... import ops
from ...datasets.decode_stage import read_sample
from ...datasets.ring import DeviceRing, RingPipeline, full_resolution_heads
from .network import Segmentor


class InferenceManager:
    def __init__(self, load_path=None, use_PSP=False, model=None):
        self.model = model if model is not None else Segmentor(pretrained=False, use_PSP=use_PSP)
        if load_path is not None:
            self.model.load_state_dict(torch.load(load_path, map_location="cpu"))        # inference.py:93-101
        self.model.cuda().eval()

    def test_batch(self, inputs):
        with torch.no_grad():
            preds = self.model(inputs["image"].cuda(non_blocking=True))
            return torch.sigmoid(preds[3][:, 0:1]).cpu().numpy()                          # "just take max resolution prediction"


class Tester(RingPipeline):
    """The reference's `Tester` (segmentation/inference.py:20-91): the trained Segmentor over every frame of the train and val splits, one
    float16 ground-probability map per frame under `<training_data>/<test_save_folder>/...` -- the files ground_truth_generation reads.

    The reference is a loop of blocking steps (DataLoader workers that decode AND resize on the host, forward, float32 copy to the host,
    cast, np.save, plt.imsave).  Here `test()` is a pipeline of three stages that overlap:
      readers  `num_workers` THREADS (default 4, at most 16; Pillow releases the GIL while it decodes) read ahead, in order;
      device   the calling thread lays a batch's frames -- uint8 at their native, mixed sizes -- out in a slot's pinned buffer and queues
               upload, Resize((H, W), ANTIALIAS) + ToTensor (ops.resize_u8_packed + ops.to_tensor_u8, bit-equal), the network in eval mode
               with `inference_scales = ("1/1",)`, ops.seg_pack (sigmoid, float16, the picture) and the copies into the slot's pinned
               result buffers; it does not wait for any of it, so batch k + 1 is queued while batch k's results come back;
      writer   ONE thread waits for a slot's `ready` event, writes its files (np.save; Pillow encodes the device-drawn picture) and hands
               the slot back.  A slot is not refilled before that.  With --device_jpeg the picture stays on the device and is encoded
               there behind seg_pack (ops.jpeg_encode_packed: the files Pillow writes, byte for byte); only the table of the scans'
               lengths comes back with the batch, and the writer, which may wait, copies the bytes in use on a stream of its own.
    An exception in a reader or in the writer ends `test()` with that exception; every wait on a queue, a future or a slot has a timeout
    after which the waiting thread looks at the error flag.  `has_gt`, tensorboard and data parallelism are not part of this mode.
    Threads, slots and the whole device side are datasets/ring.py's (`RingPipeline`, `DeviceRing`), shared with the main network's
    pipeline; this class brings the Segmentor's full-resolution head, ops.seg_pack and its datasets.  Every batch goes through the ring's
    decode stage (datasets/decode_stage.py): host-decoded frames are one upload.  With --device_decode the readers only read and parse the
    files: the frames the device decoder accepts are decoded into the slot's packed buffer one batch ahead -- batch k + 1's decode is
    queued before batch k's status is looked at -- and the calling thread's only wait is for that status; the files written are the
    same, byte for byte."""

    def __init__(self, options, model=None, dataset=None, save_path=None, slots=3):
        """model / dataset / save_path: injected (tests, benchmarks); then neither the config file nor the split files are read"""
        print("setting up...")
        self.opt = options
        self.height, self.width = int(options.height), int(options.width)
        self.batch_size = int(options.batch_size)
        self.num_workers = min(max(int(getattr(options, "num_workers", 4) or 1), 1), 16)
        self.visualise = bool(options.save_test_visualisations)
        self.device_jpeg = self.visualise and bool(getattr(options, "device_jpeg", False))
        self.device_decode = bool(getattr(options, "device_decode", False))
        if dataset is None or save_path is None:
            import yaml
            with open(self.opt.config_path) as fh:
                path_data = yaml.safe_load(fh)[self.opt.test_data_type]
            if save_path is None:
                save_path = os.path.join(path_data["training_data"], self.opt.test_save_folder)
        self.save_path = save_path
        if model is None:
            model = Segmentor(pretrained=False, use_PSP=not self.opt.no_PSP)
            print("loading weights from {}...".format(self.opt.load_path))
            model.load_state_dict(torch.load(self.opt.load_path, map_location="cpu"))
            print("successfully loaded weights!")
            model.cuda()
        self.model = model
        self.model.eval()
        if dataset is None:
            from .datasets.inference import INFERENCE_DATASETS
            filenames = []
            for textfile in ("train.txt", "val.txt"):               # train and val files, concatenated and sorted (inference.py:41-47)
                with open(os.path.join("splits", self.opt.test_data_type, textfile)) as fh:
                    filenames += fh.read().splitlines()
            dataset = INFERENCE_DATASETS[self.opt.test_data_type](path_data["dataset"], sorted(filenames), self.height, self.width)
        self.dataset = dataset
        self.n_slots = max(int(slots), 1)
        self._ring = None
        self._ring_init()

    def _new_ring(self):
        return DeviceRing(self.batch_size, self.height, self.width, self.n_slots, channels=1, network=lambda image: self.model(image)[3],
                          pack=lambda logits, image, want, half, pic: ops.seg_pack(logits, image, want_picture=want, out=(half, None, pic)),
                          visualise=self.visualise, device_jpeg=self.device_jpeg, stop=self._stop)

    @property
    def ring(self):
        """the device side (datasets/ring.py::DeviceRing), built at first use: constructing a Tester needs no device"""
        if self._ring is None:
            self._ring = self._new_ring()
        return self._ring

    @property
    def stage(self):
        """the ring's decode stage; its counters stay 0 without --device_decode"""
        return self.ring.stage

    def test_batch(self, frames):
        """frames: list of decoded RGB frames, uint8 [h, w, 3] of any (mixed) sizes -> (float16 numpy [B, 1, H, W], uint8 numpy
        [B, H, 2 W, 3] pictures or None without --save_test_visualisations); blocking, on the first slot"""
        self._stop.clear()
        with full_resolution_heads(self.model):
            self.ring.ahead(0, [{"image": f} for f in frames])
            self.ring.rest(0)
            half, pics = self.ring.collect(0, len(frames))
        return half.copy(), (pics.copy() if isinstance(pics, np.ndarray) else pics)

    def _read(self, index):
        if not self.device_decode:
            return self.dataset[index]
        sample = read_sample(self.dataset.image_path(index), True)
        sample["idx"] = index
        return sample

    def test(self):
        """Run every frame of the dataset through the network and write its result"""
        print("running inference...")
        ring = self.ring
        with full_resolution_heads(self.model):
            self.run_ring(len(self.dataset), self.batch_size, self.n_slots, self.num_workers, read=self._read, ahead=ring.ahead, rest=ring.rest,
                          collect=ring.collect, save=lambda idx, half, pic: self.dataset.save_result(idx, half, self.save_path, pic),
                          one_ahead=self.device_decode, name="seg-infer")
        print("finished testing!")
