"""Test-set inference -- counterpart of the reference's footprints/evaluation/inference.py (`InferenceManager.test_batch`
:99-123 and `InferenceDataset.save_result`, datasets/inference_dataset.py:35-43), SURVEY.md section 8(f) N1/N2.

The reference takes `model(image)['1/1']`, applies the sigmoid to the two mask channels on the host side of the graph, copies
fp32 to the CPU and lets every `save_result` cast to float16.  Here the network evaluates only the full-resolution heads
(`inference_scales`), the encoder BatchNorm is folded into the convolutions, and one kernel (`fp_pack_pred_fp16`) applies the
sigmoid and rounds to float16 on the device, so the D2H copy is half the bytes and `save_result` writes the array as is.
`run(loader)` is the blocking loop over a loader of resized tensors; `run_dataset(dataset, ...)` is the test-set program the command line
runs (`main.py --mode inference`): the readers of datasets/inference.py, and the pipeline of datasets/ring.py that the segmentation
Tester runs too -- reader threads, a ring of pinned slots, a writer thread (`RingPipeline`) and the whole device side (`DeviceRing`: the
decode stage, Resize + ToTensor, network, output kernel, copies back, JPEG encoder); this class brings `_network` and one output launch
(`fp_infer_pack`: the float16 array and the picture from one pass over the logits).  With `device_decode=True` the frames are decoded on
the device one batch ahead (datasets/decode_stage.py); PNG and what else the decoder does not take stays with Pillow.  In `test_batch` the reader's `Image.resize((W, H), LANCZOS)` + ToTensor
(datasets/inference_dataset.py:26,48) can run on the device: `InferenceManager(..., device_resize=True, height_width=(H, W))` takes
`inputs['raw_image']`, the decoded uint8 frames at their native sizes, uploads them once and produces the same input tensor bit for bit.
With `save_test_visualisations=True` (the reference's --save_test_visualisations, inference.py:110-119) `run` also writes <stem>.jpg: the
network's input beside the hidden-ground mask in the first and last colour of matplotlib's plasma map, drawn by one kernel
(`fp_vis_side_by_side`) from the logits -- `logit > 0` where the reference tests `sigmoid > 0.5`, the same except for positive logits
below fp32's resolution at 0.5.  The picture is encoded by Pillow on the host (the reference calls plt.imsave), or with `device_jpeg=True`
on the device (csrc/jpeg.hip): the same files byte for byte, and the raw picture never crosses to the host.
"""
import os

import numpy as np
import torch

from .. import ops
from ..datasets.ring import DeviceRing, RingPipeline, full_resolution_heads
from ..model_manager import ModelManager


class InferenceManager(RingPipeline):
    def __init__(self, load_path=None, model_manager=None, save_path=None, device_resize=False, height_width=None,
                 save_test_visualisations=False, device_jpeg=False):
        if device_resize and height_width is None:
            raise ValueError("device_resize=True needs height_width=(H, W), the network's input size")
        self.device_resize, self.height_width = bool(device_resize), height_width
        if model_manager is None:
            model_manager = ModelManager(use_cuda=True, is_inference=True)
            if load_path is not None:
                model_manager.load_model(weights_path=load_path, load_optimiser=False)
        self.model_manager = model_manager
        self.model = model_manager.model
        self.model.eval()
        self.model.inference_scales = ("1/1",)          # "just take max resolution prediction" (inference.py:104)
        self.savepath = save_path
        self.save_test_visualisations = bool(save_test_visualisations)
        self.device_jpeg = bool(device_jpeg)
        self.stage = None                               # run_dataset's decode stage: its counters are read by tests and benchmarks
        self.ring = None                                # run_dataset's device side (datasets/ring.py::DeviceRing)
        self._ring_init()

    @classmethod
    def from_options(cls, opt, model_manager=None, **kwargs):
        """the manager the command line describes: --load_path, --inference_save_path, --save_test_visualisations (options.py)"""
        return cls(load_path=opt.load_path, model_manager=model_manager, save_path=opt.inference_save_path,
                   save_test_visualisations=opt.save_test_visualisations, device_jpeg=getattr(opt, "device_jpeg", False), **kwargs)

    def input_tensor(self, inputs):
        """the network's input [B,3,H,W] on the device"""
        if self.device_resize:
            return ops.load_images_u8([np.asarray(im, dtype=np.uint8) for im in inputs["raw_image"]], *self.height_width)
        return inputs["image"].cuda(non_blocking=True)

    def test_batch(self, inputs):
        """inputs['image']: [B,3,H,W] float tensor -- or, with device_resize, inputs['raw_image']: list of B decoded uint8 [h,w,3] frames.
        Returns a float16 numpy array [B,4,H,W]: sigmoid(mask logits), depth."""
        return self._test_batch(inputs, False)[0]

    def _test_batch(self, inputs, visualise):
        image = self.input_tensor(inputs)
        with torch.no_grad():
            pred = self.model(image)["1/1"]
            vis = None
            if visualise and self.device_jpeg:         # the .jpg files' bytes: the picture is drawn and encoded on the device
                vis = ops.jpeg_encode(ops.vis_side_by_side(image.contiguous(), pred.contiguous()), quality=95)
            elif visualise:
                vis = self.visualise_batch(image, pred)
            return ops.pack_pred_fp16(pred).cpu().numpy(), vis

    def visualise_batch(self, image, pred):
        """image: the network's input [B,3,H,W] on the device, pred: its logits [B,4,H,W] -> uint8 numpy [B,H,2W,3]: the input beside the
        two-colour hidden-ground mask (reference inference.py:114-118), drawn on the device"""
        return ops.vis_side_by_side(image.contiguous(), pred.contiguous()).cpu().numpy()

    def save_result(self, filename, prediction, savepath=None):
        savepath = savepath or self.savepath
        os.makedirs(savepath, exist_ok=True)
        np.save(os.path.join(savepath, "{}.npy".format(filename)), np.asarray(prediction, dtype=np.float16))

    def run(self, loader):
        """loader yields dicts with 'image' and 'idx' (file stems), like the reference's InferenceDataset batches"""
        for inputs in loader:
            if not self.save_test_visualisations:
                preds, vis = self.test_batch(inputs), None
            else:
                preds, vis = self._test_batch(inputs, True)
            for i, pred in enumerate(preds):
                self.save_result(inputs["idx"][i], pred)
                if vis is not None and self.device_jpeg:
                    with open(os.path.join(self.savepath, "{}.jpg".format(inputs["idx"][i])), "wb") as fh:
                        fh.write(vis[i])
                elif vis is not None:
                    from PIL import Image
                    Image.fromarray(vis[i]).save(os.path.join(self.savepath, "{}.jpg".format(inputs["idx"][i])), quality=95)

    # ---- the test-set pipeline ------------------------------------------------------------------------------------------------------------
    def _network(self, image):
        """the logits [n, 4, H, W] of the full-resolution heads"""
        return self.model(image)["1/1"]

    def run_dataset(self, dataset, batch_size, num_workers=4, slots=3, device_decode=False):
        """Every frame of `dataset` (datasets/inference.py) through the network at (dataset.height, dataset.width); its `save_result`
        writes <name>.npy, float16 [4, H, W], and with save_test_visualisations <name>.jpg, under self.savepath.  num_workers reader
        threads (at most 16) read ahead -- with device_decode only the bytes and the headers: baseline JPEG frames are decoded on the
        device one batch ahead (needs slots >= 2) -- the calling thread queues the batches on a ring of `slots` pinned slots, one writer
        thread saves.  The files are the same with and without device_decode, byte for byte.  -> the decode stage's counters"""
        B, H, W = int(batch_size), int(dataset.height), int(dataset.width)
        if B < 1:
            raise ValueError("batch_size must be at least 1")
        num_workers = min(max(int(num_workers or 1), 1), 16)
        shape = (B, H, W, max(int(slots), 1), self.save_test_visualisations, self.save_test_visualisations and self.device_jpeg)
        if self.ring is None or not self.ring.fits(*shape):             # a second run of the same shape reuses the ring and its stage
            self.ring = DeviceRing(*shape[:4], channels=4, network=lambda image: self._network(image).contiguous(),
                                   pack=lambda logits, image, want, half, pic: ops.infer_pack(logits, image, want_picture=want, out=(half, pic)),
                                   visualise=shape[4], device_jpeg=shape[5], stop=self._stop)
            self.stage = self.ring.stage
        ring, device_decode = self.ring, bool(device_decode)
        for key in self.stage.counters:
            self.stage.counters[key] = 0
        with full_resolution_heads(self.model):
            self.run_ring(len(dataset), B, len(ring.slots), num_workers, read=lambda index: dataset.read(index, device_decode),
                          ahead=ring.ahead, rest=ring.rest, collect=ring.collect,
                          save=lambda idx, array, pic: dataset.save_result(idx, array, self.savepath, pic), one_ahead=device_decode, name="infer")
        return dict(self.stage.counters)
