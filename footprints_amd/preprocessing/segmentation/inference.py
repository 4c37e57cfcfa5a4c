"""Ground-segmentation inference -- counterpart of footprints/preprocessing/segmentation/inference.py.  `InferenceManager.test_batch` is
the bare step (:60-84): an already resized tensor through the network, the full resolution logit map through a sigmoid, as a float32
numpy array [B,1,H,W].  `Tester` is the reference's program around it (`--mode inference`): the datasets of datasets/inference.py, the
resize, the network's full-resolution head alone and the output stage (csrc/seg_infer.hip) on the device, file writing on a thread."""
import ctypes as C
import os

import numpy as np
import torch

from ... import _lib, ops
from ...datasets.ring import RingPipeline
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
      device   the calling thread packs a batch's frames -- uint8 at their native, mixed sizes -- into a slot's pinned buffer and queues
               upload, Resize((H, W), ANTIALIAS) + ToTensor (ops.resize_u8_packed + ops.to_tensor_u8, bit-equal), the network in eval mode
               with `inference_scales = ("1/1",)`, ops.seg_pack (sigmoid, float16, the picture) and the copies into the slot's pinned
               result buffers; it does not wait for any of it, so batch k + 1 is queued while batch k's results come back;
      writer   ONE thread waits for a slot's `ready` event, writes its files (np.save; Pillow encodes the device-drawn picture) and hands
               the slot back.  A slot is not refilled before that.  With --device_jpeg the picture stays on the device and is encoded
               there behind seg_pack (ops.jpeg_encode_packed: the files Pillow writes, byte for byte); only the table of the scans'
               lengths comes back with the batch, and the writer, which may wait, copies the bytes in use on a stream of its own.
    An exception in a reader or in the writer ends `test()` with that exception; every wait on a queue, a future or a slot has a timeout
    after which the waiting thread looks at the error flag (the scaffolding is datasets/ring.py's, shared with the main network's
    pipeline).  `has_gt`, tensorboard and data parallelism are not part of this mode.
    With --device_decode the readers only read and parse the files (datasets/decode_stage.py): the frames the device decoder accepts are
    decoded into the slot's packed buffer one batch ahead -- batch k + 1's decode is queued before batch k's status is looked at -- and
    the calling thread's only wait is for that status; the files written are the same, byte for byte."""

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
        self.stage = None
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
        self.slots = None
        self._ring_init()

    # ---- device half ------------------------------------------------------------------------------------------------------------------
    def _make_slots(self):
        """the ring: per slot the pinned staging buffer of the packed frames and their records, the device twins, the device outputs and
        the pinned buffers the results come back through"""
        if not torch.cuda.is_available():
            raise RuntimeError("the segmentation inference mode has no CPU compute path: it needs a MI355X")
        self.device = torch.device("cuda", torch.cuda.current_device())
        self.tables = ops.resize_table_set(self.device)
        B, H, W = self.batch_size, self.height, self.width
        rec_bytes = B * C.sizeof(_lib.ResizeSample)
        slots = []
        for _ in range(self.n_slots):
            s = dict(ready=torch.cuda.Event(), src_cap=0, h_src=None, d_src=None,
                     h_rec=torch.empty(rec_bytes, dtype=torch.uint8).pin_memory(), d_rec=torch.empty(rec_bytes, dtype=torch.uint8, device=self.device),
                     d_u8=torch.empty((B, H, W, 3), dtype=torch.uint8, device=self.device),
                     d_half=torch.empty((B, 1, H, W), dtype=torch.float16, device=self.device),
                     h_half=torch.empty((B, 1, H, W), dtype=torch.float16).pin_memory(), d_pic=None, h_pic=None)
            if self.visualise:
                s["d_pic"] = torch.empty((B, H, 2 * W, 3), dtype=torch.uint8, device=self.device)
            if self.device_jpeg:
                s["d_scan"] = torch.empty(ops.jpeg_max_scan_bytes(B, H, 2 * W), dtype=torch.uint8, device=self.device)
                s["d_tab"] = torch.empty((B + 1, 2), dtype=torch.int64, device=self.device)
                s["h_tab"] = torch.empty((B + 1, 2), dtype=torch.int64).pin_memory()
            elif self.visualise:
                s["h_pic"] = torch.empty((B, H, 2 * W, 3), dtype=torch.uint8).pin_memory()
            slots.append(s)
        if self.device_decode:
            from ...datasets.decode_stage import DecodeStage
            self.stage = DecodeStage(B, H, W, self.tables, self.device, stop=self._stop)
            for s in slots:
                self.stage.new_slot(s)
        if self.device_jpeg:
            # the pictures of a batch lie dense in d_pic: one set of records serves every slot, and its first n a batch of n
            self.jpeg_records = torch.from_numpy(ops.jpeg_records([(H, 2 * W)] * B)[0]).to(self.device)
            self.copy_stream = torch.cuda.Stream(self.device)
            self.h_scan = None                  # the writer's pinned buffer for the bytes in use; grows
        return slots

    def _reserve_src(self, s, nbytes):
        """the staging buffers of the packed frames grow when a batch needs more than they hold"""
        if nbytes > s["src_cap"]:
            ops.release(s["d_src"], "seg_tester:src")
            s["src_cap"] = nbytes + nbytes // 8
            s["h_src"] = torch.empty(s["src_cap"], dtype=torch.uint8).pin_memory()
            s["d_src"] = torch.empty(s["src_cap"], dtype=torch.uint8, device=self.device)

    def _device_half(self, s, frames):
        """queue one batch on the current stream -- upload, resize, ToTensor, network, seg_pack, copies back into the slot's pinned
        buffers -- and record the slot's `ready` event; nothing here waits for the device"""
        n = len(frames)
        if not 1 <= n <= self.batch_size:
            raise ValueError("a batch holds 1 to %d frames" % self.batch_size)
        if any(f.ndim != 3 or f.shape[2] != 3 for f in frames):
            raise ValueError("frames must be decoded RGB images, uint8 [h, w, 3]")
        H, W = self.height, self.width
        self._reserve_src(s, sum(f.shape[0] * f.shape[1] * 3 for f in frames))
        _, _, total, _, max_h, max_w = ops.resize_pack(frames, H, W, self.tables, packed=s["h_src"].numpy(), records=s["h_rec"].numpy())
        s["d_src"][:total].copy_(s["h_src"][:total], non_blocking=True)
        s["d_rec"].copy_(s["h_rec"], non_blocking=True)
        self._device_rest(s, n, total, max_h, max_w)

    def _device_rest(self, s, n, total, max_h, max_w):
        """a batch of n frames lies packed in the slot's d_src with its records in d_rec (uploaded, or decoded there): queue the rest"""
        H, W = self.height, self.width
        self.model.eval()
        with torch.no_grad():
            u8 = ops.resize_u8_packed(s["d_src"], total, s["d_rec"], n, H, W, 3, max_h, max_w, self.tables, out=s["d_u8"][:n])
            image = ops.to_tensor_u8(u8)
            scales = getattr(self.model, "inference_scales", None)            # the model may be the caller's: its setting comes back
            self.model.inference_scales = ("1/1",)          # "just take max resolution prediction" (inference.py:79)
            try:
                logits = self.model(image)[3]
            finally:
                self.model.inference_scales = scales
            pic = s["d_pic"][:n] if self.visualise else None
            ops.seg_pack(logits, image if self.visualise else None, want_picture=self.visualise, out=(s["d_half"][:n], None, pic))
            s["h_half"][:n].copy_(s["d_half"][:n], non_blocking=True)
            if self.device_jpeg:
                ops.jpeg_encode_packed(s["d_pic"].view(-1), n * H * 2 * W * 3, self.jpeg_records, n, 95, out=s["d_scan"], max_h=H, max_w=2 * W,
                                       table=s["d_tab"][:n + 1])
                s["h_tab"][:n + 1].copy_(s["d_tab"][:n + 1], non_blocking=True)
            elif self.visualise:
                s["h_pic"][:n].copy_(s["d_pic"][:n], non_blocking=True)
            s["ready"].record()

    def _wait_slot(self, s, n):
        """wait for the slot's results -> (float16 numpy [n, 1, H, W], uint8 numpy [n, H, 2 W, 3] or None): views of the pinned buffers;
        with device_jpeg the second is the list of the n .jpg files' bytes"""
        self._wait_event(s["ready"])                        # a wait with a timeout, like every other one
        if self.device_jpeg:
            return s["h_half"].numpy()[:n], self._fetch_files(s, n)
        return s["h_half"].numpy()[:n], (s["h_pic"].numpy()[:n] if self.visualise else None)

    def _fetch_files(self, s, n):
        """the slot's batch is finished and its length table is on the host: copy the scans' bytes in use -- on a stream of this thread's
        own, which it waits for; the thread that queues batches never does -- and put headers and EOI around them"""
        return self._fetch_jpeg_files(s, n, (self.height, 2 * self.width))

    def test_batch(self, frames):
        """frames: list of decoded RGB frames, uint8 [h, w, 3] of any (mixed) sizes -> (float16 numpy [B, 1, H, W], uint8 numpy
        [B, H, 2 W, 3] pictures or None without --save_test_visualisations); blocking, on the first slot"""
        if self.slots is None:
            self.slots = self._make_slots()
        s = self.slots[0]
        self._stop.clear()
        self._device_half(s, frames)
        half, pics = self._wait_slot(s, len(frames))
        return half.copy(), (pics.copy() if isinstance(pics, np.ndarray) else pics)

    # ---- the pipeline -----------------------------------------------------------------------------------------------------------------
    def _read(self, index):
        if not self.device_decode:
            return self.dataset[index]
        from ...datasets.decode_stage import read_sample
        sample = read_sample(self.dataset.image_path(index), True)
        sample["idx"] = index
        return sample

    def _writer(self, jobs, free):
        self._ring_writer(jobs, free, collect=lambda si, n: self._wait_slot(self.slots[si], n),
                          save=lambda idx, results, i: self.dataset.save_result(idx, results[0][i], self.save_path,
                                                                                results[1][i] if results[1] is not None else None))

    def _finish_decode(self, si, samples):
        s = self.slots[si]
        d = self.stage.finish(s)
        self._device_rest(s, d["n"], d["total"], d["max_h"], d["max_w"])

    def test(self):
        """Run every frame of the dataset through the network and write its result"""
        print("running inference...")
        if self.slots is None:
            self.slots = self._make_slots()
        if self.device_decode:
            ahead = lambda si, samples: self.stage.queue(self.slots[si], samples)
            rest = self._finish_decode
        else:
            ahead = None
            rest = lambda si, samples: self._device_half(self.slots[si], [smp["image"] for smp in samples])
        self.run_ring(len(self.dataset), self.batch_size, len(self.slots), self.num_workers, read=self._read, rest=rest, ahead=ahead,
                      writer=self._writer, name="seg-infer")
        print("finished testing!")
