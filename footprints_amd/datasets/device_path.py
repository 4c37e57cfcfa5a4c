"""Flip + colour jitter + ToTensor + label algebra on the GPU, fed by ONE pinned, double-buffered H2D copy per batch.

Reference (per sample, on DataLoader workers): footprints/datasets/footprint_dataset.py:55-65 (`preprocess`: ColorJitter, ToTensor,
float maps, `all_ground`), :73-75 / :84-85 (flips), kitti_dataset.py:55-56 (augmentation draws), :66-112 (label algebra),
matterport_dataset.py:69-97.  At ~650 img/s per GPU the reference's 8 PIL workers cannot feed one MI355X, let alone eight; here the
host only hands over what the file readers produce -- the resized uint8 image and the resized label maps of every sample -- plus a
36-byte parameter record per sample, and two kernels (csrc/data_path.hip) assemble the whole batch in the reference's schema.

Two more pieces of the reader can run on the device, both opt-in (csrc/reader.hip): with `raw_images=True` a sample's image is the DECODED
frame at its native size (KITTI frames come in several) and `Image.resize((W, H), LANCZOS)` (footprint_dataset.py:73-80) runs in front of
the flip and the jitter, in the reference's order and byte for byte Pillow's 8-bit path; with `filter_depth_mask=True` the depth mask
arrives unfiltered and the connected-components filter (footprint_dataset.py:96-105) runs in front of the label algebra.  With
`raw_maps=True` a sample's label maps are the arrays as `np.load` returns them -- native size, stored dtype, not flipped -- and the cv2
resizes (INTER_AREA / INTER_NEAREST on float64, footprint_dataset.py:82-94, with the fliplr in front and the disparity multiplier behind)
run in one launch in front of the filter (csrc/label_resize.hip).  No cv2 was at hand to pin them: the kernel equals, bit for bit, a
restatement of OpenCV's algorithm (tests/label_resize_restatement.py), which is anchored on the exact area average; INTER_AREA is built
for shrinking or equal sizes only -- where it would enlarge an axis cv2 switches to a linear kernel, and the pack refuses the map.

With `device_decode=True` (needs raw_images; --device_decode) a sample's image may also be the FILE: what decode_stage.read_sample returns,
{'path', 'bytes', 'info'}.  Such frames are decoded by ops.jpeg_decode_packed straight into the slot's packed source buffer, at the
offsets and with the records ops.resize_pack would have written (the sizes come from the headers); frames that arrive decoded are copied
into the pinned buffer at their offsets and uploaded alone.  Layout, pack, status copy and fallback are decode_stage.DecodeStage's, the
one owner of that protocol.  Everything is launched optimistically on the assembler's own stream, and the decoder's status is looked at
only when the batch is collected -- DeviceLoader queues the NEXT batch's decode first, so a whole training step has been queued behind
the decode whose status the host then reads, and the host does not wait for it in practice.  A frame whose status is not 0 (guarded, not
settled, corrupt) is decoded by Pillow then and uploaded to its offset, and the slot's resize and image assembly are queued once more
before the batch is handed over; both may run twice on a slot (they write every byte of their outputs from their inputs, and
fp_assemble_images clears `sums` itself).  Matterport's depth_raw may then be the uint16 PNG array at its native size, resized on the
device with Pillow's NEAREST rule.

Random decisions stay on the host and consume Python's `random` exactly like the reference does (flip draw, colour-aug draw, then
torchvision 0.4.2's ColorJitter.get_params: four uniforms in the order brightness, contrast, saturation, hue and one shuffle), so a
seeded run makes the same decisions as the reference pipeline.  Byte arithmetic is bit-exact with Pillow 12 (tests).
"""
import ctypes as C
import random

import numpy as np
import torch

from .. import _lib, ops

BRIGHTNESS, CONTRAST, SATURATION, HUE = 0, 1, 2, 3
JITTER_RANGES = ((0.8, 1.2), (0.8, 1.2), (0.8, 1.2), (-0.1, 0.1))          # footprint_dataset.py:37-40
MAP_KEYS = {"kitti": ("visible_ground", "ground_depth", "depth_mask", "disparity", "moving_objects"),
            "matterport": ("visible_ground", "ground_depth", "depth_mask", "depth_raw")}
# cv2.resize's interpolation per map in the reference (kitti_dataset.py:67-105, matterport_dataset.py:57-82); Matterport's raw depth arrives
# at the target size (Pillow's NEAREST on the reader thread) and is copied -- or, under device_decode, as the PNG's uint16 array at its native
# size, which goes through 'pil_nearest' instead
MAP_METHODS = {"visible_ground": "area", "ground_depth": "area", "depth_mask": "nearest", "disparity": "area", "moving_objects": "nearest",
               "depth_raw": "nearest"}
OUT_KEYS = ("visible_ground", "depth", "ground_depth", "moving_object_mask", "depth_mask", "all_ground")


class AugParams(C.Structure):
    """fp_aug_params (include/footprints_hip.h)"""
    _fields_ = [("flip", C.c_int32), ("n_ops", C.c_int32), ("ops", C.c_int32 * 4), ("factor", C.c_float * 4), ("hue_shift", C.c_int32),
                ("pad", C.c_int32)]


def draw_jitter(p, ranges=JITTER_RANGES, rng=random):
    """torchvision 0.4.2's ColorJitter.get_params into `p`: four uniforms in the order brightness, contrast, saturation, hue over
    `ranges`, then one shuffle of the order in which the four operations are applied"""
    factors = [rng.uniform(lo, hi) for lo, hi in ranges]
    order = [BRIGHTNESS, CONTRAST, SATURATION, HUE]
    rng.shuffle(order)
    p.n_ops = 4
    for k in range(4):
        p.ops[k] = order[k]
        p.factor[k] = factors[k]
    p.hue_shift = int(factors[HUE] * 255) & 0xFF                         # np.uint8(hue_factor * 255): truncation, wrap-around
    return p


def draw_augmentation(is_train=True, rng=random):
    """the reference's draws for one sample, in its order (kitti_dataset.py:55-56, then ColorJitter.get_params only when the colour
    augmentation fires) -> AugParams"""
    p = AugParams()
    p.flip = int(bool(is_train and rng.random() > 0.5))
    color_aug = bool(is_train and rng.random() > 0.5)
    if color_aug:
        draw_jitter(p, JITTER_RANGES, rng)
    return p


class SlotAssembler:
    """What every batch assembler shares: a ring of slots (dicts of pinned and device buffers, made by the subclass), the copy / assembly
    stream, and the events that order a slot's reuse -- `ready` (its copies and kernels are done) and `consumed` (the consumer has
    finished reading its outputs).  A subclass fills a slot's pinned buffers in `fill` (after `_take_slot`), queues the copies and
    kernels in `_launch(s)` and names the outputs in `_batch(s)`."""

    def _init_slots(self, device, stream):
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            # "cuda" means the CURRENT device at construction, pinned to an explicit index: under a launcher the current device
            # changes when DistContext.from_env selects LOCAL_RANK, and a bare "cuda" stream / buffer created before that lives on GPU 0
            self.device = torch.device("cuda", torch.cuda.current_device())
        # the copy / assembly stream.  A process owns four hardware queues and the engine uses all four (footprints_amd/engine.py): a
        # stream of its own is a fifth one and shares a queue with whichever engine stream the runtime picks -- a 3.6 ms H2D copy then
        # sits in front of that stream's kernels (637 vs 851 img/s on two boxes of the pool).  Pass the engine's decoder weight-gradient
        # stream (`model.engine().dwg[0]`): the next batch is staged before the current step is launched, the copy is done long before
        # that stream's first kernel of the step (6 ms in), and nothing on the critical path ever waits behind it.
        self.stream = stream if stream is not None else torch.cuda.Stream(device=self.device)
        self.slots = []
        self._next = 0

    def use_stream(self, stream):
        """move the copies and kernels to `stream` -- an engine stream that did not exist yet when the assembler was built (main.py builds
        the loaders before the model) -- before the first launch only"""
        if any(s["launched"] for s in self.slots):
            raise RuntimeError("SlotAssembler.use_stream: a slot has been launched on the old stream already")
        self.stream = stream

    def _add_slot(self, **buffers):
        self.slots.append(dict(buffers, ready=torch.cuda.Event(), consumed=None, launched=False))
        return self.slots[-1]

    def _take_slot(self):
        """the next slot of the ring, once its previous H2D copies have landed (its pinned buffers are free then) -> (index, slot)"""
        i = self._next
        self._next = (self._next + 1) % len(self.slots)
        s = self.slots[i]
        if s["launched"]:
            s["ready"].synchronize()
        return i, s

    def launch(self, i):
        """device half: H2D copies + assembly kernels of a filled slot on the copy stream, behind the consumer's last read of the slot's
        device buffers (an event wait on the stream: the host does not block)."""
        s = self.slots[i]
        if s["consumed"] is not None:
            self.stream.wait_event(s["consumed"])            # the consumer finished reading this slot's outputs
        with ops.on_stream(self.stream):
            self._launch(s)
            s["ready"].record(self.stream)
        s["launched"] = True
        return i

    def submit(self, samples, params):
        """stage one batch (fill + launch); returns the slot index to pass to collect()"""
        return self.launch(self.fill(samples, params))

    def collect(self, slot):
        """batch dict (reference schema) of the slot; the current stream waits for the slot's kernels.  The tensors are views of the
        slot's buffers: they stay valid until the slot is submitted again (call `release(slot)` after the step that used them was
        queued, or let DeviceLoader do it)."""
        s = self.slots[slot]
        torch.cuda.current_stream().wait_event(s["ready"])
        return self._batch(s)

    def release(self, slot):
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream())
        self.slots[slot]["consumed"] = ev


class DeviceBatchAssembler(SlotAssembler):
    """Pinned staging buffers (one set per slot), a copy stream, and the two assembly kernels.  Three slots by default: while the
    network works on batch i (slot a) and batch i + 1 sits assembled in slot b, the host can already fill slot c with batch i + 2 --
    with two slots the refill of a slot has to wait for the step that last read it, and the GPU idles for the host's memcpy.

        asm = DeviceBatchAssembler(12, 192, 640, dataset="kitti")
        slot = asm.submit(samples, params)        # host memcpy into pinned memory + async H2D + kernels on the copy stream
        batch = asm.collect(slot)                 # the consumer's stream waits for that slot's event; dict with the reference keys

    samples: list of (image uint8 [H,W,3], {map name: [H,W] array}) as the file readers deliver them (resized, NOT flipped; the depth
    mask already through filter_depth_mask).  map_dtype float64 reproduces the reference's numpy arithmetic bit for bit; float32
    halves the H2D bytes (inputs rounded once before the same float64 algebra).

    raw_images=True: the image of a sample is the decoded frame uint8 [h,w,3] at its native size, any h <= max_src_hw[0] and
    w <= max_src_hw[1] (they size the staging buffers), and is resized with Pillow's LANCZOS on the device.  filter_depth_mask=True:
    the depth mask of a sample is the unfiltered one (zeros and ones).  raw_maps=True (needs map_dtype float64): the maps of a sample are
    the arrays as loaded -- any h <= max_map_hw[0] and w <= max_map_hw[1], uint8 / bool / float16 / float32 / float64 (anything else is
    converted to float64 first), None for a missing depth mask -- and are resized on the device with cv2's INTER_AREA / INTER_NEAREST per
    MAP_METHODS; every other map must be present (a KeyError names a missing one).  max_map_itemsize (8 = float64 maps) is the stored
    element the staging buffers are sized for at the start; a batch that needs more makes its slot's buffers grow.

    device_decode=True (needs raw_images): the image of a sample may be a file as decode_stage.read_sample(path, True) returns it (or a
    decoded frame, as before); see the top of this file.  This is shape 2 of the two ways to keep the training thread from waiting for a
    decode: everything is launched optimistically and `collect` looks at the status, one DeviceLoader iteration after the decode was
    queued, so no slot is added.  decode: bytes -> uint8 [h, w, 3] for frames the device turns down (Pillow by default).  `counters`
    has the decode stage's three."""

    def __init__(self, batch_size, height, width, dataset="kitti", map_dtype=np.float64, slots=3, no_depth_mask=False,
                 project_down_baseline=False, moving_objects_method="ours", footprint_threshold=0.75, baseline=0.54,
                 depth_scaling=0.25e-3, device="cuda", stream=None, raw_images=False, max_src_hw=None, filter_depth_mask=False,
                 raw_maps=False, max_map_hw=None, max_map_itemsize=8, check=False, device_decode=False, decode=None):
        if dataset not in MAP_KEYS:
            raise ValueError("dataset must be 'kitti' or 'matterport'")
        if device_decode and not raw_images:
            raise ValueError("device_decode=True needs raw_images=True: the decoder writes frames at their native sizes")
        if raw_images and (max_src_hw is None or min(max_src_hw) <= 0):
            raise ValueError("raw_images=True needs max_src_hw=(largest source height, largest source width)")
        if raw_maps and (max_map_hw is None or min(max_map_hw) <= 0):
            raise ValueError("raw_maps=True needs max_map_hw=(largest map height, largest map width)")
        if raw_maps and np.dtype(map_dtype) != np.dtype(np.float64):
            raise ValueError("raw_maps=True needs map_dtype=float64: the device resize restates cv2's float64 arithmetic")
        self.raw_images, self.filter_mask, self.raw_maps = bool(raw_images), bool(filter_depth_mask), bool(raw_maps)
        self.max_map_hw = tuple(int(v) for v in max_map_hw) if raw_maps else None
        self.check = bool(check)          # read fp_label_resize's status word after every launch (this WAITS for the stream): tests, debugging
        self.max_src_hw = tuple(int(v) for v in max_src_hw) if raw_images else None
        self.device_decode = bool(device_decode)
        _lib.load()
        assert _lib.load().fp_aug_params_bytes() == C.sizeof(AugParams)
        self.B, self.H, self.W, self.dataset = batch_size, height, width, dataset
        self.map_dtype = np.dtype(map_dtype)
        if self.map_dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
            raise ValueError("map_dtype must be float32 or float64")
        self.keys = MAP_KEYS[dataset]
        self.no_depth_mask, self.pdb = bool(no_depth_mask), bool(project_down_baseline)
        self.use_moving = dataset == "kitti" and moving_objects_method == "ours"
        self.threshold = float(footprint_threshold)
        # focal * baseline exactly as the reference evaluates it (utils.py:31 with self.K[0, 0], a float32 scalar, kitti_dataset.py:23-28):
        # left to numpy so that the scalar promotion rules of the installed numpy apply, as they do to the reference's own code
        self.fxb = float(np.float32(0.58 * width) * baseline) if dataset == "kitti" else 0.0
        self.depth_scaling = float(depth_scaling)
        self._init_slots(device, stream)
        npx = batch_size * height * width
        tdt = torch.float64 if self.map_dtype == np.float64 else torch.float32
        self.tables = ops.resize_table_set(self.device) if self.raw_images else None
        self.map_tables = ops.label_table_set(self.device) if self.raw_maps else None
        self.stage = None
        if self.device_decode:              # decode: bytes -> uint8 [h, w, 3] for the frames the device turns down (Pillow; tests inject one)
            from .decode_stage import DecodeStage, host_decode
            self.stage = DecodeStage(batch_size, height, width, self.tables, self.device, decode=decode or host_decode, max_hw=self.max_src_hw)
        if self.raw_maps:
            lib = _lib.load()
            assert lib.fp_label_sample_bytes() == C.sizeof(_lib.LabelSample) and lib.fp_label_table_bytes() == C.sizeof(_lib.LabelTable)
        for _ in range(slots):
            h_img = torch.empty((batch_size, height, width, 3), dtype=torch.uint8).pin_memory()
            h_maps = torch.empty((0 if self.raw_maps else len(self.keys), batch_size, height, width), dtype=tdt).pin_memory()
            h_par = torch.empty(batch_size * C.sizeof(AugParams), dtype=torch.uint8).pin_memory()
            self._add_slot(
                h_img=h_img, h_maps=h_maps, h_par=h_par,
                d_img=torch.empty_like(h_img, device=self.device),
                d_maps=torch.empty((len(self.keys), batch_size, height, width), dtype=tdt, device=self.device),
                d_par=torch.empty_like(h_par, device=self.device), sums=torch.zeros(batch_size, dtype=torch.int64, device=self.device),
                image=torch.empty((batch_size, 3, height, width), device=self.device),
                out=torch.empty((len(OUT_KEYS), batch_size, height, width), device=self.device))
            if self.raw_images:             # the packed native-size frames and their fp_resize_sample records
                h_src = torch.empty(batch_size * self.max_src_hw[0] * self.max_src_hw[1] * 3, dtype=torch.uint8).pin_memory()
                h_rec = torch.empty(batch_size * C.sizeof(_lib.ResizeSample), dtype=torch.uint8).pin_memory()
                self.slots[-1].update(h_src=h_src, h_rec=h_rec, d_src=torch.empty_like(h_src, device=self.device),
                                      d_rec=torch.empty_like(h_rec, device=self.device), src_bytes=0)
                if self.device_decode:      # the decode stage's part of the slot; its pinned scan / record / table buffers come with the first batch
                    self.slots[-1].update(src_cap=h_src.numel(), h_status=torch.empty(batch_size + 1, dtype=torch.int32).pin_memory(),
                                          d_status=torch.empty(batch_size + 1, dtype=torch.int32, device=self.device),
                                          decoded=torch.cuda.Event(), batch=None, pack=None)
            if self.raw_maps:               # the packed native-size maps and their fp_label_sample records
                n = len(self.keys) * batch_size
                per_map = (self.max_map_hw[0] * self.max_map_hw[1] * int(max_map_itemsize) + 7) // 8 * 8
                h_msrc = torch.empty(n * per_map, dtype=torch.uint8).pin_memory()
                h_mrec = torch.empty(n * C.sizeof(_lib.LabelSample), dtype=torch.uint8).pin_memory()
                self.slots[-1].update(h_msrc=h_msrc, h_mrec=h_mrec, d_msrc=torch.empty_like(h_msrc, device=self.device),
                                      d_mrec=torch.empty_like(h_mrec, device=self.device), msrc_bytes=0,
                                      status=torch.zeros(1, dtype=torch.int32, device=self.device))
        assert npx > 0

    @property
    def counters(self):
        """DecodeStage.counters: frames decoded by the device, refused by the parser, decoded again after a non-zero status"""
        return dict(self.stage.counters) if self.stage is not None else dict(device=0, host_parser=0, host_status=0)

    def fill(self, samples, params):
        """host half of staging one batch: copy the samples and augmentation draws into the next slot's pinned buffers (60 MB of numpy
        copies for a KITTI batch with float64 maps at the target size; with raw_maps the maps as stored at their native size, 78 MB for
        float32 maps of 375 x 1242, plus their records and, once per distinct size, the INTER_AREA tables -- DeviceLoader runs this in a
        worker thread).  Waits only for the slot's previous H2D copies.  Returns the slot index for launch()."""
        if len(samples) != self.B or len(params) != self.B:
            raise ValueError("expected %d samples" % self.B)
        i, s = self._take_slot()
        img_np, maps_np = s["h_img"].numpy(), s["h_maps"].numpy()
        if self.device_decode:              # files and decoded frames: the stage lays them out, refuses what is too large, packs the scans
            s["src_bytes"] = self.stage.prepare(s, [img if isinstance(img, dict) else {"image": img} for img, _ in samples])["total"]
        elif self.raw_images:
            images = [img for img, _ in samples]
            if any(im.ndim != 3 or im.shape[2] != 3 or im.shape[0] > self.max_src_hw[0] or im.shape[1] > self.max_src_hw[1] for im in images):
                raise ValueError("raw images must be uint8 [h, w, 3] within max_src_hw = %r" % (self.max_src_hw,))
            s["src_bytes"] = ops.resize_pack(images, self.H, self.W, self.tables, packed=s["h_src"].numpy(), records=s["h_rec"].numpy())[2]
        for b, (img, maps) in enumerate(samples):
            if not self.raw_images:
                img_np[b] = img
            if not self.raw_maps:
                for k, key in enumerate(self.keys):
                    maps_np[k, b] = maps[key]
        if self.raw_maps:                   # map-major, like d_maps; a flipped sample's maps are read and stored mirrored
            raw, methods, flips, mults = [], [], [], []
            for key in self.keys:
                off = key == "moving_objects" and not self.use_moving
                for (_, maps), p in zip(samples, params):
                    # None only where the reference has no file either: a missing depth mask, moving objects with the masking off
                    m = None if off else maps[key]
                    if m is None and key not in ("depth_mask", "moving_objects"):
                        raise ValueError("the map %r of a sample is None: only depth_mask (and moving_objects) may be missing" % key)
                    raw.append(m)
                    pil = key == "depth_raw" and self.device_decode and getattr(m, "dtype", None) == np.uint16     # the PNG as stored
                    methods.append("zero" if m is None else "pil_nearest" if pil else MAP_METHODS[key])
                    flips.append(bool(p.flip))
                    mults.append(self.W / m.shape[1] if key == "disparity" and m is not None else 1.0)     # footprint_dataset.py:92
            need = ops.label_pack_bytes(raw)
            if need > s["h_msrc"].numel():  # wider stored dtypes than max_map_itemsize foresaw: the slot's pair grows, as the segmentation assembler's do
                ops.release(s["d_msrc"], "assembler:label maps")
                s["h_msrc"] = torch.empty(need + need // 4, dtype=torch.uint8).pin_memory()
                s["d_msrc"] = torch.empty_like(s["h_msrc"], device=self.device)
            s["msrc_bytes"] = ops.label_resize_pack(raw, self.H, self.W, methods, flips, mults, tables=self.map_tables, packed=s["h_msrc"].numpy(),
                                                    records=s["h_mrec"].numpy(), max_map_hw=self.max_map_hw)[2]
        arr = (AugParams * self.B)(*params)
        s["h_par"].numpy()[:] = np.frombuffer(bytes(arr), dtype=np.uint8)
        return i

    def _resize_frames(self, s):
        ops.resize_u8_packed(s["d_src"], s["src_bytes"], s["d_rec"], self.B, self.H, self.W, 3, self.max_src_hw[0], self.max_src_hw[1], self.tables,
                             out=s["d_img"])

    def _assemble_images(self, s):
        _lib.check(_lib.load().fp_assemble_images(s["d_img"].data_ptr(), s["d_par"].data_ptr(), s["sums"].data_ptr(), s["image"].data_ptr(),
                                                  self.B, self.H, self.W, ops.stream()), "fp_assemble_images")

    def collect(self, slot):
        s = self.slots[slot]
        if self.device_decode and s["batch"] is not None:
            # the decode was queued a whole step ago (DeviceLoader): its status is there.  What the device turned down goes through Pillow
            # now, and the image half of the slot's chain runs again on the repaired source buffer; the label half never read it
            def again():
                self._resize_frames(s)
                self._assemble_images(s)
                s["ready"].record(self.stream)
            with ops.on_stream(self.stream):
                self.stage.collect(s, again)
        return super().collect(slot)

    def _launch(self, s):
        if self.device_decode:              # uploads of the records, the host frames and the scans, the decode into d_src, the status copy
            self.stage.launch(s)
            self._resize_frames(s)
        elif self.raw_images:               # Image.resize first, like the reference (footprint_dataset.py:77), straight into d_img
            n = s["src_bytes"]
            s["d_src"][:n].copy_(s["h_src"][:n], non_blocking=True)
            s["d_rec"].copy_(s["h_rec"], non_blocking=True)
            self._resize_frames(s)
        else:
            s["d_img"].copy_(s["h_img"], non_blocking=True)
        if self.raw_maps:                   # cv2.resize of every map, straight into d_maps
            n = s["msrc_bytes"]
            s["d_msrc"][:n].copy_(s["h_msrc"][:n], non_blocking=True)
            s["d_mrec"].copy_(s["h_mrec"], non_blocking=True)
            ops.label_resize_packed(s["d_msrc"], n, s["d_mrec"], len(self.keys) * self.B, self.H, self.W, self.map_tables, out=s["d_maps"],
                                    status=s["status"], check=self.check)
        else:
            s["d_maps"].copy_(s["h_maps"], non_blocking=True)
        s["d_par"].copy_(s["h_par"], non_blocking=True)
        if self.filter_mask:                # filter_depth_mask in place, in front of the label algebra
            ops.filter_depth_mask(s["d_maps"][2], out=s["d_maps"][2])
        lib = _lib.load()
        st = ops.stream()
        self._assemble_images(s)
        m, o = s["d_maps"], s["out"]
        kitti = self.dataset == "kitti"
        _lib.check(lib.fp_assemble_labels(m[0].data_ptr(), m[1].data_ptr(), m[2].data_ptr(), m[3].data_ptr(),
                                          m[4].data_ptr() if kitti else None, int(self.map_dtype == np.float64), s["d_par"].data_ptr(),
                                          o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), o[3].data_ptr(), o[4].data_ptr(), o[5].data_ptr(),
                                          self.B, self.H, self.W, 0 if kitti else 1, int(self.no_depth_mask), int(self.pdb),
                                          int(self.use_moving), self.threshold, self.fxb, self.depth_scaling, st), "fp_assemble_labels")

    def _batch(self, s):
        batch = {"image": s["image"]}
        for k, key in enumerate(OUT_KEYS):
            batch[key] = s["out"][k]
        return batch


class DeviceLoader:
    """Iterable of device batches over a host sample source: while the network works on batch i, batch i + 1 is being copied and
    assembled on the copy stream (the assembler's second slot).

    source: iterable yielding lists of `batch_size` samples (image uint8 [H,W,3], maps dict); rng: Python RNG for the reference's
    augmentation draws (the module-level `random` by default, like the reference); draw(samples, is_train, rng) -> the list of
    per-sample parameters handed to the assembler's fill() (by default one `draw_augmentation` per sample, in batch order)."""

    def __init__(self, source, assembler, is_train=True, rng=random, draw=None):
        self.source, self.asm, self.is_train, self.rng = source, assembler, is_train, rng
        self.draw = draw if draw is not None else (lambda samples, is_train, rng: [draw_augmentation(is_train, rng) for _ in samples])

    @property
    def counters(self):
        """the assembler's decode counters (device, host_parser, host_status); zeros without device_decode"""
        return getattr(self.asm, "counters", None) or dict(device=0, host_parser=0, host_status=0)

    def __len__(self):
        return len(self.source)

    def shard(self, rank, world):
        """per-rank view for parallel.ShardedLoader: the SOURCE is sharded by index (a rank decodes, stages and assembles only its own
        batches), the assembler and its slots stay this process's"""
        if not hasattr(self.source, "shard"):
            raise TypeError("DeviceLoader.shard: the sample source has no shard(rank, world)")
        return DeviceLoader(self.source.shard(rank, world), self.asm, self.is_train, self.rng, self.draw)

    def __iter__(self):
        # one worker thread does the host half of staging (augmentation draws in batch order + the copies into pinned memory: numpy
        # releases the GIL for them), one batch ahead of the batch whose copies and kernels are in flight, two ahead of the consumer
        from concurrent.futures import ThreadPoolExecutor
        it = iter(self.source)

        def fill_next():
            try:
                samples = next(it)
            except StopIteration:
                return None
            return self.asm.fill(samples, self.draw(samples, self.is_train, self.rng))

        with ThreadPoolExecutor(1) as ex:
            pending = fill_next()
            if pending is None:
                return
            self.asm.launch(pending)
            fut = ex.submit(fill_next)
            # an assembler that decodes on the device reads the decoder's status in collect: the next batch's decode is queued in front of
            # that, so that batch `pending`'s decode has a whole step of queued work behind it when the host looks at its status
            launch_first = bool(getattr(self.asm, "device_decode", False))
            while True:
                if not launch_first:
                    batch = self.asm.collect(pending)
                nxt = fut.result()
                if nxt is not None:
                    self.asm.launch(nxt)                  # the OTHER slot: copied and assembled while the consumer works on `pending`
                if launch_first:
                    batch = self.asm.collect(pending)
                if nxt is not None:
                    fut = ex.submit(fill_next)
                yield batch
                self.asm.release(pending)                 # the step that used it has been queued: its completion frees the slot
                if nxt is None:
                    return
                pending = nxt


class SyntheticSampleSource:
    """`steps` batches of host samples with the shapes / dtypes the file readers deliver (stand-in for the KITTI reader, whose file
    decoding stays on the host): a small pool of random samples, cycled.  raw_hw: a list of (h, w) -- the images are then decoded frames
    at these native sizes, taken in turn (for DeviceBatchAssembler(raw_images=True)); the label maps stay at height x width."""

    def __init__(self, batch_size, height, width, steps, seed=10, pool=24, raw_hw=None):
        rng = np.random.default_rng(seed)
        self.B, self.steps, self.first, self.stride = batch_size, steps, 0, 1
        self.pool = []
        for j in range(pool):
            maps = {"visible_ground": rng.random((height, width)), "ground_depth": rng.random((height, width)) * 30 * (rng.random((height, width)) < 0.5),
                    "depth_mask": (rng.random((height, width)) < 0.1).astype(np.float64), "disparity": rng.random((height, width)) * 60,
                    "moving_objects": (rng.random((height, width)) < 0.05).astype(np.float64)}
            ih, iw = raw_hw[j % len(raw_hw)] if raw_hw else (height, width)
            self.pool.append((rng.integers(0, 256, (ih, iw, 3), dtype=np.uint8), maps))
        self.dataset = range(steps * batch_size)

    def __len__(self):
        return len(range(self.first, self.steps, self.stride))

    def shard(self, rank, world):
        import copy
        v = copy.copy(self)
        v.steps = (self.steps // world) * world
        v.first, v.stride = rank, world
        return v

    def __iter__(self):
        for i in range(self.first, self.steps, self.stride):
            yield [self.pool[(i * self.B + j) % len(self.pool)] for j in range(self.B)]


class SegBatchAssembler(SlotAssembler):
    """Batches of the ground-segmentation trainer, assembled on the device in the reference's schema {image, ground_mask, labelled_pix}
    (footprints/preprocessing/segmentation/datasets/base_dataset.py:76-102) from decoded frames and label images at their native sizes.

        asm = SegBatchAssembler(12, 192, 640, max_src_hw=(795, 2048))
        plans = asm.draw(samples, is_train=True, rng=random)      # host: every size, crop offset and augmentation draw of the reference
        batch = asm.collect(asm.submit(samples, plans))

    samples: list of (dataset name, image uint8 [h, w, 3], labels uint8 [h, w] or [h, w, 3]); one batch may mix datasets.  The crop
    window is known before any pixel is touched (preprocessing/segmentation/datasets/plan.py), so `fill` stages only the rectangle of
    the frame that the window's resize taps reach and the rectangle of the label image that the composed NEAREST tables address;
    `launch` copies them and runs one or two windowed resizes (csrc/seg_reader.hip; two when _preprocess AND prepare_size resize), the
    flip + ColorJitter + ToTensor kernel of the Footprints trainer, and the label kernel.  max_src_hw = the staged rectangle of a sample
    the pinned buffers are sized for at the start (batch_size of them; they grow when a batch needs more).

    device_decode=True (--device_decode): the image of a sample may also be the FILE, as decode_stage.read_sample(path, True) returns it.
    {'path', 'image', 'refused'} is a frame the reader thread decoded and is staged like any array.  For {'path', 'bytes', 'info'} the plan
    is drawn from the header's size, the same offset of the packed source buffer is reserved and nothing is copied: fp_jpeg_decode_window
    decodes the staged rectangle -- not the frame -- straight to that offset, so a device-decoded sample and a host-decoded one occupy the
    same bytes, and records, tables and resizes are the same either way.  The protocol is decode_stage.DecodeStage's, as for
    DeviceBatchAssembler: scans, records and table blocks in pinned buffers of the slot, everything launched optimistically, the status
    read in `collect` -- a DeviceLoader iteration after the decode was queued -- and a frame the device turned down decoded by `decode`
    (bytes -> uint8 [h, w, 3]; Pillow by default), its rectangle uploaded to its offset and the image half of the chain (resizes,
    fp_assemble_images) queued once more; the label half never read the frames.  `counters`: device / host_parser / host_status."""

    def __init__(self, batch_size, height, width, max_src_hw, slots=3, device="cuda", stream=None, check=False, device_decode=False, decode=None):
        from ..preprocessing.segmentation.datasets import plan as P
        self.P = P
        self.device_decode = bool(device_decode)
        lib = _lib.load()
        assert lib.fp_aug_params_bytes() == C.sizeof(AugParams)
        assert lib.fp_resize_window_sample_bytes() == C.sizeof(_lib.ResizeWindowSample)
        assert lib.fp_resize_window_table_bytes() == C.sizeof(_lib.ResizeWindowTable)
        assert lib.fp_seg_label_sample_bytes() == C.sizeof(_lib.SegLabelSample)
        self.B, self.H, self.W = int(batch_size), int(height), int(width)
        self.max_src_hw = (int(max_src_hw[0]), int(max_src_hw[1]))
        self.check = bool(check)          # read the kernels' status words after every launch (this WAITS for the stream): tests, debugging
        self._init_slots(device, stream)
        B, H, W = self.B, self.H, self.W
        self.out_bytes = B * H * W * 3
        self.mid_bytes = B * (H + 32) * (W + 32) * 3          # the first resize's windows of two-stage samples: the second never shrinks
        ids, offs = [], [0]
        for name in P.DATASETS:
            ids += sorted(P.GROUND_IDS[name])
            offs.append(len(ids))
        self.ground_ids = torch.tensor(ids, dtype=torch.int32, device=self.device)
        self.set_offsets = torch.tensor(offs, dtype=torch.int32, device=self.device)
        src_cap = B * self.max_src_hw[0] * self.max_src_hw[1] * 3
        for _ in range(slots):
            s = self._add_slot(
                d_buf=torch.empty(self.out_bytes + self.mid_bytes, dtype=torch.uint8, device=self.device),
                sums=torch.zeros(B, dtype=torch.int64, device=self.device), image=torch.empty((B, 3, H, W), device=self.device),
                ground_mask=torch.empty((B, H, W), device=self.device), labelled_pix=torch.empty((B, H, W), device=self.device),
                status=torch.zeros(1, dtype=torch.int32, device=self.device), used={}, calls=[])
            self._pair(s, "src", src_cap, torch.uint8)
            self._pair(s, "lab", src_cap, torch.uint8)
            self._pair(s, "par", B * C.sizeof(AugParams), torch.uint8)
            self._pair(s, "lrec", B * C.sizeof(_lib.SegLabelSample), torch.uint8)
            self._pair(s, "lidx", B * (H + W), torch.int32)
            for k in (0, 1):
                self._pair(s, "rec%d" % k, B * C.sizeof(_lib.ResizeWindowSample), torch.uint8)
                self._pair(s, "tab%d" % k, 2 * B * C.sizeof(_lib.ResizeWindowTable), torch.uint8)
                self._pair(s, "coef%d" % k, B * (H + W + 64) * 24, torch.int32)
        self.stage = self._make_stage(decode) if self.device_decode else None
        if self.device_decode:              # the decode stage's part of a slot; its pinned scan / record / table buffers come with the first batch
            for s in self.slots:
                self._pair(s, "status", B + 1, torch.int32)
                s.update(decoded=self.stage._event(), batch=None, pack=None)

    def _make_stage(self, decode):
        """the owner of the decode protocol (pack, status copy, fallback); its own layout, whole frames one after the other, is not used:
        `fill` lays out rectangles"""
        from .decode_stage import DecodeStage, host_decode
        return DecodeStage(self.B, self.H, self.W, None, self.device, decode=decode or host_decode)

    @property
    def counters(self):
        """DecodeStage.counters: frames decoded by the device, refused by the parser, decoded again after a non-zero status"""
        return dict(self.stage.counters) if self.stage is not None else dict(device=0, host_parser=0, host_status=0)

    def _pair(self, s, name, n, dtype):
        """a pinned host buffer and its device twin"""
        s["h_" + name] = torch.empty(int(n), dtype=dtype).pin_memory()
        s["d_" + name] = torch.empty(int(n), dtype=dtype, device=self.device)

    def _reserve(self, s, name, n):
        """the buffers grow when a batch needs more than they hold (a frame larger than max_src_hw; longer tap rows than the reference's
        resize factors give)"""
        if n > s["h_" + name].numel():
            ops.release(s["d_" + name], "seg_assembler:" + name)
            self._pair(s, name, n + n // 2, s["h_" + name].dtype)

    def _put(self, s, name, arr):
        """`arr` into the pinned buffer `name` from its start"""
        n = arr.size
        self._reserve(s, name, n)
        s["h_" + name].numpy()[:n] = arr
        s["used"][name] = n

    def draw(self, samples, is_train=True, rng=random):
        """the reference's draws for every sample of a batch, in batch order -> list of SegPlan (the `draw` of a DeviceLoader)"""
        return [self.P.draw_seg_plan(name, self._frame_hw(img), (self.H, self.W), is_train, rng) for name, img, _ in samples]

    @staticmethod
    def _frame_hw(img):
        """the frame's (h, w): an array's shape, a decoded file sample's, or the header's of a file the device decodes"""
        if isinstance(img, dict):
            return tuple(img["image"].shape[:2]) if "image" in img else (int(img["info"]["h"]), int(img["info"]["w"]))
        return tuple(img.shape[:2])

    def loader(self, source, is_train=True, rng=random):
        return DeviceLoader(source, self, is_train, rng, draw=self.draw)

    def fill(self, samples, plans):
        """host half: the plans' tables, the staged rectangles and every record into the next slot's pinned buffers"""
        if len(samples) != self.B or len(plans) != self.B:
            raise ValueError("expected %d samples" % self.B)
        P, H, W = self.P, self.H, self.W
        i, s = self._take_slot()
        nearest = {}

        def nearest_index(a, b):
            if (a, b) not in nearest:
                nearest[(a, b)] = ops.nearest_index(a, b)
            return nearest[(a, b)]

        # ---- file samples (device_decode): a frame the reader thread decoded is an array from here on; a file stays a dict
        files = [None] * self.B
        if any(isinstance(img, dict) for _, img, _ in samples):
            if not self.device_decode:
                raise ValueError("a sample's image is a file sample (decode_stage.read_sample): that needs device_decode=True")
            samples = list(samples)
            for b, (name, img, labels) in enumerate(samples):
                if isinstance(img, dict):
                    if "image" in img:
                        self.stage.counters["host_parser"] += 1 if "refused" in img else 0
                        samples[b] = (name, img["image"], labels)
                    else:
                        files[b] = img
        # ---- geometry first: what every sample needs staged, so that the pinned buffers can grow before anything is copied
        geo = []
        for b, ((name, img, labels), plan) in enumerate(zip(samples, plans)):
            hw = self._frame_hw(img)
            if plan.dataset != name or tuple(plan.src_hw) != hw or labels.shape[:2] != hw or tuple(plan.window[2:]) != (H, W):
                raise ValueError("sample %d: the plan was drawn for another sample" % b)
            if (files[b] is None and (img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3)) or labels.dtype != np.uint8:
                raise ValueError("sample %d: the image must be uint8 [h, w, 3] and the labels uint8" % b)
            ade = name == "ADE20K"
            if ade and (labels.ndim != 3 or labels.shape[2] != 3):
                raise ValueError("sample %d: ADE20K labels are the RGB segmentation image" % b)
            stages, rect = P.image_stages(plan, ops.resize_window_axis)         # the rectangle of the frame the window's taps reach
            rows, cols = P.label_tables(plan, nearest_index)                    # the rectangle the composed tables address
            lrect = (int(rows.min()), int(rows.max()) + 1, int(cols.min()), int(cols.max()) + 1)
            geo.append((stages, rect, rows, cols, lrect, 3 if ade else 1))
        self._reserve(s, "src", sum(g[1][2] * g[1][3] * 3 for g in geo))
        self._reserve(s, "lab", sum((g[4][1] - g[4][0]) * (g[4][3] - g[4][2]) * g[5] for g in geo))
        src_np, lab_np = s["h_src"].numpy(), s["h_lab"].numpy()
        calls = [ops.WindowBatch(3), ops.WindowBatch(3)]
        lrec = (_lib.SegLabelSample * self.B)()
        lidx = np.empty(self.B * (H + W), np.int32)
        src_off = lab_off = 0
        src_offsets = []
        mid_off = self.out_bytes
        for b, ((name, img, labels), (stages, (y0, x0, rh, rw), rows, cols, (r0, r1, c0, c1), lc)) in enumerate(zip(samples, geo)):
            # ---- image: its staged rectangle and the records of its one or two resizes
            n = rh * rw * 3
            if files[b] is None:
                src_np[src_off:src_off + n].reshape(rh, rw, 3)[:] = img[y0:y0 + rh, x0:x0 + rw]
            offset, rect = src_off, (y0, x0, rh, rw)                # a file: the decoder writes this rectangle to this offset
            src_offsets.append(src_off)
            src_off += n
            for k, st in enumerate(stages):
                last = k == len(stages) - 1
                out_offset = b * H * W * 3 if last else mid_off
                call = calls[k]
                call.add(offset, rect, call.table(st["in_hw"][1], st["out_hw"][1], st["table_h"]),
                         call.table(st["in_hw"][0], st["out_hw"][0], st["table_v"]), st["window"], out_offset)
                if not last:                    # the next resize reads this one's window as its staged rectangle
                    offset, rect = mid_off, st["window"]
                    mid_off += st["window"][2] * st["window"][3] * 3
                    if mid_off > self.out_bytes + self.mid_bytes:
                        raise ValueError("sample %d: the intermediate of its two resizes does not fit" % b)
            # ---- labels: one channel, but ADE20K's R and G
            lab = labels[r0:r1, c0:c1] if lc == 3 or labels.ndim == 2 else labels[r0:r1, c0:c1, 0]
            lab_np[lab_off:lab_off + lab.size].reshape(lab.shape)[:] = lab
            lidx[b * (H + W):b * (H + W) + H] = rows - r0
            lidx[b * (H + W) + H:(b + 1) * (H + W)] = cols - c0
            lrec[b] = _lib.SegLabelSample(lab_off, r1 - r0, c1 - c0, lc, b * (H + W), b * (H + W) + H,
                                          _lib.SEG_DECODE_ADE20K if lc == 3 else _lib.SEG_DECODE_CHANNEL0,
                                          _lib.SEG_LABELLED_NONZERO if name == "cityscapes" else _lib.SEG_LABELLED_ONES, P.DATASETS.index(name))
            lab_off += lab.size
        s["used"] = {"src": src_off, "lab": lab_off}
        if self.device_decode:              # the decode call's part: the files' scans, window records and table blocks into the slot's pinned buffers
            shapes = [self._frame_hw(img) for _, img, _ in samples]
            s["batch"] = dict(n=self.B, samples=[f if f is not None else {"image": img} for f, (_, img, _) in zip(files, samples)], shapes=shapes,
                              offsets=src_offsets, rects=[g[1] for g in geo], total=src_off, max_h=max(h for h, _ in shapes),
                              max_w=max(w for _, w in shapes), on_host=[b for b in range(self.B) if files[b] is None],
                              on_device=[b for b in range(self.B) if files[b] is not None])
            self.stage.pack_into(s, s["batch"])
        s["calls"] = []
        for k, call in enumerate(calls):
            if call.samples:
                rec, tab, coef = call.arrays()
                self._put(s, "rec%d" % k, rec)
                self._put(s, "tab%d" % k, tab)
                self._put(s, "coef%d" % k, coef)
                s["calls"].append((k, len(call.samples), len(call.tables), coef.size, call.max_src_h, call.max_src_w, call.max_win_h, call.max_win_w))
        self._put(s, "lrec", np.frombuffer(bytes(lrec), dtype=np.uint8))
        self._put(s, "lidx", lidx)
        self._put(s, "par", np.frombuffer(bytes((AugParams * self.B)(*[p.aug for p in plans])), dtype=np.uint8))
        return i

    def _launch(self, s, copies=True):
        """copies=False: the kernels alone, on what an earlier launch of the slot uploaded (benchmarks)"""
        decoding = self.device_decode and s["pack"] is not None
        for name, n in s["used"].items():
            if n and copies and not (decoding and name == "src"):
                self._upload(s, name, 0, n)
        if decoding and copies:
            # the staged rectangles of the frames that arrived decoded (neighbours in one copy), then the decode of the others into the
            # gaps and the copy of its status words, which `collect` reads; nothing waits
            batch, runs = s["batch"], []
            for b in batch["on_host"]:
                off, (_, _, rh, rw) = batch["offsets"][b], batch["rects"][b]
                if runs and runs[-1][1] == off:
                    runs[-1][1] = off + rh * rw * 3
                else:
                    runs.append([off, off + rh * rw * 3])
            for lo, hi in runs:
                self.stage._upload(s, lo, hi - lo)
            self.stage._decode(s, s["pack"], batch)
            s["decoded"].record()
        self._image_half(s)
        self._label_half(s)

    def _upload(self, s, name, lo, n):
        s["d_" + name][lo:lo + n].copy_(s["h_" + name][lo:lo + n], non_blocking=True)

    def collect(self, slot):
        s = self.slots[slot]
        if self.device_decode and s["batch"] is not None:
            with ops.on_stream(self.stream):
                self._repair(s)
        return super().collect(slot)

    def _repair(self, s):
        """the decode was queued a whole step ago (DeviceLoader): its status is there.  What the device turned down goes through `decode`
        now, its rectangle to its offset, and the image half of the slot's chain runs again; the label half never read the frames"""
        def again():
            self._image_half(s)
            s["ready"].record(self.stream)
        self.stage.collect(s, again)

    def _image_half(self, s):
        """the one or two windowed resizes and the flip + jitter + ToTensor kernel: everything that reads the packed source buffer"""
        buf = s["d_buf"]
        for k, n, n_tables, coeffs_len, msh, msw, mwh, mww in s["calls"]:
            # the first call reads the staged rectangles; the second one reads the first one's windows inside `buf`
            src, src_bytes = (s["d_src"], s["used"]["src"]) if k == 0 else (buf, buf.numel())
            ops.resize_window_u8(src, src_bytes, s["d_rec%d" % k], n, s["d_tab%d" % k], n_tables, s["d_coef%d" % k], coeffs_len, buf, 3,
                                 msh, msw, mwh, mww, check=self.check)
        _lib.check(_lib.load().fp_assemble_images(buf.data_ptr(), s["d_par"].data_ptr(), s["sums"].data_ptr(), s["image"].data_ptr(),
                                                  self.B, self.H, self.W, ops.stream()), "fp_assemble_images")

    def _label_half(self, s):
        ops.seg_labels(s["d_lab"], s["used"]["lab"], s["d_lrec"], self.B, s["d_lidx"], s["used"]["lidx"], self.ground_ids, self.set_offsets,
                       self.H, self.W, ground_mask=s["ground_mask"], labelled_pix=s["labelled_pix"], status=s["status"], check=self.check)

    def _batch(self, s):
        return {"image": s["image"], "ground_mask": s["ground_mask"], "labelled_pix": s["labelled_pix"]}


class SyntheticSegSource:
    """`steps` batches of host samples (dataset name, image uint8 [h, w, 3], labels uint8) with the shapes the segmentation file readers
    deliver, for the benchmark and the tests: a small pool of random frames, cycled.  frames: list of (dataset name, (h, w)), taken in
    turn.  Label images carry ids of the dataset's range, a fair share of them ground ids."""

    def __init__(self, batch_size, steps, frames, seed=10, pool=None):
        from ..preprocessing.segmentation.datasets.plan import GROUND_IDS
        rng = np.random.default_rng(seed)
        self.B, self.steps, self.first, self.stride = batch_size, steps, 0, 1
        self.pool = []
        for j in range(pool or max(len(frames), batch_size)):
            name, (h, w) = frames[j % len(frames)]
            image = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
            blocks = rng.integers(0, 4, ((h + 15) // 16, (w + 15) // 16))             # 16 x 16 patches: 0 unlabelled, 1-2 ground, 3 other
            ground = np.asarray(GROUND_IDS[name])[rng.integers(0, len(GROUND_IDS[name]), blocks.shape)]
            ids = np.where(blocks == 0, 0, np.where(blocks == 3, ground + 1, ground))
            ids = np.kron(ids, np.ones((16, 16), np.int64))[:h, :w]
            if name == "ADE20K":
                labels = np.stack([ids // 256 * 10 + rng.integers(0, 10, ids.shape), ids % 256, rng.integers(0, 256, ids.shape)], -1).astype(np.uint8)
            elif name == "cityscapes":
                labels = np.repeat(ids[..., None], 3, -1).astype(np.uint8)
            else:
                labels = (ids == 1).astype(np.uint8)
            self.pool.append((name, image, labels))
        self.dataset = range(steps * batch_size)

    def __len__(self):
        return len(range(self.first, self.steps, self.stride))

    def shard(self, rank, world):
        import copy
        v = copy.copy(self)
        v.steps = (self.steps // world) * world
        v.first, v.stride = rank, world
        return v

    def __iter__(self):
        for i in range(self.first, self.steps, self.stride):
            yield [self.pool[(i * self.B + j) % len(self.pool)] for j in range(self.B)]
