"""JPEG decoding for the inference pipelines, one batch ahead of the network.

ops.jpeg_decode waits for the device's status before it returns, which is right for one call and wrong inside a pipeline whose calling
thread never waits.  `DecodeStage` splits the call in two around a batch:

  reader threads  `read_sample(path, device_decode)`: the file's bytes and ops.jpeg_parse.  A file the parser refuses (PNG, progressive,
                  restart markers, ...) is decoded by Pillow at once, on that thread; for the others nothing is decoded on the host.
  queue(s, samples)   lays the batch out in the slot's packed source buffer -- dense [h][w][3], one picture after the other, with the
                  fp_resize_sample records ops.resize_pack writes; the sizes come from the headers -- copies the host-decoded frames into
                  the pinned buffer at their offsets, queues their upload, the uploads of the scans and ops.jpeg_decode_packed into the
                  same device buffer, a copy of the status into pinned memory, and records an event.  Waits for nothing.
                  A batch the host decoded entirely -- every batch without --device_decode -- is one upload of the bytes in use.
  finish(s)       waits for that event, decodes every sample whose status is not 0 with Pillow and uploads it to the sample's offset
                  (whatever Pillow raises ends the run, with the file's path in the message), and returns what ops.resize_u8_packed
                  needs, with the frames' shapes.

Every user goes through the stage, with or without device decoding: the two pipelines' device side (datasets/ring.py::DeviceRing), and
predict_simple, which calls queue and finish back to back.  A pipeline that decodes on the device calls queue(k + 1) before finish(k) and
queues the rest of batch k after it, so the only device wait of the calling thread is for decode work queued a whole network pass
earlier; with every status 0 the host decodes nothing.  Counters: `device` (decoded by the
device), `host_parser` (refused by the parser), `host_status` (decoded again after a non-zero status).

The trainer's loaders (datasets/device_path.py, --device_decode) run the same protocol with the halves of `queue` apart, because their
host half and their device half live on two threads: fill + pack_into on the staging thread -- pack_into writes the scans, records and
table blocks into pinned buffers of the SLOT, which grow when a batch needs more, so that a warmed-up ring allocates no pinned memory per
training step -- queue_packed on the thread that launches, finish when the batch is collected.

The segmentation trainer's assembler (device_path.SegBatchAssembler) lays its batch out itself -- the rectangle of each frame that its
crop window needs, not the frame -- and hands the stage a batch description with 'rects': pack_into then writes fp_jpeg_decode_window's
records, `_decode` calls ops.jpeg_decode_window_packed, and `finish` repairs the rectangle of a frame the device turned down."""
import ctypes as C
import io
import time

import numpy as np
import torch

from .. import _lib, ops

MAX_ROW_BYTES = 65528           # the resize stages one source row: max_w * 3 bytes (fp_resize_u8)
SPIN = 0.0002                   # seconds between two queries of a device event (a batch takes milliseconds)


def wait_event(event, stop, doing):
    """wait for a device event as the pipelines' threads wait for everything: looking at the `stop` flag (may be None) in between"""
    while not event.query():
        if stop is not None and stop.is_set():
            raise RuntimeError("the inference pipeline was stopped while a batch was %s" % doing)
        time.sleep(SPIN)


def host_decode(data):
    """`np.asarray(Image.open(f).convert("RGB"))` of a file's bytes: the decoder of every host reader of this package"""
    from PIL import Image
    with Image.open(io.BytesIO(data)) as im:
        return np.asarray(im.convert("RGB"), dtype=np.uint8)


def read_sample(path, device_decode, decode=host_decode):
    """a reader thread's work for one file -> {'path', 'image': uint8 [h, w, 3]} (decoded on the host; 'refused': the parser's reason
    when device decoding was asked for) or {'path', 'bytes', 'info'} (for the device)"""
    with open(path, "rb") as fh:
        data = fh.read()
    if device_decode:
        info = ops.jpeg_parse(data)
        if info["device"]:
            return {"path": path, "bytes": data, "info": info}
        return {"path": path, "image": _decode_named(decode, data, path), "refused": info["reason"]}
    return {"path": path, "image": _decode_named(decode, data, path)}


def _decode_named(decode, data, path):
    """decode(data); whatever it raises is raised again with the file's path in front of its message"""
    try:
        return decode(data)
    except Exception as exc:
        try:
            named = type(exc)("%s: %s" % (path, exc))
        except Exception:                                   # an exception class that does not take one string
            named = RuntimeError("%s: %r" % (path, exc))
        raise named from exc


class DecodeStage:

    def __init__(self, batch_size, H, W, tables, device, decode=host_decode, stop=None, max_hw=None):
        """tables: the device's ops.resize_table_set; decode: bytes -> uint8 [h, w, 3] (Pillow; tests inject a recording one); stop: a
        threading.Event the wait in `finish` looks at; max_hw: the largest frame (h, w) the layout accepts (None: any that fits a row)"""
        self.batch_size, self.H, self.W = int(batch_size), int(H), int(W)
        self.max_hw = None if max_hw is None else (int(max_hw[0]), int(max_hw[1]))
        self.tables, self.device, self.decode, self.stop = tables, device, decode, stop
        self.counters = dict(device=0, host_parser=0, host_status=0)

    # ---- the slot's buffers -------------------------------------------------------------------------------------------------------------
    def new_slot(self):
        """the stage's part of a ring slot: a dict, to which a pipeline adds its own buffers"""
        rec_bytes = self.batch_size * C.sizeof(_lib.ResizeSample)
        return dict(src_cap=0, h_src=None, d_src=None, h_rec=self._pinned(rec_bytes, torch.uint8), d_rec=self._empty(rec_bytes, torch.uint8),
                    h_status=self._pinned(self.batch_size + 1, torch.int32), d_status=self._empty(self.batch_size + 1, torch.int32),
                    decoded=self._event(), batch=None)

    def _pinned(self, n, dtype):
        return torch.empty(n, dtype=dtype).pin_memory()

    def _empty(self, n, dtype):
        return torch.empty(n, dtype=dtype, device=self.device)

    def _event(self):
        return torch.cuda.Event()

    def reserve(self, s, nbytes):
        """the packed source buffers grow when a batch needs more than they hold (the slot's previous batch has left the device)"""
        if nbytes > s["src_cap"]:
            ops.release(s["d_src"], "decode_stage:src")
            s["src_cap"] = nbytes + nbytes // 8
            s["h_src"] = self._pinned(s["src_cap"], torch.uint8)
            s["d_src"] = self._empty(s["src_cap"], torch.uint8)

    # ---- host half ----------------------------------------------------------------------------------------------------------------------
    def layout(self, samples):
        """-> (shapes [(h, w)], offsets, total bytes, max_h, max_w) of the batch in the packed buffer, from the frames and the headers"""
        n = len(samples)
        if not 1 <= n <= self.batch_size:
            raise ValueError("a batch holds 1 to %d frames" % self.batch_size)
        shapes = []
        for smp in samples:
            if "image" in smp:
                im = smp["image"]
                if im.ndim != 3 or im.shape[2] != 3 or im.dtype != np.uint8:
                    raise ValueError("%s: frames must be decoded RGB images, uint8 [h, w, 3]" % smp.get("path", "a sample"))
                shapes.append((int(im.shape[0]), int(im.shape[1])))
            else:
                shapes.append((int(smp["info"]["h"]), int(smp["info"]["w"])))
            if shapes[-1][1] * 3 > MAX_ROW_BYTES:
                raise ValueError("%s: a frame of %d columns is wider than the resize's row buffer (%d bytes)"
                                 % (smp.get("path", "a sample"), shapes[-1][1], MAX_ROW_BYTES))
            if self.max_hw is not None and (shapes[-1][0] > self.max_hw[0] or shapes[-1][1] > self.max_hw[1]):
                raise ValueError("%s: a frame of %d x %d is larger than max_src_hw = %r" % (smp.get("path", "a sample"), *shapes[-1], self.max_hw))
        offsets, at = [], 0
        for h, w in shapes:
            offsets.append(at)
            at += h * w * 3
        return shapes, offsets, at, max(h for h, _ in shapes), max(w for _, w in shapes)

    def fill(self, s, samples):
        """records and host-decoded frames into the slot's pinned buffers -> the batch's description (kept in s['batch'])"""
        shapes, offsets, total, max_h, max_w = self.layout(samples)
        self.reserve(s, total)
        rec = (_lib.ResizeSample * len(samples))()
        src = s["h_src"].numpy()
        on_host, on_device = [], []
        for b, (smp, (h, w), off) in enumerate(zip(samples, shapes, offsets)):
            rec[b] = _lib.ResizeSample(off, h, w, self.tables.index(w, self.W, "lanczos"), self.tables.index(h, self.H, "lanczos"))
            if "image" in smp:
                src[off:off + h * w * 3] = smp["image"].reshape(-1)
                on_host.append(b)
                if "refused" in smp:
                    self.counters["host_parser"] += 1
            else:
                on_device.append(b)
        raw = np.frombuffer(bytes(rec), dtype=np.uint8)
        s["h_rec"].numpy()[:raw.size] = raw
        s["batch"] = dict(n=len(samples), samples=samples, shapes=shapes, offsets=offsets, total=total, max_h=max_h, max_w=max_w,
                          on_host=on_host, on_device=on_device)
        return s["batch"]

    PACK_ARRAYS = (("scans", np.uint8, torch.uint8), ("records", np.uint8, torch.uint8), ("tables", np.int32, torch.int32))

    def _pack_arrays(self, batch):
        """ops.jpeg_decode_pack of the batch's device samples, or None"""
        idx = batch["on_device"]
        if not idx:
            return None
        smp = batch["samples"]
        rects = [batch["rects"][b] for b in idx] if batch.get("rects") else None        # a batch of windows: fp_jpeg_decode_window's records
        return ops.jpeg_decode_pack([smp[b]["bytes"] for b in idx], [smp[b]["info"] for b in idx], out_offsets=[batch["offsets"][b] for b in idx],
                                    rects=rects)

    def pack(self, batch):
        """ops.jpeg_decode_pack of the batch's device samples, every array in pinned memory, or None"""
        pack = self._pack_arrays(batch)
        if pack is None:
            return None
        for key, np_type, dtype in self.PACK_ARRAYS:
            host = self._pinned(pack[key].size, dtype)
            host.numpy()[:] = pack[key].view(np_type)
            pack[key] = host
        return pack

    def pack_into(self, s, batch):
        """`pack` into pinned buffers that belong to the slot (h_scans, h_records, h_tables; made on first use, replaced by larger ones when
        a batch needs more: the slot's previous uploads have landed when it is filled again) -> the pack (kept in s['pack']), or None"""
        pack = self._pack_arrays(batch)
        if pack is not None:
            for key, np_type, dtype in self.PACK_ARRAYS:
                n = pack[key].size
                host = s.get("h_" + key)
                if host is None or host.numel() < n:
                    host = s["h_" + key] = self._pinned(n + n // 4, dtype)
                host.numpy()[:n] = pack[key].view(np_type)
                pack[key] = host[:n]
        s["pack"] = pack
        return pack

    # ---- device half --------------------------------------------------------------------------------------------------------------------
    def queue(self, s, samples):
        """queue a batch's uploads and its decode on the current stream; waits for nothing"""
        batch = self.fill(s, samples)
        self.queue_packed(s, batch, self.pack(batch))

    def queue_packed(self, s, batch, pack):
        """the device half of `queue`, for a batch that `fill` laid out and `pack` / `pack_into` packed"""
        self._upload_records(s)
        if pack is None:                                    # the host decoded every frame: they lie dense from 0, one copy
            self._upload(s, 0, batch["total"])
            return
        for b in batch["on_host"]:
            h, w = batch["shapes"][b]
            self._upload(s, batch["offsets"][b], h * w * 3)
        self._decode(s, pack, batch)
        s["decoded"].record()

    # ---- the same, in the three pieces a training loader calls (host half on its staging thread, device half on the launching one) ---------
    def prepare(self, s, samples):
        """fill + pack_into -> the batch's description"""
        batch = self.fill(s, samples)
        self.pack_into(s, batch)
        return batch

    def launch(self, s):
        """queue_packed of what `prepare` left in the slot"""
        self.queue_packed(s, s["batch"], s["pack"])

    def collect(self, s, again):
        """finish; when a frame had to be decoded by the host, `again()` queues the work that read the packed buffer once more -> finish's dict"""
        done = self.finish(s)
        if any(st > 0 for st in done["status"]):
            again()
        return done

    def _upload_records(self, s):
        s["d_rec"].copy_(s["h_rec"], non_blocking=True)

    def _upload(self, s, off, nbytes):
        s["d_src"][off:off + nbytes].copy_(s["h_src"][off:off + nbytes], non_blocking=True)

    def _decode(self, s, pack, batch):
        nd = len(batch["on_device"])
        decode = ops.jpeg_decode_window_packed if "rects" in pack else ops.jpeg_decode_packed
        decode(pack, out=s["d_src"], out_bytes=batch["total"], status=s["d_status"][:nd + 1], device=self.device)
        s["h_status"][:nd + 1].copy_(s["d_status"][:nd + 1], non_blocking=True)

    def _status(self, s, nd):
        return s["h_status"].numpy()[:nd].copy()

    def finish(self, s):
        """wait for the batch's decode; Pillow decodes what the device turned down -> dict(src, total, records, n, max_h, max_w, shapes,
        status): the arguments of ops.resize_u8_packed, the frames' (h, w) in the buffer's order, and the device's status per sample
        (-1: decoded on the host from the start)"""
        batch = s["batch"]
        if batch is None:
            raise RuntimeError("DecodeStage.finish: no batch was queued on this slot")
        s["batch"] = None
        if batch["on_device"]:                              # nothing to wait for when the host decoded every frame
            wait_event(s["decoded"], self.stop, "being decoded")
        status = [-1] * batch["n"]
        device_status = self._status(s, len(batch["on_device"])) if batch["on_device"] else []
        for b, st in zip(batch["on_device"], device_status):
            status[b] = int(st)
            smp = batch["samples"][b]
            if status[b] == 0:
                self.counters["device"] += 1
                continue
            frame = _decode_named(self.decode, smp["bytes"], smp.get("path", "sample %d" % b))
            h, w = batch["shapes"][b]
            if frame.shape != (h, w, 3):
                raise ValueError("%s: the header says %d x %d, Pillow decoded %r" % (smp.get("path", "sample %d" % b), h, w, frame.shape))
            off = batch["offsets"][b]
            if batch.get("rects"):                          # the buffer holds the sample's rectangle alone: that is what is repaired
                y0, x0, rh, rw = batch["rects"][b]
                frame = frame[y0:y0 + rh, x0:x0 + rw]
            s["h_src"].numpy()[off:off + frame.size] = frame.reshape(-1)
            self._upload(s, off, frame.size)
            self.counters["host_status"] += 1
        return dict(src=s["d_src"], total=batch["total"], records=s.get("d_rec"), n=batch["n"], max_h=batch["max_h"], max_w=batch["max_w"],
                    shapes=batch["shapes"], status=status)
