"""What the two inference pipelines (preprocessing/segmentation/inference.py::Tester.test and
evaluation/inference.py::InferenceManager.run_dataset) share, which is everything but the network and its output kernel.

`RingPipeline` is the thread, ring and writer scaffolding:
  readers  `num_workers` THREADS read ahead, in order;
  device   the calling thread queues each batch on a ring of slots, in two parts (`ahead`, `rest`), and does not wait for the device; with
           `one_ahead` batch k + 1's `ahead` is queued before batch k's `rest`;
  writer   ONE thread waits for a slot's results, saves its files and hands the slot back.  A slot is not refilled before that.
An exception in any thread ends the run with that exception; every wait on a queue, a future or a slot has a timeout after which the
waiting thread looks at the error flag.

`DeviceRing` is the device side of such a ring, the three calls `run_ring` is given: the slots' buffers and one decode stage
(datasets/decode_stage.py), `ahead` (the stage's queue), `rest` (the stage's finish, Resize + ToTensor, network, output kernel, copies
back, JPEG encoder) and `collect` (the writer's wait and its views of the results).  A network brings its number of output channels and
two callables, `network` and `pack`."""
import collections
import contextlib
import queue
import threading

import torch

from .. import ops
from .decode_stage import DecodeStage, wait_event


@contextlib.contextmanager
def full_resolution_heads(model):
    """eval mode and "just take max resolution prediction" (reference inference.py:79, :104) for the length of a run or of a blocking
    batch; the model may be the caller's: its `inference_scales` comes back"""
    scales = getattr(model, "inference_scales", None)
    model.eval()
    model.inference_scales = ("1/1",)
    try:
        yield
    finally:
        model.inference_scales = scales


class DeviceRing:

    def __init__(self, B, H, W, n_slots, channels, network, pack, visualise=False, device_jpeg=False, stop=None):
        """per slot the decode stage's buffers (packed frames, records, status), the device outputs and the pinned buffers the results
        come back through.  network(image [n, 3, H, W]) -> logits; pack(logits, image or None, want_picture, out_half [n, channels, H, W]
        float16, out_picture [n, H, 2 W, 3] uint8 or None): the output kernel; stop: the threading.Event the waits look at"""
        if not torch.cuda.is_available():
            raise RuntimeError("test-set inference has no CPU compute path: it needs a MI355X")
        self.B, self.H, self.W, self.visualise, self.device_jpeg = B, H, W, bool(visualise), bool(visualise and device_jpeg)
        self.network, self.pack, self.stop = network, pack, stop
        self.device = torch.device("cuda", torch.cuda.current_device())
        self.tables = ops.resize_table_set(self.device)
        self.stage = DecodeStage(B, H, W, self.tables, self.device, stop=stop)
        self.slots = []
        for _ in range(n_slots):
            s = self.stage.new_slot()
            s.update(ready=torch.cuda.Event(), d_u8=torch.empty((B, H, W, 3), dtype=torch.uint8, device=self.device),
                     d_half=torch.empty((B, channels, H, W), dtype=torch.float16, device=self.device),
                     h_half=torch.empty((B, channels, H, W), dtype=torch.float16).pin_memory(), d_pic=None, h_pic=None)
            if self.visualise:
                s["d_pic"] = torch.empty((B, H, 2 * W, 3), dtype=torch.uint8, device=self.device)
            if self.device_jpeg:
                s["d_scan"] = torch.empty(ops.jpeg_max_scan_bytes(B, H, 2 * W), dtype=torch.uint8, device=self.device)
                s["d_tab"] = torch.empty((B + 1, 2), dtype=torch.int64, device=self.device)
                s["h_tab"] = torch.empty((B + 1, 2), dtype=torch.int64).pin_memory()
            elif self.visualise:
                s["h_pic"] = torch.empty((B, H, 2 * W, 3), dtype=torch.uint8).pin_memory()
            self.slots.append(s)
        if self.device_jpeg:
            # the pictures of a batch lie dense in d_pic: one set of records serves every slot, and its first n a batch of n
            self.jpeg_records = torch.from_numpy(ops.jpeg_records([(H, 2 * W)] * B)[0]).to(self.device)
            self.copy_stream = torch.cuda.Stream(self.device)
            self.h_scan = None                      # the writer's pinned buffer for the bytes in use; grows

    def fits(self, *shape):
        """was this ring built for (B, H, W, slots, visualise, device_jpeg), on the current device?"""
        return (shape == (self.B, self.H, self.W, len(self.slots), self.visualise, self.device_jpeg)
                and self.device.index == torch.cuda.current_device())

    def ahead(self, si, samples):
        """calling thread: the batch's uploads and its decode; waits for nothing"""
        self.stage.queue(self.slots[si], samples)

    def rest(self, si):
        """calling thread: the stage's wait for the decode, then the batch packed in the slot's d_src through resize, ToTensor, network,
        the output kernel, the copies back into the slot's pinned buffers and the JPEG encoder; records the slot's `ready` event.  Nothing
        here waits for the device but the stage"""
        s = self.slots[si]
        d = self.stage.finish(s)
        n, H, W = d["n"], self.H, self.W
        with torch.no_grad():
            u8 = ops.resize_u8_packed(d["src"], d["total"], d["records"], n, H, W, 3, d["max_h"], d["max_w"], self.tables, out=s["d_u8"][:n])
            image = ops.to_tensor_u8(u8)
            self.pack(self.network(image), image if self.visualise else None, self.visualise, s["d_half"][:n],
                      s["d_pic"][:n] if self.visualise else None)
            s["h_half"][:n].copy_(s["d_half"][:n], non_blocking=True)
            if self.device_jpeg:
                ops.jpeg_encode_packed(s["d_pic"].view(-1), n * H * 2 * W * 3, self.jpeg_records, n, 95, out=s["d_scan"], max_h=H, max_w=2 * W,
                                       table=s["d_tab"][:n + 1])
                s["h_tab"][:n + 1].copy_(s["d_tab"][:n + 1], non_blocking=True)
            elif self.visualise:
                s["h_pic"][:n].copy_(s["d_pic"][:n], non_blocking=True)
            s["ready"].record()

    def collect(self, si, n):
        """writer thread: wait for the slot's results -> (float16 numpy [n, channels, H, W], the n pictures -- uint8 numpy [n, H, 2 W, 3],
        or the .jpg files' bytes with device_jpeg -- or None): views of the slot's pinned buffers"""
        s = self.slots[si]
        self._wait_event(s["ready"])                        # a wait with a timeout, like every other one
        if self.device_jpeg:
            return s["h_half"].numpy()[:n], self._fetch_jpeg_files(s, n)
        return s["h_half"].numpy()[:n], (s["h_pic"].numpy()[:n] if self.visualise else None)

    def _wait_event(self, event):
        wait_event(event, self.stop, "in flight")

    def _fetch_jpeg_files(self, s, n):
        """the slot's batch of n pictures was encoded on the device (ops.jpeg_encode_packed into s['d_scan']) and its length table is on
        the host (s['h_tab']): copy the scans' bytes in use -- on `self.copy_stream`, a stream of the writer thread's own, which it waits
        for; the thread that queues batches never does -- into the pinned `self.h_scan`, which grows, and put headers and EOI around them
        -> the .jpg files' bytes"""
        table = s["h_tab"].numpy()[:n + 1]
        used = int(table[n][0])
        if self.h_scan is None or self.h_scan.numel() < used:
            self.h_scan = torch.empty(max(used + used // 4, 1 << 16), dtype=torch.uint8).pin_memory()
        if used:
            with torch.cuda.stream(self.copy_stream):
                self.h_scan[:used].copy_(s["d_scan"][:used], non_blocking=True)
            self.copy_stream.synchronize()
        return ops.jpeg_files(self.h_scan.numpy()[:used], table, [(self.H, 2 * self.W)] * n, 95)


class RingPipeline:

    POLL = 0.05          # seconds between two looks at the error flag while a thread waits

    def _ring_init(self):
        self._error = None
        self._stop = threading.Event()

    def _fail(self, exc):
        if self._error is None:
            self._error = exc
        self._stop.set()

    def _check(self):
        if self._error is not None:
            raise self._error

    def _wait(self, done):
        """poll `done(timeout)` (True when what is waited for has happened), looking at the error flag in between"""
        while not done(self.POLL):
            self._check()

    def _release(self, free, si):
        """writer thread: only now may the slot's pinned buffers be refilled"""
        free[si].set()

    def _ring_writer(self, jobs, free, collect, save):
        try:
            while True:
                try:
                    job = jobs.get(timeout=self.POLL)
                except queue.Empty:
                    if self._stop.is_set():
                        return
                    continue
                if job is None:
                    return
                si, indices = job
                arrays, pictures = collect(si, len(indices))
                for i, idx in enumerate(indices):
                    save(idx, arrays[i], None if pictures is None else pictures[i])
                self._release(free, si)
        except BaseException as exc:                        # noqa: handed to the thread that called run_ring()
            self._fail(exc)

    def run_ring(self, N, B, n_slots, num_workers, read, ahead, rest, collect, save, one_ahead=False, name="infer"):
        """N samples in batches of B (the last may be short) through n_slots slots.
        read(index) -> sample with 'idx' (reader threads); ahead(slot index, samples) and rest(slot index): the calling thread's two parts
        of a batch -- one after the other, or with one_ahead the next batch's `ahead` in between; collect(slot index, n) -> (arrays,
        pictures or None) (writer thread; may wait); save(idx, array, picture or None) (writer thread)"""
        from concurrent.futures import ThreadPoolExecutor, TimeoutError as FutureTimeout
        if one_ahead and n_slots < 2:
            raise ValueError("decoding one batch ahead needs a ring of at least 2 slots")
        self._error = None
        self._stop.clear()
        jobs = queue.Queue()
        free = [threading.Event() for _ in range(n_slots)]
        for ev in free:
            ev.set()
        writer = threading.Thread(target=self._ring_writer, args=(jobs, free, collect, save), name="%s-writer" % name, daemon=True)
        readers = ThreadPoolExecutor(num_workers, thread_name_prefix="%s-reader" % name)
        pending = collections.deque()
        read_ahead = B * (n_slots + 1)                      # frames read ahead of the batch being queued
        submitted = 0

        def guarded_read(index):
            return None if self._stop.is_set() else read(index)

        def result_of(fut):
            def done(timeout):
                try:
                    fut.result(timeout=timeout)
                    return True
                except FutureTimeout:
                    return False
            self._wait(done)
            return fut.result()

        def second_part(si, samples):
            rest(si)
            jobs.put((si, [smp["idx"] for smp in samples]))

        writer.start()
        try:
            n_batches = (N + B - 1) // B
            held = None                                     # the batch whose first part is queued and whose second is not
            for k in range(n_batches):
                indices = list(range(k * B, min((k + 1) * B, N)))               # the last batch may be short
                while submitted < min(N, k * B + read_ahead):
                    pending.append(readers.submit(guarded_read, submitted))
                    submitted += 1
                samples = [result_of(pending.popleft()) for _ in indices]
                si = k % n_slots
                self._wait(free[si].wait)                   # the writer is done with this slot's previous batch
                free[si].clear()
                ahead(si, samples)
                if not one_ahead:
                    second_part(si, samples)
                    continue
                if held is not None:
                    second_part(*held)
                held = (si, samples)
            if held is not None:
                second_part(*held)
            jobs.put(None)
            self._wait(lambda timeout: (writer.join(timeout), not writer.is_alive())[1])
            self._check()
        except BaseException as exc:
            self._fail(exc)
            raise
        finally:
            self._stop.set()
            for fut in pending:
                fut.cancel()
            readers.shutdown(wait=True)
            while writer.is_alive():
                writer.join(self.POLL)
