"""The thread, ring and writer scaffolding of the two inference pipelines (preprocessing/segmentation/inference.py::Tester.test and
evaluation/inference.py::InferenceManager.run_dataset):
  readers  `num_workers` THREADS read ahead, in order;
  device   the calling thread queues each batch on a ring of slots and does not wait for the device -- with a decode stage
           (datasets/decode_stage.py) in two parts: batch k + 1's `ahead` is queued before batch k's `rest`;
  writer   ONE thread waits for a slot's results, saves its files and hands the slot back.  A slot is not refilled before that.
An exception in any thread ends the run with that exception; every wait on a queue, a future or a slot has a timeout after which the
waiting thread looks at the error flag."""
import collections
import queue
import threading
import time


class RingPipeline:

    POLL = 0.05          # seconds between two looks at the error flag while a thread waits
    SPIN = 0.0002        # seconds between two queries of a slot's `ready` event (a batch takes milliseconds)

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

    def _wait_event(self, event):
        """wait for a device event with a timeout, like every other wait: look at the stop flag in between"""
        while not event.query():
            if self._stop.is_set():
                raise RuntimeError("the inference pipeline was stopped while a batch was in flight")
            time.sleep(self.SPIN)

    def _fetch_jpeg_files(self, s, n, shape):
        """the slot's batch of n pictures of `shape` was encoded on the device (ops.jpeg_encode_packed into s['d_scan']) and its length
        table is on the host (s['h_tab']): copy the scans' bytes in use -- on `self.copy_stream`, a stream of the writer thread's own,
        which it waits for -- into the pinned `self.h_scan`, which grows, and put headers and EOI around them -> the .jpg files' bytes"""
        import torch
        from .. import ops
        table = s["h_tab"].numpy()[:n + 1]
        used = int(table[n][0])
        if self.h_scan is None or self.h_scan.numel() < used:
            self.h_scan = torch.empty(max(used + used // 4, 1 << 16), dtype=torch.uint8).pin_memory()
        if used:
            with torch.cuda.stream(self.copy_stream):
                self.h_scan[:used].copy_(s["d_scan"][:used], non_blocking=True)
            self.copy_stream.synchronize()
        return ops.jpeg_files(self.h_scan.numpy()[:used], table, [shape] * n, 95)

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
                results = collect(si, len(indices))
                for i, idx in enumerate(indices):
                    save(idx, results, i)
                free[si].set()                              # only now may the slot's pinned buffers be refilled
        except BaseException as exc:                        # noqa: handed to the thread that called run_ring()
            self._fail(exc)

    def run_ring(self, N, B, n_slots, num_workers, read, rest, collect=None, save=None, ahead=None, writer=None, name="infer"):
        """N samples in batches of B (the last may be short) through n_slots slots.
        read(index) -> sample with 'idx' (reader threads); ahead(slot index, samples) / rest(slot index, samples): the calling thread's
        two parts of a batch (ahead may be None: then a batch is one part); collect(slot index, n) -> results (writer thread; may wait);
        save(idx, results, i) (writer thread) -- or writer(jobs, free): the writer thread's whole body, for a class that has its own
        around `_ring_writer`"""
        from concurrent.futures import ThreadPoolExecutor, TimeoutError as FutureTimeout
        if ahead is not None and n_slots < 2:
            raise ValueError("decoding one batch ahead needs a ring of at least 2 slots")
        self._error = None
        self._stop.clear()
        jobs = queue.Queue()
        free = [threading.Event() for _ in range(n_slots)]
        for ev in free:
            ev.set()
        if writer is None:
            writer = lambda jobs, free: self._ring_writer(jobs, free, collect, save)
        writer = threading.Thread(target=writer, args=(jobs, free), name="%s-writer" % name, daemon=True)
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
            rest(si, samples)
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
                if ahead is None:
                    second_part(si, samples)
                    continue
                ahead(si, samples)
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
