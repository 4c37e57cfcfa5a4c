"""The trainer's TensorBoard log event -- counterpart of footprints/training/logger.py (`log` and `TimeLogger`).

The reference's `log` holds the training thread while it brings twenty tensors to the host, normalises and colour-maps them in numpy and
encodes forty-eight PNGs.  Here the training thread only queues work:

  training stream   ops.log_panels: the twelve pictures of each logged sample as bytes, two launches.  Running on the stream that trains is
                    what keeps the next step from overwriting the network's outputs and the loader's slot under the kernels.  Behind
                    them, on the same stream, the copy of the bytes into a pinned slot (0.3 - 0.8 ms once per log event) and an event.
                    No stream is created for the copy: the engine owns the layout of streams on the hardware queues (engine.py), and one
                    more stream anywhere in the process shifts which streams share a queue.
  writer thread     polls that event (as datasets/decode_stage.py::wait_event does), then encodes the PNGs, writes `lr`, `loss` and the
                    pictures through the `SummaryWriter`, flushes, and frees the slot.

There are two slots because the train and the val batch are logged at the same step; with none free `log` waits for the writer, and
nothing is dropped.  Whatever fails -- the renderer when it is queued, or anything on the writer thread -- is raised by the next `log` or
by `close`, and the events still queued behind a failure are let go."""
import queue
import threading
import time

import torch

SPIN = 0.0002           # seconds between two queries of the copy's event
SLOTS = 2


def scale_one_prediction(outputs):
    """the raw [B, 4, H, W] output of scale 1/1 out of what the trainer has at hand: the dict `model(x)` returns, TrainStep.outputs (the
    four scales in order), or the tensor itself"""
    if isinstance(outputs, dict):
        return outputs["1/1"]
    if isinstance(outputs, (list, tuple)):
        return outputs[-1]
    return outputs


class PanelLogger:
    """`log(writer, inputs, outputs, losses, lr, step)` with the reference's arguments, returning as soon as the work is queued.  `queue`
    is the same machinery with the renderer and the scalar list from the caller (preprocessing/segmentation/logger.py uses it).

    panels: the renderer, `panels(inputs, pred, depth_range, n=..., out=...) -> (uint8 tensor [n, P, H, W, 3], tags)`; ops.log_panels by
    default.  A renderer that returns a host tensor (the tests' stand-in) needs no copy and no event."""

    def __init__(self, depth_range=(0.1, 100.0), panels=None, n=4):
        if panels is None:
            from .. import ops
            panels = ops.log_panels
        self.panels, self.depth_range, self.n = panels, tuple(depth_range), n
        self._free, self._jobs = queue.Queue(), queue.Queue()
        for _ in range(SLOTS):
            self._free.put({"device": None, "host": None, "event": None})
        self._error = None
        self._thread = None
        self.events = 0                         # log events handed to the writer thread
        self.writer_seconds = []                # per event: the writer thread's encode + write time (after the copy has arrived)

    # ---- training thread ----------------------------------------------------------------------------------------------------------------
    def log(self, writer, inputs, outputs, losses, lr, step):
        """the footprint trainer's event: `lr`, `loss`, and the twelve pictures of each logged sample"""
        def render(device_out):
            pred = scale_one_prediction(outputs)
            if not pred.is_contiguous():
                pred = pred.contiguous()
            batch = {k: (v if v is None or v.is_contiguous() else v.contiguous()) for k, v in inputs.items()}
            B, _, H, W = pred.shape
            P = 12 if batch.get("moving_object_mask") is not None else 11
            out = device_out(pred.device, (min(self.n, B), P, H, W, 3))
            return self.panels(batch, pred, self.depth_range, n=self.n, out=out)
        self.queue(writer, render, lambda: [("lr", float(lr)), ("loss", float(losses["loss"]))], step)

    def queue(self, writer, render, scalars, step):
        """one log event of any trainer.  render(device_out) -> (uint8 tensor whose last three dimensions are one picture [h, w, 3], one
        tag per picture), where device_out(device, shape) is the slot's device buffer if it has that device and shape, else None (the
        renderer then allocates, and its result becomes the slot's buffer); scalars() -> [(tag, value), ...], written before the
        pictures.  Both run here, on the training thread; whatever they raise is raised by the next call or by close()."""
        self._raise_pending()
        if self._thread is None:
            self._thread = threading.Thread(target=self._run, name="footprints-summary-writer", daemon=True)
            self._thread.start()
        slot = self._take_slot()
        try:
            wall = time.time()

            def device_out(device, shape):
                out = slot["device"]
                return out if out is not None and out.device == device and tuple(out.shape) == tuple(shape) else None
            panels, tags = render(device_out)
            if panels.is_cuda:
                slot["device"] = panels
                nbytes = panels.numel()
                if slot["host"] is None or slot["host"].numel() < nbytes:
                    slot["host"] = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
                if slot["event"] is None:
                    slot["event"] = torch.cuda.Event()
                slot["host"][:nbytes].copy_(panels.view(-1), non_blocking=True)      # on the current stream, behind the two launches
                slot["event"].record(torch.cuda.current_stream(panels.device))
                pixels, event = slot["host"][:nbytes].numpy().reshape(tuple(panels.shape)), slot["event"]
            else:
                pixels, event = panels.numpy(), None
            scalars = list(scalars())
        except Exception as exc:                 # like a failure of the writer thread: raised by the next log or by close
            self._free.put(slot)
            if self._error is None:
                self._error = exc
            return
        self.events += 1
        self._jobs.put((slot, writer, pixels, event, list(tags), scalars, int(step), wall))

    def _take_slot(self):
        while True:
            try:
                return self._free.get(timeout=0.05)
            except queue.Empty:
                self._raise_pending()
                if not self._thread.is_alive():
                    raise RuntimeError("the summary writer thread has ended with log events outstanding")

    def _raise_pending(self):
        if self._error is not None:
            err, self._error = self._error, None
            raise err

    def drain(self):
        """wait until every queued log event is in its file (or has failed)"""
        self._jobs.join()
        self._raise_pending()

    def close(self):
        """finish the queued events, end the writer thread, and raise what it raised"""
        if self._thread is not None:
            self._jobs.put(None)
            self._thread.join()
            self._thread = None
        self._raise_pending()

    # ---- writer thread ------------------------------------------------------------------------------------------------------------------
    def _run(self):
        while True:
            job = self._jobs.get()
            if job is None:
                self._jobs.task_done()
                return
            slot, writer, pixels, event, tags, scalars, step, wall = job
            try:
                if self._error is None:              # after a failure the remaining events are let go: the error is what gets reported
                    if event is not None:
                        while not event.query():
                            time.sleep(SPIN)
                    t0 = time.time()
                    for tag, value in scalars:
                        writer.add_scalar(tag, value, step, walltime=wall)
                    flat = pixels.reshape((-1,) + pixels.shape[-3:])
                    if len(tags) != flat.shape[0]:
                        raise RuntimeError("log: %d tags for %d pictures" % (len(tags), flat.shape[0]))
                    for tag, picture in zip(tags, flat):
                        writer.add_image(tag, picture, step, walltime=wall)
                    writer.flush()
                    self.writer_seconds.append(time.time() - t0)
            except BaseException as exc:             # kept for the training thread
                if self._error is None:
                    self._error = exc
            finally:
                self._free.put(slot)
                self._jobs.task_done()


def log(writer, inputs, outputs, losses, lr, step, logger=None, depth_range=(0.1, 100.0)):
    """the reference's call.  With a `PanelLogger` it returns once the work is queued; without one it writes the event before it returns."""
    if logger is not None:
        return logger.log(writer, inputs, outputs, losses, lr, step)
    once = PanelLogger(depth_range)
    try:
        once.log(writer, inputs, outputs, losses, lr, step)
    finally:
        once.close()


class TimeLogger:
    """training/logger.py:70-92: seconds spent training, validating and logging since the last printed line"""

    def __init__(self, log=print):
        self.log = log
        self._reset()

    def _reset(self):
        self.train_network_time = 0
        self.val_time = 0
        self.log_time = 0

    def add_time(self, timer, time):
        setattr(self, timer, getattr(self, timer) + time)

    def print_time(self):
        self.log("{:.2f}s/{:.2f}s/{:.2f}s -- train/val/log".format(self.train_network_time, self.val_time, self.log_time))
        self._reset()
