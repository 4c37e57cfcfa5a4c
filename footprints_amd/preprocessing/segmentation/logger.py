"""The segmentation trainer's TensorBoard log event -- counterpart of footprints/preprocessing/segmentation/logger.py (`log`).

The reference's `log` writes every tracked loss under its own name, then `learning rate`, then up to ten pictures `Image/<i>`: the
stretched image beside the ground-truth mask in red and the predicted probability through the plasma map.  It brings three tensors per
sample to the host and colour-maps them in numpy on the training thread.  Here the event goes through the machinery of
training/logger.py: ops.seg_log_panels renders the pictures as bytes in two launches on the training stream, the copy into a pinned slot
and an event follow on the same stream, and the writer thread encodes and writes.  The training thread only queues.

One difference in what is handed over: the reference's trainer passes `{'ground': sigmoid(logits)}`; here `prediction` is the logits
themselves -- the list `Segmentor.forward` returns, its full-resolution map, or a dict with that map under 'ground' -- and the sigmoid is
part of the kernel."""
from ...training.logger import PanelLogger


def full_resolution_logits(prediction):
    if isinstance(prediction, dict):
        return prediction["ground"]
    if isinstance(prediction, (list, tuple)):
        return prediction[-1]
    return prediction


class SegPanelLogger(PanelLogger):
    """`log(writer, inputs, prediction, losses, lr, step, num_outputs=10)`, returning as soon as the work is queued.

    panels: the renderer, `panels(inputs, logits, n=..., out=...) -> (uint8 tensor [n, H, 3 W, 3], tags)`; ops.seg_log_panels by default.
    A renderer that returns a host tensor (the tests' stand-in) needs no copy and no event."""

    def __init__(self, panels=None):
        if panels is None:
            from ... import ops
            panels = ops.seg_log_panels
        super().__init__(panels=panels)

    def log(self, writer, inputs, prediction, losses, lr, step, num_outputs=10):
        def render(device_out):
            logits = full_resolution_logits(prediction)
            B, _, H, W = inputs["image"].shape
            out = device_out(logits.device, (min(num_outputs, B), H, 3 * W, 3))
            return self.panels(inputs, logits, n=num_outputs, out=out)
        self.queue(writer, render, lambda: [(str(k), float(v)) for k, v in losses.items()] + [("learning rate", float(lr))], step)


def log(writer, inputs, prediction, losses, lr, step, num_outputs=10, logger=None):
    """the reference's call.  With a `SegPanelLogger` it returns once the work is queued; without one it writes the event before it returns."""
    if logger is not None:
        return logger.log(writer, inputs, prediction, losses, lr, step, num_outputs=num_outputs)
    once = SegPanelLogger()
    try:
        once.log(writer, inputs, prediction, losses, lr, step, num_outputs=num_outputs)
    finally:
        once.close()
