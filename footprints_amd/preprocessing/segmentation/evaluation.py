"""The reference's Evaluator (footprints/preprocessing/segmentation/evaluation.py:13-59) over the fused loss kernel: per-image masked
BCE-with-logits of the four up-sized logit maps, their mean over the scales, the batch mean for backprop, and per-key running lists."""
from .losses import SegmentationLoss


class Evaluator:
    def __init__(self):
        self._loss = SegmentationLoss()

    def compute_losses(self, outputs, ground_mask, loss_mask):
        """outputs: the four logit maps of Segmentor.forward (the bilinear up-sizing of train.py:184-190 happens inside the kernel)
        -> the batch loss, differentiable"""
        return self._loss(outputs, ground_mask, loss_mask)

    def get_tracked_losses(self):
        """{'ground_loss_0' .. 'ground_loss_3', 'loss'} -> means since the last call; the lists start again"""
        return self._loss.tracked()
