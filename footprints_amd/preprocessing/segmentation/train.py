"""Trainer of the ground-segmentation network on device-assembled batches (reference: footprints/preprocessing/segmentation/train.py).

Per step: forward, the four bilinear up-sizes + per-sample masked BCE / 4 (one kernel, losses.py), backward, Adam at `lr`.  StepLR(10) is
stepped at the START of every epoch, as the reference does.  Every `log_freq` steps the tracked losses are printed after `val_batches`
validation batches from a cycling iterator; with `summaries=True` the train batch and the last validation batch are also logged to
`<log_path>/<model_name>/{train,val}` event files at the reference's points (train.py:132, 167), rendered on the device and written by a
thread of their own (logger.py).  `epoch_{n}.pth` holds the model's state_dict alone.
Single process: data parallelism is not part of this trainer."""
import os
import random

import torch

from ...optim import FusedAdam
from .evaluation import Evaluator
from .network import Segmentor


class Trainer:
    def __init__(self, options, model=None, train_loader=None, val_loader=None, summaries=False, panels=None):
        """model / train_loader / val_loader: injected objects (tests, benchmarks); by default the Segmentor of the options and
        DeviceLoaders over the file readers named in the config file.  summaries: write the TensorBoard files (train.py:58-62);
        panels: the renderer handed to logger.SegPanelLogger (ops.seg_log_panels by default)"""
        print("setting up...")
        self.opt = options
        if not torch.cuda.is_available():
            raise RuntimeError("the segmentation trainer has no CPU compute path: it needs a MI355X")
        if model is None:
            model = Segmentor(pretrained=True, use_PSP=not self.opt.no_PSP)
            if self.opt.load_path is not None:
                print("loading weights from {}...".format(self.opt.load_path))
                model.load_state_dict(torch.load(self.opt.load_path, map_location="cpu"))
            model.cuda()
        self.model = model
        self.evaluator = Evaluator()
        self.optimiser = FusedAdam(self.model, lr=self.opt.lr)
        self.scheduler = torch.optim.lr_scheduler.StepLR(self.optimiser, step_size=10)
        print("models done!")
        if train_loader is None or val_loader is None:
            made = self.create_dataloaders()
            train_loader, val_loader = train_loader or made[0], val_loader or made[1]
        self.train_loader, self.val_loader = train_loader, val_loader
        self.val_iter = iter(self.val_loader)
        print("datasets done!")
        print("training images: {}".format(len(self.train_loader.dataset)))
        print("validation images: {}".format(len(self.val_loader.dataset)))
        self.step, self.epoch, self.lr = 0, 0, self.opt.lr
        self.history = []                    # one entry per logged step: dict(epoch, step, lr, batch_loss, train, val)
        self.writers, self.logger = {}, None
        if summaries:
            from ...training.summary import SummaryWriter
            from .logger import SegPanelLogger
            for mode in ("train", "val"):
                self.writers[mode] = SummaryWriter(os.path.join(self.opt.log_path, self.opt.model_name, mode))
            self.logger = SegPanelLogger(panels=panels)

    def create_dataloaders(self):
        """train.py:64-101 with the file readers of datasets/ and the device path: ConcatDataset of the chosen datasets, shuffled, so
        one batch mixes datasets.  max_src_hw is Cityscapes' cropped frame, the largest of the three.  The samples of upcoming batches
        are read on --num_workers threads (train; min(2, num_workers) for validation, as the Footprints trainer's loaders): the shuffle,
        the batch boundaries and the `random` stream are BatchSource's; num_workers <= 0 keeps the plain BatchSource, which reads a batch's
        files one after the other on the staging thread.  --device_decode: the readers hand over files and the assemblers decode baseline
        JPEGs on the device (datasets/device_path.SegBatchAssembler)."""
        import yaml
        from ...datasets.device_path import SegBatchAssembler
        from ...datasets.training import ThreadedBatchSource
        from .datasets import READERS, BatchSource
        with open(self.opt.config_path) as fh:
            config = yaml.safe_load(fh)
        device_decode = bool(getattr(self.opt, "device_decode", False))
        num_workers = int(getattr(self.opt, "num_workers", 0))
        loaders = []
        for split, is_train, workers in (("train", True, num_workers), ("val", False, min(2, num_workers))):
            readers = []
            for dataset in self.opt.training_datasets:
                with open(os.path.join("splits", dataset, split + ".txt")) as fh:
                    files = fh.read().splitlines()
                if dataset == "matterport" and is_train:
                    files = files[:5000]
                readers.append(READERS[dataset](config[dataset]["dataset"], files, device_decode=device_decode))
            if workers > 0:
                source = ThreadedBatchSource(readers, self.opt.batch_size, shuffle=True, rng=random, num_workers=workers)
            else:
                source = BatchSource(readers, self.opt.batch_size, shuffle=True)
            asm = SegBatchAssembler(self.opt.batch_size, self.opt.height, self.opt.width, max_src_hw=(1280, 2048), device_decode=device_decode)
            loader = asm.loader(source, is_train, random)
            loader.dataset = source.dataset
            loaders.append(loader)
        return loaders

    def train(self):
        print("training")
        self.step = 0
        try:
            for self.epoch in range(self.opt.epochs):
                self.run_epoch()
        finally:
            self.close_summaries()

    def close_summaries(self):
        """write what is queued, end the writer thread and close the files; raises what the writer thread raised"""
        logger, writers = self.logger, self.writers
        self.logger, self.writers = None, {}
        try:
            if logger is not None:
                logger.close()
        finally:
            for w in writers.values():
                w.close()

    def log_summaries(self, mode, inputs, outputs, losses):
        """train.py:132 / 167: queue one log event on the stream that trains (logger.py)"""
        if self.logger is not None:
            self.logger.log(self.writers[mode], inputs, outputs, losses, self.lr, self.step, num_outputs=10)

    def run_epoch(self):
        self.scheduler.step()                # at the start of the epoch (train.py:111)
        for inputs in self.train_loader:
            self.model.train()
            outputs, batch_loss = self.forward(inputs)
            self.model.zero_grad()
            batch_loss.backward()
            self.optimiser.step()
            self.lr = self.scheduler.get_last_lr()[0]
            if (self.step % self.opt.log_freq) == 0:
                tracked = self.evaluator.get_tracked_losses()
                self.log_summaries("train", inputs, outputs, tracked)
                val = self.run_validation(self.opt.val_batches)
                self.history.append(dict(epoch=self.epoch, step=self.step, lr=self.lr, batch_loss=float(batch_loss.detach()),
                                         train={k: float(v) for k, v in tracked.items()}, val={k: float(v) for k, v in val.items()}))
                print("Epoch {} -- Step {} -- lr {} -- Train Loss {} -- Val Loss {}".format(self.epoch, self.step, self.lr,
                                                                                           self.history[-1]["train"]["loss"],
                                                                                           self.history[-1]["val"]["loss"]))
            self.step += 1
        for name, loader in (("train", self.train_loader), ("val", self.val_loader)):
            if getattr(getattr(loader, "asm", None), "device_decode", False):            # --device_decode: where the frames were decoded
                c = loader.counters
                print("Epoch {} -- {} frames decoded so far: device {}, host (parser) {}, host (status) {}".format(
                    self.epoch, name, c["device"], c["host_parser"], c["host_status"]))
        self.save_model()

    def run_validation(self, batches=10):
        """`batches` batches from the cycling validation iterator, in the reference's mode: the model stays as the training loop left it
        (train.py:148-170 never calls eval()), without gradients"""
        with torch.no_grad():
            for _ in range(batches):
                try:
                    inputs = next(self.val_iter)
                except StopIteration:
                    self.val_iter = iter(self.val_loader)
                    inputs = next(self.val_iter)
                outputs, _ = self.forward(inputs)
            tracked = self.evaluator.get_tracked_losses()
            if batches > 0:
                self.log_summaries("val", inputs, outputs, tracked)
            return tracked

    def forward(self, inputs):
        outputs = self.model(inputs["image"])
        return outputs, self.evaluator.compute_losses(outputs, inputs["ground_mask"], inputs["labelled_pix"])

    def save_model(self):
        save_path = os.path.join(self.opt.log_path, self.opt.model_name, "models")
        os.makedirs(save_path, exist_ok=True)
        torch.save(self.model.state_dict(), os.path.join(save_path, "epoch_{}.pth".format(self.epoch)))
