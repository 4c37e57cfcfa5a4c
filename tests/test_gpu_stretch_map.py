"""GPU: the stretched-map pictures on the device (csrc/stretch_map.hip) -- fp_seg_log_panels against the two host restatements of
tests/seg_log_restatement.py, fp_stretch_colour byte for byte against tests/stretch_restatement.py, the JPEG files with a density against
Pillow's, the segmentation trainer with summaries=True end to end, and the label generators with --save_visualisations.

The image and ground-truth panels of the log contain only IEEE operations: byte for byte equal to the float32 restatement.  The prediction
panel goes through the device's own exponential, so it gets the band of tests/test_gpu_log_panels.py: a colour-table index is accepted if
it is floor(v64) or floor(v64 +- delta), v64 the float64 restatement's value before truncation and delta = 4 x the largest |v32 - v64| the
CPU float32 restatement itself shows on the case's prediction panels; and per panel at most 1 % of the pixels may differ from the CPU
float32 index, none by more than 1 (the host confirms float32 against float64 under that cap in tests/test_stretch_map_cpu.py)."""
import io
import os
import random
import threading

import numpy as np
import pytest
import torch

from tests import event_file_reader as ER
from tests import seg_log_restatement as SR
from tests import stretch_restatement as ST

pytestmark = pytest.mark.gpu

# a workgroup takes 1024 pixels (256 threads x 4): 3 x 700 = 2100 is two full workgroups and a ragged third on the 16-byte path,
# 33 x 63 = 2079 the same on the scalar path (H * W odd)
SEG_CASES = {
    "b2_5x7": dict(B=2, H=5, W=7, seed=21),
    "b4_32x64": dict(B=4, H=32, W=64, seed=22),
    "blocks_wide": dict(B=1, H=3, W=700, seed=23),
    "blocks_scalar": dict(B=1, H=33, W=63, seed=24),
    "b12_8x12": dict(B=12, H=8, W=12, seed=25),
    "constant": dict(B=2, H=8, W=12, seed=26, constant=True),
}
BLOCK_SHAPES = ((5, 7), (32, 64), (3, 700), (33, 63))
_cache = {}


def _reference(case):
    """computed once per case and left unchanged: inputs, logits, float32 and float64 parts, float32 bytes"""
    if case not in _cache:
        inputs, logits = SR.make_inputs(**SEG_CASES[case])
        p32 = SR.float_parts(inputs, logits)
        p64 = SR.float_parts(inputs, logits, dtype=np.float64)
        _cache[case] = (inputs, logits, p32, p64, SR.to_bytes(p32))
    return _cache[case]


def _clip(v):
    return np.clip(np.floor(v), 0, 255).astype(np.int64)


@pytest.mark.parametrize("case", list(SEG_CASES))
def test_seg_log_panels_match_the_restatements(case):
    from footprints_amd import ops
    inputs, logits, p32, p64, bytes32 = _reference(case)
    B, _, H, W = inputs["image"].shape
    n = min(10, B)
    dev_in = {k: torch.from_numpy(v).cuda() for k, v in inputs.items()}
    head = torch.full((B, 2, H, W), 7.0, device="cuda")                  # the engine's head buffer: channel 0 holds the logits
    head[:, 0:1] = torch.from_numpy(logits).cuda()
    out, tags = ops.seg_log_panels(dev_in, head[:, 0:1])
    dense, _ = ops.seg_log_panels(dev_in, torch.from_numpy(logits).cuda(), n=10)
    again, _ = ops.seg_log_panels(dev_in, head[:, 0:1], n=10, out=torch.empty_like(out))
    torch.cuda.synchronize()
    assert tuple(out.shape) == (n, H, 3 * W, 3) and out.dtype == torch.uint8 and tags == SR.tags(n)
    assert torch.equal(out, dense) and torch.equal(out, again)
    got = out.cpu().numpy()
    assert np.array_equal(got[:, :, :2 * W], bytes32[:, :, :2 * W]), (case, int((got[:, :, :2 * W] != bytes32[:, :, :2 * W]).sum()))
    table = SR.byte_table()
    index_of = {tuple(int(c) for c in rgb): i for i, rgb in enumerate(table)}
    assert len(index_of) == 256                                          # the colour table is one to one: a colour names its index
    delta = 4.0 * max(float(np.abs(SR.index_scaled(a).astype(np.float64) - SR.index_scaled(b)).max()) for (_, _, a), (_, _, b) in zip(p32, p64))
    needed_band = 0
    for i in range(n):
        values = np.array([index_of[tuple(int(c) for c in px)] for px in got[i, :, 2 * W:].reshape(-1, 3)]).reshape(H, W)
        want32 = np.minimum(SR.index_scaled(p32[i][2]).astype(np.int64), 255)
        v64 = SR.index_scaled(p64[i][2])
        exact = values == _clip(v64)
        ok = exact | (values == _clip(v64 + delta)) | (values == _clip(v64 - delta))
        diff = np.abs(values - want32)
        needed_band += int((~exact).sum())
        print("%s Image/%d: delta %.3e, outside floor(v64) %d of %d, differing from the float32 index %d (max %d)"
              % (case, i, delta, int((~exact).sum()), values.size, int((diff > 0).sum()), int(diff.max())))
        assert ok.all(), (case, i, int((~ok).sum()), delta)
        assert diff.max() <= 1 and (diff > 0).mean() <= 0.01, (case, i, int(diff.max()), float((diff > 0).mean()))
        image = got[i, :, :W]
        if case == "constant" and i == 0:
            assert (image == 0).all()                                    # denom = 1e5
        else:
            assert image.min() == 0 and image.max() == 255               # the map saw the bits the reduction saw
        assert set(np.unique(got[i, :, W:2 * W, 0])) <= {0, 255} and (got[i, :, W:2 * W, 1:] == 0).all()
    print("%s: delta %.3e, %d prediction pixels needed the band" % (case, delta, needed_band))


def test_seg_log_panels_refuses_bad_arguments():
    from footprints_amd import ops
    inputs, logits = SR.make_inputs(2, 5, 7, seed=3)
    dev = {k: torch.from_numpy(v).cuda() for k, v in inputs.items()}
    with pytest.raises(RuntimeError, match="out must be"):
        ops.seg_log_panels(dev, torch.from_numpy(logits).cuda(), out=torch.empty(5, dtype=torch.uint8, device="cuda"))
    with pytest.raises(RuntimeError, match="dense planes"):
        ops.seg_log_panels(dev, torch.zeros(2, 1, 5, 14, device="cuda")[:, :, :, ::2])
    with pytest.raises(RuntimeError, match="float32 \\[B, 1, H, W\\]"):
        ops.seg_log_panels(dev, torch.zeros(2, 1, 5, 8, device="cuda"))


# ---- imsave ---------------------------------------------------------------------------------------------------------------------------------
def _stretch_maps():
    maps = dict(ST.cases())
    rng = np.random.default_rng(77)
    for h, w in BLOCK_SHAPES:
        maps["float_%dx%d" % (h, w)] = ((rng.random((h, w)) * 50.0 - 5.0) * (rng.random((h, w)) < 0.7)).astype(np.float32)
        maps["bytes_%dx%d" % (h, w)] = rng.integers(3, 200, (h, w)).astype(np.uint8)
        maps["mask_%dx%d" % (h, w)] = rng.random((h, w)) < 0.5
    return maps


@pytest.mark.parametrize("name", list(_stretch_maps()))
def test_stretch_colour_equals_the_restatement(name):
    from footprints_amd import ops
    x = _stretch_maps()[name]
    want = ST.rgb(x)
    got = ops.stretch_colour(torch.from_numpy(x).cuda())
    again = ops.stretch_colour(torch.from_numpy(x).cuda().unsqueeze(0))
    torch.cuda.synchronize()
    assert tuple(got.shape) == x.shape + (3,) and got.dtype == torch.uint8 and torch.equal(got, again[0])
    assert np.array_equal(got.cpu().numpy(), want), (name, int((got.cpu().numpy() != want).sum()))
    if x.dtype == np.bool_:                                              # booleans go up as bytes: the same picture from uint8
        assert torch.equal(ops.stretch_colour(torch.from_numpy(x.astype(np.uint8)).cuda()), got)


@pytest.mark.parametrize("dtype", [np.float32, np.uint8])
def test_stretch_colour_batch_equals_single_calls(dtype):
    from footprints_amd import ops
    rng = np.random.default_rng(78)
    maps = (rng.random((3, 33, 63)) * np.array([1.0, 200.0, 17.0])[:, None, None]).astype(dtype)
    maps[2] = 5                                                          # each map has its own range; one is constant
    batch = ops.stretch_colour(torch.from_numpy(maps).cuda())
    singles = torch.stack([ops.stretch_colour(torch.from_numpy(m).cuda()) for m in maps])
    torch.cuda.synchronize()
    assert torch.equal(batch, singles)
    assert np.array_equal(batch.cpu().numpy(), np.stack([ST.rgb(m) for m in maps]))
    with pytest.raises(RuntimeError, match="float32, uint8 or bool"):
        ops.stretch_colour(torch.zeros(4, 4, dtype=torch.float64, device="cuda"))


# ---- JPEG files with a density --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(192, 640), (5, 7)])
def test_jpeg_encode_with_a_density_equals_pillows_file(hw):
    from footprints_amd import ops
    from tests.test_gpu_jpeg import recorded_tables_are_installed
    assert recorded_tables_are_installed(75)                             # the installed Pillow writes the standard tables, as recorded
    rng = np.random.default_rng(hw[0])
    x = (rng.random(hw) * 30.0).astype(np.float32) * (rng.random(hw) < 0.6)
    picture = ops.stretch_colour(torch.from_numpy(x.astype(np.float32)).cuda())
    files = ops.jpeg_encode(picture.unsqueeze(0), quality=75, dpi=(100, 100))
    assert len(files) == 1 and files[0] == ST.pillow_file(ST.rgb(x.astype(np.float32)))
    plain = ops.jpeg_encode(picture.unsqueeze(0), quality=75)
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(picture.cpu().numpy()).save(buf, format="JPEG")
    assert plain[0] == buf.getvalue() and plain[0] != files[0]


# ---- the segmentation trainer ---------------------------------------------------------------------------------------------------------------
def test_seg_log_returns_before_the_writer_has_encoded(tmp_path):
    """the training thread waits for nothing: with the PNG encoder held back until `log()` has returned, the writer thread's flag is
    still unset when it does; afterwards the file holds the device's bytes"""
    from footprints_amd import ops
    from footprints_amd.preprocessing.segmentation.logger import SegPanelLogger
    from footprints_amd.training.summary import SummaryWriter, encode_png
    gate, encoded = threading.Event(), threading.Event()

    def held_back(rgb):
        assert gate.wait(timeout=120)
        encoded.set()
        return encode_png(rgb)
    inputs, logits = SR.make_inputs(**SEG_CASES["b4_32x64"])
    dev_in, dev_logits = {k: torch.from_numpy(v).cuda() for k, v in inputs.items()}, torch.from_numpy(logits).cuda()
    writer = SummaryWriter(str(tmp_path), encode_png=held_back)
    logger = SegPanelLogger()
    logger.log(writer, dev_in, [None, None, None, dev_logits], {"loss": torch.tensor(0.5, device="cuda")}, 1e-4, 3)
    assert not encoded.is_set()
    gate.set()
    logger.close()
    writer.close()
    assert encoded.is_set()
    want, tags = ops.seg_log_panels(dev_in, dev_logits)
    _, got = ER.read_log(writer.path)
    assert [(s, t) for s, t, _ in got] == [(3, "loss"), (3, "learning rate")] + [(3, t) for t in tags]
    for (_, tag, pic), w in zip(got[2:], want.cpu().numpy()):
        assert np.array_equal(pic, w), tag


def test_seg_trainer_logs_end_to_end_and_training_is_undisturbed(tmp_path):
    """B = 2 at 64 x 96, one epoch of three steps at log_freq 2: log events at steps 0 and 2.  Both files parse; tags, scalar names and
    picture sizes are the reference's; the image and ground-truth panels are the restatement of the batches that were logged; the weights
    after the run are bit-equal to a run without summaries"""
    from footprints_amd.datasets.device_path import SegBatchAssembler, SyntheticSegSource
    from footprints_amd.preprocessing.segmentation.network import Segmentor
    from footprints_amd.preprocessing.segmentation.options import SegmentationOptions
    from footprints_amd.preprocessing.segmentation.train import Trainer
    from oracle import restatement as R
    B, H, W = 2, 64, 96
    frames = [("cityscapes", (800, 200)), ("ADE20K", (70, 110)), ("matterport", (128, 160)), ("ADE20K", (50, 90))]
    P, Bf = R.make_seg_state(True, tag="segtrain")
    keys = ["ground_loss_0", "ground_loss_1", "ground_loss_2", "ground_loss_3", "loss"]

    class Kept:
        """a loader that keeps a host copy of every batch it hands out"""

        def __init__(self, loader):
            self.loader, self.batches = loader, []
            self.dataset = loader.source.dataset

        def __len__(self):
            return len(self.loader)

        def __iter__(self):
            for batch in self.loader:
                self.batches.append({k: v.cpu().numpy().copy() for k, v in batch.items()})
                yield batch

    def run(summaries, folder):
        opts = SegmentationOptions().parse(["--height", str(H), "--width", str(W), "--batch_size", str(B), "--log_freq", "2", "--epochs", "1",
                                            "--val_batches", "2", "--log_path", str(folder), "--model_name", "seg"])
        model = Segmentor(pretrained=False, use_PSP=True)
        model.load_state_dict({**P, **Bf})
        model.cuda()
        train = Kept(SegBatchAssembler(B, H, W, max_src_hw=(800, 200)).loader(SyntheticSegSource(B, 3, frames, seed=1), True, random.Random(1)))
        val = Kept(SegBatchAssembler(B, H, W, max_src_hw=(800, 200)).loader(SyntheticSegSource(B, 3, frames, seed=2), False, random.Random(2)))
        trainer = Trainer(opts, model=model, train_loader=train, val_loader=val, summaries=summaries)
        trainer.train()
        torch.cuda.synchronize()
        assert trainer.logger is None and trainer.writers == {}
        return trainer, train, val, {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}

    t1, train, val, state1 = run(True, tmp_path / "on")
    t0, _, _, state0 = run(False, tmp_path / "off")
    assert sorted(os.listdir(tmp_path / "off" / "seg")) == ["models"]
    assert list(state1) == list(state0) and all(torch.equal(state1[k], state0[k]) for k in state1)
    assert t1.history == t0.history and [h["step"] for h in t1.history] == [0, 2]
    # validation cycles over three batches, two per event: the last of each event is logged
    logged = {"train": [(0, train.batches[0]), (2, train.batches[2])], "val": [(0, val.batches[1]), (2, val.batches[3])]}
    assert len(val.batches) == 4
    per = len(keys) + 1 + B
    for mode in ("train", "val"):
        files = os.listdir(tmp_path / "on" / "seg" / mode)
        assert len(files) == 1 and files[0].startswith("events.out.tfevents.")
        version, got = ER.read_log(str(tmp_path / "on" / "seg" / mode / files[0]))
        assert version == "brain.Event:2" and len(got) == 2 * per
        for e, (step, batch) in enumerate(logged[mode]):
            ev = got[e * per:(e + 1) * per]
            assert all(s == step for s, _, _ in ev) and [t for _, t, _ in ev] == keys + ["learning rate"] + SR.tags(B)
            assert [v for _, _, v in ev[:5]] == [np.float32(t1.history[e][mode][k]) for k in keys] and ev[5][2] == np.float32(1e-4)
            want = SR.to_bytes(SR.float_parts(batch, np.zeros((B, 1, H, W), np.float32)))
            for (_, tag, pic), w in zip(ev[6:], want):
                assert pic.shape == (H, 3 * W, 3)
                assert np.array_equal(pic[:, :2 * W], w[:, :2 * W]), (mode, step, tag)      # (the prediction panel is the kernel test's)
                assert len(np.unique(pic[:, 2 * W:].reshape(-1, 3), axis=0)) > 1


# ---- the label generators -------------------------------------------------------------------------------------------------------------------
def _saved(folder):
    out = {}
    for root, _, files in os.walk(folder):
        for f in files:
            with open(os.path.join(root, f), "rb") as fh:
                out[os.path.relpath(os.path.join(root, f), folder)] = fh.read()
    return out


def _three_runs(tmp_path, cls, data_type, lines):
    """the generator over the textfile without pictures, with them, and with them encoded on the device -> the three folders' files"""
    from footprints_amd.preprocessing.ground_truth_generation import get_options
    (tmp_path / "files.txt").write_text("\n".join(lines) + "\n")
    argv = ["--config_path", str(tmp_path / "paths.yaml"), "--textfile", str(tmp_path / "files.txt"), "--data_type", data_type]
    out = []
    for name, extra in (("plain", []), ("viz", ["--save_visualisations"]), ("viz_dev", ["--save_visualisations", "--device_jpeg"])):
        np.random.seed(123)
        gen = cls.from_options(get_options(argv + ["--save_folder_name", "out_" + name] + extra))
        gen.run()
        torch.cuda.synchronize()
        out.append(_saved(os.path.join(gen.training_datapath, "out_" + name)))
    return out


def _check_pictures(plain, viz, viz_dev, count):
    assert len(plain) == count and all(k.endswith(".npy") for k in plain)
    arrays = {k: v for k, v in viz.items() if k.endswith(".npy")}
    assert arrays == plain and {k: v for k, v in viz_dev.items() if k.endswith(".npy")} == plain      # byte-equal with and without the flag
    pictures = {k: v for k, v in viz.items() if k.endswith(".jpg")}
    assert len(pictures) == count and len(viz) == 2 * count and set(viz_dev) == set(viz)
    seen = set()
    for name, data in pictures.items():
        folder, base = os.path.split(name)
        assert os.path.basename(folder) == "visualisations" and len(base) >= len("0000000000.jpg")
        npy = os.path.join(os.path.dirname(folder), "data", base[:-4] + ".npy")
        result = np.load(io.BytesIO(plain[npy]))
        assert data == ST.pillow_file(ST.rgb(result)), name
        assert viz_dev[name] == data, name
        seen.add(result.dtype)
    return seen


def test_kitti_hidden_depths_with_visualisations(tmp_path):
    from footprints_amd.preprocessing.ground_truth_generation import ground_truth_generator as G
    from tests.test_gt_frames_cpu import SEQ, write_kitti_gt_tree

    class Small(G.generator_class("kitti", "hidden_depths")):
        height, width = 12, 40
    t = write_kitti_gt_tree(tmp_path, SEQ, range(8), native=(24, 80), seed=24)
    (tmp_path / "paths.yaml").write_text("kitti:\n  dataset: %s\n  training_data: %s\n" % (tmp_path / "raw", t))
    runs = _three_runs(tmp_path, Small, "kitti", ["%s 3 l" % SEQ, "%s 4 r" % SEQ, "%s 5 l" % SEQ])
    assert _check_pictures(*runs, count=3) == {np.dtype(np.float32)}


def test_matterport_depth_masks_with_visualisations(tmp_path):
    from footprints_amd.preprocessing.ground_truth_generation import ground_truth_generator as G
    from tests.test_gt_frames_cpu import write_matterport_gt_tree

    class Small(G.generator_class("matterport", "depth_masks")):
        height, width = 12, 40
    names = [("aa11", "0", "3"), ("aa11", "1", "0"), ("bb22", "0", "1"), ("bb22", "2", "5"), ("cc33", "1", "2")]
    raw, t = write_matterport_gt_tree(tmp_path, "scanA", names, native=(24, 80), depth_native=(30, 100), seed=7)
    (tmp_path / "paths.yaml").write_text("matterport:\n  dataset: %s\n  training_data: %s\n" % (raw, t))
    runs = _three_runs(tmp_path, Small, "matterport", ["scanA %s %s %s" % n for n in (names[0], names[2], names[4])])
    assert np.dtype(np.bool_) in _check_pictures(*runs, count=3)
