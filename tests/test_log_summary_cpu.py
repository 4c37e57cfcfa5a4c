"""CPU: the trainer's TensorBoard logging without a device -- the panel rules against the reference's own `log` (tests/golden/g21_log.npz),
the event file against an independent reader (tests/event_file_reader.py), CRC-32C in the library and in Python, and TrainManager's loop
with stand-ins for the step, the model and the renderer (there is no CPU compute path in the product)."""
import ctypes as C
import os
import threading

import numpy as np
import pytest
import torch

from tests import event_file_reader as ER
from tests import log_panels_restatement as LR
from tests.test_train_manager_dp_cpu import _FakeModelManager

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g21_log.npz")
DEPTH_RANGE = (0.1, 100)


def _golden_case(g, name):
    inputs = {k[len(name) + 4:]: torch.from_numpy(g[k]) for k in g.files if k.startswith(name + ".in.") and not k.endswith(".pred")}
    return inputs, torch.from_numpy(g[name + ".in.pred"])


@pytest.mark.parametrize("name", ["plain", "constant"])
def test_float32_restatement_reproduces_the_reference_log(name):
    """tags in order; every grey panel and the image bit for bit before the byte rule; the colour-mapped disparity, which the reference hands
    over as matplotlib's float64 colours, as bytes"""
    g = np.load(GOLDEN)
    inputs, pred = _golden_case(g, name)
    panels = LR.float_panels(inputs, pred, DEPTH_RANGE)
    assert [t for t, _ in panels] == list(g[name + ".tags"]) == LR.tags(4) and len(panels) == 48
    assert list(g[name + ".scalar_tags"]) == ["lr", "loss"]
    by = LR.to_bytes(panels)
    for i, (tag, x) in enumerate(panels):
        a = g["%s.img.%03d" % (name, i)]
        if tag.startswith("pred_disp_1/"):
            assert a.shape == (3,) + tuple(x.shape)
            assert np.array_equal((a.astype(np.float32) * np.float32(255)).astype(np.uint8).transpose(1, 2, 0), by[i]), tag
        else:
            assert a.dtype == np.float32 and a.shape == tuple(x.shape), tag
            assert np.array_equal(a.view(np.uint32), x.numpy().view(np.uint32)), tag
    if name == "constant":      # denom = 1e5: all zeros
        for tag, x in panels:
            if tag.startswith(("depth_mask/", "pred_ground_visible_1/")):
                assert float(x.abs().max()) == 0.0, tag


def test_float32_and_float64_restatements_stay_under_the_device_cap():
    """the cap of the device test, confirmed on the host for its inputs: per panel, float32 against float64 bytes differ on at most 1 % of
    the pixels and never by more than 1"""
    from tests.test_gpu_log_panels import CASES, case_inputs
    for case in CASES:
        inputs, pred = case_inputs(case)
        p32 = LR.float_panels(inputs, pred, DEPTH_RANGE, n=4)
        p64 = LR.float_panels(inputs, pred, DEPTH_RANGE, n=4, dtype=torch.float64)
        for (tag, a), (_, b) in zip(p32, p64):
            va = np.minimum(np.floor(LR.scaled(tag, a).numpy().astype(np.float64)), 255)
            vb = np.minimum(np.floor(LR.scaled(tag, b).numpy()), 255)
            d = np.abs(va - vb)
            assert d.max() <= 1 and (d > 0).mean() <= 0.01, (case, tag, d.max(), (d > 0).mean())


# ---- CRC-32C ------------------------------------------------------------------------------------------------------------------------------------
_VECTORS = ((b"123456789", 0xE3069283), (bytes(32), 0x8A9136AA), (b"\xff" * 32, 0x62A8AB43))


def test_crc32c_known_values_and_agreement():
    from footprints_amd import _lib
    from footprints_amd.training import summary
    native = _lib.load().fp_crc32c
    for data, want in _VECTORS:
        assert native(0, data, len(data)) == want
        assert summary.crc32c_python(data) == want
        assert summary.crc32c(data) == want
        assert ER.crc32c_bitwise(data) == want and ER.crc32c_table(data) == want
    rng = np.random.default_rng(5)
    for size in (0, 1, 7, 8, 9, 4097):
        data = rng.integers(0, 256, size, dtype=np.uint8).tobytes()
        whole = native(0, data, len(data))
        assert whole == summary.crc32c_python(data) == ER.crc32c_bitwise(data)
        for cut in sorted({0, size // 3, size // 2, size}):
            a, b = data[:cut], data[cut:]
            assert native(native(0, a, len(a)), b, len(b)) == whole
            assert summary.crc32c_python(b, summary.crc32c_python(a)) == whole
            assert summary.crc32c(b, summary.crc32c(a)) == whole
    # an unaligned start: the native loop reads eight bytes at a time from wherever it is pointed
    buf = C.create_string_buffer(data, len(data))
    assert native(0, C.addressof(buf) + 3, len(data) - 3) == summary.crc32c_python(data[3:])


def test_crc32c_fallback_without_the_library(monkeypatch):
    from footprints_amd.training import summary
    monkeypatch.setattr(summary, "_native", [None])
    for data, want in _VECTORS:
        assert summary.crc32c(data) == want
    assert summary.masked_crc(b"123456789") == ER.masked(0xE3069283)


# ---- the event file -----------------------------------------------------------------------------------------------------------------------------
def test_event_file_round_trips_through_an_independent_reader(tmp_path):
    from footprints_amd.training.summary import SummaryWriter
    rng = np.random.default_rng(9)
    pics = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in ((5, 7), (1, 1), (16, 24))]
    w = SummaryWriter(str(tmp_path / "run" / "train"))
    assert os.path.basename(w.path).startswith("events.out.tfevents.") and w.path.endswith(__import__("socket").gethostname())
    assert os.path.basename(w.path).split(".")[3].isdigit()
    w.add_scalar("lr", 1e-4, 0)
    w.add_scalar("loss", 5.25, 0)
    w.add_image("image/0", pics[0], 0)
    w.add_image("target_disp/0", pics[1], 250)
    w.add_scalar("loss", -0.0, (1 << 40) + 3)
    w.add_image("pred_disp_1/3", pics[2], 300)
    w.flush()
    version, got = ER.read_log(w.path, crc=ER.crc32c_bitwise)
    w.close()
    assert version == "brain.Event:2"
    assert [(s, t) for s, t, _ in got] == [(0, "lr"), (0, "loss"), (0, "image/0"), (250, "target_disp/0"), ((1 << 40) + 3, "loss"),
                                           (300, "pred_disp_1/3")]
    assert got[0][2] == np.float32(1e-4) and got[1][2] == 5.25 and got[4][2] == 0.0
    for (_, _, pic), want in zip([got[2], got[3], got[5]], pics):
        assert pic.dtype == np.uint8 and np.array_equal(pic, want)
    with pytest.raises(ValueError):
        w.add_scalar("lr", 0.0, 1)                   # closed
    with pytest.raises(ValueError):
        SummaryWriter(str(tmp_path / "other")).add_image("x", np.zeros((4, 4), np.uint8), 0)
    assert sorted(os.listdir(tmp_path / "run" / "train")) == [os.path.basename(w.path)]


# ---- the trainer's loop -------------------------------------------------------------------------------------------------------------------------
B, H, W = 2, 6, 10


def _num(batch_image):
    """the number a stand-in batch carries in its first image value"""
    return int(round(float(batch_image.flatten()[0]) * 1000))


class _Scheduler:
    def get_last_lr(self):
        return [2.5e-4]

    def step(self):
        pass


class _ModelManager(_FakeModelManager):
    """the stand-in of the data-parallel CPU test, with a `model(x)` that returns the four scales"""

    def __init__(self, preds):
        super().__init__(None)
        self.scheduler = _Scheduler()
        calls = self.calls = []

        class Model(torch.nn.Module):
            def forward(self, x):
                calls.append(_num(x))
                return {k: preds[_num(x)] for k in ("1/8", "1/4", "1/2", "1/1")}
        self.model = Model()


class _Step:
    """a train step whose 21 'losses' are the batch's number and whose outputs are that batch's prediction"""

    def __init__(self, preds):
        self.preds, self.outputs = preds, None

    def __call__(self, batch):
        i = _num(batch["image"])
        self.outputs = [None, None, None, self.preds[i]]
        return torch.full((21,), float(i))


def _batches(count, first):
    """batches whose first image value names them (i / 1000), and their predictions by that number"""
    batches, preds = [], {}
    for j in range(count):
        inputs, pred = LR.make_inputs(B, H, W, seed=300 + first + j)
        inputs["image"].view(-1)[0] = (first + j) / 1000.0
        batches.append(inputs)
        preds[first + j] = pred
    return batches, preds


class _Loader(list):
    dataset = range(0)


def _manager(tmp_path, summaries, panels=LR.render, steps=101):
    from footprints_amd.training.train import TrainManager
    train, preds = _batches(3, 0)
    val, vpreds = _batches(2, 500)
    preds.update(vpreds)
    loader = _Loader(train[i % 3] for i in range(steps))
    mm = _ModelManager(preds)
    tm = TrainManager(loader, val_loader=_Loader(val), epochs=1, log=lambda *a: None, log_freq=100, val_batches=3, model_manager=mm,
                      train_step=_Step(preds), log_path=str(tmp_path), model_name="run", summaries=summaries, panels=panels)
    tm.evaluator.loss_manager = lambda predictions, targets: {k: torch.tensor(7.0) for k in __import__(
        "footprints_amd.training.losses", fromlist=["LOSS_KEYS"]).LOSS_KEYS}
    return tm, train, val, preds


def test_train_manager_writes_both_logs_at_the_reference_steps(tmp_path):
    tm, train, val, preds = _manager(tmp_path, summaries=True)
    tm.train()
    assert tm.logger is None and tm.writers == {} and tm.log_time > 0.0
    assert [s for s, _ in tm.history["train"]] == [s for s, _ in tm.history["val"]] == [0, 100]
    P = 12
    # the train batches at steps 0 and 100 are batches 0 and 100 % 3 = 1; validation cycles 500, 501, 500 | 501, 500, 501: the last ones
    logged = {"train": [(0, train[0], preds[0]), (100, train[1], preds[1])], "val": [(0, val[0], preds[500]), (100, val[1], preds[501])]}
    for mode in ("train", "val"):
        folder = tmp_path / "run" / mode
        files = os.listdir(folder)
        assert len(files) == 1 and files[0].startswith("events.out.tfevents.")
        version, got = ER.read_log(str(folder / files[0]))
        assert version == "brain.Event:2" and len(got) == 2 * (2 + B * P)
        for e, (step, inputs, pred) in enumerate(logged[mode]):
            ev = got[e * (2 + B * P):(e + 1) * (2 + B * P)]
            assert all(s == step for s, _, _ in ev)
            assert [t for _, t, _ in ev] == ["lr", "loss"] + LR.tags(B)
            assert ev[0][2] == np.float32(2.5e-4)
            assert ev[1][2] == np.float32(tm.history[mode][e][1]["loss"])
            want = LR.to_bytes(LR.float_panels(inputs, pred, DEPTH_RANGE))
            for (_, tag, pic), w in zip(ev[2:], want):
                assert np.array_equal(pic, w), (mode, step, tag)
            assert np.array_equal(ev[2][2], (inputs["image"][0] * 255).to(torch.uint8).permute(1, 2, 0).numpy())     # image/0
    assert os.path.isdir(tmp_path / "run" / "train") and sorted(os.listdir(tmp_path / "run")) == ["train", "val"]


def test_summaries_off_writes_nothing(tmp_path):
    tm, *_ = _manager(tmp_path, summaries=False, steps=3)
    tm.train()
    assert tm.logger is None and os.listdir(tmp_path) == []
    from footprints_amd.options import Options
    assert "no_summaries" not in vars(Options().parse([])) and Options().parse(["--no_summaries"]).no_summaries is True


def test_a_failing_renderer_surfaces(tmp_path):
    """whatever fails in logging is raised by the next log call or by close(): a renderer that raises when it is queued, and a failure
    that only the writer thread finds"""
    def broken(inputs, pred, depth_range, n=4, out=None):
        raise FloatingPointError("renderer")
    tm, *_ = _manager(tmp_path / "a", summaries=True, panels=broken, steps=3)
    tm.val_loader = None                                          # one log call in the run: nothing after it to raise the error
    tm.epoch = 0
    tm.run_epoch()
    assert tm.step == 3
    with pytest.raises(FloatingPointError):
        tm.close_summaries()
    assert tm.logger is None and tm.writers == {}
    tm, *_ = _manager(tmp_path / "c", summaries=True, panels=broken, steps=3)
    with pytest.raises(FloatingPointError):                       # with validation the val log call of the same step raises it
        tm.train()
    assert tm.logger is None

    def short_of_tags(inputs, pred, depth_range, n=4, out=None):
        panels, tags = LR.render(inputs, pred, depth_range, n=n)
        return panels, tags[:-1]                                  # found by the writer thread
    tm, *_ = _manager(tmp_path / "b", summaries=True, panels=short_of_tags, steps=3)
    tm.val_loader = None
    tm.epoch = 0
    tm.run_epoch()
    with pytest.raises(RuntimeError, match="tags for"):
        tm.close_summaries()


def test_panel_logger_does_not_wait_for_the_writer_and_drops_nothing(tmp_path):
    """with the PNG encoder held back, two log calls return with nothing encoded (two slots); a third, made once the encoder is let go, takes
    the first slot that comes free; every event reaches the file, in order"""
    from footprints_amd.training.logger import PanelLogger
    from footprints_amd.training.summary import SummaryWriter, encode_png
    gate, encoded = threading.Event(), []

    def held_back(rgb):
        assert gate.wait(timeout=60)
        encoded.append(1)
        return encode_png(rgb)
    inputs, pred = LR.make_inputs(B, H, W, seed=77)
    writer = SummaryWriter(str(tmp_path), encode_png=held_back)
    logger = PanelLogger(DEPTH_RANGE, panels=LR.render)
    logger.log(writer, inputs, pred, {"loss": 1.0}, 1e-4, 0)
    logger.log(writer, inputs, {"1/1": pred}, {"loss": 2.0}, 1e-4, 1)
    assert encoded == []                                          # both calls returned with nothing encoded
    gate.set()
    logger.log(writer, inputs, [None, None, None, pred], {"loss": 3.0}, 1e-4, 2)     # waits for a slot if the writer has not freed one yet
    logger.close()
    writer.close()
    _, got = ER.read_log(writer.path)
    assert [v for _, t, v in got if t == "loss"] == [1.0, 2.0, 3.0] and len(got) == 3 * (2 + B * 12) and logger.events == 3
