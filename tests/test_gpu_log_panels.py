"""GPU: the trainer's TensorBoard logging on the device -- fp_log_panels (csrc/log_panels.hip) against the two host restatements of
tests/log_panels_restatement.py, and TrainManager with summaries=True end to end: the event files parsed by tests/event_file_reader.py,
training bit-identical with and without logging, and `log()` returning before the writer thread has encoded anything.

The image and the six target panels contain only IEEE add, subtract, multiply and divide: byte for byte equal to the float32 restatement.
The five prediction panels go through the device's own exponential, so they get a band: a byte (or colour-table index) is accepted if it
is floor(v64) or floor(v64 +- delta), v64 the float64 restatement's value before truncation and delta = 4 x the largest |v32 - v64| the
CPU float32 restatement itself shows on the case's prediction panels; and per panel at most 1 % of the pixels may differ from the CPU
float32 byte, none by more than 1 (the host confirms float32 against float64 under that cap in tests/test_log_summary_cpu.py)."""
import os
import threading

import numpy as np
import pytest
import torch

from tests import event_file_reader as ER
from tests import log_panels_restatement as LR

pytestmark = pytest.mark.gpu

DEPTH_RANGE = (0.1, 100)
# the reduction and the map give a workgroup 1024 pixels (256 threads x 4): 3 x 700 = 2100 is two full workgroups and a ragged third on
# the 16-byte path, 33 x 63 = 2079 the same on the scalar path (H * W odd)
CASES = {
    "b4_32x64": dict(B=4, H=32, W=64, seed=11, channel_dim=True),
    "b2_5x7": dict(B=2, H=5, W=7, seed=12),
    "b5_64x96": dict(B=5, H=64, W=96, seed=13),
    "blocks_wide": dict(B=1, H=3, W=700, seed=14),
    "blocks_scalar": dict(B=1, H=33, W=63, seed=15),
    "no_moving": dict(B=2, H=8, W=12, seed=16, moving=False),
    "constant": dict(B=2, H=8, W=12, seed=17, constant=True),
}
_cache = {}


def case_inputs(case):
    return LR.make_inputs(**CASES[case])


def _reference(case):
    """computed once per case and left unchanged: inputs, float32 and float64 panels, float32 bytes"""
    if case not in _cache:
        inputs, pred = case_inputs(case)
        p32 = LR.float_panels(inputs, pred, DEPTH_RANGE)
        p64 = LR.float_panels(inputs, pred, DEPTH_RANGE, dtype=torch.float64)
        _cache[case] = (inputs, pred, p32, p64, LR.to_bytes(p32))
    return _cache[case]


def _clip(v):
    return np.clip(np.floor(v), 0, 255).astype(np.int64)


@pytest.mark.parametrize("case", list(CASES))
def test_log_panels_match_the_restatements(case):
    from footprints_amd import ops
    inputs, pred, p32, p64, bytes32 = _reference(case)
    B, _, H, W = inputs["image"].shape
    n = min(4, B)
    moving = inputs["moving_object_mask"] is not None
    dev_in = {k: (v.cuda() if v is not None else None) for k, v in inputs.items()}
    if case == "no_moving":
        del dev_in["moving_object_mask"]                      # missing and None are the same to the reference's `inputs.get`
    out, tags = ops.log_panels(dev_in, pred.cuda(), DEPTH_RANGE)
    again, _ = ops.log_panels(dev_in, pred.cuda(), DEPTH_RANGE, n=4)
    torch.cuda.synchronize()
    P = 12 if moving else 11
    assert tuple(out.shape) == (n, P, H, W, 3) and out.dtype == torch.uint8
    assert tags == [t for t, _ in p32] == LR.tags(n, moving) and len(tags) == n * P
    assert torch.equal(out, again)
    got = out.cpu().numpy().reshape(n * P, H, W, 3)
    table = LR.lut()
    index_of = {tuple(int(c) for c in rgb): i for i, rgb in enumerate(table)}
    assert len(index_of) == 256                               # the colour table is one to one: a colour names its index
    pred_panels = [(i, t) for i, t in enumerate(tags) if t.split("/")[0] in LR.PRED_PANELS]
    delta = 4.0 * max(float((LR.scaled(t, p32[i][1]).double() - LR.scaled(t, p64[i][1])).abs().max()) for i, t in pred_panels)
    needed_band = total = 0
    for i, tag in enumerate(tags):
        name = tag.split("/")[0]
        if name in LR.TARGET_PANELS:
            assert np.array_equal(got[i], bytes32[i]), (case, tag, int((got[i] != bytes32[i]).sum()))
            values = got[i][..., 0]
        else:
            if name == "pred_disp_1":
                values = np.array([index_of[tuple(int(c) for c in px)] for px in got[i].reshape(-1, 3)]).reshape(H, W)
                want32 = np.minimum((LR.scaled(tag, p32[i][1]).numpy()).astype(np.int64), 255)
            else:
                assert (got[i][..., 0] == got[i][..., 1]).all() and (got[i][..., 0] == got[i][..., 2]).all(), (case, tag)
                values = got[i][..., 0].astype(np.int64)
                want32 = bytes32[i][..., 0].astype(np.int64)
            v64 = LR.scaled(tag, p64[i][1]).numpy()
            exact = values == _clip(v64)
            ok = exact | (values == _clip(v64 + delta)) | (values == _clip(v64 - delta))
            needed_band += int((~exact).sum())
            total += values.size
            diff = np.abs(values - want32)
            print("%s %s: delta %.3e, outside floor(v64) %d of %d, differing from the float32 byte %d (max %d)"
                  % (case, tag, delta, int((~exact).sum()), values.size, int((diff > 0).sum()), int(diff.max())))
            assert ok.all(), (case, tag, int((~ok).sum()), delta)
            assert diff.max() <= 1 and (diff > 0).mean() <= 0.01, (case, tag, int(diff.max()), float((diff > 0).mean()))
        if name != "image" and values.min() != values.max():
            assert values.min() == 0 and values.max() == 255, (case, tag, int(values.min()), int(values.max()))
        if case == "constant" and name in ("depth_mask", "pred_ground_visible_1"):
            assert (got[i] == 0).all(), (case, tag)
    print("%s: delta %.3e, %d of %d prediction pixels needed the band" % (case, delta, needed_band, total))


def test_log_panels_refuses_bad_arguments():
    from footprints_amd import _lib, ops
    inputs, pred = case_inputs("b2_5x7")
    dev = {k: v.cuda() for k, v in inputs.items()}
    with pytest.raises(RuntimeError, match="no 'depth'"):
        ops.log_panels({k: v for k, v in dev.items() if k != "depth"}, pred.cuda(), DEPTH_RANGE)
    with pytest.raises(RuntimeError, match="out must be"):
        ops.log_panels(dev, pred.cuda(), DEPTH_RANGE, out=torch.empty(5, dtype=torch.uint8, device="cuda"))
    lib = _lib.load()
    assert lib.fp_log_panels_workspace(0, 5, 7) == -1 and lib.fp_log_panels_workspace(2, 5, 7) == 2 * 22 * 4
    assert lib.fp_log_panels(1, 1, 1, 1, None, 1, 1, 1, 1, 1, 2, 3, 5, 7, 0.1, 100.0, 1, 1 << 20, None) == -1     # n > B
    assert b"bad sizes" in lib.fp_last_error_string()


def test_log_returns_before_the_writer_has_encoded(tmp_path):
    """the training thread waits for nothing: with the PNG encoder held back until `log()` has returned, the writer thread's flag is
    still unset when it does; afterwards the file holds the device's bytes"""
    from footprints_amd import ops
    from footprints_amd.training.logger import PanelLogger
    from footprints_amd.training.summary import SummaryWriter, encode_png
    gate, encoded = threading.Event(), threading.Event()

    def held_back(rgb):
        assert gate.wait(timeout=120)
        encoded.set()
        return encode_png(rgb)
    inputs, pred = case_inputs("b4_32x64")
    dev_in, dev_pred = {k: v.cuda() for k, v in inputs.items()}, pred.cuda()
    writer = SummaryWriter(str(tmp_path), encode_png=held_back)
    logger = PanelLogger(DEPTH_RANGE)
    logger.log(writer, dev_in, [None, None, None, dev_pred], {"loss": 0.5}, 1e-4, 3)
    assert not encoded.is_set()
    gate.set()
    logger.close()
    writer.close()
    assert encoded.is_set()
    want, tags = ops.log_panels(dev_in, dev_pred, DEPTH_RANGE)
    want = want.cpu().numpy().reshape((-1,) + tuple(want.shape[2:]))
    _, got = ER.read_log(writer.path)
    assert [(s, t) for s, t, _ in got] == [(3, "lr"), (3, "loss")] + [(3, t) for t in tags]
    for (_, tag, pic), w in zip(got[2:], want):
        assert np.array_equal(pic, w), tag


def test_trainer_logs_end_to_end_and_training_is_undisturbed(tmp_path):
    """B = 2 at 64 x 96, 101 steps: log events with validation at steps 0 and 100.  The files' image and target panels are the restatement
    of the batches that were logged; the 21 losses of every step and the final state_dict are bit-identical with and without summaries."""
    from footprints_amd.training.train import TrainManager
    from oracle import restatement as R
    B, H, W = 2, 64, 96
    P, Bf = R.make_state(tag="tm")
    train_cpu = [R.make_batch(B, H, W, tag="tm.train%d" % i) for i in range(3)]
    val_cpu = [R.make_batch(B, H, W, tag="tm.val%d" % i) for i in range(2)]
    train = [{k: v.cuda() for k, v in b.items()} for b in train_cpu]
    val = [{k: v.cuda() for k, v in b.items()} for b in val_cpu]

    def run(summaries, folder):
        tm = TrainManager([train[i % 3] for i in range(101)], val_loader=val, epochs=1, learning_rate=1e-4, log_freq=100, val_batches=2,
                          log_path=str(folder), model_name="run", summaries=summaries, log=lambda *a: None)
        tm.model_manager.save_folder = None                    # no checkpoint: this test is about the logs
        tm.model.load_state_dict({**P, **Bf})
        seen, add = [], tm.evaluator.add_loss_vector
        tm.evaluator.add_loss_vector = lambda vec, mode="train": (seen.append(vec.detach().clone()), add(vec, mode=mode))[1]
        tm.train()
        torch.cuda.synchronize()
        return tm, torch.stack(seen).cpu(), {k: v.detach().cpu().clone() for k, v in tm.model.state_dict().items()}

    tm1, losses1, state1 = run(True, tmp_path / "on")
    tm0, losses0, state0 = run(False, tmp_path / "off")
    assert not os.path.exists(tmp_path / "off")
    assert losses1.shape == (101, 21) and torch.equal(losses1.view(torch.int32), losses0.view(torch.int32))
    assert list(state1) == list(state0) and all(torch.equal(state1[k], state0[k]) for k in state1)
    assert tm1.history == tm0.history and tm1.log_time > 0.0 and tm0.log_time == 0.0

    logged = {"train": [(0, train_cpu[0]), (100, train_cpu[1])], "val": [(0, val_cpu[1]), (100, val_cpu[1])]}
    for mode in ("train", "val"):
        files = os.listdir(tmp_path / "on" / "run" / mode)
        assert len(files) == 1
        version, got = ER.read_log(str(tmp_path / "on" / "run" / mode / files[0]))
        per = 2 + B * 12
        assert version == "brain.Event:2" and len(got) == 2 * per
        for e, (step, batch) in enumerate(logged[mode]):
            ev = got[e * per:(e + 1) * per]
            assert all(s == step for s, _, _ in ev) and [t for _, t, _ in ev] == ["lr", "loss"] + LR.tags(B)
            assert ev[0][2] == np.float32(1e-4) and ev[1][2] == np.float32(tm1.history[mode][e][1]["loss"])
            panels = LR.float_panels(batch, torch.zeros(B, 4, H, W), DEPTH_RANGE)
            want = LR.to_bytes(panels)
            for (_, tag, pic), (t, _), w in zip(ev[2:], panels, want):
                assert tag == t and pic.shape == (H, W, 3)
                if tag.split("/")[0] in LR.TARGET_PANELS:        # (the prediction panels are test_log_panels_match_the_restatements')
                    assert np.array_equal(pic, w), (mode, step, tag)
