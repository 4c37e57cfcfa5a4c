"""GPU: the reader of the ground-segmentation trainer on the device (csrc/resample_u8.hip, csrc/seg_reader.hip,
datasets/device_path.SegBatchAssembler) against the NumPy restatement (tests/seg_reader_restatement.py, pinned to Pillow and to the reference on the CPU) and against what the
reference's own dataset code wrote (tests/golden/g16_seg_reader.npz), and the segmentation trainer on device-assembled batches.
Everything but the trainer's loss is compared with np.array_equal.  Needs neither Pillow nor the reference."""
import ctypes as C
import hashlib
import random

import numpy as np
import pytest
import torch

from tests import seg_reader_restatement as SR
from tests.golden import digest, seg_reader_inputs as SI

pytestmark = pytest.mark.gpu

ALL_CASES = SI.WINDOW_CASES + SI.GREY_CASES


@pytest.fixture(scope="module")
def gold():
    return digest.load("g16_seg_reader")


def _case_item(case, seed=3, **kw):
    name, (h, w), target, window, c = case
    return dict(img=SI.image(h, w, c, seed), target=target, window=window, **kw)


def run_windows(items, channels=3, pad=0):
    """one fp_resize_window_u8 call over `items` = dicts(img, target (th, tw), window, rect "tight" | "whole" | (y0, x0, h, w),
    whole_tables, record = function that may spoil the finished record) -> (list of uint8 [h, w, C] outputs or None where nothing was
    written, status word).  `pad` bytes in front of the first source shift every offset."""
    from footprints_amd import ops
    batch = ops.WindowBatch(channels)
    chunks, outs = [np.zeros(pad, np.uint8)], []
    src_off, out_off = pad, 0
    for it in items:
        img = it["img"].reshape(it["img"].shape[0], it["img"].shape[1], channels)
        (h, w), (th, tw), (top, left, wh, ww) = img.shape[:2], it["target"], it["window"]
        whole = it.get("whole_tables", False)
        tv, y_lo, y_hi = ops.resize_window_axis(h, th, top, wh, whole_table=whole)
        th_, x_lo, x_hi = ops.resize_window_axis(w, tw, left, ww, whole_table=whole)
        rect = it.get("rect", "tight")
        rect = (y_lo, x_lo, y_hi - y_lo, x_hi - x_lo) if rect == "tight" else (0, 0, h, w) if rect == "whole" else rect
        y0, x0, rh, rw = rect
        chunks.append(np.ascontiguousarray(img[y0:y0 + rh, x0:x0 + rw]).reshape(-1))
        batch.add(src_off, rect, batch.table(w, tw, th_), batch.table(h, th, tv), (top, left, wh, ww), out_off)
        if "record" in it:
            it["record"](batch.samples[-1])
        outs.append((out_off, wh, ww))
        src_off += chunks[-1].size
        out_off += wh * ww * channels
    rec, tab, coef = batch.arrays()
    src = torch.from_numpy(np.concatenate(chunks)).cuda()
    out = torch.full((out_off,), 0xAB, dtype=torch.uint8, device="cuda")
    d_tab, d_coef = (torch.from_numpy(tab.copy()).cuda(), torch.from_numpy(coef).cuda()) if batch.tables else (None, None)
    ops.resize_window_u8(src, src.numel(), torch.from_numpy(rec.copy()).cuda(), len(items), d_tab, len(batch.tables), d_coef, coef.size, out, channels,
                         batch.max_src_h, batch.max_src_w, batch.max_win_h, batch.max_win_w)
    status = ops.resize_window_status("cuda", len(items), batch.max_src_h, batch.max_win_w, channels)
    host = out.cpu().numpy()
    return [host[o:o + wh * ww * channels].reshape(wh, ww, channels) for o, wh, ww in outs], status


def expect(case_or_item, seed=3):
    it = _case_item(case_or_item, seed) if isinstance(case_or_item, tuple) else case_or_item
    img = it["img"]
    return SR.resize_window(img, it["target"][0], it["target"][1], it["window"]).reshape(it["window"][2], it["window"][3], -1)


@pytest.mark.parametrize("case", ALL_CASES, ids=[c[0] for c in ALL_CASES])
def test_window_equals_resize_then_crop(case):
    """window position and scale, skipped passes, the equal-ratio target, C = 1: each alone, from the tightest staged rectangle"""
    got, status = run_windows([_case_item(case)], channels=case[4])
    assert status == 0 and np.array_equal(got[0], expect(case))


def test_skipped_pass_records_carry_minus_one():
    from footprints_amd import ops
    assert ops.resize_window_axis(30, 30, 7, 16)[0] is None and ops.WindowBatch(3).table(30, 30, None) == -1
    b = ops.WindowBatch(3)
    t, lo, hi = ops.resize_window_axis(53, 44, 11, 24)
    assert b.table(53, 44, t) == 0 and b.tables[0].first == 11 and b.tables[0].count == 24


def test_two_stage_chain_through_a_device_intermediate():
    """20 x 70 -> 10 x 35 -> 16 x 56 -> crop: the first call produces what the second call's taps reach, the second call reads it on the
    device"""
    from footprints_amd import ops
    name, (h, w), s1, s2, window, c = SI.CHAIN_CASE
    img = SI.image(h, w, c, 5)
    top, left, wh, ww = window
    tv2, y_lo, y_hi = ops.resize_window_axis(s1[0], s2[0], top, wh)
    th2, x_lo, x_hi = ops.resize_window_axis(s1[1], s2[1], left, ww)
    mid_window = (y_lo, x_lo, y_hi - y_lo, x_hi - x_lo)
    mid, status = run_windows([dict(img=img, target=s1, window=mid_window)])
    assert status == 0 and np.array_equal(mid[0], SR.resize_window(img, s1[0], s1[1], mid_window))
    # second call: the source is the first call's window, a rectangle of the 10 x 35 image with its origin
    b = ops.WindowBatch(3)
    b.add(0, mid_window, b.table(s1[1], s2[1], th2), b.table(s1[0], s2[0], tv2), window, 0)
    rec, tab, coef = b.arrays()
    out = torch.zeros(wh * ww * 3, dtype=torch.uint8, device="cuda")
    src = torch.from_numpy(mid[0].copy()).cuda().reshape(-1)
    ops.resize_window_u8(src, src.numel(), torch.from_numpy(rec.copy()).cuda(), 1, torch.from_numpy(tab.copy()).cuda(), 2, torch.from_numpy(coef).cuda(),
                         coef.size, out, 3, b.max_src_h, b.max_src_w, b.max_win_h, b.max_win_w, check=True)
    assert np.array_equal(out.cpu().numpy().reshape(wh, ww, 3), SR.image_u8(img, h, [(h, w), s1, s2], window))


def test_ragged_sources_at_odd_byte_offsets():
    items = [_case_item(SI.WINDOW_CASES[8], seed=s) for s in (1, 2, 3)]                     # 37 x 53 x 3 = 5883 bytes each: odd
    got, status = run_windows(items, pad=1)
    assert status == 0
    for g, it in zip(got, items):
        assert np.array_equal(g, expect(it))


def test_staged_rectangle_and_window_tables_change_nothing():
    """the same bytes from the tightest rectangle, from a larger one with an origin, from the whole frame, and with whole tables"""
    case = SI.WINDOW_CASES[2]
    ref = expect(case)
    variants = [_case_item(case), _case_item(case, rect="whole"), _case_item(case, rect="whole", whole_tables=True), _case_item(case, whole_tables=True),
                _case_item(case, rect=(40, 80, 70, 100))]
    got, status = run_windows(variants)
    assert status == 0
    for g in got:
        assert np.array_equal(g, ref)


def _leave_target(rec):
    rec.top += 20                                  # 30-row target: rows 34 .. 49 do not exist


def _miss_a_tap(rec):
    rec.src_x0 += 1                                # the rectangle now starts one column after the first tap
    rec.src_w -= 1


@pytest.mark.parametrize("spoil", [_leave_target, _miss_a_tap], ids=["window_leaves_target", "rectangle_misses_a_tap"])
def test_bad_record_is_turned_down_and_the_others_are_right(spoil):
    good = [_case_item(SI.WINDOW_CASES[0]), _case_item(SI.WINDOW_CASES[2])]
    bad = _case_item(SI.WINDOW_CASES[1], record=spoil)
    got, status = run_windows([good[0], bad, good[1]])
    assert status == 1
    assert np.array_equal(got[0], expect(good[0])) and np.array_equal(got[2], expect(good[1]))
    assert bool((got[1] == 0xAB).all())                                                # left alone, whole


def test_records_beyond_the_stated_maxima_are_turned_down():
    from footprints_amd import ops
    it = _case_item(SI.WINDOW_CASES[0])
    h, w = it["img"].shape[:2]
    b = ops.WindowBatch(3)
    tv, y_lo, y_hi = ops.resize_window_axis(h, 30, 0, 16)
    th, x_lo, x_hi = ops.resize_window_axis(w, 44, 0, 24)
    b.add(0, (0, 0, h, w), b.table(w, 44, th), b.table(h, 30, tv), (0, 0, 16, 24), 0)
    rec, tab, coef = b.arrays()
    src = torch.from_numpy(it["img"].reshape(-1).copy()).cuda()
    out = torch.full((16 * 24 * 3,), 0xAB, dtype=torch.uint8, device="cuda")
    args = (src, src.numel(), torch.from_numpy(rec.copy()).cuda(), 1, torch.from_numpy(tab.copy()).cuda(), 2, torch.from_numpy(coef).cuda(), coef.size, out, 3)
    for maxima in [(h - 1, w, 16, 24), (h, w - 1, 16, 24), (h, w, 15, 24), (h, w, 16, 23)]:
        with pytest.raises(ValueError):
            ops.resize_window_u8(*args, *maxima, check=True)
        assert bool((out == 0xAB).all())
    ops.resize_window_u8(*args, h, w, 16, 24, check=True)
    assert np.array_equal(out.cpu().numpy().reshape(16, 24, 3), expect(it))


def test_mixed_batch_in_one_call():
    """every RGB case above in one call: per-sample target sizes, skipped passes next to resized ones, odd offsets, a bad record between"""
    items = [_case_item(c, seed=10 + i, rect=("whole" if i % 3 == 1 else "tight"), whole_tables=(i % 2 == 1)) for i, c in enumerate(SI.WINDOW_CASES)]
    items.insert(4, _case_item(SI.WINDOW_CASES[1], record=_leave_target))
    got, status = run_windows(items, pad=3)
    assert status == 1
    for i, (g, it) in enumerate(zip(got, items)):
        if "record" in it:
            assert bool((g == 0xAB).all())
        else:
            assert np.array_equal(g, expect(it)), i
    grey, status = run_windows([_case_item(c, seed=20 + i) for i, c in enumerate(SI.GREY_CASES)], channels=1)
    assert status == 0
    for i, (g, c) in enumerate(zip(grey, SI.GREY_CASES)):
        assert np.array_equal(g, expect(c, seed=20 + i))


@pytest.mark.parametrize("channels, shapes", [(3, [(37, 53), (17, 53), (37, 23), (17, 23), (5, 7), (41, 23)]), (1, [(37, 53), (17, 53), (37, 23)])],
                         ids=["rgb", "grey"])
def test_whole_frame_resize_is_the_window_resize_of_the_whole_target(channels, shapes):
    """fp_resize_u8 = fp_resize_window_u8 with window = target and rectangle = source, byte for byte: the ragged batch of
    test_gpu_reader.test_resize_ragged_batch_mixed_passes (both passes, each alone, neither, 5 -> 17 with the taps clamped at both borders,
    23 * C bytes per row, 17 rows for a tile of 8), the window call's sources at odd byte offsets"""
    from footprints_amd import ops
    from tests.golden import reader_inputs as RI
    H, W = 17, 23
    imgs = [RI.image(h, w, channels, 40 + i) for i, (h, w) in enumerate(shapes)]
    whole = ops.resize_u8(imgs, H, W).cpu().numpy()
    got, status = run_windows([dict(img=im, target=(H, W), window=(0, 0, H, W), rect="whole", whole_tables=True) for im in imgs], channels=channels, pad=1)
    assert status == 0
    for i, g in enumerate(got):
        assert np.array_equal(g, whole[i]), shapes[i]


# ---- labels ---------------------------------------------------------------------------------------------------------------------------
def run_labels(items, H, W):
    """items = dicts(dataset, labels, rows, cols) -> (ground_mask, labelled_pix, status)"""
    from footprints_amd import _lib, ops
    from footprints_amd.preprocessing.segmentation.datasets import plan as P
    ids, offs = [], [0]
    for name in P.DATASETS:
        ids += sorted(P.GROUND_IDS[name])
        offs.append(len(ids))
    rec = (_lib.SegLabelSample * len(items))()
    chunks, index, off = [], [], 0
    for b, it in enumerate(items):
        lab = it["labels"]
        ade = it["dataset"] == "ADE20K"
        lab = lab if ade or lab.ndim == 2 else lab[..., 0]
        chunks.append(np.ascontiguousarray(lab).reshape(-1))
        index += [it["rows"], it["cols"]]
        rec[b] = _lib.SegLabelSample(off, lab.shape[0], lab.shape[1], 3 if ade else 1, b * (H + W), b * (H + W) + H,
                                     _lib.SEG_DECODE_ADE20K if ade else _lib.SEG_DECODE_CHANNEL0,
                                     _lib.SEG_LABELLED_NONZERO if it["dataset"] == "cityscapes" else _lib.SEG_LABELLED_ONES, P.DATASETS.index(it["dataset"]))
        if "record" in it:
            it["record"](rec[b])
        off += chunks[-1].size
    src = torch.from_numpy(np.concatenate(chunks)).cuda()
    idx = torch.from_numpy(np.concatenate(index).astype(np.int32)).cuda()
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    gm = torch.full((len(items), H, W), -7.0, device="cuda")
    lp = torch.full((len(items), H, W), -7.0, device="cuda")
    ops.seg_labels(src, src.numel(), torch.from_numpy(np.frombuffer(bytes(rec), dtype=np.uint8).copy()).cuda(), len(items), idx, idx.numel(),
                   torch.tensor(ids, dtype=torch.int32, device="cuda"), torch.tensor(offs, dtype=torch.int32, device="cuda"), H, W,
                   ground_mask=gm, labelled_pix=lp, status=status)
    return gm.cpu().numpy(), lp.cpu().numpy(), int(status.item())


def test_label_kernel_mixed_batch_against_restatement_and_fixture(gold):
    """the three decode / labelled modes in one call, flips on and off, ids 0 and 6655, ids next to ground ids (the inputs' palettes)"""
    from footprints_amd import ops
    from footprints_amd.preprocessing.segmentation.datasets import plan as P
    H, W = SI.FEED
    items, refs = [], []
    for case in SI.SAMPLES:
        name, dataset, hw, is_train, seed = case
        _, image, labels = SI.sample_inputs(case)
        plan = P.draw_seg_plan(dataset, hw, SI.FEED, is_train, random.Random(seed))
        rows, cols = P.label_tables(plan, ops.nearest_index)
        items.append(dict(dataset=dataset, labels=labels, rows=rows, cols=cols))
        ids = SR.label_ids(dataset, labels, plan.rows, P.plan_sizes(plan), plan.window)
        refs.append((name, dataset, ids[:, ::-1] if plan.aug.flip else ids, plan.aug.flip))
    gm, lp, status = run_labels(items, H, W)
    assert status == 0
    seen = set()
    for b, (name, dataset, ids, flip) in enumerate(refs):
        assert np.array_equal(gm[b], np.isin(ids, SR.GROUND_IDS[dataset]).astype(np.float32)), name
        assert np.array_equal(lp[b], (ids != 0).astype(np.float32) if dataset == "cityscapes" else np.ones((H, W), np.float32)), name
        assert np.array_equal(gm[b], gold[name + ".ground_mask"]) and np.array_equal(lp[b], gold[name + ".labelled_pix"]), name
        seen |= {(dataset, int(flip))} | {(dataset, "id", int(v)) for v in np.unique(ids)}
    assert {(d, f) for d in SR.GROUND_IDS for f in (0, 1)} <= seen                       # every dataset with and without the flip
    assert {("ADE20K", "id", v) for v in (0, 6655, 975, 976, 977, 2531, 2532)} <= seen   # both ends of the range, neighbours of ground ids
    assert {("cityscapes", "id", v) for v in (0, 5, 6, 9, 10, 21, 22, 23)} <= seen


def test_label_record_outside_its_buffer_is_turned_down():
    H, W = SI.FEED
    lab = SI.labels("cityscapes", 20, 30, 1)
    rows, cols = np.arange(H, dtype=np.int32), np.arange(W, dtype=np.int32)
    good = dict(dataset="cityscapes", labels=lab, rows=rows, cols=cols)

    def too_tall(rec):
        rec.h += 40
    gm, lp, status = run_labels([good, dict(good, record=too_tall), dict(good, rows=rows + 5)], H, W)       # the last one: rows 20 don't exist
    assert status == 1
    ids = lab[:H, :W, 0]
    assert np.array_equal(gm[0], np.isin(ids, SR.GROUND_IDS["cityscapes"]).astype(np.float32)) and np.array_equal(lp[0], (ids != 0).astype(np.float32))
    assert bool((gm[1] == -7.0).all()) and bool((lp[1] == -7.0).all())
    assert np.array_equal(gm[2][:15], np.isin(lab[5:20, :W, 0], SR.GROUND_IDS["cityscapes"]).astype(np.float32)) and bool((gm[2][15:] == -7.0).all())


# ---- the assembler ---------------------------------------------------------------------------------------------------------------------
def _plans(cases, feed):
    from footprints_amd.preprocessing.segmentation.datasets import plan as P
    return [P.draw_seg_plan(c[1], c[2], feed, c[3], random.Random(c[4])) for c in cases]


def test_assembler_equals_the_reference_written_batch(gold):
    """the fixture's samples as one mixed batch with the fixture's draws, four submissions over three slots"""
    from footprints_amd.datasets.device_path import SegBatchAssembler
    H, W = SI.FEED
    cases = SI.SAMPLES
    samples = [SI.sample_inputs(c) for c in cases]
    plans = _plans(cases, SI.FEED)
    asm = SegBatchAssembler(len(cases), H, W, max_src_hw=(810, 100), check=True)
    order = list(range(len(cases)))
    for submission in range(4):
        slot = asm.submit([samples[i] for i in order], [plans[i] for i in order])
        assert slot == submission % 3
        batch = asm.collect(slot)
        torch.cuda.synchronize()
        assert set(batch) == {"image", "ground_mask", "labelled_pix"}
        for b, i in enumerate(order):
            name = cases[i][0]
            for key in batch:
                assert np.array_equal(batch[key][b].cpu().numpy(), gold["%s.%s" % (name, key)]), (submission, name, key)
        asm.release(slot)
        order = order[3:] + order[:3]                       # another batch in the slot the next time round


def test_assembler_at_the_realistic_size(gold):
    """two Cityscapes frames of 1024 x 2048 at resize factors near 0.7 -> 192 x 640, against the reference-written batch's digest"""
    from footprints_amd.datasets.device_path import SegBatchAssembler
    H, W = SI.BIG_FEED
    samples = [SI.sample_inputs(c) for c in SI.BIG]
    plans = _plans(SI.BIG, SI.BIG_FEED)
    assert all(0.65 < p.factor < 0.75 for p in plans)
    asm = SegBatchAssembler(2, H, W, max_src_hw=(512, 1400), slots=1, check=True)          # the staged rectangles, not the frames
    assert asm.slots[0]["h_src"].numel() < samples[0][1].size
    batch = asm.collect(asm.submit(samples, plans))
    torch.cuda.synchronize()
    for key in ("image", "ground_mask", "labelled_pix"):
        got = batch[key].cpu().contiguous()
        assert np.array_equal(np.frombuffer(hashlib.sha256(got.numpy().tobytes()).digest(), np.uint8), gold["big.%s#sha256" % key]), key
        assert np.array_equal(got.reshape(-1)[::digest.STRIDE].numpy(), gold["big.%s#sample" % key]) and tuple(got.shape) == tuple(gold["big.%s#shape" % key])


def test_device_loader_with_the_seg_draws():
    from footprints_amd.datasets.device_path import SegBatchAssembler, SyntheticSegSource
    from footprints_amd.preprocessing.segmentation.datasets import plan as P
    frames = [("cityscapes", (800, 90)), ("ADE20K", (37, 53)), ("matterport", (64, 80)), ("ADE20K", (10, 40))]
    H, W = SI.FEED
    source = SyntheticSegSource(4, 5, frames, seed=3)
    asm = SegBatchAssembler(4, H, W, max_src_hw=(800, 90), check=True)
    rng = random.Random(5)
    ref_rng = random.Random(5)
    n = 0
    for batch, samples in zip(asm.loader(source, True, rng), source):
        torch.cuda.synchronize()
        for b, (name, image, labels) in enumerate(samples):
            plan = P.draw_seg_plan(name, image.shape[:2], SI.FEED, True, ref_rng)
            a = plan.aug
            ref = SR.sample(name, image, labels, plan.rows, P.plan_sizes(plan), plan.window, a.flip, a.n_ops, list(a.ops), list(a.factor), a.hue_shift)
            for got, want in zip((batch["image"], batch["ground_mask"], batch["labelled_pix"]), ref):
                assert np.array_equal(got[b].cpu().numpy(), want), (n, b, name)
        n += 1
    assert n == 5


# ---- the trainer -----------------------------------------------------------------------------------------------------------------------
def test_trainer_on_device_assembled_batches(tmp_path):
    from collections import OrderedDict
    from footprints_amd.datasets.device_path import SegBatchAssembler, SyntheticSegSource
    from footprints_amd.preprocessing.segmentation.network import Segmentor
    from footprints_amd.preprocessing.segmentation.options import SegmentationOptions
    from footprints_amd.preprocessing.segmentation.train import Trainer
    from oracle import restatement as R
    B, H, W = 2, 64, 96
    frames = [("cityscapes", (800, 200)), ("ADE20K", (70, 110)), ("matterport", (128, 160)), ("ADE20K", (50, 90))]
    opts = SegmentationOptions().parse(["--height", str(H), "--width", str(W), "--batch_size", str(B), "--log_freq", "1", "--epochs", "2",
                                        "--log_path", str(tmp_path), "--model_name", "seg_test"])
    P, Bf = R.make_seg_state(True, tag="segtrain")
    model = Segmentor(pretrained=False, use_PSP=True)
    model.load_state_dict({**P, **Bf})
    model.cuda()

    class Counted:
        """a loader that counts the batches taken from it and keeps the first one"""

        def __init__(self, loader):
            self.loader, self.taken, self.first = loader, 0, None
            self.dataset = loader.source.dataset

        def __len__(self):
            return len(self.loader)

        def __iter__(self):
            for batch in self.loader:
                self.taken += 1
                if self.first is None:
                    self.first = {k: v.clone() for k, v in batch.items()}
                yield batch

    train = Counted(SegBatchAssembler(B, H, W, max_src_hw=(800, 200)).loader(SyntheticSegSource(B, 2, frames, seed=1), True, random.Random(1)))
    val = Counted(SegBatchAssembler(B, H, W, max_src_hw=(800, 200)).loader(SyntheticSegSource(B, 3, frames, seed=2), False, random.Random(2)))
    trainer = Trainer(opts, model=model, train_loader=train, val_loader=val)
    assert trainer.optimiser.param_groups[0]["lr"] == pytest.approx(1e-4)
    trainer.train()
    assert trainer.step == 4 and train.taken == 4
    assert val.taken == 4 * 10                                                          # ten batches per logged step, cycling over three
    assert len(trainer.history) == 4
    for entry in trainer.history:
        assert set(entry["train"]) == set(entry["val"]) == {"ground_loss_0", "ground_loss_1", "ground_loss_2", "ground_loss_3", "loss"}
    # StepLR(10) stepped at the START of every epoch: after two epochs the scheduler has made two steps
    assert trainer.scheduler.last_epoch == 2 and trainer.history[0]["lr"] == pytest.approx(1e-4)
    fresh = Segmentor(pretrained=False, use_PSP=True)
    state = torch.load(str(tmp_path / "seg_test" / "models" / "epoch_0.pth"), map_location="cpu")
    assert set(state) == set(fresh.state_dict())
    fresh.load_state_dict(state)
    assert (tmp_path / "seg_test" / "models" / "epoch_1.pth").exists()
    # the first step's loss against the float64 oracle on the same assembled batch and initial state
    batch = {k: v.cpu() for k, v in train.first.items()}
    Pd = OrderedDict((k, v.detach().clone().double()) for k, v in P.items())
    Bd = OrderedDict((k, v.double() if v.is_floating_point() else v.clone()) for k, v in Bf.items())
    with torch.no_grad():
        ref = float(R.seg_loss(R.segmentor(batch["image"].double(), Pd, Bd, True, True), batch["ground_mask"].double(), batch["labelled_pix"].double(), H, W))
    got = float(trainer.history[0]["batch_loss"])
    print("first step loss: trainer %.9g oracle %.9g rel %.3e" % (got, ref, abs(got - ref) / abs(ref)))
    assert abs(got - ref) <= 1e-5 * abs(ref)
