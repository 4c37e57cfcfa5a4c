"""CPU: the segmentation trainer's readers that read ahead and its windowed device decode, without a device -- the threaded source against
BatchSource (samples and the `random` stream), what --num_workers builds, what the readers hand over under device_decode, plans drawn from
headers, the assembler's decode protocol with the device half stubbed at its seams (in the manner of tests/test_train_decode_cpu.py), and
the content of every JPEG the GPU tests expect the device to decode.  tests/test_gpu_seg_train_decode.py imports the catalogue, the mixed
batches and the tree helper from here."""
import argparse
import functools
import io
import os
import random

import numpy as np
import pytest
import torch

from tests import jpeg_decode_restatement as JR
from tests.golden import make_golden_jpeg_decode as G
from tests.golden import seg_reader_inputs as SI

FEED = (64, 96)                 # the smallest size tests/test_gpu_segmentation.py trains at
# every JPEG the GPU tests expect the device to decode: name -> (dataset, h, w, quality, Pillow's subsampling, grey)
JPEGS = {"ade 420": ("ADE20K", 70, 150, 90, 2, False), "ade 444": ("ADE20K", 96, 200, 95, 0, False), "ade grey": ("ADE20K", 52, 164, 90, None, True),
         "ade 422": ("ADE20K", 80, 100, 85, 1, False), "ade small": ("ADE20K", 50, 72, 75, 2, False),
         "mp a": ("matterport", 80, 100, 90, 2, False), "mp b": ("matterport", 96, 128, 85, 2, False), "mp c": ("matterport", 72, 120, 92, 0, False)}
CITY_HW = (800, 60)             # a Cityscapes frame keeps at least the 795 rows its _preprocess crops to
MIXED_SEED = 3                  # of the draws of the mixed batches: makes the Matterport frame of the first a two-stage resize


@functools.lru_cache(None)
def jpeg_file(name):
    from PIL import Image
    _, h, w, quality, sampling, grey = JPEGS[name]
    a = G.photo(h, w, 500 + h + 3 * sorted(JPEGS).index(name))
    if grey:
        a = np.asarray(Image.fromarray(a).convert("L"))
    return G.write(a, quality, sampling)


@functools.lru_cache(None)
def progressive_file(h=40, w=56, seed=7):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(G.photo(h, w, seed)).save(buf, format="JPEG", progressive=True)
    return buf.getvalue()


@functools.lru_cache(None)
def noise_frame():
    """tests/test_gpu_jpeg_decode.py's: noise at quality 100 does not settle inside the default launch budget (status 2)"""
    rng = np.random.default_rng(96128)
    return G.write(rng.integers(0, 256, (96, 128, 3), dtype=np.uint8), 100)


@functools.lru_cache(None)
def city_png(seed=0):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(G.photo(CITY_HW[0], CITY_HW[1], 40 + seed)).save(buf, format="PNG")
    return buf.getvalue()


def _labels(dataset, data, seed):
    h, w = G.pillow_decode(data).shape[:2]
    return SI.labels(dataset, h, w, seed)


@functools.lru_cache(None)
def mixed_batches():
    """two batches of (dataset, file bytes, labels, kind): the first holds the three ADE20K samplings, a Cityscapes PNG, a Matterport JPEG, a
    progressive JPEG and the noise frame; the second has no noise frame.  kind: 'device' | 'parser' | 'status' -- who decodes it"""
    first = [("ADE20K", jpeg_file("ade 420"), "device"), ("ADE20K", jpeg_file("ade 444"), "device"), ("ADE20K", jpeg_file("ade grey"), "device"),
             ("cityscapes", city_png(), "parser"), ("matterport", jpeg_file("mp a"), "device"), ("ADE20K", progressive_file(), "parser"),
             ("ADE20K", noise_frame(), "status")]
    second = [("matterport", jpeg_file("mp b"), "device"), ("ADE20K", jpeg_file("ade 422"), "device"), ("cityscapes", city_png(1), "parser"),
              ("ADE20K", jpeg_file("ade small"), "device"), ("matterport", jpeg_file("mp c"), "device"), ("ADE20K", progressive_file(), "parser"),
              ("ADE20K", jpeg_file("ade 420"), "device")]
    return tuple(tuple((d, f, _labels(d, f, 10 * k + n), kind) for n, (d, f, kind) in enumerate(batch)) for k, batch in enumerate((first, second)))


def as_samples(batch, folder, device_decode):
    """the (name, image, labels) samples of a batch as the readers deliver them: decoded frames, or file samples under device_decode"""
    from footprints_amd.datasets.decode_stage import read_sample
    os.makedirs(str(folder), exist_ok=True)
    out = []
    for n, (dataset, data, labels, _) in enumerate(batch):
        path = os.path.join(str(folder), "%d.%s" % (n, "png" if data[:4] == b"\x89PNG" else "jpg"))
        with open(path, "wb") as fh:
            fh.write(data)
        smp = read_sample(path, device_decode)
        out.append((dataset, smp if device_decode else smp["image"], labels))
    return out


def write_seg_tree(root, n=4):
    """a tiny tree of the three datasets with train / val split files under root/splits, and root/paths.yaml -> the config path.  Per
    dataset n train and 2 val samples; ADE20K: baseline JPEGs and one progressive file; Matterport: baseline JPEGs; Cityscapes: PNGs"""
    from PIL import Image
    root = str(root)
    ade, city, mp = (os.path.join(root, d) for d in ("ade", "city", "mp"))
    lines = {"ADE20K": [], "cityscapes": [], "matterport": []}
    ade_names, mp_names = [k for k in sorted(JPEGS) if JPEGS[k][0] == "ADE20K"], [k for k in sorted(JPEGS) if JPEGS[k][0] == "matterport"]
    for i in range(n + 2):
        # ADE20K: <stem>.jpg and <stem>_seg.png
        data = progressive_file() if i == 1 else jpeg_file(ade_names[i % len(ade_names)])
        os.makedirs(os.path.join(ade, "images"), exist_ok=True)
        with open(os.path.join(ade, "images", "f%d.jpg" % i), "wb") as fh:
            fh.write(data)
        Image.fromarray(_labels("ADE20K", data, i)).save(os.path.join(ade, "images", "f%d_seg.png" % i))
        lines["ADE20K"].append("images/f%d.jpg" % i)
        # Cityscapes
        for sub in ("leftImg8bit", "gtFine"):
            os.makedirs(os.path.join(city, sub, "train", "aachen"), exist_ok=True)
        with open(os.path.join(city, "leftImg8bit", "train", "aachen", "f%d_leftImg8bit.png" % i), "wb") as fh:
            fh.write(city_png(i))
        Image.fromarray(SI.labels("cityscapes", CITY_HW[0], CITY_HW[1], 30 + i)).save(
            os.path.join(city, "gtFine", "train", "aachen", "f%d_gtFine_labelIds.png" % i))
        lines["cityscapes"].append("train aachen f%d" % i)
        # Matterport
        scans = os.path.join(mp, "sample_dataset/v1/scans", "scanA")
        os.makedirs(os.path.join(scans, "scanA", "matterport_color_images"), exist_ok=True)
        os.makedirs(os.path.join(scans, "nia_ground_masks"), exist_ok=True)
        data = jpeg_file(mp_names[i % len(mp_names)])
        with open(os.path.join(scans, "scanA", "matterport_color_images", "p%d_i1_2.jpg" % i), "wb") as fh:
            fh.write(data)
        np.save(os.path.join(scans, "nia_ground_masks", "out_p%d_1_2_visibleground.npy" % i), _labels("matterport", data, 60 + i).astype(np.float32) * 3)
        lines["matterport"].append("scanA p%d 1 2" % i)
    for dataset, ls in lines.items():
        os.makedirs(os.path.join(root, "splits", dataset), exist_ok=True)
        for split, part in (("train", ls[:n]), ("val", ls[n:])):
            with open(os.path.join(root, "splits", dataset, split + ".txt"), "w") as fh:
                fh.write("\n".join(part) + "\n")
    with open(os.path.join(root, "paths.yaml"), "w") as fh:
        fh.write("ADE20K:\n  dataset: %s\ncityscapes:\n  dataset: %s\nmatterport:\n  dataset: %s\n" % (ade, city, mp))
    return os.path.join(root, "paths.yaml")


# ---- the read-ahead source ------------------------------------------------------------------------------------------------------------------
class _Reader:
    def __init__(self, tag, n):
        self.tag, self.n = tag, n

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        return (self.tag, i)


@pytest.mark.parametrize("workers", (1, 4))
def test_the_threaded_source_yields_batch_sources_samples_and_leaves_the_rng_where_it_does(workers):
    from footprints_amd.datasets.training import ThreadedBatchSource
    from footprints_amd.preprocessing.segmentation.datasets import BatchSource
    readers = [_Reader("a", 7), _Reader("b", 12)]
    random.seed(21)
    plain = list(BatchSource(readers, 3, shuffle=True))                 # the module-level `random`, as the trainer uses it
    after_plain = random.getstate()
    random.seed(21)
    threaded = list(ThreadedBatchSource(readers, 3, shuffle=True, rng=random, num_workers=workers))
    assert threaded == plain and len(plain) == 6 and random.getstate() == after_plain
    assert sorted(s for b in plain for s in b) != [s for b in plain for s in b]            # it did shuffle
    for r in range(2):                                                  # and `shard` is BatchSource's
        a, b = random.Random(4), random.Random(4)
        assert list(ThreadedBatchSource(readers, 3, rng=a, num_workers=workers).shard(r, 2)) == list(BatchSource(readers, 3, rng=b).shard(r, 2))
        assert a.getstate() == b.getstate()


class _NoAssembler:
    def __init__(self, *args, **kw):
        self.args, self.kw = args, kw

    def loader(self, source, is_train, rng):
        return argparse.Namespace(source=source, asm=self, is_train=is_train, rng=rng)


@pytest.mark.parametrize("num_workers,device_decode", ((0, False), (1, False), (4, True), (16, False)))
def test_num_workers_and_device_decode_reach_the_loaders(tmp_path, monkeypatch, num_workers, device_decode):
    from footprints_amd.datasets import device_path
    from footprints_amd.datasets.training import ThreadedBatchSource
    from footprints_amd.preprocessing.segmentation.datasets import BatchSource
    from footprints_amd.preprocessing.segmentation.options import SegmentationOptions
    from footprints_amd.preprocessing.segmentation.train import Trainer
    config = write_seg_tree(tmp_path, n=2)
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(device_path, "SegBatchAssembler", _NoAssembler)
    trainer = Trainer.__new__(Trainer)                                  # create_dataloaders alone: the constructor needs a device
    trainer.opt = SegmentationOptions().parse(["--config_path", config, "--batch_size", "2", "--num_workers", str(num_workers),
                                               "--training_datasets", "ADE20K", "cityscapes", "matterport"]
                                              + (["--device_decode"] if device_decode else []))
    train, val = trainer.create_dataloaders()
    if num_workers == 0:
        assert type(train.source) is BatchSource and type(val.source) is BatchSource
    else:
        assert type(train.source) is ThreadedBatchSource and type(val.source) is ThreadedBatchSource
        assert (train.source.num_workers, val.source.num_workers) == (num_workers, min(2, num_workers))
        assert train.source.ahead == val.source.ahead == ThreadedBatchSource([], 1).ahead          # the Footprints trainer's
        assert train.source.rng is random and val.source.rng is random
    assert train.is_train and not val.is_train and train.rng is random
    for loader in (train, val):
        assert loader.asm.kw["device_decode"] is device_decode
        assert [r.device_decode for r in loader.source.readers] == [device_decode] * 3
    assert len(train.dataset) == 6 and len(val.dataset) == 6


def test_the_help_text_names_both_modes():
    from footprints_amd.preprocessing.segmentation.options import SegmentationOptions
    text = " ".join(SegmentationOptions().parser.format_help().split())
    at = text.rindex("--device_decode")                                  # the option's entry, not the usage line
    assert "Training mode" in text[at:at + 600] and "Inference mode" in text[at:at + 600]


# ---- what the readers return ------------------------------------------------------------------------------------------------------------------
def test_the_readers_hand_over_bytes_or_a_refused_frame_and_the_same_labels(tmp_path):
    from footprints_amd.preprocessing.segmentation.datasets import READERS
    write_seg_tree(tmp_path, n=2)
    seen = set()
    for dataset, folder in (("ADE20K", "ade"), ("cityscapes", "city"), ("matterport", "mp")):
        with open(os.path.join(str(tmp_path), "splits", dataset, "train.txt")) as fh:
            lines = fh.read().splitlines()
        plain = READERS[dataset](os.path.join(str(tmp_path), folder), lines)
        dev = READERS[dataset](os.path.join(str(tmp_path), folder), lines, device_decode=True)
        assert plain.device_decode is False and dev.device_decode is True and len(dev) == 2
        for i in range(2):
            name, smp, labels = dev[i]
            ref_name, image, ref_labels = plain[i]
            assert name == ref_name == dataset and isinstance(image, np.ndarray) and image.dtype == np.uint8
            assert labels.dtype == ref_labels.dtype == np.uint8 and np.array_equal(labels, ref_labels)
            with open(smp["path"], "rb") as fh:
                data = fh.read()
            if dataset == "cityscapes" or (dataset == "ADE20K" and i == 1):      # PNG; the progressive file
                assert set(smp) == {"path", "image", "refused"} and smp["refused"] and np.array_equal(smp["image"], image)
                seen.add("png" if data[:4] == b"\x89PNG" else "progressive")
            else:
                assert set(smp) == {"path", "bytes", "info"} and smp["bytes"] == data and smp["info"]["device"]
                assert (smp["info"]["h"], smp["info"]["w"]) == image.shape[:2]
                seen.add("baseline")
    assert seen == {"png", "progressive", "baseline"}


# ---- plans from headers ---------------------------------------------------------------------------------------------------------------------
def _plan_key(p):
    a = p.aug
    return (p.dataset, p.src_hw, p.rows, p.stage1, p.stage2, p.window, p.factor, a.flip, a.n_ops, tuple(a.ops), tuple(a.factor), a.hue_shift)


def test_draw_on_file_samples_gives_the_plans_of_the_decoded_arrays(tmp_path):
    from footprints_amd.datasets.device_path import SegBatchAssembler
    asm = SegBatchAssembler.__new__(SegBatchAssembler)                  # draw alone: the constructor needs a device
    from footprints_amd.preprocessing.segmentation.datasets import plan as P
    asm.P, asm.H, asm.W = P, *FEED
    for k, batch in enumerate(mixed_batches()):
        arrays, files = as_samples(batch, tmp_path / "a", False), as_samples(batch, tmp_path / "f", True)
        assert [isinstance(img, dict) for _, img, _ in files] == [True] * len(batch)
        assert ["bytes" in img for _, img, _ in files] == [kind != "parser" for *_, kind in batch]
        a, b = random.Random(MIXED_SEED + k), random.Random(MIXED_SEED + k)
        plans, ref = asm.draw(files, True, a), asm.draw(arrays, True, b)
        assert [_plan_key(p) for p in plans] == [_plan_key(p) for p in ref] and a.getstate() == b.getstate()
        if k == 0:                                                      # the GPU test's two-stage sample
            assert plans[4].dataset == "matterport" and plans[4].stage1 is not None and plans[4].stage2 is not None


# ---- the protocol, with a fake device ---------------------------------------------------------------------------------------------------------
class _Event:
    def record(self, stream=None):
        pass

    def query(self):
        return True

    def synchronize(self):
        pass


def _fake_assembler(B, decode, statuses, log, slots=2):
    """a SegBatchAssembler(device_decode=True) whose device is host memory: every pinned allocation, upload, queued decode, status read
    and half of the chain goes into `log` with the number of the batch its slot carries; statuses: {batch number: [status per file]}"""
    from footprints_amd.datasets.decode_stage import DecodeStage
    from footprints_amd.datasets.device_path import SegBatchAssembler

    class Stage(DecodeStage):
        def _pinned(self, n, dtype):
            log.append(("pinned", "stage", n))
            return torch.zeros(n, dtype=dtype)

        def _event(self):
            return _Event()

        def _upload(self, s, off, nbytes):
            log.append(("upload", s["k"], off, nbytes, s["h_src"].numpy()[off:off + nbytes].copy()))
            super()._upload(s, off, nbytes)

        def _decode(self, s, pack, batch):
            assert "rects" in pack and len(pack["rects"]) == pack["B"] == len(batch["on_device"])
            log.append(("decode", s["k"], [(batch["offsets"][b], batch["rects"][b]) for b in batch["on_device"]], dict(pack)))

        def _status(self, s, nd):
            log.append(("status", s["k"]))
            return np.asarray(statuses.get(s["k"], [0] * nd)[:nd])

    class Fake(SegBatchAssembler):
        filled = 0

        def _init_slots(self, device, stream):
            self.device, self.stream, self.slots, self._next = torch.device("cpu"), None, [], 0

        def _add_slot(self, **buffers):
            self.slots.append(dict(buffers, ready=_Event(), consumed=None, launched=False, k=None))
            return self.slots[-1]

        def _pair(self, s, name, n, dtype):
            log.append(("pinned", name, int(n)))
            s["h_" + name], s["d_" + name] = torch.zeros(int(n), dtype=dtype), torch.zeros(int(n), dtype=dtype)

        def _reserve(self, s, name, n):
            if n > s["h_" + name].numel():
                self._pair(s, name, n + n // 2, s["h_" + name].dtype)

        def _make_stage(self, decode):
            return Stage(self.B, self.H, self.W, None, "cpu", decode=decode)

        def _take_slot(self):
            i, s = super()._take_slot()
            s["k"] = self.filled
            log.append(("fill", self.filled))
            self.filled += 1
            return i, s

        def launch(self, i):                                            # SlotAssembler.launch without its stream
            self._launch(self.slots[i])
            self.slots[i]["launched"] = True
            return i

        def collect(self, slot):                                        # SegBatchAssembler.collect without its stream
            s = self.slots[slot]
            if s["batch"] is not None:
                self._repair(s)
            log.append(("collected", s["k"]))
            return s["k"]

        def release(self, slot):
            pass

        def _upload(self, s, name, lo, n):
            log.append(("upload other", s["k"], name))

        def _image_half(self, s):
            log.append(("image half", s["k"]))

        def _label_half(self, s):
            log.append(("label half", s["k"]))

    return Fake(B, FEED[0], FEED[1], max_src_hw=(100, 200), slots=slots, device_decode=True, decode=decode)


def test_the_assemblers_protocol_on_a_fake_device(tmp_path):
    from footprints_amd.datasets.decode_stage import host_decode
    batch = mixed_batches()[1]
    files = as_samples(batch, tmp_path, True)
    device = [n for n, (*_, kind) in enumerate(batch) if kind == "device"]
    log, calls = [], []
    asm = _fake_assembler(len(batch), lambda data: calls.append(data) or host_decode(data), {3: [0, 0, 2, 0, 0]}, log)
    assert asm.device_decode is True
    got = list(asm.loader([files] * 6, True, random.Random(2)))
    assert got == [0, 1, 2, 3, 4, 5]
    at = {e[:2]: n for n, e in enumerate(log) if e[0] in ("status", "collected", "fill")}
    queued = {e[1]: n for n, e in enumerate(log) if e[0] == "decode"}
    for k in range(6):
        assert queued[k] < at[("status", k)] < at[("collected", k)]
        if k < 5:
            assert queued[k + 1] < at[("status", k)], k                 # no status is read before the next batch's decode is queued
    # every batch: the uploads of the host frames' rectangles, the decode of the others into the gaps, both halves of the chain, once
    for k in range(6):
        mine = [e for e in log if e[0] in ("upload", "decode", "image half", "label half", "status", "collected") and e[1] == k]
        kinds = [e[0] for e in mine]
        first = kinds.index("decode")
        assert set(kinds[:first]) == {"upload"} and kinds[first:first + 3] == ["decode", "image half", "label half"]
        rest = kinds[first + 3:]
        assert rest == (["status", "upload", "image half", "collected"] if k == 3 else ["status", "collected"]), (k, rest)
        decode = mine[first]
        covered = sorted([(e[2], e[2] + e[3]) for e in mine[:first]] + [(off, off + r[2] * r[3] * 3) for off, r in decode[2]])
        assert covered[0][0] == 0 and all(a[1] == b[0] for a, b in zip(covered, covered[1:]))      # back to back: no overlap, no gap
        pack = decode[3]
        assert pack["B"] == len(device) and pack["max_win_h"] == max(r[2] for _, r in decode[2]) and pack["max_win_w"] == max(r[3] for _, r in decode[2])
        assert all(torch.is_tensor(pack[key]) for key in ("scans", "records", "tables"))           # the slot's buffers, not fresh arrays
    # batch 3: exactly the file with the non-zero status went to the injected decoder, once, and its RECTANGLE was repaired
    assert calls == [batch[device[2]][1]]
    decode3 = next(e for e in log if e[0] == "decode" and e[1] == 3)
    off, (y0, x0, rh, rw) = decode3[2][2]
    repair = [e for e in log if e[0] == "upload" and e[1] == 3][-1]
    assert repair[:4] == ("upload", 3, off, rh * rw * 3)
    want = G.pillow_decode(batch[device[2]][1])[y0:y0 + rh, x0:x0 + rw]
    assert np.array_equal(repair[4].reshape(rh, rw, 3), want)
    assert asm.counters == dict(device=6 * len(device) - 1, host_parser=6 * 2, host_status=1)
    # after the ring's first turn (two slots: where batch 2 is filled) nothing pinned is allocated
    second_turn = log.index(("fill", 2))
    assert [e for e in log[:second_turn] if e[0] == "pinned"] and not [e for e in log[second_turn:] if e[0] == "pinned"]


def test_a_file_sample_without_device_decode_is_refused(tmp_path):
    from footprints_amd.datasets.device_path import SegBatchAssembler

    class Bare(SegBatchAssembler):
        def __init__(self):                                             # fill's first checks alone: the constructor needs a device
            from footprints_amd.preprocessing.segmentation.datasets import plan as P
            self.P, self.B, self.H, self.W, self.device_decode = P, 7, FEED[0], FEED[1], False

        def _take_slot(self):
            return 0, {}

    asm = Bare()
    files = as_samples(mixed_batches()[0], tmp_path, True)
    with pytest.raises(ValueError, match="device_decode=True"):
        asm.fill(files, asm.draw(files, True, random.Random(1)))


# ---- honesty condition of the GPU tests -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(JPEGS))
def test_catalogue_frames_settle_well_inside_the_decoders_budget(name):
    """then a counter assertion on the GPU cannot be met by falling back: every file the tests count as `device` settles in half the budget"""
    from footprints_amd import ops
    data = jpeg_file(name)
    info = ops.jpeg_parse(data)
    assert info["device"] and (info["h"], info["w"]) == JPEGS[name][1:3]
    m = JR.model(data, ops.JPEG_DECODE_SUBSEQ_BITS)
    print(name, "launches", m["launches"], "hops", m["hops"], "nsub", m["nsub"])
    assert m["launches"] <= ops.JPEG_DECODE_MAX_ROUNDS / 2 and m["hops"] < JR.GROUP


def test_the_files_the_gpu_tests_count_as_turned_down_are_turned_down():
    from footprints_amd import ops
    assert not ops.jpeg_parse(progressive_file())["device"] and not ops.jpeg_parse(city_png())["device"]
    noise = ops.jpeg_parse(noise_frame())
    assert noise["device"] and JR.model(noise_frame(), ops.JPEG_DECODE_SUBSEQ_BITS)["launches"] > ops.JPEG_DECODE_MAX_ROUNDS
    kinds = [[kind for *_, kind in b] for b in mixed_batches()]
    assert kinds[0].count("status") == 1 and kinds[1].count("status") == 0
    assert {ops.jpeg_parse(f).get("hs", 0) * 2 + ops.jpeg_parse(f).get("vs", 0) for _, f, _, k in mixed_batches()[0] if k == "device"} == {3, 6}
    assert sum(ops.jpeg_parse(f)["ncomp"] == 1 for _, f, _, k in mixed_batches()[0] if k == "device") == 1
