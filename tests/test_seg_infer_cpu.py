"""The segmentation network's inference mode without a GPU: the NumPy restatement of fp_seg_pack against what the reference's own
Tester.test_batch, save_result and matplotlib wrote (tests/golden/g17_seg_infer.npz), the inference datasets' parsing and file layout,
the command line's way into Tester, and the pipeline's bookkeeping with a stub in place of the device side, in both schedules."""
import argparse
import os
import threading
import time

import numpy as np
import pytest

from tests import seg_infer_restatement as SR
from tests.golden import digest


@pytest.fixture(scope="module")
def g17():
    return digest.load("g17_seg_infer")


def _lut():
    from footprints_amd import ops
    return ops.vis_colour_table()


def test_restatement_reproduces_matplotlib_picture(g17):
    """[image | plasma(prediction)] through plt.imsave(format='png'), byte for byte, from the reference's own float32 predictions"""
    got = SR.picture(g17["preds"], g17["images"], _lut())
    assert got.dtype == np.uint8 and got.shape == g17["pictures"].shape
    assert np.array_equal(got, g17["pictures"])


def test_restatement_reproduces_float16_files(g17):
    """the .npy contents save_result wrote are to_half of the reference's float32 predictions, bit for bit -- subnormals included"""
    preds = g17["preds"]
    for i in range(preds.shape[0]):
        want = g17["npy.%d" % i]
        got = SR.to_half(preds[i])
        assert want.dtype == np.float16 and want.shape == got.shape == (1,) + preds.shape[2:]
        assert np.array_equal(got.view(np.uint16), want.view(np.uint16))
    halves = np.stack([g17["npy.%d" % i] for i in range(preds.shape[0])])
    sub = (halves > 0) & (halves < np.float16(6.104e-5))
    assert sub.any() and (halves == 0).any() and (halves == 1).any()          # the fixture does reach the subnormals and both ends


def test_restatement_sigmoid_against_reference_predictions(g17):
    """torch's CPU float32 sigmoid, which the reference ran, is within 4 ulp of the float64 sigmoid the restatement takes as the truth, for
    logits in [-30, 30] -- the range and the bound the kernel is held to (beyond it the float32 result is subnormal: the planted -100)"""
    r = SR.pack(g17["logits"], g17["images"], _lut())
    inside = np.abs(g17["logits"]) <= 30
    ulp = np.spacing(r["p64"].astype(np.float32)).astype(np.float64)
    assert inside.sum() >= inside.size - 2
    assert (np.abs(g17["preds"].astype(np.float64) - r["p64"])[inside] <= 4 * ulp[inside]).all()


def test_kitti_dataset_parsing_and_layout(g17, tmp_path):
    from footprints_amd.preprocessing.segmentation.datasets.inference import KITTIInferenceDataset
    names = [str(n) for n in g17["filenames"]]
    ds = KITTIInferenceDataset("/data/kitti", names, 8, 24)
    assert len(ds) == 2 and ds.image_ext == "jpg"
    assert ds._parse_index(0) == ("2011_09_26/2011_09_26_drive_0001_sync", "5", "image_02")
    assert ds._parse_index(1) == ("2011_09_28/2011_09_28_drive_0002_sync", "17", "image_03")
    assert ds.image_path(0) == "/data/kitti/2011_09_26/2011_09_26_drive_0001_sync/image_02/data/0000000005.jpg"
    assert KITTIInferenceDataset("/d", names, 8, 24, image_ext="png").image_path(1).endswith("image_03/data/0000000017.png")
    read = []
    ds.pil_loader = lambda path: read.append(path) or np.zeros((5, 7, 3), np.uint8)
    sample = ds[1]
    assert read == [ds.image_path(1)] and sample["idx"] == 1
    assert sample["image"].dtype == np.uint8 and sample["image"].shape == (5, 7, 3)          # native size: the resize is the device's
    pictures = g17["pictures"]
    for i in range(2):
        ds.save_result(i, SR.to_half(g17["preds"][i]), str(tmp_path), pictures[i])
    found = sorted(os.path.relpath(os.path.join(r, f), str(tmp_path)) for r, _, fs in os.walk(str(tmp_path)) for f in fs)
    assert found == sorted([str(p) for p in g17["npy_paths"]] + [str(p) for p in g17["jpg_paths"]])
    for i, rel in enumerate(str(p) for p in g17["npy_paths"]):
        got = np.load(os.path.join(str(tmp_path), rel))
        assert got.dtype == np.float16 and got.shape == (1, 8, 24)
        assert np.array_equal(got.view(np.uint16), g17["npy.%d" % i].view(np.uint16))
    from PIL import Image
    for rel, size in zip((str(p) for p in g17["jpg_paths"]), g17["jpg_sizes"]):
        with Image.open(os.path.join(str(tmp_path), rel)) as im:
            assert im.size[::-1] == tuple(size) == (8, 48)


def test_matterport_dataset_parsing_and_layout(tmp_path):
    """the class the reference cannot construct, built as meant: the image path of the trainer's Matterport reader and the file name
    ground_truth_generation's loader reads (`<scan>/data/<pos>_<height>_<direction>.npy`; the zero fill to 10 characters only shows on
    names shorter than Matterport's)"""
    from footprints_amd.preprocessing.segmentation.datasets.inference import INFERENCE_DATASETS, MatterportInferenceDataset
    pos = "0f37bd0737e349de9d536263a4bdd60d"
    ds = MatterportInferenceDataset("/data/mp", ["17DRP5sb8fy %s 1 3" % pos, "s p 2 4"], 8, 24)
    assert INFERENCE_DATASETS["matterport"] is MatterportInferenceDataset and len(ds) == 2
    assert ds.image_path(0) == "/data/mp/sample_dataset/v1/scans/17DRP5sb8fy/17DRP5sb8fy/matterport_color_images/%s_i1_3.jpg" % pos
    read = []
    ds.pil_loader = lambda path: read.append(path) or np.zeros((4, 6, 3), np.uint8)
    assert ds[0]["image"].shape == (4, 6, 3) and read == [ds.image_path(0)]
    pred = np.linspace(0, 1, 8 * 24, dtype=np.float32).reshape(1, 8, 24)
    ds.save_result(0, pred.astype(np.float16), str(tmp_path), np.zeros((8, 48, 3), np.uint8))
    ds.save_result(1, pred, str(tmp_path))
    got = np.load(os.path.join(str(tmp_path), "17DRP5sb8fy", "data", "%s_1_3.npy" % pos))
    assert got.dtype == np.float16 and got.shape == (1, 8, 24) and np.array_equal(got, pred.astype(np.float16))
    assert os.path.exists(os.path.join(str(tmp_path), "17DRP5sb8fy", "visualisations", "%s_1_3.jpg" % pos))
    short = np.load(os.path.join(str(tmp_path), "s", "data", "00000p_2_4.npy"))          # str(name).zfill(10), as for KITTI's frames
    assert short.dtype == np.float16 and not os.path.exists(os.path.join(str(tmp_path), "s", "visualisations"))


def test_main_inference_mode_reaches_tester(monkeypatch, capsys):
    """`--mode inference` constructs Tester(options) and calls test() (it raised NotImplementedError before)"""
    from footprints_amd.preprocessing.segmentation import inference, main as seg_main
    calls = []

    class FakeTester:
        def __init__(self, options):
            calls.append(("init", options))

        def test(self):
            calls.append(("test",))

    monkeypatch.setattr(inference, "Tester", FakeTester)
    seg_main.main(["--mode", "inference", "--test_data_type", "matterport", "--height", "64", "--width", "96", "--batch_size", "3",
                   "--save_test_visualisations", "--no_PSP", "--load_path", "weights.pth"])
    assert [c[0] for c in calls] == ["init", "test"]
    opt = calls[0][1]
    assert (opt.mode, opt.test_data_type, opt.height, opt.width, opt.batch_size) == ("inference", "matterport", 64, 96, 3)
    assert opt.save_test_visualisations and opt.no_PSP and opt.load_path == "weights.pth" and opt.test_save_folder == "ground_seg"
    assert "In inference mode!" in capsys.readouterr().out


# ---- the pipeline with a stub device half ----------------------------------------------------------------------------------------------
class _MemoryDataset:
    """frames in memory, results in memory; a frame is [2, 3, 3] filled with a function of its index"""

    def __init__(self, n, fail_at=None, slow_save=0.0):
        self.n, self.fail_at, self.slow_save = n, fail_at, slow_save
        self.saved, self.lock = [], threading.Lock()

    def __len__(self):
        return self.n

    def __getitem__(self, index):
        if index == self.fail_at:
            raise OSError("frame %d cannot be read" % index)
        return {"image": np.full((2, 3, 3), (index * 7 + 3) % 251, np.uint8), "idx": index}

    def save_result(self, index, prediction, savepath, visualisation=None):
        time.sleep(self.slow_save)
        with self.lock:
            self.saved.append((index, np.array(prediction), None if visualisation is None else np.array(visualisation), savepath))


class _StubRing:
    """the device side echoes a function of the frame into the slot's buffers; a slot refilled while the writer still owns it trips"""

    def __init__(self, owner):
        self.owner, self.stage = owner, None
        self.slots = [dict(half=np.zeros((owner.batch_size, 1, 2, 3), np.float16), pic=np.zeros((owner.batch_size, 2, 6, 3), np.uint8), frames=None)
                      for _ in range(owner.n_slots)]

    def ahead(self, si, samples):
        if self.owner.busy[si]:
            self.owner.trips.append(si)
        self.owner.busy[si] = True
        self.slots[si]["frames"] = [smp["image"] for smp in samples]

    def rest(self, si):
        s = self.slots[si]
        for j, f in enumerate(s["frames"]):
            s["half"][j] = np.float16(f[0, 0, 0]) / np.float16(256)
            s["pic"][j] = f[0, 0, 0]
        s["frames"] = None

    def collect(self, si, n):
        s = self.slots[si]
        return s["half"][:n], (s["pic"][:n] if self.owner.visualise else None)


def _stub_tester(dataset, batch_size=3, slots=2, visualise=True, num_workers=3, one_ahead=False):
    """one_ahead: the two-part schedule of --device_decode (batch k + 1's `ahead` before batch k's `rest`), on the same in-memory frames"""
    from footprints_amd.preprocessing.segmentation.inference import Tester

    class StubTester(Tester):
        def _new_ring(self):
            self.busy = [False] * self.n_slots
            self.trips = []
            return _StubRing(self)

        def _read(self, index):
            return self.dataset[index]

        def _release(self, free, si):         # the slot stops being busy exactly where the real writer hands it back
            self.busy[si] = False
            super()._release(free, si)

    opt = argparse.Namespace(height=2, width=3, batch_size=batch_size, num_workers=num_workers, save_test_visualisations=visualise,
                             device_decode=one_ahead)

    class Model:
        def eval(self):
            return self
    return StubTester(opt, model=Model(), dataset=dataset, save_path="/nowhere", slots=slots)


def test_pipeline_writes_every_index_once_with_its_own_data(one_ahead=False):
    """5 batches of 3 and a tail of 1 through 2 slots, the writer slower than the device half"""
    ds = _MemoryDataset(16, slow_save=0.002)
    t = _stub_tester(ds, one_ahead=one_ahead)
    t.test()
    assert sorted(s[0] for s in ds.saved) == list(range(16)) and t.trips == []
    for index, pred, vis, savepath in ds.saved:
        v = (index * 7 + 3) % 251
        assert savepath == "/nowhere" and pred.dtype == np.float16 and pred.shape == (1, 2, 3) and vis.shape == (2, 6, 3)
        assert (pred == np.float16(v) / np.float16(256)).all() and (vis == v).all()
    assert not [th for th in threading.enumerate() if th.name.startswith("seg-infer")]


def test_pipeline_without_pictures_and_workers_clamped(one_ahead=False):
    """the smallest ring: 1 slot, or the 2 slots that decoding one batch ahead needs"""
    ds = _MemoryDataset(4)
    t = _stub_tester(ds, batch_size=3, slots=2 if one_ahead else 1, visualise=False, num_workers=999, one_ahead=one_ahead)
    assert t.num_workers == 16
    t.test()
    assert sorted(s[0] for s in ds.saved) == [0, 1, 2, 3] and all(s[2] is None for s in ds.saved)


def test_pipeline_reader_error_ends_test(one_ahead=False):
    ds = _MemoryDataset(16, fail_at=7)
    t = _stub_tester(ds, one_ahead=one_ahead)
    with pytest.raises(OSError, match="frame 7"):
        t.test()
    assert not [th for th in threading.enumerate() if th.name.startswith("seg-infer")]          # nothing is left waiting
    assert all(s[0] < 6 for s in ds.saved)                                                      # batches in front of the failing one only


def test_pipeline_writer_error_ends_test(one_ahead=False):
    ds = _MemoryDataset(16)

    def save_result(index, prediction, savepath, visualisation=None):
        raise OSError("disk full")
    ds.save_result = save_result
    t = _stub_tester(ds, one_ahead=one_ahead)
    with pytest.raises(OSError, match="disk full"):
        t.test()
    assert not [th for th in threading.enumerate() if th.name.startswith("seg-infer")]


@pytest.mark.parametrize("check", [test_pipeline_writes_every_index_once_with_its_own_data, test_pipeline_without_pictures_and_workers_clamped,
                                   test_pipeline_reader_error_ends_test, test_pipeline_writer_error_ends_test],
                         ids=lambda check: check.__name__[len("test_pipeline_"):])
def test_pipeline_one_ahead(check):
    """the same four with the schedule both pipelines take with --device_decode: batch k + 1's `ahead` before batch k's `rest`"""
    check(one_ahead=True)
