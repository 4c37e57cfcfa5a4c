"""GPU: the segmentation trainer with --device_decode and --num_workers -- SegBatchAssembler(device_decode=True) over mixed batches of files
against the same batches decoded by Pillow (torch.equal, same draws), its counters, and two steps of the trainer from a tiny on-disk tree
with and without the flag and with and without the reader threads, bit for bit.  The files, and the proof that the device-decoded ones
cannot fall back unnoticed, are tests/test_seg_train_decode_cpu.py's."""
import random

import pytest
import torch

from tests.test_seg_train_decode_cpu import FEED, MIXED_SEED, as_samples, mixed_batches, write_seg_tree

pytestmark = pytest.mark.gpu


def _run(tmp_path, device_decode):
    """both mixed batches through one assembler behind a DeviceLoader -> ([batch dicts, cloned], [counters after each], the first plans)"""
    from footprints_amd.datasets.device_path import SegBatchAssembler
    batches = mixed_batches()
    B = len(batches[0])
    asm = SegBatchAssembler(B, FEED[0], FEED[1], max_src_hw=(100, 200), device_decode=device_decode, check=True)
    source = [as_samples(b, tmp_path / ("%s%d" % (device_decode, k)), device_decode) for k, b in enumerate(batches)]
    plans = asm.draw(source[0], True, random.Random(MIXED_SEED))
    out, counters = [], []
    for batch in asm.loader(source, True, random.Random(MIXED_SEED)):
        torch.cuda.synchronize()
        out.append({k: v.clone() for k, v in batch.items()})
        counters.append(asm.counters)
    return out, counters, plans


def test_a_mixed_batch_of_files_equals_the_batch_of_decoded_frames(tmp_path):
    kinds = [[kind for *_, kind in b] for b in mixed_batches()]
    host, host_counters, _ = _run(tmp_path, False)
    dev, dev_counters, plans = _run(tmp_path, True)
    assert plans[4].dataset == "matterport" and plans[4].stage1 is not None and plans[4].stage2 is not None      # a two-stage resize
    assert len(host) == len(dev) == 2
    for k in range(2):
        assert set(dev[k]) == {"image", "ground_mask", "labelled_pix"}
        for key in dev[k]:
            assert torch.equal(dev[k][key], host[k][key]), (k, key)
    assert not torch.equal(dev[0]["image"], dev[1]["image"])
    assert host_counters[-1] == dict(device=0, host_parser=0, host_status=0)
    # after the first batch: its baseline files bar the noise frame on the device, the noise frame again on the host.  The second batch
    # was filled by then (its parser refusals are counted) but not collected
    assert dev_counters[0] == dict(device=kinds[0].count("device"), host_parser=kinds[0].count("parser") + kinds[1].count("parser"), host_status=1)
    # the second batch holds no noise frame: the device turns nothing down that it should take
    assert dev_counters[1] == dict(device=kinds[0].count("device") + kinds[1].count("device"),
                                   host_parser=kinds[0].count("parser") + kinds[1].count("parser"), host_status=1)
    assert kinds[1].count("status") == 0 and kinds[1].count("device") == 5 and kinds[0].count("device") == 4


def _train(tmp_path, config, tag, extra, capsys):
    from footprints_amd.preprocessing.segmentation.network import Segmentor
    from footprints_amd.preprocessing.segmentation.options import SegmentationOptions
    from footprints_amd.preprocessing.segmentation.train import Trainer
    from oracle import restatement as R
    opts = SegmentationOptions().parse(["--height", str(FEED[0]), "--width", str(FEED[1]), "--batch_size", "6", "--log_freq", "1", "--epochs", "1",
                                        "--val_batches", "1", "--training_datasets", "ADE20K", "cityscapes", "matterport", "--config_path", config,
                                        "--log_path", str(tmp_path / "logs"), "--model_name", tag] + extra)
    P, Bf = R.make_seg_state(True, tag="segdecode")
    model = Segmentor(pretrained=False, use_PSP=True)
    model.load_state_dict({**P, **Bf})
    model.cuda()
    random.seed(17)
    trainer = Trainer(opts, model=model)
    trainer.train()
    torch.cuda.synchronize()
    assert trainer.step == 2 and len(trainer.history) == 2             # 12 train samples in batches of 6
    return trainer, {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}, capsys.readouterr().out


def test_two_steps_of_the_trainer_are_bit_equal_with_the_flag_and_with_the_reader_threads(tmp_path, monkeypatch, capsys):
    from footprints_amd.datasets.training import ThreadedBatchSource
    from footprints_amd.preprocessing.segmentation.datasets import BatchSource
    config = write_seg_tree(tmp_path, n=4)
    monkeypatch.chdir(tmp_path)
    runs = {tag: _train(tmp_path, config, tag, extra, capsys) for tag, extra in (
        ("plain", ["--num_workers", "0"]), ("threads", ["--num_workers", "2"]), ("device", ["--num_workers", "2", "--device_decode"]))}
    assert type(runs["plain"][0].train_loader.source) is BatchSource and type(runs["threads"][0].train_loader.source) is ThreadedBatchSource
    ref_trainer, ref_state, ref_out = runs["threads"]
    assert "frames decoded so far" not in ref_out
    for tag in ("plain", "device"):
        trainer, state, out = runs[tag]
        assert trainer.history == ref_trainer.history, tag              # tracked losses, batch loss, lr: floats, compared exactly
        assert set(state) == set(ref_state)
        for key in state:
            assert torch.equal(state[key], ref_state[key]), (tag, key)
    trainer, _, out = runs["device"]
    c = trainer.train_loader.counters
    # 12 train frames: 4 Cityscapes PNGs and one progressive ADE20K file through the parser's refusal, 7 baseline JPEGs on the device
    assert c == dict(device=7, host_parser=5, host_status=0)
    assert "Epoch 0 -- train frames decoded so far: device 7, host (parser) 5, host (status) 0" in out
    v = trainer.val_loader.counters
    assert v["host_status"] == 0 and v["device"] > 0 and "Epoch 0 -- val frames decoded so far" in out
