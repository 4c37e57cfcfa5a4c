"""CPU: the stretched-map pictures without a device -- the two numpy restatements against the reference's own `log`
(tests/golden/g_seg_log.npz), against matplotlib's imsave and its recorded bytes (tests/golden/g_stretch.npz); the JPEG header with a
density; the tolerance band of the device test confirmed on its inputs; and the surface: symbols, option parsers, and the generalised
PanelLogger run with a host stand-in renderer."""
import io
import os
import re

import numpy as np
import pytest

from tests import event_file_reader as ER
from tests import seg_log_restatement as SR
from tests import stretch_restatement as ST

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
LOSS_KEYS = ["ground_loss_0", "ground_loss_1", "ground_loss_2", "ground_loss_3", "loss"]


def _have_matplotlib():
    try:
        import matplotlib  # noqa: F401
        return True
    except ImportError:
        return False


# ---- the reference's log ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n", [("b2", 2), ("b12", 10), ("constant", 1)])
def test_seg_log_restatement_reproduces_the_reference_log(name, n):
    """the fixture is the reference's own `log` run with a recording writer (tests/golden/make_golden_seg_log.py): tags in order, the
    scalar names and values, and its float pictures turned to bytes by tensorboardX's rule"""
    g = np.load(os.path.join(GOLDEN, "g_seg_log.npz"))
    inputs = {k[len(name) + 4:]: g[k] for k in g.files if k.startswith(name + ".in.") and not k.endswith(".logits")}
    logits = g[name + ".in.logits"]
    assert list(g[name + ".tags"]) == SR.tags(n)                                   # ten pictures of a batch of twelve
    assert list(g[name + ".scalar_tags"]) == LOSS_KEYS + ["learning rate"]
    assert list(g[name + ".scalars"]) == [0.25, 0.5, 0.75, 1.0, 1.25, 1e-4]
    want = g[name + ".pictures"]
    H, W = logits.shape[2:]
    assert want.shape == (n, H, 3 * W, 3) and want.dtype == np.uint8
    got = SR.to_bytes(SR.float_parts(inputs, logits))
    assert np.array_equal(got, want)
    if name == "constant":                                                         # denom = 1e5: the image panel is black
        assert (got[0, :, :W] == 0).all()
    table = SR.byte_table()
    assert table.shape == (256, 3) and len({tuple(c) for c in table}) == 256
    from footprints_amd import ops
    assert np.array_equal(ops.colour_table("plasma", "float32"), table) and ops.colour_table("plasma", "float32") is ops.colour_table("plasma", "float32")
    with pytest.raises(ValueError):
        ops.colour_table("plasma", "rounded")


# ---- imsave -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ST.cases()))
def test_stretch_restatement_is_the_recorded_imsave(name):
    g = np.load(os.path.join(GOLDEN, "g_stretch.npz"))
    x = ST.cases()[name]
    assert np.array_equal(g[name + ".in"], x) and g[name + ".in"].dtype == x.dtype
    assert np.array_equal(ST.rgb(x), g[name + ".rgb"])
    from footprints_amd import ops
    assert np.array_equal(ops.colour_table("viridis", "bytes"), ST.byte_table())


@pytest.mark.skipif(not _have_matplotlib(), reason="matplotlib is not installed")
@pytest.mark.parametrize("name", list(ST.cases()))
def test_stretch_restatement_is_what_imsave_writes(name):
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    x = ST.cases()[name]
    buf = io.BytesIO()
    plt.imsave(buf, x, format="jpg")
    assert buf.getvalue() == ST.pillow_file(ST.rgb(x))


# ---- the JPEG header ------------------------------------------------------------------------------------------------------------------------
def test_jpeg_tables_with_a_density_differ_in_the_density_bytes_alone():
    from PIL import Image
    from footprints_amd import ops
    before95 = ops.jpeg_tables(95).header
    plain, dense = ops.jpeg_tables(75), ops.jpeg_tables(75, dpi=(100, 100))
    assert ops.jpeg_tables(75, dpi=(100, 100)) is dense and ops.jpeg_tables(75) is plain and ops.jpeg_tables(75, None) is plain
    assert ops.jpeg_tables(95).header == before95
    a, b = plain.header, dense.header
    assert len(a) == len(b) and a[2:4] == b"\xff\xe0" and a[6:11] == b"JFIF\0"
    differing = [i for i in range(len(a)) if a[i] != b[i]]
    assert differing and set(differing) <= set(range(13, 18))                      # JFIF: units at 13, x density 14-15, y density 16-17
    assert b[13] == 1 and b[14:18] == bytes((0, 100, 0, 100))
    assert np.array_equal(plain.words, dense.words) and plain.size_at == dense.size_at
    # today's bytes without a density: the dummy's own header
    buf = io.BytesIO()
    Image.fromarray(np.zeros((16, 16, 3), np.uint8)).save(buf, format="JPEG", quality=75)
    assert buf.getvalue().startswith(plain.header)
    buf = io.BytesIO()
    Image.fromarray(np.zeros((16, 16, 3), np.uint8)).save(buf, format="JPEG", quality=75, dpi=(100, 100))
    assert buf.getvalue().startswith(dense.header)
    assert ops.jpeg_files(b"\x01\x02", np.array([[0, 2], [2, 0]]), [(5, 7)], 75, dpi=(100, 100)) == [dense.file_header(5, 7) + b"\x01\x02\xff\xd9"]
    assert ops.jpeg_files(b"\x01\x02", np.array([[0, 2], [2, 0]]), [(5, 7)], 75) == [plain.file_header(5, 7) + b"\x01\x02\xff\xd9"]


# ---- the band of the device test ------------------------------------------------------------------------------------------------------------
def test_float32_and_float64_restatements_stay_under_the_device_cap():
    """the cap of the device test, confirmed on the host for its inputs: on the prediction panel, the only one that goes through an
    exponential, the float32 index differs from the float64 one on at most 1 % of a panel's pixels and never by more than one"""
    from tests.test_gpu_stretch_map import SEG_CASES
    for case, kw in SEG_CASES.items():
        inputs, logits = SR.make_inputs(**kw)
        p32 = SR.float_parts(inputs, logits)
        p64 = SR.float_parts(inputs, logits, dtype=np.float64)
        assert len(p32) == min(10, kw["B"])
        for (_, _, a), (_, _, b) in zip(p32, p64):
            ia = np.minimum(np.floor(SR.index_scaled(a).astype(np.float64)), 255)
            ib = np.minimum(np.floor(SR.index_scaled(b)), 255)
            d = np.abs(ia - ib)
            assert d.max() <= 1 and (d > 0).mean() <= 0.01, (case, d.max(), (d > 0).mean())


# ---- surface -------------------------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("fp_seg_log_panels_workspace", "fp_seg_log_panels", "fp_stretch_colour_workspace", "fp_stretch_colour")


def test_header_binding_and_library_agree_on_the_new_symbols():
    from footprints_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "footprints_hip.h")).read()
    declared = set(re.findall(r"\b(fp_[a-z0-9_]+)\s*\(", hdr))
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    # host-side answers need no device: the workspace is one (min, max) pair of floats per 1024 pixels and sample
    assert lib.fp_seg_log_panels_workspace(10, 192, 640) == 10 * 120 * 8 and lib.fp_stretch_colour_workspace(1, 5, 7) == 8
    assert lib.fp_seg_log_panels_workspace(0, 5, 7) == -1 and lib.fp_stretch_colour_workspace(1, 0, 7) == -1
    assert lib.fp_seg_log_panels(4096, 4096, 4096, 35, 4096, 4096, 2, 3, 5, 7, 4096, 1 << 20, None) == -1          # n > B
    assert b"bad sizes" in lib.fp_last_error_string()
    assert lib.fp_seg_log_panels(4096, 4096, 4096, 34, 4096, 4096, 2, 2, 5, 7, 4096, 1 << 20, None) == -1          # stride < H * W
    assert b"stride" in lib.fp_last_error_string()
    assert lib.fp_stretch_colour(4096, 0, 4096, 4096, 1, 5, 7, 4096, 4, None) == -1
    assert b"workspace too small" in lib.fp_last_error_string()
    makefile = open(os.path.join(ROOT, "footprints_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\bstretch_map\.hip\b", makefile, re.M)
    assert re.search(r"^stretch_map\.o:.*\n\t.*-ffp-contract=off", makefile, re.M)


def test_both_option_parsers_take_the_new_flags():
    from footprints_amd.preprocessing.ground_truth_generation.ground_truth_generator import get_options
    from footprints_amd.preprocessing.segmentation.options import SegmentationOptions
    assert SegmentationOptions().parse([]).no_summaries is False and SegmentationOptions().parse(["--no_summaries"]).no_summaries is True
    base = ["--data_type", "kitti", "--type", "hidden_depths"]
    off, on = get_options(base), get_options(base + ["--save_visualisations", "--device_jpeg"])
    assert off.save_visualisations is False and "device_jpeg" not in vars(off)          # the namespace without the flag is the reference's
    assert (on.save_visualisations, on.device_jpeg) == (True, True)
    text = SegmentationOptions().parser.format_help() + " ".join(open(os.path.join(
        ROOT, "footprints_amd", "preprocessing", "ground_truth_generation", "ground_truth_generator.py")).read().split())
    assert "images are not written" not in text


def test_seg_logger_with_a_host_renderer_writes_the_reference_event(tmp_path):
    """the generalised PanelLogger: scalars and picture shape from the caller.  Every loss under its own name, then `learning rate`, then
    the pictures [H, 3 W, 3]; ten of a batch of twelve; two events in order through the two slots"""
    import torch
    from footprints_amd.preprocessing.segmentation.logger import SegPanelLogger, log
    from footprints_amd.training.summary import SummaryWriter
    B, H, W = 12, 8, 12
    inputs, logits = SR.make_inputs(B, H, W, seed=9)
    t_inputs, t_logits = {k: torch.from_numpy(v) for k, v in inputs.items()}, torch.from_numpy(logits)
    losses = {k: torch.tensor(0.5 + i) for i, k in enumerate(LOSS_KEYS)}
    writer = SummaryWriter(str(tmp_path / "a"))
    logger = SegPanelLogger(panels=SR.render)
    logger.log(writer, t_inputs, [None, None, None, t_logits], losses, 1e-4, 3)
    log(writer, t_inputs, {"ground": t_logits}, losses, 2e-4, 4, num_outputs=2, logger=logger)
    logger.close()
    writer.close()
    assert logger.events == 2
    _, got = ER.read_log(writer.path)
    want = SR.to_bytes(SR.float_parts(inputs, logits))
    first, second = got[:6 + 10], got[6 + 10:]
    assert [(s, t) for s, t, _ in first] == [(3, k) for k in LOSS_KEYS + ["learning rate"] + SR.tags(10)]
    assert [(s, t) for s, t, _ in second] == [(4, k) for k in LOSS_KEYS + ["learning rate"] + SR.tags(2)]
    assert [v for _, _, v in first[:6]] == [0.5, 1.5, 2.5, 3.5, 4.5, np.float32(1e-4)] and second[5][2] == np.float32(2e-4)
    for (_, _, pic), w in zip(first[6:] + second[6:], list(want) + list(want[:2])):
        assert pic.shape == (H, 3 * W, 3) and np.array_equal(pic, w)
    # without a logger of its own the call writes before it returns; a renderer that fails surfaces at close
    def broken(inputs, logits, n=10, out=None):
        raise FloatingPointError("renderer")
    bad = SegPanelLogger(panels=broken)
    bad.log(writer, t_inputs, t_logits, losses, 1e-4, 5)
    with pytest.raises(FloatingPointError):
        bad.close()
