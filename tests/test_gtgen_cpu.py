"""CPU: label generation -- the NumPy restatement (tests/gtgen_restatement.py) reproduces what the reference's own code computed
(fixture g13_gtgen, written by tests/golden/make_golden_gtgen.py), so that the GPU tests, which compare the kernels to the restatement,
mean something; host-side entry points and argument checks; code-object checks of the new kernels.  No kernel is launched here."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import gtgen_restatement as GR
from tests.golden import gtgen_inputs as GI
from tests.golden.digest import load

H, W = GI.H, GI.W


@pytest.fixture(scope="module")
def gold():
    return load("g13_gtgen")


def unpack(bits, shape=(H, W)):
    return np.unpackbits(bits)[: int(np.prod(shape))].reshape(shape).astype(bool)


def test_aggregate_reproduces_the_reference_medians_bit_for_bit(gold):
    P = gold["hd.projections"]
    for robust, key in ((True, "hd.median_robust"), (False, "hd.median_plain")):
        assert np.array_equal(GR.aggregate(P, robust).view(np.uint32), gold[key].view(np.uint32)), key
    n = (P > 0).sum(0)
    assert ((n > 0) & (n % 2 == 0)).any() and (n > 2).any() and ((n > 0) & (n <= 2)).any()      # even, odd, and filtered counts occur


def test_aggregate_equals_numpy_masked_median():
    rng = np.random.RandomState(3)
    P = (rng.rand(7, 16, 24).astype(np.float32) * 30) * (rng.rand(7, 16, 24) < 0.6)
    for robust in (True, False):
        F = P * ((P > 0).sum(0, keepdims=True) > 2) if robust else P
        ref = np.ma.median(np.ma.MaskedArray(F, mask=F == 0), axis=0).filled(0)
        assert np.array_equal(GR.aggregate(P, robust), ref.astype(np.float32))


def test_splat_reproduces_the_reference_from_its_own_coordinates(gold):
    """the reference's decisions (target pixel of every point) and, for three frames, its fp32 depths -> its projections, bit for bit:
    highest source index wins"""
    pix, frames = gold["hd.ref_pix"].astype(np.int64), gold["hd.ref_z_frames"]
    got = GR.scatter(pix[frames], gold["hd.ref_z"], H, W)
    assert np.array_equal(got.view(np.uint32), gold["hd.projections"][frames].view(np.uint32))
    collisions = sum((np.bincount(p[p >= 0], minlength=H * W) > 1).sum() for p in pix[frames])
    assert collisions > 100                                        # the rule was exercised


def test_restatement_from_raw_inputs_matches_wherever_rounding_cannot_decide(gold):
    """float64 warp of the raw inputs: the same decisions as the reference's fp32 run except at a few points; at every pixel none of
    those can reach, the same winner in every frame (its depth equal to fp32 rounding) and the same median to that precision"""
    data = GI.hidden_depth_inputs()
    cp = GR.warp(data["depths"], data["inv_intrinsics"], data["poses"], data["intrinsics"])
    pix64, pix32 = GR.decide(cp, H, W), gold["hd.ref_pix"].astype(np.int64)
    reach, diff = GR.differing_reach(pix32, pix64, H, W)
    assert diff.sum() / (pix64 >= 0).sum() == pytest.approx(float(gold["hd.differing_share"]))
    assert np.array_equal(reach.any(0), unpack(gold["hd.ref_excluded"], (H * W,)))
    assert reach.any(0).mean() <= 0.005
    # an infinite or NaN depth is an invalid point on both sides
    bad = ~np.isfinite(data["depths"].reshape(GI.B, -1))
    assert bad.sum() > 20 and (pix64[bad] == -1).all() and (pix32[bad] == -1).all()
    proj = GR.splat(cp, H, W).reshape(GI.B, -1)
    ref = gold["hd.projections"].reshape(GI.B, -1)
    ok = ~reach
    # the reference's depths deviate from float64 by at most the stored relative figure; rounding the float64 depth to fp32 and the
    # fp32 average of the two middle values add half an ulp each
    tol = float(gold["hd.deviation_uvz"][2]) + 2 * 2.0 ** -24
    assert np.array_equal(proj[ok] > 0, ref[ok] > 0)
    assert np.all(np.abs(proj[ok].astype(np.float64) - ref[ok]) <= tol * np.abs(ref[ok]))
    keep = ~reach.any(0)
    for robust, key in ((True, "hd.median_robust"), (False, "hd.median_plain")):
        med, want = GR.aggregate(proj.reshape(GI.B, H, W), robust).reshape(-1)[keep], gold[key].reshape(-1)[keep]
        assert np.array_equal(med > 0, want > 0)
        assert np.all(np.abs(med.astype(np.float64) - want) <= tol * np.abs(want))     # an order statistic moves no further than its inputs


def test_moving_mask_restatement_matches_the_reference(gold):
    mv = GI.moving_inputs()
    K, invK = GI.intrinsics()
    mask = unpack(gold["mv.mask"])
    assert 0.01 <= mask.mean() <= 0.5
    n64 = GR.moving_norm(mv["disparity"], mv["flow"], invK[None], mv["T"][None], K[None], mv["fx_baseline"])
    band = 4 * float(gold["mv.norm_deviation"])
    with np.errstate(invalid="ignore"):
        excluded = np.abs(n64 - 3) <= band
    assert excluded.mean() <= 0.01
    assert np.array_equal((n64 > 3)[~excluded], mask[~excluded])
    assert np.isnan(n64).sum() > 20 and not mask[np.isnan(n64)].any()                  # zero disparities: NaN compares false


def test_depth_mask_restatement_matches_the_reference_bit_for_bit(gold):
    dm = GI.depth_mask_inputs()
    K, invK = GI.intrinsics()
    ground = (dm["ground_seg"] > GI.FOOTPRINT_THRESHOLD).reshape(-1)
    samples = GI.draw_samples(int(ground.sum()))
    assert np.array_equal(samples, gold["dm.samples"])
    world = GR.project_to_world(dm["depth"][None], invK[None], np.float32)[0, :3].T
    planes, counts, best = GR.plane_scores(world, ground, samples)
    assert best == int(gold["dm.best"]) and counts[best] == int(gold["dm.best_count"])
    ref_plane = gold["dm.plane"]
    unit = lambda p: p / np.linalg.norm(p[:3])
    s = np.sign(np.dot(planes[best][:3], ref_plane[:3]))
    assert np.allclose(unit(planes[best]) * s, unit(ref_plane), atol=1e-9)             # the SVD null vector, up to scale and sign
    cp = GR.flatten_copies(world, ground, ref_plane, K)
    mask = GR.depth_mask_filter(GR.splat(cp, H, W)[0], dm["depth"], dm["ground_seg"])
    want = unpack(gold["dm.mask"])
    assert np.array_equal(mask, want) and 0.01 <= want.mean() <= 0.5
    assert len(GR.OFFSETS) == 8


def test_workspace_and_argument_checks_without_gpu():
    from footprints_amd import _lib, ops
    lib = _lib.load()
    assert lib.fp_gt_workspace(76, 192, 640) == 76 * 192 * 640 * 8
    assert ops.gt_workspace_bytes(1, 480, 640) == 480 * 640 * 8
    assert lib.fp_gt_workspace(512, 8, 8) == 512 * 64 * 8
    assert lib.fp_gt_workspace(513, 8, 8) == -1 and b"512" in lib.fp_last_error_string()
    assert lib.fp_gt_workspace(0, 8, 8) == -1
    # H * W * 64 must leave room for source_index + 1 in 32 bits
    assert lib.fp_gt_workspace(1, 8192, 8192) == -1 and b"2^32" in lib.fp_last_error_string()
    assert lib.fp_gt_workspace(1, 8192, 8191) == 8192 * 8191 * 8
    with pytest.raises(RuntimeError, match="512"):
        ops.gt_workspace_bytes(600, 192, 640)
    one = 1                                                                             # a non-null pointer nothing dereferences: the checks fail first
    assert lib.fp_gt_aggregate(one, 513, 8, 8, 1, one, None, None) == -1 and b"fp_gt_aggregate" in lib.fp_last_error_string()
    assert lib.fp_gt_warp_splat(one, one, one, one, 513, 8, 8, one, 1 << 40, None) == -1
    assert lib.fp_gt_warp_splat(one, one, one, one, 2, 8192, 8192, one, 1 << 40, None) == -1
    assert lib.fp_gt_warp_splat(None, one, one, one, 2, 8, 8, one, 1 << 20, None) == -1 and b"null" in lib.fp_last_error_string()
    assert lib.fp_gt_warp_splat(one, one, one, one, 2, 8, 8, one, 2 * 64 * 8 - 1, None) == -1 and b"key plane" in lib.fp_last_error_string()
    assert lib.fp_gt_splat(one, 2, 8, 8, None, 1 << 20, None) == -1
    assert lib.fp_gt_project(one, one, one, None, 2, 8, 8, one, None) == -1
    assert lib.fp_gt_aggregate(None, 2, 8, 8, 1, one, None, None) == -1
    assert lib.fp_gt_moving_mask(one, None, one, one, one, 1.0, 8, 8, one, None) == -1
    assert lib.fp_gt_plane_score(one, one, 0.75, one, 0, 8, 8, one, one, one, one, one, None, None) == -1
    assert lib.fp_gt_flatten_splat(one, one, 0.75, one, None, 8, 8, one, 1 << 20, None, None) == -1
    assert lib.fp_gt_depth_mask(one, one, one, 8, 8, None, None, None) == -1


def test_python_surface_refuses_cpu_tensors():
    from footprints_amd.preprocessing.ground_truth_generation import BatchProjector, GroundTruthGenerator, fit_plane, get_options

    class Gen(GroundTruthGenerator):
        height, width = 8, 8
    p = BatchProjector(8, 8)
    eye = torch.eye(4)[None]
    with pytest.raises(RuntimeError, match="no CPU path"):
        p.project_to_world(torch.ones(1, 8, 8), eye)
    with pytest.raises(RuntimeError, match="no CPU path"):
        p.project_to_camera(torch.ones(1, 4, 64), eye, eye)
    with pytest.raises(RuntimeError, match="no CPU path"):
        p.extract_depth_from_projections(torch.ones(1, 4, 64))
    with pytest.raises(RuntimeError, match="no CPU path"):
        fit_plane(torch.ones(4, 64), torch.ones(8, 8))
    gen = Gen(get_options([]), loader=None)
    with pytest.raises(RuntimeError, match="no CPU path"):
        gen.process_data({"depths": torch.ones(1, 8, 8), "poses": eye, "intrinsics": eye, "inv_intrinsics": eye})
    with pytest.raises(RuntimeError, match="no CPU path"):
        gen.compute_depth_mask(torch.ones(1, 8, 8), torch.ones(8, 8), eye, eye)


def test_options_equal_the_reference_flags():
    from oracle import ref_import
    if not ref_import.available():
        pytest.skip("the reference checkout is not on this machine")
    import sys
    from tests.golden.make_golden_gtgen import load_reference_gtgen
    from footprints_amd.preprocessing.ground_truth_generation import get_options
    saved_cuda = torch.Tensor.cuda
    try:
        _, generator = load_reference_gtgen()
    finally:
        torch.Tensor.cuda = saved_cuda
    argv, sys.argv = sys.argv, ["prog"]
    try:
        theirs = vars(generator.get_options())
    finally:
        sys.argv = argv
    assert vars(get_options([])) == theirs
    line = ["--type", "depth_masks", "--data_type", "matterport", "--idx_start", "3", "--footprint_threshold", "0.5", "--save_visualisations"]
    argv, sys.argv = sys.argv, ["prog"] + line
    try:
        theirs = vars(generator.get_options())
    finally:
        sys.argv = argv
    assert vars(get_options(line)) == theirs


def test_save_result_layout(tmp_path):
    from footprints_amd.preprocessing.ground_truth_generation import (KITTIGroundTruthGenerator, MatterportGroundTruthGenerator,
                                                                      get_options)
    arr = np.arange(6, dtype=np.float32).reshape(2, 3)
    k = KITTIGroundTruthGenerator(get_options([]), loader=None, training_datapath=str(tmp_path))
    k.save_result(arr, "2011_09_26/2011_09_26_drive_0001_sync 27 r")
    path = tmp_path / "hidden_depths" / "2011_09_26/2011_09_26_drive_0001_sync" / "image_03" / "data" / "0000000027.npy"
    assert np.array_equal(np.load(path), arr)
    m = MatterportGroundTruthGenerator(get_options(["--save_folder_name", "x"]), loader=None, training_datapath=str(tmp_path))
    m.save_result(arr, "scanA 12 1 3")
    assert np.array_equal(np.load(tmp_path / "x" / "scanA" / "data" / "000012_1_3.npy"), arr)


def test_new_kernels_keep_nothing_in_scratch(tmp_path):
    """No register spills and no private segment in any label-generation kernel -- the aggregation sorts up to 128 frames (KITTI: 76: the 80-frame
    instantiation) in registers and selects the median of larger stacks from the key plane, never from a per-lane array in memory -- and the splats use the
    native 64-bit unsigned max, not a compare-and-swap loop."""
    from footprints_amd import _lib
    objdump, readelf = "/opt/rocm/lib/llvm/bin/llvm-objdump", "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not (os.path.exists(objdump) and os.path.exists(readelf) and os.path.exists(_lib.LIB_PATH)):
        pytest.skip("llvm tools or the built library are not available")
    so = shutil.copy(_lib.LIB_PATH, tmp_path / "lib.so")
    subprocess.run([objdump, "--offloading", str(so)], cwd=tmp_path, check=True, capture_output=True)
    expected = {"gt_project_kernel", "gt_world_kernel", "gt_camera_kernel", "gt_splat_kernel", "gt_warp_splat_kernel", "gt_aggregate_sorted_kernelILi80E",
                "gt_aggregate_sorted_kernelILi128E", "gt_aggregate_select_kernel", "gt_moving_mask_kernel", "gt_ground_count_kernel", "gt_plane_build_kernel", "gt_plane_score_kernel",
                "gt_plane_select_kernel", "gt_inlier_mask_kernel", "gt_flatten_splat_kernel", "gt_depth_mask_kernel"}
    seen = {}
    for pth in tmp_path.iterdir():
        if not pth.name.endswith("gfx950"):
            continue
        notes = subprocess.run([readelf, "--notes", str(pth)], check=True, capture_output=True, text=True).stdout
        if "gt_warp_splat_kernel" not in notes:
            continue
        for record in notes.split("- .agpr_count:")[1:]:           # one record per kernel, its fields in alphabetical order
            fields = {}
            for line in record.splitlines():
                line = line.strip()
                if line.startswith(".name:"):
                    fields["name"] = line.split(":", 1)[1].strip()
                elif line.startswith((".vgpr_spill_count:", ".sgpr_spill_count:", ".private_segment_fixed_size:", ".group_segment_fixed_size:")):
                    fields[line.split(":")[0]] = int(line.split(":")[1])
            if "gt_" in fields.get("name", ""):
                seen[fields["name"]] = fields
        asm = subprocess.run([objdump, "-d", str(pth)], check=True, capture_output=True, text=True).stdout
        assert asm.count("global_atomic_umax_x2") >= 3 and "cmpswap" not in asm
    for want in expected:
        hits = [n for n in seen if want in n]
        assert hits, want
        for n in hits:
            assert seen[n][".vgpr_spill_count"] == 0 and seen[n][".sgpr_spill_count"] == 0, (n, seen[n])
            assert seen[n][".private_segment_fixed_size"] == 0, (n, seen[n])
    # the sorting aggregation holds its frames in registers; LDS only parks the lower half of the sorted values, one column per lane
    lds = {n: seen[n][".group_segment_fixed_size"] for n in seen if "gt_aggregate_sorted_kernel" in n}
    assert sorted(lds.values()) == [(cap // 2 + 1) * 64 * 4 for cap in (8, 32, 48, 80, 128)]
