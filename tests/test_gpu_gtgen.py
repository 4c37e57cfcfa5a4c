"""GPU: label generation (csrc/gt_gen.hip) against the NumPy restatement (tests/gtgen_restatement.py) and the reference's own results
(fixture g13_gtgen).  tests/test_gtgen_cpu.py pins the restatement to the reference; nothing here reads the reference.

Where a comparison cannot be exact the bound comes from the fixture: make_golden_gtgen.py measured how far the reference's own fp32
run is from float64 on the same inputs, and the device gets 4x that (it orders the 4-term sums differently and does not fuse)."""
import os
import types

import numpy as np
import pytest
import torch

from tests import gtgen_restatement as GR
from tests.golden import gtgen_inputs as GI
from tests.golden.digest import load

pytestmark = pytest.mark.gpu
H, W = GI.H, GI.W
EPS32 = 2.0 ** -24


@pytest.fixture(scope="module")
def gold():
    return load("g13_gtgen")


@pytest.fixture(scope="module")
def ops():
    from footprints_amd import ops
    return ops


def dev(x, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x))
    return (t.to(dtype) if dtype is not None else t).cuda()


def unpack(bits, shape=(H, W)):
    return np.unpackbits(bits)[: int(np.prod(shape))].reshape(shape).astype(bool)


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def device_data(data):
    return {k: dev(v) for k, v in data.items()}


def fused(ops, d, robust, want_projections=False):
    B, h, w = d["depths"].shape
    keys = ops.gt_warp_splat(d["depths"], d["inv_intrinsics"], d["poses"], d["intrinsics"])
    return keys, ops.gt_aggregate(keys, h, w, robust, want_projections=want_projections)


def staged(ops, d, robust):
    B, h, w = d["depths"].shape
    cam_pix = ops.gt_project(d["depths"], d["inv_intrinsics"], d["poses"], d["intrinsics"])
    keys = ops.gt_splat(cam_pix, h, w)
    return cam_pix, keys, ops.gt_aggregate(keys, h, w, robust)


# ---- 4. warp arithmetic --------------------------------------------------------------------------------------------------------------
def test_project_matches_float64_within_four_times_the_reference_deviation(gold, ops):
    data = GI.hidden_depth_inputs()
    cp = ops.gt_project(dev(data["depths"]), dev(data["inv_intrinsics"]), dev(data["poses"]), dev(data["intrinsics"])).cpu().numpy()
    cp64 = GR.warp(data["depths"], data["inv_intrinsics"], data["poses"], data["intrinsics"])
    ok = (GR.decide(cp, H, W) >= 0) & (GR.decide(cp64, H, W) >= 0)
    du = np.abs(cp[:, 0] - cp64[:, 0])[ok].max()
    dv = np.abs(cp[:, 1] - cp64[:, 1])[ok].max()
    dz = (np.abs(cp[:, 2] - cp64[:, 2]) / np.abs(cp64[:, 2]))[ok].max()
    ref = gold["hd.deviation_uvz"]
    print("device vs float64: |du| %.3e |dv| %.3e rel |dz| %.3e; reference fp32 vs float64: %s" % (du, dv, dz, ref))
    assert ok.sum() > 50000
    assert du <= 4 * ref[0] and dv <= 4 * ref[1] and dz <= 4 * ref[2]
    # infinite / NaN depths: invalid on both sides, and the coordinates are NaN as in the reference (not clamped, not zeroed)
    bad = ~np.isfinite(data["depths"].reshape(GI.B, -1))
    assert bad.sum() > 20 and (GR.decide(cp, H, W)[bad] == -1).all() and (GR.decide(cp64, H, W)[bad] == -1).all()
    assert np.isnan(cp[:, 0][bad]).all()
    # the two halves on their own compose to the same bits
    world = ops.gt_project_to_world(dev(data["depths"]), dev(data["inv_intrinsics"]))
    cp2 = ops.gt_project_to_camera(world, dev(data["poses"]), dev(data["intrinsics"])).cpu().numpy()
    assert np.array_equal(bits(cp2), bits(cp))
    w64 = GR.project_to_world(data["depths"], data["inv_intrinsics"])
    fin = np.isfinite(w64)
    assert np.allclose(world.cpu().numpy()[fin], w64[fin], rtol=1e-6, atol=3e-5)          # three roundings of terms up to 60 m x 2


# ---- 5. splat and aggregate are exact ------------------------------------------------------------------------------------------------
def adversarial_cam_pix(B, h, w, seed):
    rng = np.random.RandomState(seed)
    N = h * w
    u = rng.uniform(-2, w + 2, (B, N)).astype(np.float32)
    v = rng.uniform(-2, h + 2, (B, N)).astype(np.float32)
    z = rng.uniform(0.5, 40, (B, N)).astype(np.float32)
    c3 = np.ones((B, N), np.float32)
    crowd = rng.rand(B, N) < 0.5                                   # half of the points into a 6 x 5 corner: many collisions
    u[crowd] = rng.uniform(0, 6, crowd.sum())
    v[crowd] = rng.uniform(0, 5, crowd.sum())
    whole = rng.rand(B, N) < 0.2                                   # integer coordinates, the borders included
    u[whole] = rng.randint(0, w + 1, whole.sum())
    v[whole] = np.round(v[whole])
    u[:, 0:N:97], u[:, 1:N:97] = 0.0, float(w)
    v[:, 2:N:97], v[:, 3:N:97] = 0.0, float(h)
    u[:, 13:N:97] = np.nextafter(np.float32(w), np.float32(0))    # the last representable column position
    z[:, 4:N:97], z[:, 5:N:97], z[:, 6:N:97] = 0.0, -1.0, np.nan
    c3[:, 7:N:97], c3[:, 8:N:97] = 0.0, -1.0
    u[:, 9:N:97], v[:, 10:N:97] = np.nan, np.inf
    z[:, 11:N:97] = np.inf                                         # a valid depth, and the largest one
    z[:, 12:N:97] = z[:, 14:N:97]                                  # equal depths in one frame
    z[rng.rand(B, N) < 0.3] = np.float32(7.25)                     # and across frames: ties in the median
    return np.stack([u, v, z, c3], 1)


@pytest.mark.parametrize("B", [1, 2, 3, 4, 8, 9, 32, 33, 48, 49, 76, 77, 80, 81, 128, 129, 512])      # every tier of the aggregation, both sides
def test_splat_and_aggregate_equal_the_restatement_bit_for_bit(B, ops):
    h, w = 24, 40
    cp = adversarial_cam_pix(B, h, w, seed=B)
    want_proj = GR.splat(cp, h, w)
    keys = ops.gt_splat(dev(cp), h, w)
    for robust in (True, False):
        med, proj = ops.gt_aggregate(keys, h, w, robust, want_projections=True)
        assert np.array_equal(bits(proj.cpu().numpy()), bits(want_proj)), "projections"
        assert np.array_equal(bits(med.cpu().numpy()), bits(GR.aggregate(want_proj, robust))), "median robust=%s" % robust
    n = (want_proj > 0).sum(0)
    assert (n > 0).any() and (B < 3 or (n > 2).any())
    # the key's high word is the winner's source index + 1
    k = keys.cpu().numpy().view(np.uint64).reshape(B, -1)
    pix = GR.decide(cp, h, w)
    for b in range(min(B, 3)):
        last = np.full(h * w, -1, np.int64)
        keep = np.flatnonzero(pix[b] >= 0)
        np.maximum.at(last, pix[b][keep], keep)
        assert np.array_equal((k[b] >> np.uint64(32)).astype(np.int64), last + 1)


def test_aggregate_reproduces_the_fixture_medians_from_the_fixture_projections(gold, ops):
    """keys written from the reference's projections (source index 0): the device's medians equal the reference's bit for bit"""
    P = gold["hd.projections"]
    keys = dev(bits(P).astype(np.int64).reshape(GI.B, -1))
    for robust, key in ((True, "hd.median_robust"), (False, "hd.median_plain")):
        med, proj = ops.gt_aggregate(keys, H, W, robust, want_projections=True)
        assert np.array_equal(bits(proj.cpu().numpy()), bits(P))
        assert np.array_equal(bits(med.cpu().numpy()), bits(gold[key])), key


@pytest.mark.parametrize("B", [5, 80, 128, 200])
def test_aggregate_treats_any_key_plane_like_the_comparison_does(B, ops):
    """low words that no splat writes (negative, -0, NaN, denormal, the largest finite value): a frame counts exactly when `depth > 0`"""
    h, w = 16, 32
    rng = np.random.RandomState(100 + B)
    special = np.array([0x00000000, 0x80000000, 0x7F800000, 0x7F800001, 0x7FC00000, 0xFF800000, 0xFFC00000, 0x00000001, 0x007FFFFF, 0x7F7FFFFF,
                        0xBF800000, 0x3F800000], np.uint32)
    low = special[rng.randint(0, len(special), (B, h * w))]
    rnd = rng.rand(B, h * w) < 0.5
    low[rnd] = rng.uniform(0.1, 50, rnd.sum()).astype(np.float32).view(np.uint32)
    keys = (rng.randint(1, 1 << 20, (B, h * w)).astype(np.int64) << 32) | low.astype(np.int64)
    P = low.view(np.float32).reshape(B, h, w)
    for robust in (True, False):
        med, proj = ops.gt_aggregate(dev(keys), h, w, robust, want_projections=True)
        assert np.array_equal(proj.cpu().numpy().view(np.uint32), P.view(np.uint32))
        assert np.array_equal(bits(med.cpu().numpy()), bits(GR.aggregate(P, robust)))


# ---- 6. fused = staged ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(GI.B, GI.H, GI.W), (76, 192, 640), (40, 480, 640)])
def test_fused_equals_staged_bit_for_bit(shape, ops):
    d = device_data(GI.hidden_depth_inputs(*shape))
    robust = shape[1] == 192 or shape[0] == GI.B
    keys_f, med_f = fused(ops, d, robust)
    _, keys_s, med_s = staged(ops, d, robust)
    assert torch.equal(keys_f, keys_s)
    assert torch.equal(med_f.view(torch.int32), med_s.view(torch.int32))
    assert (med_f > 0).float().mean().item() > 0.05
    keys_again, _ = fused(ops, d, robust)                          # atomics in another order: the same keys
    assert torch.equal(keys_again, keys_f)


# ---- 7. end to end under the device's own decisions ----------------------------------------------------------------------------------
def test_end_to_end_under_the_devices_own_decisions(gold, ops):
    data = GI.hidden_depth_inputs()
    d = device_data(data)
    cp = ops.gt_project(d["depths"], d["inv_intrinsics"], d["poses"], d["intrinsics"]).cpu().numpy()
    proj_r = GR.splat(cp, H, W)
    out = {}
    for robust in (True, False):
        _, (med, proj) = fused(ops, d, robust, want_projections=True)
        out[robust] = med.cpu().numpy()
        assert np.array_equal(bits(proj.cpu().numpy()), bits(proj_r))
        assert np.array_equal(bits(out[robust]), bits(GR.aggregate(proj_r, robust)))
    # decisions against the float64 run
    cp64 = GR.warp(data["depths"], data["inv_intrinsics"], data["poses"], data["intrinsics"])
    pix_d, pix64 = GR.decide(cp, H, W), GR.decide(cp64, H, W)
    reach, diff = GR.differing_reach(pix_d, pix64, H, W)
    share = diff.sum() / (pix64 >= 0).sum()
    print("decisions differing from float64: %d of %d valid points (%.2e; reference fp32: %.2e)" % (
        diff.sum(), (pix64 >= 0).sum(), share, float(gold["hd.differing_share"])))
    assert share <= 4 * float(gold["hd.differing_share"])
    # against the reference's medians: the same contributing points at every pixel that no differing point (the device's or the
    # reference's own) reaches, so the medians agree to the precision of the depths -- an order statistic moves no further than its
    # inputs: the device's depths are within 4x and the reference's within 1x the stored deviation of float64, and the fp32 average of
    # the two middle values rounds once on each side
    excluded = reach.any(0) | unpack(gold["hd.ref_excluded"], (H * W,))
    print("pixels excluded: %.4f %%" % (100 * excluded.mean()))
    assert excluded.mean() <= 0.02
    tol = 5 * float(gold["hd.deviation_uvz"][2]) + 2 * EPS32
    for robust, key in ((True, "hd.median_robust"), (False, "hd.median_plain")):
        got, want = out[robust].reshape(-1)[~excluded], gold[key].reshape(-1)[~excluded]
        assert np.array_equal(got > 0, want > 0), key
        assert np.all(np.abs(got.astype(np.float64) - want) <= tol * np.abs(want)), key
        assert (want > 0).mean() > 0.1
    keep = ~(reach | unpack(gold["hd.ref_excluded"], (H * W,))[None])
    assert np.array_equal(proj_r.reshape(GI.B, -1)[keep] > 0, gold["hd.projections"].reshape(GI.B, -1)[keep] > 0)


# ---- 8. moving mask ------------------------------------------------------------------------------------------------------------------
def test_moving_mask_equals_the_fixture_outside_the_band(gold, ops):
    mv = GI.moving_inputs()
    K, invK = GI.intrinsics()
    mask = ops.gt_moving_mask(dev(mv["disparity"]), dev(mv["flow"], torch.float32), dev(invK[None]), dev(mv["T"][None]), dev(K[None]),
                              mv["fx_baseline"]).cpu().numpy()
    want = unpack(gold["mv.mask"])
    assert 0.01 <= want.mean() <= 0.5
    n64 = GR.moving_norm(mv["disparity"], mv["flow"], invK[None], mv["T"][None], K[None], mv["fx_baseline"])
    band = 4 * float(gold["mv.norm_deviation"])
    with np.errstate(invalid="ignore"):
        excluded = np.abs(n64 - 3) <= band
    print("moving mask: %d pixels differ from the fixture, %d inside the band of %.2e" % ((mask != want).sum(), excluded.sum(), band))
    assert excluded.mean() <= 0.01
    assert np.array_equal(mask[~excluded], want[~excluded])
    assert not mask[np.isnan(n64)].any() and np.isnan(n64).sum() > 20


# ---- 9. depth mask -------------------------------------------------------------------------------------------------------------------
def depth_mask_case():
    dm = GI.depth_mask_inputs()
    K, invK = GI.intrinsics()
    return dm, K, invK, (dm["ground_seg"] > GI.FOOTPRINT_THRESHOLD).reshape(-1)


def test_plane_scoring_picks_the_fixture_candidate(gold, ops):
    dm, K, invK, ground = depth_mask_case()
    world = ops.gt_project_to_world(dev(dm["depth"][None]), dev(invK[None]))[0]
    seg = dev(dm["ground_seg"])
    assert int(ops.gt_ground_count(seg, GI.FOOTPRINT_THRESHOLD).item()) == int(ground.sum())
    r = ops.gt_plane_score(world, seg, GI.FOOTPRINT_THRESHOLD, dev(gold["dm.samples"]), want_inlier_mask=True)
    world_xyz = world.cpu().numpy()[:3].T
    planes, counts, best = GR.plane_scores(world_xyz, ground, gold["dm.samples"])
    assert np.array_equal(r["sample_pix"].cpu().numpy(), np.flatnonzero(ground)[gold["dm.samples"]])
    assert np.array_equal(r["planes"].cpu().numpy(), planes)                      # float64, unfused: the same bits
    assert np.array_equal(r["counts"].cpu().numpy(), counts)
    assert r["best"].cpu().tolist() == [int(gold["dm.best"]), int(gold["dm.best_count"])] and best == int(gold["dm.best"])
    assert np.array_equal(r["best_plane"].cpu().numpy(), planes[best])
    inl = np.zeros(H * W, bool)
    inl[ground] = np.abs(GR.plane_distance(planes[best], world_xyz[ground])) < GR.INLIER_THRESHOLD
    assert np.array_equal(r["inlier_mask"].cpu().numpy().reshape(-1), inl)
    # degenerate samples score 0 and never win; out-of-range ranks likewise
    samples = gold["dm.samples"].copy()
    samples[0] = [5, 5, 9]
    samples[1] = [int(ground.sum()), 1, 2]
    r2 = ops.gt_plane_score(world, seg, GI.FOOTPRINT_THRESHOLD, dev(samples))
    c2 = r2["counts"].cpu().numpy()
    assert c2[0] == 0 and c2[1] == 0 and np.array_equal(c2[2:], counts[2:]) and not r2["planes"][:2].cpu().numpy().any()
    assert r2["sample_pix"].cpu().numpy()[1, 0] == -1


def test_depth_mask_equals_the_restatement_on_the_devices_coordinates_and_the_fixture(gold, ops):
    dm, K, invK, ground = depth_mask_case()
    depth, seg = dev(dm["depth"]), dev(dm["ground_seg"])
    world = ops.gt_project_to_world(depth[None], dev(invK[None]))[0]
    # the reference's own plane (its SVD's scale and sign): v1 = n x (0,0,1) follows the normal's sign, so the fixture's mask does too
    plane = dev(gold["dm.plane"])
    keys, cp = ops.gt_flatten_splat(world, seg, GI.FOOTPRINT_THRESHOLD, dev(K[None]), plane, want_cam_pix=True)
    mask, proj = ops.gt_depth_mask(keys, depth, seg, want_projection=True)
    mask, proj, cp = mask.cpu().numpy(), proj.cpu().numpy(), cp.cpu().numpy()[None]
    # (a) under the device's own coordinates: exact
    proj_r = GR.splat(cp, H, W)[0]
    assert np.array_equal(bits(proj), bits(proj_r))
    assert np.array_equal(mask, GR.depth_mask_filter(proj_r, dm["depth"], dm["ground_seg"]))
    assert np.isnan(cp[0, 0].reshape(64, -1)[:, ground]).all()                    # ground pixels have no copies
    # (b) the fixture: outside the pixels a point can reach whose decision differs from the float64 projection (the device's points or
    # the reference's own) and outside the band of the 10 % / 30 m comparisons
    world_xyz = world.cpu().numpy()[:3].T
    cp64 = GR.flatten_copies(world_xyz, ground, gold["dm.plane"], K, np.float64)
    pix64 = GR.decide(cp64, H, W)
    reach, diff = GR.differing_reach(GR.decide(cp, H, W), pix64, H, W)
    proj64 = GR.scatter(pix64, cp64[:, 2], H, W)[0]
    band = 4 * max(float(gold["dm.deviation_uvz"][2]), EPS32)
    excluded = reach[0].reshape(H, W) | unpack(gold["dm.ref_excluded"]) | GR.filter_band(proj64, dm["depth"], band)
    want = unpack(gold["dm.mask"])
    print("depth mask: %d pixels differ from the fixture, %.3f %% excluded, %d copies decided differently from float64" % (
        (mask != want).sum(), 100 * excluded.mean(), diff.sum()))
    assert excluded.mean() <= 0.02
    assert 0.01 <= want.mean() <= 0.5
    assert np.array_equal(mask[~excluded], want[~excluded])
    # the device's own candidate is the same plane up to scale and sign
    r = ops.gt_plane_score(world, seg, GI.FOOTPRINT_THRESHOLD, dev(gold["dm.samples"]))
    own = r["best_plane"].cpu().numpy()
    unit = lambda p: p / np.linalg.norm(p[:3])
    assert np.allclose(unit(own) * np.sign(np.dot(own[:3], gold["dm.plane"][:3])), unit(gold["dm.plane"]), atol=1e-9)


def stub_options(**kw):
    from footprints_amd.preprocessing.ground_truth_generation import get_options
    o = get_options([])
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def test_frame_with_99_ground_pixels_gives_zeros(ops):
    from footprints_amd.preprocessing.ground_truth_generation import KITTIDepthMaskingGenerator, MatterportDepthMaskingGenerator
    dm, K, invK, ground = depth_mask_case()
    seg = np.zeros((H, W), np.float32)
    seg.reshape(-1)[np.flatnonzero(ground)[:99]] = 0.9
    loader = types.SimpleNamespace(K=K, invK=invK, stereo_baseline=GI.STEREO_BASELINE)

    class Small(KITTIDepthMaskingGenerator):
        height, width = H, W
    gen = Small(stub_options(), loader)
    disparity = (np.float32(float(K[0, 0]) * GI.STEREO_BASELINE) / dm["depth"]).astype(np.float32)
    res = gen.process_data({"disparity": dev(disparity), "ground_seg": dev(seg)})
    assert res.shape == (H, W) and not res.any()
    seg.reshape(-1)[np.flatnonzero(ground)[99]] = 0.9              # the 100th ground pixel: the mask is computed
    np.random.seed(1)
    res = gen.process_data({"disparity": dev(disparity), "ground_seg": dev(seg)})
    assert res.dtype == bool and res.shape == (H, W)

    class SmallM(MatterportDepthMaskingGenerator):
        height, width = H, W
    seg.reshape(-1)[np.flatnonzero(ground)[99]] = 0.0
    res = SmallM(stub_options(), None).process_data({"depth": dev(dm["depth"][None]), "ground_seg": dev(seg), "intrinsics": dev(K[None]),
                                                     "inv_intrinsics": dev(invK[None])})
    assert res.shape == (H, W) and not res.any()


# ---- 10. the generator classes -------------------------------------------------------------------------------------------------------
def test_generators_process_device_tensors_through_a_stub_loader(gold, ops, tmp_path):
    from footprints_amd.preprocessing.ground_truth_generation import (BatchProjector, KITTIDepthMaskingGenerator, KITTIGroundTruthGenerator,
                                                                      KITTIMovingObjectDetector, MatterportGroundTruthGenerator, fit_plane)
    K, invK = GI.intrinsics()
    loader = types.SimpleNamespace(K=K, invK=invK, stereo_baseline=GI.STEREO_BASELINE, buffer={}, purge_buffer=lambda: None)
    data = GI.hidden_depth_inputs()

    class HD(KITTIGroundTruthGenerator):
        height, width = H, W

    class MP(MatterportGroundTruthGenerator):
        height, width = H, W
    gen = HD(stub_options(), loader, training_datapath=str(tmp_path))
    assert gen.robust_aggregation is True and MP(stub_options(), loader).robust_aggregation is False
    d = device_data(data)
    res = gen.process_data(d, robust_aggregation=True)
    _, med = fused(ops, d, True)
    assert res.dtype == np.float32 and res.shape == (H, W) and np.array_equal(bits(res), bits(med.cpu().numpy()))
    plain = MP(stub_options(), loader).process_data(d, robust_aggregation=False)
    assert np.array_equal(bits(plain), bits(fused(ops, d, False)[1].cpu().numpy())) and (plain > 0).sum() > (res > 0).sum()
    gen.save_result(res, "seq/drive 7 l")
    assert np.array_equal(np.load(tmp_path / "hidden_depths" / "seq/drive" / "image_02" / "data" / "0000000007.npy"), res)
    # the projector's reference-shaped methods compose to the same projections as the fused path
    p = BatchProjector(H, W)
    cam_pix = p.project_to_camera(p.project_to_world(d["depths"], d["inv_intrinsics"]), d["poses"], d["intrinsics"])
    proj = p.extract_depth_from_projections(cam_pix)
    assert tuple(cam_pix.shape) == (GI.B, 4, H * W) and tuple(proj.shape) == (GI.B, H, W)
    assert torch.equal(proj, ops.gt_aggregate(fused(ops, d, True)[0], H, W, True, want_projections=True)[1])

    class MV(KITTIMovingObjectDetector):
        height, width = H, W
    mv = GI.moving_inputs()
    det = MV(stub_options(), loader)
    assert det.save_folder == "moving_object_masks"
    m1 = det.process_data({"base_data": {"pose": mv["base_pose"], "disparity": dev(mv["disparity"]), "flow": dev(mv["flow"], torch.float32)},
                           "lookup_data": {"pose": mv["lookup_pose"]}})
    m2 = det.process_data({"base_data": {"pose": mv["base_pose"], "disparity": mv["disparity"], "flow": mv["flow"]},
                           "lookup_data": {"pose": mv["lookup_pose"]}})                # arrays, as a loader gives them
    direct = ops.gt_moving_mask(dev(mv["disparity"]), dev(mv["flow"], torch.float32), dev(invK[None]), dev(mv["T"][None]), dev(K[None]),
                                mv["fx_baseline"]).cpu().numpy()
    assert m1.dtype == bool and np.array_equal(m1, direct) and np.array_equal(m2, direct)

    class DM(KITTIDepthMaskingGenerator):
        height, width = H, W
    dm, _, _, ground = depth_mask_case()
    dmg = DM(stub_options(), loader)
    assert dmg.save_folder == "depth_masks"
    disparity = np.float32(float(K[0, 0]) * GI.STEREO_BASELINE) / dm["depth"]
    np.random.seed(GI.SAMPLE_SEED)                                  # the host's stream: the fixture's samples are drawn
    res = dmg.process_data({"disparity": dev(disparity.astype(np.float32)), "ground_seg": dev(dm["ground_seg"])})
    assert res.dtype == bool and res.shape == (H, W) and 0.01 <= res.mean() <= 0.5
    # fit_plane draws from the same stream and finds the fixture's candidate
    world = p.project_to_world(dev(dm["depth"][None]), dev(invK[None]))
    np.random.seed(GI.SAMPLE_SEED)
    plane, count, inliers = fit_plane(world, dev(dm["ground_seg"]), GI.FOOTPRINT_THRESHOLD)
    assert count == inliers.sum().item() == int(gold["dm.best_count"]) and tuple(inliers.shape) == (H, W) and plane.dtype == torch.float64
    with pytest.raises(RuntimeError, match="no CPU path"):
        gen.process_data({k: v.cpu() for k, v in d.items()})
