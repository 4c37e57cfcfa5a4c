"""Writes tests/golden/g20_baselines.npz: what the REFERENCE's own footprints/baselines/ransac.py and utils.py compute on the scenes of
tests/golden/baselines_inputs.py, plus the reference's own deviation from an extended-precision evaluation, which sets the tolerance
of the tests.

Needs the reference checkout (oracle/ref_import.py); run as `python -m tests.golden.make_golden_baselines` from the repository root.
Both modules need numpy only.  Per frame it follows RansacPlane.frame_predict -> ransac_depth_inpaint -> fit_plane with fit_plane's
constants and a fixed seed, records the rank triples run_ransac drew (replayed from the same seed), the model, best_ic and plane_depth,
and recomputes every hypothesis's inlier count with the reference's estimate / is_inlier.  A seed is rejected, and the next one tried,
unless (a) the winner's ranks are distinct and at most 2 of the 100 samples repeat a rank, and (b) no | |m . p| - 0.05 | over the
non-degenerate hypotheses and the masked points is below 1e-9, so that the integer counts are decided by the arithmetic and not by
rounding.  `dev_ref` is the largest relative difference of plane_depth between the reference's float64 evaluation with its SVD model
and an evaluation of the same winning triple in numpy.longdouble with the closed-form minors."""
import importlib
import os

import numpy as np

from oracle import ref_import
from tests import baselines_restatement as BR
from tests.golden import baselines_inputs as BI

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "g20_baselines.npz")
THRESHOLD, ITERATIONS = 0.05, 100            # ransac.fit_plane's constants
FIRST_SEED = 20


def reference_plane_depth(utils, ransac, depth, inv_K, mask, m):
    """footprint_baseline.ransac_depth_inpaint after fit_plane, with the reference's own functions"""
    xyz = utils.BackprojectDepth(*depth.shape)(depth, inv_K)
    rays = utils.generate_camera_rays(mask.shape[0], mask.shape[1], inv_K).T
    normalised_rays = rays / np.sqrt((rays ** 2).sum(1, keepdims=True))
    dot_product = np.sum(normalised_rays * m[:3][None, :], 1)
    extra = ransac.plane_distance(m, xyz) / dot_product
    return depth - extra.reshape(depth.shape)


def one_frame(utils, ransac, fr, seed):
    depth, inv_K = fr["depth"], fr["inv_K"]
    mask = fr["visible_ground"] > 0.5
    xyz = utils.BackprojectDepth(*depth.shape)(depth, inv_K)
    data = xyz[mask.ravel()]
    n = len(data)
    samples = BR.draw_samples(n, seed, ITERATIONS)
    model, best_ic, _ = ransac.run_ransac(data, ransac.estimate, lambda x, y: ransac.is_inlier(x, y, THRESHOLD), 3, ITERATIONS * 0.3, ITERATIONS,
                                          random_seed=seed)
    counts, degenerate, margin = np.zeros(ITERATIONS, np.int64), np.zeros(ITERATIONS, bool), np.inf
    for i, idx in enumerate(samples):
        degenerate[i] = len(set(int(k) for k in idx)) < 3
        m = ransac.estimate(data[idx, :])
        counts[i] = int(ransac.is_inlier(m, data, THRESHOLD).sum())
        if not degenerate[i]:
            margin = min(margin, float(np.abs(np.abs(ransac.plane_distance(m, data)) - THRESHOLD).min()))
    winner = int(np.argmax(counts))                                                   # first of the largest: run_ransac's `ic > best_ic`
    ok = not degenerate[winner] and degenerate.sum() <= 2 and margin >= 1e-9
    if not ok:
        return None
    assert counts[winner] == best_ic and np.array_equal(ransac.estimate(data[samples[winner], :]), model)
    assert counts[~degenerate].max() == counts[winner]
    plane_depth = reference_plane_depth(utils, ransac, depth, inv_K, mask, model)
    exact = BR.plane_depth(depth, inv_K, BR.estimate(data[samples[winner]].astype(np.longdouble), np.longdouble), np.longdouble)
    dev_ref = float((np.abs(plane_depth - exact) / np.abs(exact)).max())
    return {"depth": depth, "inv_K": inv_K, "visible_ground": fr["visible_ground"], "samples": samples, "model": model,
            "best_ic": np.int64(best_ic), "best_index": np.int64(winner), "counts": counts, "degenerate": degenerate, "plane_depth": plane_depth,
            "dev_ref": np.float64(dev_ref), "seed": np.int64(seed), "margin": np.float64(margin), "n": np.int64(n)}


def main():
    if ref_import.load_reference() is None:
        raise SystemExit("the reference checkout is not available")
    ransac = importlib.import_module("footprints.baselines.ransac")
    utils = importlib.import_module("footprints.baselines.utils")
    out = {}
    for k, (H, W) in enumerate(BI.SHAPES):
        fr = BI.frame(H, W, FIRST_SEED + k)
        for seed in range(FIRST_SEED, FIRST_SEED + 50):
            rec = one_frame(utils, ransac, fr, seed)
            if rec is not None:
                break
        else:
            raise SystemExit("no seed passes the fixture's conditions for %d x %d" % (H, W))
        print("%d x %d: %d masked points, seed %d, winner %d with %d inliers, %d degenerate samples, threshold margin %.2e, dev_ref %.2e" % (
            H, W, rec["n"], seed, rec["best_index"], rec["best_ic"], rec["degenerate"].sum(), rec["margin"], rec["dev_ref"]))
        out.update({"f%d.%s" % (k, key): v for key, v in rec.items()})
    np.savez_compressed(PATH, **out)
    print(PATH, os.path.getsize(PATH))


if __name__ == "__main__":
    main()
