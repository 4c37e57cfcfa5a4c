"""NumPy restatement of the training-label generation (warp, splat, median, moving-object mask, depth mask).

Test infrastructure: written from the semantics the kernels of footprints_amd/csrc/gt_gen.hip implement, in float64 unless a
dtype is asked for, and pinned to the reference's own results by tests/test_gtgen_cpu.py (fixture g13_gtgen).

Layouts: depths [B,H,W]; matrices [B,4,4]; cam_pix [B,4,N] = u, v, z, c3; a *decision* is the target pixel `v_int * W + u_int`
of a point, or -1 when the point is invalid.
"""
import numpy as np

N_CANDIDATES = 100                      # RANSAC iterations of the reference's fit_plane
INLIER_THRESHOLD = 0.05
OFFSETS = np.arange(-0.1, 0.1, 0.025)   # the 8 x 8 splat offsets, exactly the reference's expression


def pixel_grid(H, W, dtype=np.float64):
    x, y = np.meshgrid(np.arange(W), np.arange(H))
    return np.stack([x.reshape(-1), y.reshape(-1), np.ones(H * W)]).astype(dtype)


def project_to_world(depths, inv_intrinsics, dtype=np.float64):
    """[B,H,W] -> [B,4,H*W]: (invK[:3,:3] . (x, y, 1)) * d, homogeneous coordinate (d > 0)"""
    B, H, W = depths.shape
    d = np.asarray(depths).reshape(B, 1, -1).astype(dtype)
    iK = np.asarray(inv_intrinsics).astype(dtype)[:, :3, :3]
    g = pixel_grid(H, W, dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        rays = (iK[:, :, 0:1] * g[0] + iK[:, :, 1:2] * g[1]) + iK[:, :, 2:3] * g[2]
        w = rays * d
    m = (d > 0).astype(dtype)
    return np.concatenate([w, m], 1)


def _mat4(M, p):
    return ((M[:, :, 0:1] * p[:, 0:1] + M[:, :, 1:2] * p[:, 1:2]) + M[:, :, 2:3] * p[:, 2:3]) + M[:, :, 3:4] * p[:, 3:4]


def project_to_camera(world, poses, intrinsics, dtype=np.float64):
    """[B,4,N] -> cam_pix [B,4,N]: K . (T . world), u and v divided by (z + 1e-7)"""
    T, K = np.asarray(poses).astype(dtype), np.asarray(intrinsics).astype(dtype)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        c = _mat4(K, _mat4(T, np.asarray(world).astype(dtype)))
        den = c[:, 2:3] + dtype(1e-7)
        return np.concatenate([c[:, :2] / den, c[:, 2:]], 1)


def warp(depths, inv_intrinsics, poses, intrinsics, dtype=np.float64):
    return project_to_camera(project_to_world(depths, inv_intrinsics, dtype), poses, intrinsics, dtype)


def decide(cam_pix, H, W):
    """target pixel of every point, -1 for the invalid ones (strict comparisons; NaN fails every one)"""
    u, v, z, c3 = (cam_pix[:, i] for i in range(4))
    with np.errstate(invalid="ignore"):
        valid = (u > 0) & (u < W) & (v > 0) & (v < H) & (z > 0) & (c3 > 0)
        ui = np.where(valid, u, 0).astype(np.int64)
        vi = np.where(valid, v, 0).astype(np.int64)
    return np.where(valid, vi * W + ui, -1)


def scatter(pix, z, H, W):
    """decisions [B,N] and depths [B,N] -> projections [B,H,W] fp32; of several points in one pixel the highest index wins"""
    B, N = pix.shape
    out = np.zeros((B, H * W), np.float32)
    for b in range(B):
        keep = np.flatnonzero(pix[b] >= 0)
        last = np.full(H * W, -1, np.int64)
        np.maximum.at(last, pix[b][keep], keep)
        hit = last >= 0
        out[b, hit] = np.asarray(z[b], np.float32)[last[hit]]
    return out.reshape(B, H, W)


def splat(cam_pix, H, W):
    return scatter(decide(cam_pix, H, W), cam_pix[:, 2], H, W)


def aggregate(projections, robust):
    """[B,H,W] fp32 -> [H,W] fp32: 0 unless more than 2 (robust) / 0 frames are positive, else the mean of the two middle positive
    values, fp32"""
    P = np.asarray(projections, np.float32)
    B, H, W = P.shape
    flat = P.reshape(B, -1)
    with np.errstate(invalid="ignore"):
        pos = flat > 0
    n = pos.sum(0)
    s = np.sort(np.where(pos, flat, np.float32(np.inf)), axis=0)           # the n positive values first, ascending
    cols = np.arange(flat.shape[1])
    lo = s[np.maximum(n - 1, 0) // 2, cols]
    hi = s[np.minimum(n // 2, B - 1), cols]
    with np.errstate(invalid="ignore", over="ignore"):
        med = ((lo + hi) * np.float32(0.5)).astype(np.float32)
    return np.where(n > (2 if robust else 0), med, np.float32(0)).reshape(H, W)


def differing_reach(pix_a, pix_b, H, W):
    """pixels [B,H*W] that a point whose decision differs between two runs can reach in either run"""
    B = pix_a.shape[0]
    reach = np.zeros((B, H * W), bool)
    diff = pix_a != pix_b
    for b in range(B):
        for pix in (pix_a[b], pix_b[b]):
            t = pix[diff[b]]
            reach[b, t[t >= 0]] = True
    return reach, diff


def moving_norm(disparity, flow, inv_intrinsics, pose, intrinsics, fx_baseline, dtype=np.float64):
    """norm of (induced flow - given flow) [H,W]; the mask is `norm > 3`.  With an fp32 dtype the coordinates are fp32 and the
    differences float64, as in the reference (its flow is a float64 array)."""
    H, W = disparity.shape
    with np.errstate(divide="ignore", invalid="ignore"):
        depth = (dtype(fx_baseline) / np.asarray(disparity).astype(dtype)).reshape(1, H, W)
    cp = warp(depth, inv_intrinsics, pose, intrinsics, dtype)[0, :2].reshape(2, H, W)
    x, y = np.meshgrid(np.arange(W), np.arange(H))
    with np.errstate(invalid="ignore"):
        ind = np.stack([(cp[0] - x.astype(dtype)), (cp[1] - y.astype(dtype))]).astype(np.float64)
        diff = ind - np.asarray(flow, np.float64)
        return np.sqrt(diff[0] * diff[0] + diff[1] * diff[1])


def plane_from_points(p0, p1, p2):
    """float64 plane through three points: normal (p1 - p0) x (p2 - p0), d = -n . p0; all zero when degenerate"""
    p0, p1, p2 = (np.asarray(p, np.float64) for p in (p0, p1, p2))
    a, b = p1 - p0, p2 - p0
    n = np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])
    d = -((n[0] * p0[0] + n[1] * p0[1]) + n[2] * p0[2])
    nn = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]
    if not (nn > 0 and np.isfinite(nn) and np.isfinite(d)):
        return np.zeros(4)
    return np.array([n[0], n[1], n[2], d])


def plane_distance(plane, xyz):
    """signed distances of xyz [N,3] (fp32 values, float64 arithmetic)"""
    xyz = np.asarray(xyz, np.float64)
    norm = np.sqrt((plane[0] * plane[0] + plane[1] * plane[1]) + plane[2] * plane[2])
    with np.errstate(invalid="ignore", over="ignore"):
        return (((plane[0] * xyz[:, 0] + plane[1] * xyz[:, 1]) + plane[2] * xyz[:, 2]) + plane[3]) / norm


def plane_scores(world_xyz, ground, samples):
    """world_xyz [H*W,3] fp32, ground bool [H*W], samples [C,3] indices into the ground points -> (planes [C,4], counts [C], best)
    counts are over the ground points, as in the reference (its RANSAC runs on `world_points[ground_pix]`)"""
    g = np.asarray(world_xyz)[ground]
    planes = np.stack([plane_from_points(*g[idx]) for idx in samples])
    counts = np.zeros(len(samples), np.int64)
    for c, pl in enumerate(planes):
        if pl[:3].any():
            with np.errstate(invalid="ignore"):
                counts[c] = int((np.abs(plane_distance(pl, g)) < INLIER_THRESHOLD).sum())
    best = int(np.argmax(counts)) if counts.max() > 0 else -1          # argmax: the first of the largest
    return planes, counts, best


def flatten_copies(world_xyz, ground, plane, K, proj_dtype=np.float32):
    """cam_pix [1,4,64*H*W] (fp32; float64 projection of the same fp32 points when `proj_dtype` says so) of the 8 x 8 offset copies of every point flattened onto `plane` (copy k of pixel p at k*H*W + p);
    copies of ground pixels are NaN: they do not exist in the reference's list"""
    xyz = np.asarray(world_xyz, np.float64)
    norm = np.sqrt((plane[0] * plane[0] + plane[1] * plane[1]) + plane[2] * plane[2])
    n = plane[:3] / norm
    dist = plane_distance(plane, xyz)
    with np.errstate(invalid="ignore", over="ignore"):
        flat = xyz - n.reshape(1, 3) * dist.reshape(-1, 1)
    flat = np.concatenate([flat, np.ones((len(flat), 1))], 1)
    v1, v2 = np.zeros(4), np.zeros(4)
    v1[:3] = np.cross(n, np.array([0, 0, 1]))
    v2[:3] = np.cross(n, v1[:3])
    pts = []
    with np.errstate(invalid="ignore", over="ignore"):
        for d1 in OFFSETS:
            for d2 in OFFSETS:
                pts.append((flat + v1.reshape(1, 4) * d1) + v2.reshape(1, 4) * d2)
    pts = np.concatenate(pts, 0).T.astype(np.float32)[None]             # [1,4,64*HW]
    # the reference hands K over as the pose and the identity as the intrinsics
    cp = project_to_camera(pts, np.asarray(K, np.float32).reshape(1, 4, 4), np.eye(4, dtype=np.float32)[None], proj_dtype)
    cp[:, :, np.tile(np.asarray(ground, bool), len(OFFSETS) ** 2)] = np.nan
    return cp


def depth_mask_filter(projection, depth, ground_seg):
    pr, d, g = np.asarray(projection, np.float32), np.asarray(depth, np.float32), np.asarray(ground_seg, np.float32)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        rel = np.abs(pr - d) / (d + np.float32(1e-7))
        return (pr > 0) & (g < np.float32(0.5)) & (rel < np.float32(0.10)) & (pr < 30) & (d > 0)


def filter_band(projection, depth, rel_band):
    """pixels whose 10 % / 30 m comparisons a relative change of `rel_band` in the projected depth can flip"""
    pr, d = np.asarray(projection, np.float64), np.asarray(depth, np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        rel = np.abs(pr - d) / (d + 1e-7)
        return (pr > 0) & ((np.abs(rel - 0.10) <= rel_band * (1 + pr / np.maximum(d, 1e-30))) | (np.abs(pr - 30) <= 30 * rel_band))
