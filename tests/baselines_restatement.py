"""Independent host restatement of footprints_amd/csrc/baselines.hip, in numpy / scipy.

The hull restates skimage.morphology.convex_hull_image with its defaults (offset_coordinates=True, tolerance=1e-10): Qhull over the
foreground pixels' four half-pixel offset points, then `equations @ p + b < tolerance` on every facet for every pixel centre.
skimage is not installed where this suite runs: the semantics are restated from skimage's documented behaviour and its published
source, and are NOT pinned by a run of skimage itself.

The RANSAC path restates footprints/baselines/ransac.py and footprint_baseline.ransac_depth_inpaint in float64, with the closed-form
null vector (the 3 x 3 minors of the augmented sample matrix) in place of numpy.linalg.svd; tests/golden/g20_baselines.npz pins it to a
run of the reference's own modules."""
import numpy as np

INLIER_THRESHOLD = 0.05            # ransac.fit_plane
ITERATIONS = 100
MIN_POINTS = 20                    # RansacPlane.frame_predict


def hull(mask, tolerance=1e-10):
    """mask bool / uint8 [H,W] -> bool [H,W]; an empty mask gives zeros (safe_convex_hull_image's `im * 0`)"""
    from scipy.spatial import ConvexHull
    mask = np.asarray(mask) != 0
    if not mask.any():
        return np.zeros(mask.shape, bool)
    coords = np.argwhere(mask).astype(np.float64)
    offsets = np.array([[0.5, 0.0], [-0.5, 0.0], [0.0, 0.5], [0.0, -0.5]])
    points = np.unique((coords[:, None, :] + offsets[None]).reshape(-1, 2), axis=0)
    eq = ConvexHull(points).equations                                       # [facets, 3]: normal . p + offset <= 0 inside
    grid = np.mgrid[0:mask.shape[0], 0:mask.shape[1]].reshape(2, -1).astype(np.float64)
    inside = np.all(eq[:, :2] @ grid + eq[:, 2:] < tolerance, axis=0)
    return inside.reshape(mask.shape)


def bounding_box_mask(visible_ground, bounding_box):
    """BoundingBox.frame_predict over the restated hull"""
    vis = visible_ground > 0.5
    out = hull(vis)
    out[bounding_box < 0.5] = 0
    out[vis == 1] = 1
    return out


def backproject(depth, inv_K):
    """utils.BackprojectDepth: [H*W, 3] float64, and the rays inv_K . (x, y, 1) as [H*W, 3]"""
    H, W = depth.shape
    x, y = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    pix = np.stack([x.ravel(), y.ravel(), np.ones(H * W)])
    rays = (np.asarray(inv_K, np.float64)[:3, :3] @ pix).T
    return depth.reshape(-1, 1).astype(np.float64) * rays, rays


def estimate(p, dtype=np.float64):
    """unit 4-vector spanning the null space of [p_i, 1] (i = 0, 1, 2), closed form; zeros when the minors vanish"""
    p = np.asarray(p, dtype)
    a, b = p[1] - p[0], p[2] - p[0]
    n = np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], dtype)
    m = np.array([n[0], n[1], n[2], -(n[0] * p[0, 0] + n[1] * p[0, 1] + n[2] * p[0, 2])], dtype)
    if not (n * n).sum() > 0:
        return np.zeros(4, dtype)
    return m / np.sqrt((m * m).sum())


def plane_distance(m, xyz):
    return xyz @ m[:3] + m[3]


def plane_fit(depth, inv_K, mask, samples):
    """-> planes [C,4], counts [C], (best index, best count): a sample that repeats a rank or has a rank out of range scores 0"""
    xyz, _ = backproject(depth, inv_K)
    data = xyz[np.asarray(mask).ravel()]
    C = len(samples)
    planes, counts = np.zeros((C, 4)), np.zeros(C, np.int64)
    for c, idx in enumerate(np.asarray(samples)):
        if len(set(int(i) for i in idx)) < 3 or idx.min() < 0 or idx.max() >= len(data):
            continue
        planes[c] = estimate(data[idx])
        if planes[c].any():
            counts[c] = int((np.abs(plane_distance(planes[c], data)) < INLIER_THRESHOLD).sum())
    best, best_count = -1, 0
    for c in range(C):
        if counts[c] > best_count:
            best, best_count = c, int(counts[c])
    return planes, counts, (best, best_count)


def plane_depth(depth, inv_K, m, dtype=np.float64):
    """footprint_baseline.ransac_depth_inpaint's last lines, at every pixel"""
    H, W = depth.shape
    x, y = np.meshgrid(np.arange(W), np.arange(H))
    pix = np.stack([x.ravel(), y.ravel(), np.ones(H * W)]).astype(dtype)
    rays = (np.asarray(inv_K, dtype)[:3, :3] @ pix).T
    d = depth.reshape(-1, 1).astype(dtype)
    m = np.asarray(m, dtype)
    normalised = rays / np.sqrt((rays ** 2).sum(1, keepdims=True))
    dot = (normalised * m[:3][None]).sum(1)
    dist = (d * rays) @ m[:3] + m[3]
    return depth.astype(dtype) - (dist / dot).reshape(H, W)


def ransac_plane(depth, inv_K, visible_ground, samples):
    """RansacPlane.frame_predict with given sample ranks -> floor depth (the input depth below MIN_POINTS masked pixels)"""
    mask = visible_ground > 0.5
    if mask.sum() < MIN_POINTS:
        return depth
    planes, _, (best, _) = plane_fit(depth, inv_K, mask, samples)
    return plane_depth(depth, inv_K, planes[best])


def draw_samples(n, random_seed, iterations=ITERATIONS):
    """the rank triples ransac.run_ransac draws for n points"""
    np.random.seed(random_seed)
    return np.stack([np.random.randint(n, size=3) for _ in range(iterations)]).astype(np.int32)


def same_up_to_sign(a, b):
    """max |a -+ b| for the better sign"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(min(np.abs(a - b).max(), np.abs(a + b).max()))
