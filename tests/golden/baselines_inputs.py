"""Synthetic inputs of the baselines fixture (G20): shared by the generator (which feeds them to the reference's own
footprints/baselines/ransac.py and utils.py), by the tests and by scripts/baselines_bench.py.

An indoor-like scene: a camera about 1.5 m above a ground plane whose height carries Gaussian noise (sigma 1 cm), a far wall above
the horizon and a box standing on the floor.  The intrinsics are built the way MatterportTestLoader.load_intrinsics builds them
(a 640 x 512 calibration scaled to the depth map's shape, inverted with numpy.linalg.pinv in float64)."""
import numpy as np

CAM_HEIGHT, FAR = 1.5, 8.0
SHAPES = ((24, 40), (48, 64))           # the fixture's frames: about 300 and about 1100 masked points
CALIBRATION = (0, 0, 540.0, 540.0, 318.5, 254.0)        # one line of a *_intrinsics_*.txt: width, height, fx, fy, cx, cy


def intrinsics(H, W, calibration=CALIBRATION):
    """-> K, inv_K float64 [3,3] as MatterportTestLoader.load_intrinsics makes them for a depth map of H x W"""
    fx, fy, cx, cy = (float(v) for v in calibration[2:6])
    K = np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])
    K[0] = K[0] / 640 * W
    K[1] = K[1] / 512 * H
    return K, np.linalg.pinv(K)


def frame(H, W, seed):
    """-> dict of depth float32 [H,W], K / inv_K float64 [3,3], visible_ground float32 [H,W] (a sigmoid-like map: > 0.5 on the floor
    that can be seen, below elsewhere) and bounding_box uint8 [H,W] (255 outside the box's footprint on the floor, 0 inside)"""
    rng = np.random.RandomState(seed)
    K, inv_K = intrinsics(H, W)
    y = np.arange(H, dtype=np.float64).reshape(H, 1) * np.ones((1, W))
    ray_y = (y - K[1, 2]) / K[1, 1]
    height = CAM_HEIGHT + 0.01 * rng.randn(H, W)
    with np.errstate(divide="ignore"):
        ground = np.where(ray_y > 0, height / np.maximum(ray_y, 1e-9), np.inf)
    is_ground = ground < FAR
    depth = np.minimum(ground, FAR)
    z_box = 3.0
    bottom = min(int(K[1, 2] + K[1, 1] * CAM_HEIGHT / z_box), H - 1)           # the row where the box meets the floor
    top, left, right = max(bottom - H // 4, 0), W // 3, W // 3 + max(W // 5, 2)
    depth[top:bottom, left:right] = z_box * (1.0 + 0.002 * (rng.rand(bottom - top, right - left) - 0.5))
    is_ground[top:bottom, left:right] = False
    vis = np.where(is_ground, 0.75 + 0.25 * rng.rand(H, W), 0.3 * rng.rand(H, W))
    vis[rng.rand(H, W) < 0.03] = 0.4                                             # holes in the prediction
    wrong = np.zeros((H, W), bool)                                               # and false positives: on the box's face and on the wall
    wrong[top:bottom, left:right] = rng.rand(bottom - top, right - left) < 0.5
    wrong |= ~is_ground & (rng.rand(H, W) < 0.04)
    vis[wrong] = 0.55 + 0.1 * rng.rand(int(wrong.sum()))
    bbox = np.full((H, W), 255, np.uint8)
    bbox[bottom:min(bottom + max(H // 8, 1), H), max(left - 1, 0):right + 1] = 0
    return {"depth": depth.astype(np.float32), "K": K, "inv_K": inv_K, "visible_ground": vis.astype(np.float32), "bounding_box": bbox}


def batch(B, H, W, seed=20):
    """B frames stacked: depth [B,H,W], inv_K [B,3,3], visible_ground [B,H,W], bounding_box [B,H,W]"""
    frames = [frame(H, W, seed + b) for b in range(B)]
    return {k: np.stack([f[k] for f in frames]) for k in ("depth", "inv_K", "visible_ground", "bounding_box")}


def blob(H, W, seed):
    """a random non-convex blob, uint8 [H,W]: a union of discs around the centre"""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    m = np.zeros((H, W), bool)
    for _ in range(6):
        cy, cx = H * (0.3 + 0.4 * rng.rand()), W * (0.2 + 0.6 * rng.rand())
        ry, rx = max(H * 0.18 * rng.rand(), 0.8), max(W * 0.15 * rng.rand(), 0.8)
        m |= ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0
    m &= rng.rand(H, W) < 0.9
    return m.astype(np.uint8)


def hull_cases():
    """-> list of (name, uint8 [B,H,W]): the shapes at which the hull kernels can go wrong (single pixels and lines, a row that
    crosses a wave of 64 columns, foreground only in the corners, a full-size blob, a mixed batch)"""
    rng = np.random.RandomState(7)
    cases = [("1x1", np.ones((1, 1, 1), np.uint8)), ("1x7", (rng.rand(1, 1, 7) < 0.5).astype(np.uint8)), ("7x1", (rng.rand(1, 7, 1) < 0.5).astype(np.uint8))]
    cases[1][1][0, 0, 2] = 1
    cases[2][1][0, 4, 0] = 1
    cases.append(("5x9", (rng.rand(1, 5, 9) < 0.3).astype(np.uint8)))
    cases.append(("33x70", blob(33, 70, 3)[None] | (rng.rand(1, 33, 70) < 0.01).astype(np.uint8)))
    corners = np.zeros((1, 65, 130), np.uint8)
    corners[0, 0, 0] = corners[0, 0, 129] = corners[0, 64, 0] = corners[0, 63, 128] = 1
    cases.append(("65x130 corners", corners))
    cases.append(("192x640 blob", blob(192, 640, 5)[None]))
    mixed = np.zeros((5, 21, 37), np.uint8)
    mixed[1] = 1
    mixed[2, 13, 30] = 1
    mixed[3, np.arange(21), np.arange(21) + 5] = 1
    mixed[4] = blob(21, 37, 9)
    cases.append(("batch of 5", mixed))
    return cases
