"""Synthetic inputs of the label-generation fixture (G13): shared by the generator (which feeds them to the reference's own
geometry.py / ground_truth_generator.py) and by the tests (which feed the same arrays to the restatement / the HIP kernels).

A road-like scene: a camera 1.65 m above a ground plane, depth noise, a partial ground segmentation, a few zero disparities
(infinite depths), source poses that translate, shift sideways (the stereo pair) and yaw."""
import numpy as np

from oracle import filler

B, H, W = 10, 96, 320
CAM_HEIGHT, FAR = 1.65, 60.0
STEREO_BASELINE = 0.54
FOOTPRINT_THRESHOLD = 0.75
SAMPLE_SEED = 13


def intrinsics(H=H, W=W):
    K = np.array([[0.58 * W, 0, 0.5 * W, 0], [0, 1.92 * H, 0.5 * H, 0], [0, 0, 1, 0], [0, 0, 0, 1]], np.float64)
    return K.astype(np.float32), np.linalg.pinv(K).astype(np.float32)


def scene_depth(tag, noise, H=H, W=W):
    """z-depth [H,W] of the ground plane below the horizon and a far wall above it, with multiplicative noise"""
    K, _ = intrinsics(H, W)
    y = np.arange(H, dtype=np.float64).reshape(H, 1) * np.ones((1, W))
    ray_y = (y - K[1, 2]) / K[1, 1]
    with np.errstate(divide="ignore"):
        ground = np.where(ray_y > 0, CAM_HEIGHT / np.maximum(ray_y, 1e-9), np.inf)
    depth = np.minimum(ground, FAR)
    depth = depth * (1.0 + noise * (2.0 * filler.uniform(tag + ":noise", (H, W)).astype(np.float64) - 1.0))
    return depth, ground < FAR


def hidden_depth_inputs(B=B, H=H, W=W):
    """-> dict of the reference's `data`: depths [B,H,W] (ground pixels only, as the loaders leave them), poses, intrinsics,
    inv_intrinsics [B,4,4], all fp32.  The fixture uses the default shape; other shapes serve the full-size GPU cases."""
    K, invK = intrinsics(H, W)
    depths, poses = [], []
    for b in range(B):
        depth, is_ground = scene_depth("g13:hd:%d" % b, 0.01, H, W)
        seg = is_ground & (filler.uniform("g13:hd:%d:seg" % b, (H, W)) < 0.85)           # a partial segmentation
        seg[:, (37 * b) % W: (37 * b) % W + 25] = False                                   # something stands on the road
        d = (depth * seg).astype(np.float32)
        zero_disp = filler.uniform("g13:hd:%d:zd" % b, (H, W)) < 0.002
        d[zero_disp & seg] = np.inf                                                       # disparity 0 on a ground pixel
        d[zero_disp & ~seg] = np.nan                                                      # inf * 0 in the loader's product
        depths.append(d)
        mid = 0.5 * (B - 1)
        yaw, tz, tx = 0.12 / B * (b - mid), 8.0 / B * (b - mid), STEREO_BASELINE * (b % 2)
        T = np.eye(4)
        T[:3, :3] = [[np.cos(yaw), 0, np.sin(yaw)], [0, 1, 0], [-np.sin(yaw), 0, np.cos(yaw)]]
        T[:3, 3] = [tx, 0.1 / B * (b - mid), tz]
        poses.append(T.astype(np.float32))
    return {"depths": np.stack(depths), "poses": np.stack(poses), "intrinsics": np.stack([K] * B), "inv_intrinsics": np.stack([invK] * B)}


def moving_inputs():
    """-> disparity [H,W] fp32 (some zeros), base / lookup poses (float64 4x4 as a loader gives them), flow [2,H,W] float64 holding
    fp32 values: the flow the camera motion induces, plus a patch that moves by itself"""
    from tests import gtgen_restatement as GR
    K, invK = intrinsics()
    depth, _ = scene_depth("g13:mv", 0.01)
    fb = np.float32(float(K[0, 0]) * STEREO_BASELINE)
    disparity = (fb / depth).astype(np.float32)
    disparity[filler.uniform("g13:mv:zd", (H, W)) < 0.003] = 0.0
    base_pose, lookup_pose = np.eye(4), np.eye(4)
    yaw = 0.01
    lookup_pose[:3, :3] = [[np.cos(yaw), 0, np.sin(yaw)], [0, 1, 0], [-np.sin(yaw), 0, np.cos(yaw)]]
    lookup_pose[:3, 3] = [0.05, 0.0, 0.9]
    T = np.matmul(np.linalg.pinv(lookup_pose), base_pose).astype(np.float32)
    with np.errstate(divide="ignore"):
        d64 = (np.float64(fb) / disparity.astype(np.float64)).reshape(1, H, W)
    cp = GR.warp(d64, invK[None], T[None], K[None])[0, :2].reshape(2, H, W)
    x, y = np.meshgrid(np.arange(W), np.arange(H))
    flow = np.stack([cp[0] - x, cp[1] - y])
    flow = np.where(np.isfinite(flow), flow, 0.0)
    flow += 0.3 * (filler.uniform("g13:mv:fn", (2, H, W)).astype(np.float64) - 0.5)      # an estimated flow is never exact
    flow[0, 50:80, 120:200] += 6.0                                                        # the car that drives
    flow[1, 50:80, 120:200] -= 2.0
    return {"disparity": disparity, "base_pose": base_pose, "lookup_pose": lookup_pose, "T": T,
            "flow": flow.astype(np.float32).astype(np.float64), "fx_baseline": float(K[0, 0]) * STEREO_BASELINE}


def depth_mask_inputs():
    """-> depth [H,W] fp32 (visible depth), ground_seg [H,W] fp32: the road, an obstacle standing on it whose footprint on the road
    is itself labelled non-ground (a box on the road alone gives an empty mask: every flattened point lands on ground pixels)"""
    depth, is_ground = scene_depth("g13:dm", 0.02)
    seg = np.where(is_ground, 0.8 + 0.2 * filler.uniform("g13:dm:seg", (H, W)), 0.3 * filler.uniform("g13:dm:sky", (H, W))).astype(np.float32)
    K, _ = intrinsics()
    z_box = 9.0
    bottom = int(K[1, 2] + K[1, 1] * CAM_HEIGHT / z_box)                                  # the row where the box meets the road
    depth[bottom - 30:bottom, 140:200] = z_box * (1.0 + 0.004 * (filler.uniform("g13:dm:box", (30, 60)).astype(np.float64) - 0.5))
    seg[bottom - 30:bottom, 140:200] = 0.05
    seg[bottom:bottom + 12, 130:210] = 0.2 * filler.uniform("g13:dm:foot", (12, 80))      # its footprint: road, labelled non-ground
    seg[70:90, 20:60] = 0.6                                                               # unsure: neither ground nor obstacle
    depth = depth.astype(np.float32)
    depth[filler.uniform("g13:dm:zd", (H, W)) < 0.002] = np.inf                           # zero disparities
    return {"depth": depth, "ground_seg": seg}


def draw_samples(n_ground, n_candidates=100, seed=SAMPLE_SEED):
    """the index triples the reference's run_ransac draws after numpy.random.seed(seed)"""
    np.random.seed(seed)
    return np.stack([np.random.randint(n_ground, size=3) for _ in range(n_candidates)]).astype(np.int32)
