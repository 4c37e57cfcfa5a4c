"""Device-side geometry of the label generation (reference preprocessing/ground_truth_generation/geometry.py) over the fp_gt_* kernels.

Every function takes CUDA tensors; there is no CPU compute path."""
import numpy as np
import torch

from ... import ops

RANSAC_ITERATIONS = 100          # the reference's fit_plane: max_iterations = 100, never stopped early
FOOTPRINT_THRESHOLD = 0.75


def require_cuda(t, name):
    if not (torch.is_tensor(t) and t.is_cuda):
        raise RuntimeError("footprints_amd.preprocessing.ground_truth_generation: %s must be a CUDA tensor (no CPU path in the product)" % name)
    return t.contiguous()


class BatchProjector:
    """Forward-warps depth values from multiple frames into a target frame, in batches.  Same methods, argument order and shapes as
    the reference's class; `warp_splat` is the fused production path (no world points or pixel coordinates in memory)."""

    def __init__(self, height, width):
        self.height = height
        self.width = width

    def project_to_world(self, depth, invK):
        """depth [B,H,W], invK [B,4,4] -> world points [B,4,H*W]; the fourth coordinate is (depth > 0)"""
        return ops.gt_project_to_world(require_cuda(depth, "depth"), require_cuda(invK, "invK"))

    def project_to_camera(self, world_points, T, K):
        """world points [B,4,N] -> cam_pix [B,4,N] = K . (T . world_points), rows 0 and 1 divided by (row 2 + 1e-7)"""
        return ops.gt_project_to_camera(require_cuda(world_points, "world_points"), require_cuda(T, "T"), require_cuda(K, "K"))

    def extract_depth_from_projections(self, cam_pix):
        """cam_pix [B,4,N] -> projections [B,H,W].  Where several valid points of a frame land in one pixel the one with the highest
        index wins: what the reference computes when it runs serially; on a GPU it leaves the winner to chance."""
        keys = ops.gt_splat(require_cuda(cam_pix, "cam_pix"), self.height, self.width)
        return ops.gt_aggregate(keys, self.height, self.width, False, want_projections=True)[1]

    def warp_splat(self, depth, invK, T, K):
        """depth [B,H,W] -> key plane [B,H*W] for ops.gt_aggregate: project_to_world + project_to_camera + the splat in one kernel"""
        return ops.gt_warp_splat(require_cuda(depth, "depth"), require_cuda(invK, "invK"), require_cuda(T, "T"), require_cuda(K, "K"))


def draw_samples(n_ground, iterations=RANSAC_ITERATIONS):
    """the index triples of the reference's run_ransac, drawn from the host's numpy.random stream exactly as it draws them"""
    return np.stack([np.random.randint(n_ground, size=3) for _ in range(iterations)]).astype(np.int32)


def fit_plane(world_points, ground_pix, footprint_threshold=FOOTPRINT_THRESHOLD, samples=None):
    """RANSAC plane through the ground points.  world_points [4,H*W] or [1,4,H*W] (project_to_world of one frame); ground_pix [H,W]:
    the float ground segmentation (ground = value > footprint_threshold) or a bool mask -> (plane float64 [4] on the device,
    inlier_count int, inlier_mask bool [H,W]).

    The host draws the 100 x 3 sample indices (or takes `samples`, int32 [C,3]); the device builds the candidate planes in float64
    through the sampled points -- normal (p1 - p0) x (p2 - p0), d = -n . p0 -- counts the ground points within 0.05 of each and keeps
    the first candidate with the strictly largest count, like the reference's run_ransac over `world_points[ground_pix]`.
    Differences from the reference: its plane is the SVD null vector of the three augmented points, equal to this one up to scale
    and sign (the sign is LAPACK's there and the cross product's here; distances and flattened points do not depend on it, the
    direction of v1 = n x (0,0,1) in compute_depth_mask does); a degenerate sample (a repeated point, collinear points: zero
    normal) scores 0 here, where the reference's SVD returns an arbitrary plane; the inlier mask is returned over all pixels
    rather than over the compacted ground points."""
    world_points = require_cuda(world_points, "world_points").reshape(4, -1)
    ground_pix = require_cuda(ground_pix, "ground_pix")
    if ground_pix.dtype == torch.bool:
        ground_pix, footprint_threshold = ground_pix.to(torch.float32), 0.5
    if samples is None:
        n_ground = int(ops.gt_ground_count(ground_pix, footprint_threshold).item())
        if n_ground < 1:
            raise RuntimeError("fit_plane: no ground pixel")
        samples = draw_samples(n_ground)
    if not torch.is_tensor(samples):
        samples = torch.from_numpy(np.ascontiguousarray(samples, dtype=np.int32)).to(world_points.device)
    r = ops.gt_plane_score(world_points, ground_pix, footprint_threshold, samples, want_inlier_mask=True)
    return r["best_plane"], int(r["best"][1].item()), r["inlier_mask"]
