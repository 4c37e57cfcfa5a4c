// Training-label generation (reference footprints/preprocessing/ground_truth_generation/{geometry,ground_truth_generator}.py):
// forward warp of source depths into a target camera, a deterministic splat, the per-pixel median over frames, the moving-object
// mask and the depth mask (RANSAC plane scoring, flattening, 8 x 8 offset splat, filter).
//
// Splat rule.  The reference scatters with `projection[v.long(), u.long()] = z`; when several valid points of one frame land in one
// pixel a serial CPU run keeps the LAST one (highest source index) and a CUDA run leaves it to chance.  Here the rule is the serial
// one, without a sort: every (frame, pixel) owns a 64-bit key `(source_index + 1) << 32 | float_bits(z)`, points meet in an
// atomic unsigned max, and consumers read the low word.  An untouched pixel keeps key 0 = depth 0.
//
// This file is compiled with -ffp-contract=off: the float64 plane arithmetic follows NumPy's unfused operations, and the fp32 warp is
// the same sequence of roundings wherever it is inlined (fp_gt_project and fp_gt_warp_splat share gt_warp below).
#include "fp_common.h"

namespace {

constexpr int GT_T = 256;             // threads of the elementwise kernels
constexpr int GT_MAX_FRAMES = 512;    // frames one aggregation accepts
constexpr int GT_SORT_MAX = 128;      // frames the in-register sort holds (one VGPR per frame and lane)
constexpr int GT_AGG_T = 64;          // one wave per workgroup in the aggregation
constexpr int GT_BUILD_T = 1024;      // the single workgroup that resolves the RANSAC samples
constexpr int GT_MAX_CANDIDATES = 4096;
constexpr int GT_OFFSETS = 8;         // numpy.arange(-0.1, 0.1, 0.025) has 8 entries

struct gt_pix {
  float u, v, z, c3;
};

// (invK[:3,:3] . (x, y, 1)) * d, homogeneous coordinate (d > 0)                      [BatchProjector.project_to_world]
__device__ __forceinline__ void gt_backproject(const float* __restrict__ invK, int x, int y, float d, float (&w)[4]) {
  const float fx = (float)x, fy = (float)y;
#pragma unroll
  for (int r = 0; r < 3; ++r) w[r] = ((invK[r * 4 + 0] * fx + invK[r * 4 + 1] * fy) + invK[r * 4 + 2]) * d;
  w[3] = d > 0.f ? 1.f : 0.f;
}

// K . (T . w), then the perspective division with the reference's 1e-7                [BatchProjector.project_to_camera]
__device__ __forceinline__ gt_pix gt_to_camera(const float* __restrict__ T, const float* __restrict__ K, const float (&w)[4]) {
  float t[4], c[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) t[r] = ((T[r * 4 + 0] * w[0] + T[r * 4 + 1] * w[1]) + T[r * 4 + 2] * w[2]) + T[r * 4 + 3] * w[3];
#pragma unroll
  for (int r = 0; r < 4; ++r) c[r] = ((K[r * 4 + 0] * t[0] + K[r * 4 + 1] * t[1]) + K[r * 4 + 2] * t[2]) + K[r * 4 + 3] * t[3];
  const float den = c[2] + 1e-7f;
  gt_pix q;
  q.u = __fdiv_rn(c[0], den);
  q.v = __fdiv_rn(c[1], den);
  q.z = c[2];
  q.c3 = c[3];
  return q;
}

// the one warp of this file: an infinite depth (zero disparity) runs through it unguarded and comes out as NaN coordinates
__device__ __forceinline__ gt_pix gt_warp(const float* __restrict__ invK, const float* __restrict__ T, const float* __restrict__ K, int x,
                                          int y, float d) {
  float w[4];
  gt_backproject(invK, x, y, d, w);
  return gt_to_camera(T, K, w);
}

__device__ __forceinline__ void gt_load_world(const float* __restrict__ world, int HW, int p, float (&w)[4]) {
#pragma unroll
  for (int r = 0; r < 4; ++r) w[r] = world[(size_t)r * HW + p];
}

// strict comparisons, every one false for a NaN                                       [extract_depth_from_projections]
__device__ __forceinline__ bool gt_valid(const gt_pix& q, float Wf, float Hf) {
  return q.u > 0.f && q.u < Wf && q.v > 0.f && q.v < Hf && q.z > 0.f && q.c3 > 0.f;
}

__device__ __forceinline__ void gt_splat_point(unsigned long long* __restrict__ keys, const gt_pix& q, int H, int W, unsigned src) {
  if (!gt_valid(q, (float)W, (float)H)) return;
  const int ix = (int)q.u, iy = (int)q.v;             // 0 <= ix < W and 0 <= iy < H follow from gt_valid
  atomicMax(keys + (size_t)iy * W + ix, ((unsigned long long)(src + 1u) << 32) | (unsigned long long)__float_as_uint(q.z));
}

__device__ __forceinline__ float gt_key_depth(const unsigned long long* __restrict__ keys, size_t i) {
  return __uint_as_float(reinterpret_cast<const unsigned*>(keys)[2 * i]);      // low word (little endian)
}

__global__ void __launch_bounds__(GT_T) gt_project_kernel(const float* __restrict__ depth, const float* __restrict__ invK,
                                                          const float* __restrict__ T, const float* __restrict__ K, int W, int HW,
                                                          float* __restrict__ cam_pix) {
  const int p = blockIdx.x * GT_T + threadIdx.x, b = blockIdx.y;
  if (p >= HW) return;
  const gt_pix q = gt_warp(invK + b * 16, T + b * 16, K + b * 16, p % W, p / W, depth[(size_t)b * HW + p]);
  float* o = cam_pix + (size_t)b * 4 * HW + p;
  o[0] = q.u;
  o[(size_t)HW] = q.v;
  o[(size_t)2 * HW] = q.z;
  o[(size_t)3 * HW] = q.c3;
}

__global__ void __launch_bounds__(GT_T) gt_world_kernel(const float* __restrict__ depth, const float* __restrict__ invK, int W, int HW,
                                                        float* __restrict__ world) {
  const int p = blockIdx.x * GT_T + threadIdx.x, b = blockIdx.y;
  if (p >= HW) return;
  float w[4];
  gt_backproject(invK + b * 16, p % W, p / W, depth[(size_t)b * HW + p], w);
#pragma unroll
  for (int r = 0; r < 4; ++r) world[((size_t)b * 4 + r) * HW + p] = w[r];
}

__global__ void __launch_bounds__(GT_T) gt_camera_kernel(const float* __restrict__ world, const float* __restrict__ T,
                                                         const float* __restrict__ K, int HW, float* __restrict__ cam_pix) {
  const int p = blockIdx.x * GT_T + threadIdx.x, b = blockIdx.y;
  if (p >= HW) return;
  float w[4];
  gt_load_world(world + (size_t)b * 4 * HW, HW, p, w);
  const gt_pix q = gt_to_camera(T + b * 16, K + b * 16, w);
  float* o = cam_pix + (size_t)b * 4 * HW + p;
  o[0] = q.u;
  o[(size_t)HW] = q.v;
  o[(size_t)2 * HW] = q.z;
  o[(size_t)3 * HW] = q.c3;
}

__global__ void __launch_bounds__(GT_T) gt_splat_kernel(const float* __restrict__ cam_pix, int H, int W, int HW,
                                                        unsigned long long* __restrict__ keys) {
  const int p = blockIdx.x * GT_T + threadIdx.x, b = blockIdx.y;
  if (p >= HW) return;
  const float* c = cam_pix + (size_t)b * 4 * HW + p;
  gt_pix q;
  q.u = c[0];
  q.v = c[(size_t)HW];
  q.z = c[(size_t)2 * HW];
  q.c3 = c[(size_t)3 * HW];
  gt_splat_point(keys + (size_t)b * HW, q, H, W, (unsigned)p);
}

__global__ void __launch_bounds__(GT_T) gt_warp_splat_kernel(const float* __restrict__ depth, const float* __restrict__ invK,
                                                             const float* __restrict__ T, const float* __restrict__ K, int H, int W, int HW,
                                                             unsigned long long* __restrict__ keys) {
  const int p = blockIdx.x * GT_T + threadIdx.x, b = blockIdx.y;
  if (p >= HW) return;
  const gt_pix q = gt_warp(invK + b * 16, T + b * 16, K + b * 16, p % W, p / W, depth[(size_t)b * HW + p]);
  gt_splat_point(keys + (size_t)b * HW, q, H, W, (unsigned)p);
}

// k-th smallest (0-based) of the positive depths of pixel p, found bit by bit: positive floats order like their bit patterns
__device__ __forceinline__ unsigned gt_select(const unsigned long long* __restrict__ keys, int B, size_t HW, size_t p, int k) {
  unsigned prefix = 0;
  for (int bit = 30; bit >= 0; --bit) {
    const unsigned cand = prefix | (1u << bit);
    int below = 0;
    for (int b = 0; b < B; ++b) {
      const float z = gt_key_depth(keys, (size_t)b * HW + p);
      below += (z > 0.f && __float_as_uint(z) < cand) ? 1 : 0;
    }
    if (below <= k) prefix = cand;
  }
  return prefix;
}

// compare-exchange steps of the sorting network below: every comparator leaves the smaller value at the lower index
template <int MASK, int CAP>
__device__ __forceinline__ void gt_sort_step(unsigned (&v)[CAP]) {
#pragma unroll
  for (int i = 0; i < CAP; ++i) {
    const int q = i ^ MASK;
    if (i < q && q < CAP) {
      const unsigned a = v[i], c = v[q];
      v[i] = min(a, c);
      v[q] = max(a, c);
    }
  }
}

template <int J, int CAP>
__device__ __forceinline__ void gt_sort_halves(unsigned (&v)[CAP]) {
  if constexpr (J > 0) {
    gt_sort_step<J, CAP>(v);
    gt_sort_halves<J / 2, CAP>(v);
  }
}

// merges sorted runs of K / 2 into runs of K: the mirrored step (i against i ^ (K - 1)), then halving steps; then the next K
template <int K, int CAP>
__device__ __forceinline__ void gt_sort_stage(unsigned (&v)[CAP]) {
  if constexpr (K < 2 * CAP) {
    gt_sort_step<K - 1, CAP>(v);
    gt_sort_halves<K / 4, CAP>(v);
    gt_sort_stage<2 * K, CAP>(v);
  }
}

// One lane per target pixel, up to CAP frames: the depths live in registers as order-preserving integers (every index below is a
// compile-time constant), and the positive ones sort to the front through a bitonic network whose comparators all point the same
// way -- each merge starts with the mirrored step (i against i ^ (k - 1)), so padding with the largest value at the high end turns
// every comparator that reaches past CAP into a no-op and CAP need not be a power of two.  The two middle values are read back
// from an LDS column.  No scratch.
template <int CAP>
__global__ void __launch_bounds__(GT_AGG_T) gt_aggregate_sorted_kernel(const unsigned long long* __restrict__ keys, int B, int HW,
                                                                       int min_count, float* __restrict__ median, float* __restrict__ proj) {
  const int p = blockIdx.x * GT_AGG_T + threadIdx.x;
  if (p >= HW) return;
  // a depth is positive exactly when its bit pattern lies in [1, 0x7F800000]; `bits - 1` keeps the order of those and wraps 0 to the
  // top, and everything else (negative, -0, NaN) is raised to 0xFFFFFFFF by integer arithmetic -- no compare, so no lane mask per frame
  unsigned v[CAP];
  unsigned n = 0;
#pragma unroll
  for (int b = 0; b < CAP; ++b) {
    float z = 0.f;
    if (b < B) {
      z = gt_key_depth(keys, (size_t)b * HW + p);
      if (proj) proj[(size_t)b * HW + p] = z;
    }
    const unsigned u = __float_as_uint(z) - 1u;
    const unsigned invalid = (min(u >> 23, 255u) + 1u) >> 8;          // 1 when u > 0x7F7FFFFF
    v[b] = u | (0u - invalid);
    n += min(~v[b], 1u);
  }
  if (n < (unsigned)min_count) {
    median[p] = 0.f;
    return;
  }
  gt_sort_stage<2, CAP>(v);
  // the middle values sit at run-time indices (n - 1) / 2 and n / 2 <= CAP / 2: the lane parks the lower half of its sorted
  // registers in its own LDS column (sm[i * 64 + lane]: conflict free, no barrier -- nobody else reads it) and loads the two
  __shared__ unsigned sm[(CAP / 2 + 1) * GT_AGG_T];
#pragma unroll
  for (int i = 0; i <= CAP / 2; ++i) sm[i * GT_AGG_T + threadIdx.x] = v[i];
  const float lo = __uint_as_float(sm[((n - 1) / 2) * GT_AGG_T + threadIdx.x] + 1u);
  const float hi = __uint_as_float(sm[(n / 2) * GT_AGG_T + threadIdx.x] + 1u);
  median[p] = (lo + hi) * 0.5f;
}

// More than GT_SORT_MAX frames: the two middle values are selected from the key plane itself, bit by bit (gt_select).
__global__ void __launch_bounds__(GT_AGG_T) gt_aggregate_select_kernel(const unsigned long long* __restrict__ keys, int B, int HW,
                                                                       int min_count, float* __restrict__ median, float* __restrict__ proj) {
  const int p = blockIdx.x * GT_AGG_T + threadIdx.x;
  if (p >= HW) return;
  int n = 0;
  for (int b = 0; b < B; ++b) {
    const float z = gt_key_depth(keys, (size_t)b * HW + p);
    if (proj) proj[(size_t)b * HW + p] = z;
    n += z > 0.f ? 1 : 0;
  }
  if (n < min_count) {
    median[p] = 0.f;
    return;
  }
  const unsigned lob = gt_select(keys, B, (size_t)HW, (size_t)p, (n - 1) / 2);
  float lo = __uint_as_float(lob), hi = lo;
  if ((n & 1) == 0) {
    int le = 0;
    unsigned next = 0xFFFFFFFFu;
    for (int b = 0; b < B; ++b) {
      const float z = gt_key_depth(keys, (size_t)b * HW + p);
      if (!(z > 0.f)) continue;
      const unsigned zb = __float_as_uint(z);
      if (zb <= lob) ++le;
      else if (zb < next) next = zb;
    }
    if (le <= n / 2) hi = __uint_as_float(next);
  }
  median[p] = (lo + hi) * 0.5f;
}

// depth = fx * baseline / disparity, warp, induced flow against the given flow: float64 differences of fp32 values as in the reference
// (its flow array is float64)                                                        [KITTIMovingObjectDetector.process_data]
__global__ void __launch_bounds__(GT_T) gt_moving_mask_kernel(const float* __restrict__ disp, const float* __restrict__ flow,
                                                              const float* __restrict__ invK, const float* __restrict__ T,
                                                              const float* __restrict__ K, float fb, int W, int HW,
                                                              unsigned char* __restrict__ mask) {
  const int p = blockIdx.x * GT_T + threadIdx.x;
  if (p >= HW) return;
  const int x = p % W, y = p / W;
  const gt_pix q = gt_warp(invK, T, K, x, y, __fdiv_rn(fb, disp[p]));
  const double d0 = (double)(q.u - (float)x) - (double)flow[p];
  const double d1 = (double)(q.v - (float)y) - (double)flow[(size_t)HW + p];
  mask[p] = sqrt(d0 * d0 + d1 * d1) > 3.0 ? 1 : 0;
}

__global__ void __launch_bounds__(GT_T) gt_ground_count_kernel(const float* __restrict__ seg, float thr, int HW, int* __restrict__ count) {
  const int p = blockIdx.x * GT_T + threadIdx.x;
  const bool g = p < HW && seg[p] > thr;
  const unsigned long long m = __ballot(g);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(count, __popcll(m));
}

// One workgroup.  (1) rank -> pixel: `samples` index the ground pixels (seg > thr) in raster order, as the reference's
// `world_points[ground_pix]` does; every lane counts the ground pixels of its own contiguous chunk, a scan turns the counts into
// offsets, and each sample walks the one chunk that holds its rank.  (2) each candidate's plane through its three world
// points in float64: normal (p1 - p0) x (p2 - p0), d = -n . p0; a sample that repeats a point, whose points are collinear (zero
// normal) or whose rank is out of range gives the all-zero plane, which scores 0.  (3) clears the inlier counts.
__global__ void __launch_bounds__(GT_BUILD_T) gt_plane_build_kernel(const float* __restrict__ world, const float* __restrict__ seg, float thr,
                                                                    const int* __restrict__ samples, int C, int HW, int* __restrict__ sample_pix, double* __restrict__ planes,
                                                                    int* __restrict__ counts) {
  __shared__ int off[GT_BUILD_T + 1];
  __shared__ int tmp[GT_BUILD_T];
  const int t = threadIdx.x;
  const int chunk = (HW + GT_BUILD_T - 1) / GT_BUILD_T;
  const int beg = min(t * chunk, HW), end = min(beg + chunk, HW);
  int cnt = 0;
  for (int i = beg; i < end; ++i) cnt += seg[i] > thr ? 1 : 0;
  tmp[t] = cnt;
  __syncthreads();
  for (int s = 1; s < GT_BUILD_T; s <<= 1) {                     // inclusive scan
    const int add = t >= s ? tmp[t - s] : 0;
    __syncthreads();
    tmp[t] += add;
    __syncthreads();
  }
  off[t + 1] = tmp[t];
  if (t == 0) off[0] = 0;
  __syncthreads();
  const int total = off[GT_BUILD_T];
  for (int s = t; s < 3 * C; s += GT_BUILD_T) {
    const int r = samples[s];
    int pix = -1;
    if (r >= 0 && r < total) {
      int lo = 0, hi = GT_BUILD_T;                               // largest lo with off[lo] <= r
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= r) lo = mid;
        else hi = mid;
      }
      int rank = off[lo];
      const int cb = min(lo * chunk, HW), ce = min(cb + chunk, HW);
      for (int i = cb; i < ce; ++i) {
        if (seg[i] > thr) {
          if (rank == r) {
            pix = i;
            break;
          }
          ++rank;
        }
      }
    }
    sample_pix[s] = pix;
  }
  __syncthreads();                                               // this workgroup's global writes are visible to it after the barrier
  for (int c = t; c < C; c += GT_BUILD_T) {
    double P[3][3];
    bool ok = true;
    for (int k = 0; k < 3; ++k) {
      const int pix = sample_pix[c * 3 + k];
      if (pix < 0) {
        ok = false;
        P[k][0] = P[k][1] = P[k][2] = 0.0;
        continue;
      }
      float w[4];
      gt_load_world(world, HW, pix, w);
      P[k][0] = (double)w[0];
      P[k][1] = (double)w[1];
      P[k][2] = (double)w[2];
    }
    const double a0 = P[1][0] - P[0][0], a1 = P[1][1] - P[0][1], a2 = P[1][2] - P[0][2];
    const double b0 = P[2][0] - P[0][0], b1 = P[2][1] - P[0][1], b2 = P[2][2] - P[0][2];
    double n0 = a1 * b2 - a2 * b1, n1 = a2 * b0 - a0 * b2, n2 = a0 * b1 - a1 * b0;
    double d = -((n0 * P[0][0] + n1 * P[0][1]) + n2 * P[0][2]);
    const double nn = (n0 * n0 + n1 * n1) + n2 * n2;
    if (!ok || !(nn > 0.0) || !(nn < INFINITY) || !(fabs(d) < INFINITY)) n0 = n1 = n2 = d = 0.0;
    planes[c * 4 + 0] = n0;
    planes[c * 4 + 1] = n1;
    planes[c * 4 + 2] = n2;
    planes[c * 4 + 3] = d;
    counts[c] = 0;
  }
}

// signed distance of a world point to a plane, float64, NumPy's order of operations            [geometry.plane_distance]
__device__ __forceinline__ double gt_plane_distance(const double (&pl)[4], double norm, const float (&w)[4]) {
  return (((pl[0] * (double)w[0] + pl[1] * (double)w[1]) + pl[2] * (double)w[2]) + pl[3]) / norm;
}

__device__ __forceinline__ double gt_norm3(const double (&pl)[4]) { return sqrt((pl[0] * pl[0] + pl[1] * pl[1]) + pl[2] * pl[2]); }

// counts[c] += ground points within 0.05 of candidate c.  grid (chunks, C); integer atomics: the sum does not depend on their order
__global__ void __launch_bounds__(GT_T) gt_plane_score_kernel(const float* __restrict__ world, const float* __restrict__ seg, float thr,
                                                              const double* __restrict__ planes, int HW,
                                                              int per_block, int* __restrict__ counts) {
  const int c = blockIdx.y;
  const double pl[4] = {planes[c * 4 + 0], planes[c * 4 + 1], planes[c * 4 + 2], planes[c * 4 + 3]};
  const double norm = gt_norm3(pl);
  if (!(norm > 0.0)) return;                                     // degenerate sample: scores 0
  const int beg = blockIdx.x * per_block, end = min(beg + per_block, HW);
  int mine = 0;
  for (int p = beg + threadIdx.x; p < end; p += GT_T) {
    if (!(seg[p] > thr)) continue;
    float w[4];
    gt_load_world(world, HW, p, w);
    mine += fabs(gt_plane_distance(pl, norm, w)) < 0.05 ? 1 : 0;
  }
  for (int s = 32; s > 0; s >>= 1) mine += __shfl_down(mine, s);
  if ((threadIdx.x & 63) == 0 && mine) atomicAdd(counts + c, mine);
}

// first candidate with the strictly largest count                                                       [geometry.run_ransac]
__global__ void gt_plane_select_kernel(const double* __restrict__ planes, const int* __restrict__ counts, int C, double* __restrict__ best_plane,
                                       int* __restrict__ best) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  int bi = -1, bc = 0;
  for (int c = 0; c < C; ++c) {
    if (counts[c] > bc) {
      bc = counts[c];
      bi = c;
    }
  }
  for (int k = 0; k < 4; ++k) best_plane[k] = bi >= 0 ? planes[bi * 4 + k] : 0.0;
  best[0] = bi;
  best[1] = bc;
}

__global__ void __launch_bounds__(GT_T) gt_inlier_mask_kernel(const float* __restrict__ world, const float* __restrict__ seg, float thr,
                                                              const double* __restrict__ plane, int HW,
                                                              unsigned char* __restrict__ mask) {
  const int p = blockIdx.x * GT_T + threadIdx.x;
  if (p >= HW) return;
  const double pl[4] = {plane[0], plane[1], plane[2], plane[3]};
  const double norm = gt_norm3(pl);
  bool in = false;
  if (norm > 0.0 && seg[p] > thr) {
    float w[4];
    gt_load_world(world, HW, p, w);
    in = fabs(gt_plane_distance(pl, norm, w)) < 0.05;
  }
  mask[p] = in ? 1 : 0;
}

struct gt_offsets {
  double v[GT_OFFSETS];
};

// Every non-ground point moved onto the plane along its normal, copied to the 8 x 8 offsets along v1 = n x (0,0,1), v2 = n x v1
// (float64 as in the reference), rounded to fp32, projected with K and splatted.  Copy k = i1 * 8 + i2 of pixel p has source index
// k * HW + p: the order of the reference's concatenation, of which nothing is stored.  blockIdx.y = i1.     [compute_depth_mask]
__global__ void __launch_bounds__(GT_T) gt_flatten_splat_kernel(const float* __restrict__ world, const float* __restrict__ seg, float thr,
                                                                const float* __restrict__ K,
                                                                const double* __restrict__ plane, gt_offsets offs, int H, int W, int HW,
                                                                unsigned long long* __restrict__ keys, float* __restrict__ cam_pix) {
  const int p = blockIdx.x * GT_T + threadIdx.x, i1 = blockIdx.y;
  if (p >= HW) return;
  const bool ground = seg[p] > thr;
  const double pl[4] = {plane[0], plane[1], plane[2], plane[3]};
  const double norm = gt_norm3(pl);
  const double n0 = pl[0] / norm, n1 = pl[1] / norm, n2 = pl[2] / norm;
  // numpy.cross(n, (0, 0, 1)) and numpy.cross(n, v1), term by term
  const double v10 = n1 * 1.0 - n2 * 0.0, v11 = n2 * 0.0 - n0 * 1.0, v12 = n0 * 0.0 - n1 * 0.0;
  const double v20 = n1 * v12 - n2 * v11, v21 = n2 * v10 - n0 * v12, v22 = n0 * v11 - n1 * v10;
  float w[4];
  gt_load_world(world, HW, p, w);
  const double dist = gt_plane_distance(pl, norm, w);
  const double f0 = (double)w[0] - n0 * dist, f1 = (double)w[1] - n1 * dist, f2 = (double)w[2] - n2 * dist;
  const float eye[16] = {1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f};
  const double d1 = offs.v[i1];
#pragma unroll 1
  for (int i2 = 0; i2 < GT_OFFSETS; ++i2) {
    const double d2 = offs.v[i2];
    const float pt[4] = {(float)((f0 + v10 * d1) + v20 * d2), (float)((f1 + v11 * d1) + v21 * d2), (float)((f2 + v12 * d1) + v22 * d2),
                         (float)((1.0 + 0.0 * d1) + 0.0 * d2)};
    // the reference calls project_to_camera(points, K, eye): K takes the pose's place and the identity the intrinsics'
    const gt_pix q = gt_to_camera(K, eye, pt);
    const int k = i1 * GT_OFFSETS + i2;
    if (cam_pix) {
      float* o = cam_pix + (size_t)k * HW + p;
      const size_t plane_stride = (size_t)GT_OFFSETS * GT_OFFSETS * HW;
      const float nanv = __uint_as_float(0x7FC00000u);           // a ground pixel has no copies: never valid
      o[0] = ground ? nanv : q.u;
      o[plane_stride] = ground ? nanv : q.v;
      o[2 * plane_stride] = ground ? nanv : q.z;
      o[3 * plane_stride] = ground ? nanv : q.c3;
    }
    if (!ground) gt_splat_point(keys, q, H, W, (unsigned)k * (unsigned)HW + (unsigned)p);
  }
}

// must be fairly sure it is not ground, within 10 % of the visible depth and closer than 30 m            [compute_depth_mask]
__global__ void __launch_bounds__(GT_T) gt_depth_mask_kernel(const unsigned long long* __restrict__ keys, const float* __restrict__ depth,
                                                             const float* __restrict__ seg, int HW, unsigned char* __restrict__ mask,
                                                             float* __restrict__ projection) {
  const int p = blockIdx.x * GT_T + threadIdx.x;
  if (p >= HW) return;
  const float pr = gt_key_depth(keys, (size_t)p), d = depth[p];
  if (projection) projection[p] = pr;
  const bool m = pr > 0.f && seg[p] < 0.5f && __fdiv_rn(fabsf(pr - d), d + 1e-7f) < 0.10f && pr < 30.f && d > 0.f;
  mask[p] = m ? 1 : 0;
}

// frames x pixels x 64 offset copies must leave room for `source_index + 1` in the key's high word
bool gt_shape_ok(int32_t B, int32_t H, int32_t W) {
  return B >= 1 && B <= GT_MAX_FRAMES && H >= 1 && W >= 1 && (int64_t)H * W * (GT_OFFSETS * GT_OFFSETS) < (int64_t)0xFFFFFFFF &&
         (int64_t)B * H * W <= (int64_t)1 << 40;
}

const char* const GT_SHAPE_MSG = "%s: needs 1 <= B <= 512 frames and H * W * 64 below 2^32 - 1 (got B = %d, H = %d, W = %d)";

int gt_clear_keys(uint64_t* keys, int64_t n, fp_stream_t stream) { return fp_zero_u32(reinterpret_cast<uint32_t*>(keys), n * 2, stream); }

}  // namespace

extern "C" int64_t fp_gt_workspace(int32_t B, int32_t H, int32_t W) {
  if (!gt_shape_ok(B, H, W)) {
    fp_set_error(FP_EINVAL, GT_SHAPE_MSG, "fp_gt_workspace", B, H, W);
    return -1;
  }
  return (int64_t)B * H * W * (int64_t)sizeof(uint64_t);
}

extern "C" int fp_gt_project(const float* depths, const float* inv_intrinsics, const float* poses, const float* intrinsics, int32_t B,
                             int32_t H, int32_t W, float* cam_pix, fp_stream_t stream) {
  FP_REQUIRE(gt_shape_ok(B, H, W), GT_SHAPE_MSG, "fp_gt_project", B, H, W);
  FP_REQUIRE(depths && inv_intrinsics && poses && intrinsics && cam_pix, "fp_gt_project: null pointer");
  const int HW = H * W;
  fp_launch(gt_project_kernel, dim3((unsigned)fp_ceil_div(HW, GT_T), B), dim3(GT_T), 0, (hipStream_t)stream, depths, inv_intrinsics, poses,
            intrinsics, W, HW, cam_pix);
  return fp_check_launch("fp_gt_project");
}

extern "C" int fp_gt_project_to_world(const float* depths, const float* inv_intrinsics, int32_t B, int32_t H, int32_t W, float* world,
                                      fp_stream_t stream) {
  FP_REQUIRE(gt_shape_ok(B, H, W), GT_SHAPE_MSG, "fp_gt_project_to_world", B, H, W);
  FP_REQUIRE(depths && inv_intrinsics && world, "fp_gt_project_to_world: null pointer");
  const int HW = H * W;
  fp_launch(gt_world_kernel, dim3((unsigned)fp_ceil_div(HW, GT_T), B), dim3(GT_T), 0, (hipStream_t)stream, depths, inv_intrinsics, W, HW, world);
  return fp_check_launch("fp_gt_project_to_world");
}

extern "C" int fp_gt_project_to_camera(const float* world, const float* poses, const float* intrinsics, int32_t B, int64_t points,
                                       float* cam_pix, fp_stream_t stream) {
  FP_REQUIRE(B >= 1 && B <= GT_MAX_FRAMES && points >= 1 && points < ((int64_t)1 << 31) - GT_T && B * points <= (int64_t)1 << 40,
             "fp_gt_project_to_camera: needs 1 <= B <= 512 and 1 <= points < 2^31 (got B = %d, points = %lld)", B, (long long)points);
  FP_REQUIRE(world && poses && intrinsics && cam_pix, "fp_gt_project_to_camera: null pointer");
  fp_launch(gt_camera_kernel, dim3((unsigned)fp_ceil_div(points, GT_T), B), dim3(GT_T), 0, (hipStream_t)stream, world, poses, intrinsics,
            (int)points, cam_pix);
  return fp_check_launch("fp_gt_project_to_camera");
}

extern "C" int fp_gt_splat(const float* cam_pix, int32_t B, int32_t H, int32_t W, uint64_t* keys, int64_t keys_bytes, fp_stream_t stream) {
  FP_REQUIRE(gt_shape_ok(B, H, W), GT_SHAPE_MSG, "fp_gt_splat", B, H, W);
  FP_REQUIRE(cam_pix && keys, "fp_gt_splat: null pointer");
  FP_REQUIRE(keys_bytes >= fp_gt_workspace(B, H, W), "fp_gt_splat: key plane of %lld bytes, needs %lld", (long long)keys_bytes,
             (long long)fp_gt_workspace(B, H, W));
  const int HW = H * W;
  if (int rc = gt_clear_keys(keys, (int64_t)B * HW, stream)) return rc;
  fp_launch(gt_splat_kernel, dim3((unsigned)fp_ceil_div(HW, GT_T), B), dim3(GT_T), 0, (hipStream_t)stream, cam_pix, H, W, HW,
            (unsigned long long*)keys);
  return fp_check_launch("fp_gt_splat");
}

extern "C" int fp_gt_warp_splat(const float* depths, const float* inv_intrinsics, const float* poses, const float* intrinsics, int32_t B,
                                int32_t H, int32_t W, uint64_t* keys, int64_t keys_bytes, fp_stream_t stream) {
  FP_REQUIRE(gt_shape_ok(B, H, W), GT_SHAPE_MSG, "fp_gt_warp_splat", B, H, W);
  FP_REQUIRE(depths && inv_intrinsics && poses && intrinsics && keys, "fp_gt_warp_splat: null pointer");
  FP_REQUIRE(keys_bytes >= fp_gt_workspace(B, H, W), "fp_gt_warp_splat: key plane of %lld bytes, needs %lld", (long long)keys_bytes,
             (long long)fp_gt_workspace(B, H, W));
  const int HW = H * W;
  if (int rc = gt_clear_keys(keys, (int64_t)B * HW, stream)) return rc;
  fp_launch(gt_warp_splat_kernel, dim3((unsigned)fp_ceil_div(HW, GT_T), B), dim3(GT_T), 0, (hipStream_t)stream, depths, inv_intrinsics, poses,
            intrinsics, H, W, HW, (unsigned long long*)keys);
  return fp_check_launch("fp_gt_warp_splat");
}

extern "C" int fp_gt_aggregate(const uint64_t* keys, int32_t B, int32_t H, int32_t W, int32_t robust, float* median, float* projections,
                               fp_stream_t stream) {
  FP_REQUIRE(gt_shape_ok(B, H, W), GT_SHAPE_MSG, "fp_gt_aggregate", B, H, W);
  FP_REQUIRE(keys && median, "fp_gt_aggregate: null pointer");
  const int HW = H * W, min_count = robust ? 3 : 1;
  const dim3 grid((unsigned)fp_ceil_div(HW, GT_AGG_T));
  const unsigned long long* k = (const unsigned long long*)keys;
  hipStream_t s = (hipStream_t)stream;
#define GT_AGG_LAUNCH(CAP) fp_launch(gt_aggregate_sorted_kernel<CAP>, grid, dim3(GT_AGG_T), 0, s, k, B, HW, min_count, median, projections)
  if (B <= 8) GT_AGG_LAUNCH(8);
  else if (B <= 32) GT_AGG_LAUNCH(32);
  else if (B <= 48) GT_AGG_LAUNCH(48);
  else if (B <= 80) GT_AGG_LAUNCH(80);
  else if (B <= GT_SORT_MAX) GT_AGG_LAUNCH(GT_SORT_MAX);
  else fp_launch(gt_aggregate_select_kernel, grid, dim3(GT_AGG_T), 0, s, k, B, HW, min_count, median, projections);
#undef GT_AGG_LAUNCH
  return fp_check_launch("fp_gt_aggregate");
}

extern "C" int fp_gt_moving_mask(const float* disparity, const float* flow, const float* inv_intrinsics, const float* pose,
                                 const float* intrinsics, double fx_baseline, int32_t H, int32_t W, uint8_t* mask, fp_stream_t stream) {
  FP_REQUIRE(gt_shape_ok(1, H, W), GT_SHAPE_MSG, "fp_gt_moving_mask", 1, H, W);
  FP_REQUIRE(disparity && flow && inv_intrinsics && pose && intrinsics && mask, "fp_gt_moving_mask: null pointer");
  const int HW = H * W;
  fp_launch(gt_moving_mask_kernel, dim3((unsigned)fp_ceil_div(HW, GT_T)), dim3(GT_T), 0, (hipStream_t)stream, disparity, flow, inv_intrinsics,
            pose, intrinsics, (float)fx_baseline, W, HW, mask);
  return fp_check_launch("fp_gt_moving_mask");
}

extern "C" int fp_gt_ground_count(const float* ground_seg, double threshold, int32_t H, int32_t W, int32_t* count, fp_stream_t stream) {
  FP_REQUIRE(gt_shape_ok(1, H, W), GT_SHAPE_MSG, "fp_gt_ground_count", 1, H, W);
  FP_REQUIRE(ground_seg && count, "fp_gt_ground_count: null pointer");
  const int HW = H * W;
  if (int rc = fp_zero_u32(reinterpret_cast<uint32_t*>(count), 1, stream)) return rc;
  fp_launch(gt_ground_count_kernel, dim3((unsigned)fp_ceil_div(HW, GT_T)), dim3(GT_T), 0, (hipStream_t)stream, ground_seg, (float)threshold, HW,
            count);
  return fp_check_launch("fp_gt_ground_count");
}

extern "C" int fp_gt_plane_score(const float* world, const float* ground_seg, double threshold, const int32_t* samples, int32_t C, int32_t H, int32_t W, int32_t* sample_pix, double* planes, int32_t* counts,
                                 double* best_plane, int32_t* best, uint8_t* inlier_mask, fp_stream_t stream) {
  FP_REQUIRE(gt_shape_ok(1, H, W), GT_SHAPE_MSG, "fp_gt_plane_score", 1, H, W);
  FP_REQUIRE(C >= 1 && C <= GT_MAX_CANDIDATES, "fp_gt_plane_score: needs 1 <= C <= %d candidates (got %d)", GT_MAX_CANDIDATES, C);
  FP_REQUIRE(world && ground_seg && samples && sample_pix && planes && counts && best_plane && best,
             "fp_gt_plane_score: null pointer");
  const int HW = H * W;
  hipStream_t s = (hipStream_t)stream;
  fp_launch(gt_plane_build_kernel, dim3(1), dim3(GT_BUILD_T), 0, s, world, ground_seg, (float)threshold, samples, C, HW, sample_pix, planes,
            counts);
  const int per_block = GT_T * 16;
  fp_launch(gt_plane_score_kernel, dim3((unsigned)fp_ceil_div(HW, per_block), C), dim3(GT_T), 0, s, world, ground_seg, (float)threshold,
            (const double*)planes, HW, per_block, counts);
  fp_launch(gt_plane_select_kernel, dim3(1), dim3(64), 0, s, (const double*)planes, (const int*)counts, C, best_plane, best);
  if (inlier_mask)
    fp_launch(gt_inlier_mask_kernel, dim3((unsigned)fp_ceil_div(HW, GT_T)), dim3(GT_T), 0, s, world, ground_seg, (float)threshold,
              (const double*)best_plane, HW, inlier_mask);
  return fp_check_launch("fp_gt_plane_score");
}

extern "C" int fp_gt_flatten_splat(const float* world, const float* ground_seg, double threshold, const float* intrinsics, const double* plane, int32_t H, int32_t W, uint64_t* keys, int64_t keys_bytes,
                                   float* cam_pix, fp_stream_t stream) {
  FP_REQUIRE(gt_shape_ok(1, H, W), GT_SHAPE_MSG, "fp_gt_flatten_splat", 1, H, W);
  FP_REQUIRE(world && ground_seg && intrinsics && plane && keys, "fp_gt_flatten_splat: null pointer");
  FP_REQUIRE(keys_bytes >= fp_gt_workspace(1, H, W), "fp_gt_flatten_splat: key plane of %lld bytes, needs %lld", (long long)keys_bytes,
             (long long)fp_gt_workspace(1, H, W));
  const int HW = H * W;
  gt_offsets offs;                                               // numpy.arange(-0.1, 0.1, 0.025): start + i * ((start + step) - start)
  const double start = -0.1, step = 0.025, second = start + step, delta = second - start;
  for (int i = 0; i < GT_OFFSETS; ++i) offs.v[i] = i == 0 ? start : i == 1 ? second : start + i * delta;
  if (int rc = gt_clear_keys(keys, HW, stream)) return rc;
  fp_launch(gt_flatten_splat_kernel, dim3((unsigned)fp_ceil_div(HW, GT_T), GT_OFFSETS), dim3(GT_T), 0, (hipStream_t)stream, world, ground_seg,
            (float)threshold, intrinsics, plane, offs, H, W, HW, (unsigned long long*)keys, cam_pix);
  return fp_check_launch("fp_gt_flatten_splat");
}

extern "C" int fp_gt_depth_mask(const uint64_t* keys, const float* depth, const float* ground_seg, int32_t H, int32_t W, uint8_t* mask,
                                float* projection, fp_stream_t stream) {
  FP_REQUIRE(gt_shape_ok(1, H, W), GT_SHAPE_MSG, "fp_gt_depth_mask", 1, H, W);
  FP_REQUIRE(keys && depth && ground_seg && mask, "fp_gt_depth_mask: null pointer");
  const int HW = H * W;
  fp_launch(gt_depth_mask_kernel, dim3((unsigned)fp_ceil_div(HW, GT_T)), dim3(GT_T), 0, (hipStream_t)stream, (const unsigned long long*)keys,
            depth, ground_seg, HW, mask, projection);
  return fp_check_launch("fp_gt_depth_mask");
}
