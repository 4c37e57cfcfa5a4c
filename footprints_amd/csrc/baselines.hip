// The paper's comparison baselines (reference footprints/baselines/): the convex hull of a batch of masks with the semantics of
// skimage.morphology.convex_hull_image, and the RANSAC ground plane of ransac.py / footprint_baseline.ransac_depth_inpaint for a batch
// of frames.  Wave = 64; plain C++ HIP; every launch count is independent of the batch size.
//
// A mask is uint8 (non-zero = set) or float16 / float32 with a threshold (value > threshold, compared in the mask's own dtype as
// numpy compares an array with a Python scalar: the entry point rounds the threshold to that dtype, and the comparison of the two
// values widened to float is then exact).
//
// Convex hull.  skimage takes, for every foreground pixel (r, c), the four points (r +- 1/2, c), (r, c +- 1/2) and sets a pixel iff
// its centre lies inside or on their hull.  In doubled coordinates Y = 2 r, X = 2 c every point is an integer: the set has the
// 2 H + 1 levels Y = -1 .. 2 H - 1, level Y = 2 r spans X in [2 first(r) - 1, 2 last(r) + 1] and level Y = 2 r + 1 spans
// [2 min(first(r), first(r+1)), 2 max(last(r), last(r+1))], so the hull of the whole set is the hull of at most two points per level,
// already sorted by Y.  The left side is the lower convex envelope of X_min(Y), the right side the upper concave envelope of
// X_max(Y); the centre (2 r, 2 c) is inside iff X_left(2 r) <= 2 c <= X_right(2 r), both bounds rational numbers compared with exact
// integer division.  No floating point anywhere.  |Y| <= 2 H and |X| <= 2 W + 1 fit int32 for the supported shapes and every cross
// product and numerator is formed in int64, whose magnitude stays below 2^32.
//   hull_rows_kernel   one wave per row: first and last foreground column by ballot               -> spans[b][r] = {first, last}
//   hull_chain_kernel  one workgroup per frame: levels and both monotone chains in LDS, then each row's inclusive pixel span
//                      [ceil(X_left / 2), floor(X_right / 2)]                                     -> spans[b][r] = {lo, hi} (in place)
//   hull_fill_kernel   out = lo <= c <= hi, then the BoundingBox epilogue (remove < 0.5 clears, keep sets), four pixels per thread
//
// RANSAC plane.  Points are depth * (inv_K . (x, y, 1)) in float64; a candidate is the unit 4-vector m spanning the null space of its
// three augmented sample points (normal (p1 - p0) x (p2 - p0), offset -n . p0 -- the 3 x 3 minors of ransac.estimate's matrix --
// divided by the 4-norm); a masked point is an inlier iff |m . (p, 1)| < 0.05; the winner is the first candidate with the strictly
// largest count.  A candidate that repeats a rank, has a rank out of range or whose minors are all zero is the zero vector, scores 0
// and is never chosen (the rule of gt_plane_build_kernel in gt_gen.hip).
//   plane_build_kernel  one workgroup per frame: rank -> pixel over 1024 coalesced segments (counts by ballot, a scan, then a wave
//                       per sample picks the rank's set bit), the C candidates, and zeroed counts
//   plane_score_kernel  every masked point is read ONCE and tested against all C candidates held in LDS; C LDS counters per workgroup
//   plane_select_kernel one thread per frame
//   plane_depth_kernel  depth - (m . (p, 1)) / (rhat . m[:3]) at every pixel, float64
#include <limits.h>

#include "fp_common.h"

namespace {

constexpr int BL_T = 256;
constexpr int BL_BUILD_T = 1024;
constexpr int BL_MAX_C = 100;
constexpr int BL_PTS = 4;                      // points per thread of plane_score_kernel
constexpr int BL_MAX_H = 2040;                 // 16 bytes of LDS per level, 2 H + 1 levels, 64 KiB
constexpr int BL_MAX_W = 32768;
enum { BL_U8 = 0, BL_F16 = 1, BL_F32 = 2 };

__device__ __forceinline__ bool bl_set(const void* __restrict__ p, int dtype, size_t i, float thr) {
  if (dtype == BL_U8) return static_cast<const uint8_t*>(p)[i] != 0;
  if (dtype == BL_F16) return (float)static_cast<const _Float16*>(p)[i] > thr;
  return static_cast<const float*>(p)[i] > thr;
}
// the BoundingBox baseline's `bounding_box_mask < 0.5`
__device__ __forceinline__ bool bl_below_half(const void* __restrict__ p, int dtype, size_t i) {
  if (dtype == BL_U8) return static_cast<const uint8_t*>(p)[i] == 0;
  if (dtype == BL_F16) return (float)static_cast<const _Float16*>(p)[i] < 0.5f;
  return static_cast<const float*>(p)[i] < 0.5f;
}

// ---------------------------------------------------------------------------------------------------------------- convex hull
__global__ void __launch_bounds__(BL_T) hull_rows_kernel(const void* __restrict__ x, int dtype, float thr, int rows, int W, int2* __restrict__ spans) {
  const int row = blockIdx.x * (BL_T / 64) + (int)(threadIdx.x >> 6);
  if (row >= rows) return;                                                           // wave-uniform
  const int lane = (int)(threadIdx.x & 63);
  const size_t base = (size_t)row * W;
  int first = W, last = -1;
  for (int c0 = 0; c0 < W; c0 += 64) {
    const int c = c0 + lane;
    const unsigned long long m = __ballot(c < W && bl_set(x, dtype, base + c, thr));
    if (m) {
      if (last < 0) first = c0 + __builtin_ctzll(m);
      last = c0 + 63 - __builtin_clzll(m);
    }
  }
  if (lane == 0) spans[row] = make_int2(first, last);
}

__device__ __forceinline__ long long bl_floor_div(long long a, long long b) {          // b > 0
  const long long q = a / b;
  return (a % b != 0 && a < 0) ? q - 1 : q;
}

// dynamic LDS: xmin[L], xmax[L], left[L], right[L] with L = 2 H + 1 levels (level index l = Y + 1)
__global__ void __launch_bounds__(BL_T) hull_chain_kernel(int H, int W, int2* __restrict__ spans) {
  extern __shared__ int bl_lds[];
  __shared__ int nleft, nright;
  const int L = 2 * H + 1;
  int* xmin = bl_lds;
  int* xmax = xmin + L;
  int* left = xmax + L;
  int* right = left + L;
  int2* sp = spans + (size_t)blockIdx.x * H;
  const int t = (int)threadIdx.x;
  for (int l = t; l < L; l += BL_T) {
    int lo = INT_MAX, hi = INT_MIN;
    if (l & 1) {                                                                     // Y = 2 r
      const int2 e = sp[l >> 1];
      if (e.y >= 0) lo = 2 * e.x - 1, hi = 2 * e.y + 1;
    } else {                                                                         // Y = 2 ra + 1 = 2 rb - 1
      const int ra = (l >> 1) - 1, rb = l >> 1;
      if (ra >= 0) {
        const int2 e = sp[ra];
        if (e.y >= 0) lo = 2 * e.x, hi = 2 * e.y;
      }
      if (rb < H) {
        const int2 e = sp[rb];
        if (e.y >= 0) lo = min(lo, 2 * e.x), hi = max(hi, 2 * e.y);
      }
    }
    xmin[l] = lo;
    xmax[l] = hi;
  }
  __syncthreads();
  // the two chains, one lane of two different waves each: a point stays iff it lies strictly outside the segment that skips it
  if (t == 0 || t == 64) {
    const bool is_left = t == 0;
    const int* xs = is_left ? xmin : xmax;
    int* st = is_left ? left : right;
    const int none = is_left ? INT_MAX : INT_MIN;
    int n = 0;
    long long y0 = 0, x0 = 0, y1 = 0, x1 = 0;                                          // the two topmost points, kept in registers
    for (int l0 = 0; l0 < L; l0 += 8) {
      int xv[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) xv[j] = l0 + j < L ? xs[l0 + j] : none;              // eight independent LDS reads ahead of the serial part
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        if (xv[j] == none) continue;
        const long long yp = l0 + j, xp = xv[j];
        while (n >= 2) {
          const long long cross = (y1 - y0) * (xp - x0) - (x1 - x0) * (yp - y0);
          if (is_left ? cross > 0 : cross < 0) break;
          --n;                                                                       // pop: the second point becomes the top
          y1 = y0, x1 = x0;
          if (n >= 2) y0 = st[n - 2], x0 = xs[st[n - 2]];
        }
        st[n++] = (int)yp;
        y0 = y1, x0 = x1, y1 = yp, x1 = xp;
      }
    }
    if (is_left) nleft = n;
    else nright = n;
  }
  __syncthreads();
  const int nl = nleft, nr = nright;
  for (int r = t; r < H; r += BL_T) {
    int2 out = make_int2(1, 0);                                                      // empty
    const int l = 2 * r + 1;
    if (nl >= 2 && l >= left[0] && l <= left[nl - 1]) {                                // both chains start and end on the same levels
      long long bound[2];
      for (int side = 0; side < 2; ++side) {
        const int* st = side ? right : left;
        const int* xs = side ? xmax : xmin;
        int a = 0, b = (side ? nr : nl) - 1;                                           // largest a with st[a] <= l, a < n - 1
        while (b - a > 1) {
          const int mid = (a + b) >> 1;
          if (st[mid] <= l) a = mid;
          else b = mid;
        }
        const long long y0 = st[a], x0 = xs[st[a]], dy = st[a + 1] - st[a], dx = xs[st[a + 1]] - xs[st[a]];
        const long long num = x0 * dy + dx * (l - y0);                                 // X(l) = num / dy, the pixel bound is X / 2
        bound[side] = side ? bl_floor_div(num, 2 * dy) : -bl_floor_div(-num, 2 * dy);
      }
      out = make_int2((int)max(bound[0], 0ll), (int)min(bound[1], (long long)W - 1));
    }
    sp[r] = out;
  }
}

__global__ void __launch_bounds__(BL_T) hull_fill_kernel(const int2* __restrict__ spans, const void* __restrict__ remove, int remove_dtype,
                                                         const void* __restrict__ keep, int keep_dtype, float keep_thr, long long total, int W,
                                                         uint8_t* __restrict__ out) {
  const long long i0 = ((long long)blockIdx.x * BL_T + threadIdx.x) * 4;
  if (i0 >= total) return;
  uint8_t v[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const long long i = i0 + k;
    v[k] = 0;
    if (i < total) {
      const long long row = i / W;
      const int c = (int)(i - row * W);
      const int2 s = spans[row];
      bool on = c >= s.x && c <= s.y;
      if (remove && bl_below_half(remove, remove_dtype, (size_t)i)) on = false;
      if (keep && bl_set(keep, keep_dtype, (size_t)i, keep_thr)) on = true;
      v[k] = on ? 1 : 0;
    }
  }
  if (i0 + 4 <= total) {
    *reinterpret_cast<uchar4*>(out + i0) = make_uchar4(v[0], v[1], v[2], v[3]);       // i0 is a multiple of 4
  } else {
    for (int k = 0; k < 4 && i0 + k < total; ++k) out[i0 + k] = v[k];
  }
}

// ---------------------------------------------------------------------------------------------------------------- RANSAC plane
__global__ void __launch_bounds__(BL_BUILD_T) mask_counts_kernel(const void* __restrict__ x, int dtype, float thr, int HW, int* __restrict__ counts) {
  __shared__ int part[BL_BUILD_T / 64];
  const size_t base = (size_t)blockIdx.x * HW;
  const int t = (int)threadIdx.x;
  int mine = 0;
  for (int i0 = 0; i0 < HW; i0 += BL_BUILD_T) {
    const int i = i0 + t;
    mine += __popcll(__ballot(i < HW && bl_set(x, dtype, base + i, thr)));            // the wave's count, in every lane
  }
  if ((t & 63) == 0) part[t >> 6] = mine;
  __syncthreads();
  if (t == 0) {
    int s = 0;
    for (int w = 0; w < BL_BUILD_T / 64; ++w) s += part[w];
    counts[blockIdx.x] = s;
  }
}

// camera ray of pixel (x, y): inv_K[:3, :3] . (x, y, 1)
__device__ __forceinline__ void bl_ray(const double* __restrict__ iK, int x, int y, double (&ray)[3]) {
#pragma unroll
  for (int j = 0; j < 3; ++j) ray[j] = (iK[j * 3 + 0] * (double)x + iK[j * 3 + 1] * (double)y) + iK[j * 3 + 2];
}

__global__ void __launch_bounds__(BL_BUILD_T) plane_build_kernel(const float* __restrict__ depth, const double* __restrict__ inv_K,
                                                                 const void* __restrict__ mask, int dtype, float thr,
                                                                 const int* __restrict__ samples, int C, int HW, int W,
                                                                 int* __restrict__ sample_pix, double* __restrict__ planes, int* __restrict__ counts) {
  __shared__ int off[BL_BUILD_T + 1];
  __shared__ int tmp[BL_BUILD_T];
  __shared__ int spix[3 * BL_MAX_C];
  const int b = blockIdx.x, t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
  const size_t base = (size_t)b * HW;
  const int seg = ((HW + BL_BUILD_T - 1) / BL_BUILD_T + 63) / 64 * 64;                // pixels per segment, a multiple of the wave
  int mine = 0;
  for (int k = 0; k < 64; ++k) {                                                     // this wave's 64 segments; lane k keeps segment k's count
    const long long beg = (long long)(wave * 64 + k) * seg;
    const int end = (int)min(beg + seg, (long long)HW);
    int cnt = 0;
    for (long long i0 = beg; i0 < end; i0 += 64) {
      const long long i = i0 + lane;
      cnt += __popcll(__ballot(i < end && bl_set(mask, dtype, base + (size_t)i, thr)));
    }
    if (lane == k) mine = cnt;
  }
  tmp[t] = mine;
  __syncthreads();
  for (int s = 1; s < BL_BUILD_T; s <<= 1) {                                         // inclusive scan
    const int add = t >= s ? tmp[t - s] : 0;
    __syncthreads();
    tmp[t] += add;
    __syncthreads();
  }
  off[t + 1] = tmp[t];
  if (t == 0) off[0] = 0;
  __syncthreads();
  const int total = off[BL_BUILD_T];
  const int* smp = samples + (size_t)b * 3 * C;
  for (int s = wave; s < 3 * C; s += BL_BUILD_T / 64) {                               // one wave per sample
    const int r = __builtin_amdgcn_readfirstlane(smp[s]);
    int pix = -1;
    if (r >= 0 && r < total) {
      int lo = 0, hi = BL_BUILD_T;                                                   // largest lo with off[lo] <= r
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= r) lo = mid;
        else hi = mid;
      }
      int rank = off[lo];
      const long long beg = (long long)lo * seg;
      const int end = (int)min(beg + seg, (long long)HW);
      for (long long i0 = beg; i0 < end; i0 += 64) {
        const long long i = i0 + lane;
        const bool g = i < end && bl_set(mask, dtype, base + (size_t)i, thr);
        const unsigned long long m = __ballot(g);
        const int pc = __popcll(m);
        if (rank + pc > r) {                                                         // the rank's pixel is the (r - rank)-th set bit of m
          const bool hit = g && __popcll(m & ((1ull << lane) - 1ull)) == r - rank;
          pix = (int)i0 + __builtin_ctzll(__ballot(hit));
          break;
        }
        rank += pc;
      }
    }
    if (lane == 0) {
      spix[s] = pix;
      sample_pix[(size_t)b * 3 * C + s] = pix;
    }
  }
  __syncthreads();
  if (t < C) {
    const double* iK = inv_K + (size_t)b * 9;
    double P[3][3];
    bool ok = smp[3 * t] != smp[3 * t + 1] && smp[3 * t] != smp[3 * t + 2] && smp[3 * t + 1] != smp[3 * t + 2];
    for (int k = 0; k < 3; ++k) {
      const int pix = spix[3 * t + k];
      P[k][0] = P[k][1] = P[k][2] = 0.0;
      if (pix < 0) {
        ok = false;
        continue;
      }
      double ray[3];
      bl_ray(iK, pix % W, pix / W, ray);
      const double d = (double)depth[base + pix];
      for (int j = 0; j < 3; ++j) P[k][j] = d * ray[j];
    }
    const double a0 = P[1][0] - P[0][0], a1 = P[1][1] - P[0][1], a2 = P[1][2] - P[0][2];
    const double b0 = P[2][0] - P[0][0], b1 = P[2][1] - P[0][1], b2 = P[2][2] - P[0][2];
    double m[4] = {a1 * b2 - a2 * b1, a2 * b0 - a0 * b2, a0 * b1 - a1 * b0, 0.0};
    m[3] = -((m[0] * P[0][0] + m[1] * P[0][1]) + m[2] * P[0][2]);
    const double n3 = (m[0] * m[0] + m[1] * m[1]) + m[2] * m[2];
    const double n4 = sqrt(n3 + m[3] * m[3]);
    const bool good = ok && n3 > 0.0 && n4 < INFINITY;
    for (int k = 0; k < 4; ++k) planes[((size_t)b * C + t) * 4 + k] = good ? m[k] / n4 : 0.0;
    counts[(size_t)b * C + t] = 0;
  }
}

// grid (chunks, B): BL_T * BL_PTS pixels per workgroup; the candidates and their counters live in LDS
__global__ void __launch_bounds__(BL_T) plane_score_kernel(const float* __restrict__ depth, const double* __restrict__ inv_K,
                                                           const void* __restrict__ mask, int dtype, float thr,
                                                           const double* __restrict__ planes, int C, int HW, int W, int* __restrict__ counts) {
  __shared__ double pl[BL_MAX_C * 4];
  __shared__ int cnt[BL_MAX_C];
  const int b = blockIdx.y, t = (int)threadIdx.x;
  const size_t base = (size_t)b * HW;
  for (int i = t; i < 4 * C; i += BL_T) pl[i] = planes[(size_t)b * C * 4 + i];
  if (t < C) cnt[t] = 0;
  const double* iK = inv_K + (size_t)b * 9;
  double px[BL_PTS], py[BL_PTS], pz[BL_PTS];
  bool on[BL_PTS];
#pragma unroll
  for (int j = 0; j < BL_PTS; ++j) {
    const long long p = ((long long)blockIdx.x * BL_PTS + j) * BL_T + t;
    on[j] = p < HW && bl_set(mask, dtype, base + (size_t)p, thr);
    px[j] = py[j] = pz[j] = 0.0;
    if (on[j]) {
      double ray[3];
      bl_ray(iK, (int)(p % W), (int)(p / W), ray);
      const double d = (double)depth[base + p];
      px[j] = d * ray[0], py[j] = d * ray[1], pz[j] = d * ray[2];
    }
  }
  __syncthreads();
  for (int c = 0; c < C; ++c) {
    const double m0 = pl[4 * c], m1 = pl[4 * c + 1], m2 = pl[4 * c + 2], m3 = pl[4 * c + 3];
    if (m0 == 0.0 && m1 == 0.0 && m2 == 0.0 && m3 == 0.0) continue;                     // degenerate sample: scores 0 (block-uniform)
    int s = 0;
#pragma unroll
    for (int j = 0; j < BL_PTS; ++j) {
      const double dist = ((m0 * px[j] + m1 * py[j]) + m2 * pz[j]) + m3;
      s += __popcll(__ballot(on[j] && fabs(dist) < 0.05));
    }
    if ((t & 63) == 0 && s) atomicAdd(cnt + c, s);
  }
  __syncthreads();
  if (t < C && cnt[t]) atomicAdd(counts + (size_t)b * C + t, cnt[t]);                  // integer sums: independent of the order
}

// first candidate with the strictly largest count                                                            [ransac.run_ransac]
__global__ void plane_select_kernel(const double* __restrict__ planes, const int* __restrict__ counts, int C, int B, double* __restrict__ best_plane,
                                    int* __restrict__ best) {
  const int b = blockIdx.x * 64 + (int)threadIdx.x;
  if (b >= B) return;
  int bi = -1, bc = 0;
  for (int c = 0; c < C; ++c) {
    const int n = counts[(size_t)b * C + c];
    if (n > bc) bc = n, bi = c;
  }
  for (int k = 0; k < 4; ++k) best_plane[b * 4 + k] = bi >= 0 ? planes[((size_t)b * C + bi) * 4 + k] : 0.0;
  best[b * 2 + 0] = bi;
  best[b * 2 + 1] = bc;
}

// grid (chunks, B)                                                                       [footprint_baseline.ransac_depth_inpaint]
__global__ void __launch_bounds__(BL_T) plane_depth_kernel(const float* __restrict__ depth, const double* __restrict__ inv_K,
                                                           const double* __restrict__ best_plane, const uint8_t* __restrict__ passthrough, int HW,
                                                           int W, double* __restrict__ out) {
  const int b = blockIdx.y;
  const long long p = (long long)blockIdx.x * BL_T + threadIdx.x;
  if (p >= HW) return;
  const size_t i = (size_t)b * HW + (size_t)p;
  const double d = (double)depth[i];
  if (passthrough && passthrough[b]) {
    out[i] = d;
    return;
  }
  const double* m = best_plane + (size_t)b * 4;
  double ray[3];
  bl_ray(inv_K + (size_t)b * 9, (int)(p % W), (int)(p / W), ray);
  const double dist = ((m[0] * (d * ray[0]) + m[1] * (d * ray[1])) + m[2] * (d * ray[2])) + m[3];
  const double len = sqrt((ray[0] * ray[0] + ray[1] * ray[1]) + ray[2] * ray[2]);
  const double dot = ((ray[0] / len) * m[0] + (ray[1] / len) * m[1]) + (ray[2] / len) * m[2];
  out[i] = d - dist / dot;
}

bool bl_shape_ok(int64_t B, int64_t H, int64_t W) { return B >= 1 && B <= 65535 && H >= 1 && W >= 1 && W <= BL_MAX_W && H * W < ((int64_t)1 << 30) && B * H * W < ((int64_t)1 << 40); }
#define BL_SHAPE_MSG "%s: needs 1 <= B <= 65535 frames, W <= 32768 and H * W < 2^30 (got %d x %d x %d)"
bool bl_dtype_ok(int d) { return d == BL_U8 || d == BL_F16 || d == BL_F32; }
// the threshold in the mask's own dtype, widened back to float
float bl_threshold(int dtype, double threshold) { return dtype == BL_F16 ? (float)(_Float16)threshold : (float)threshold; }

}  // namespace

extern "C" int fp_baseline_hull(const void* x, int32_t dtype, double threshold, const void* remove, int32_t remove_dtype, const void* keep,
                                int32_t keep_dtype, double keep_threshold, int32_t B, int32_t H, int32_t W, int32_t* spans, uint8_t* out,
                                fp_stream_t stream) {
  FP_REQUIRE(bl_shape_ok(B, H, W), BL_SHAPE_MSG, "fp_baseline_hull", B, H, W);
  // 2 H + 1 levels of four int32 in 64 KiB of LDS; doubled coordinates |X| <= 2 W + 1 in int32, cross products in int64 (< 2^32)
  FP_REQUIRE(H <= BL_MAX_H, "fp_baseline_hull: needs H <= %d rows (got %d)", BL_MAX_H, H);
  FP_REQUIRE(x && spans && out, "fp_baseline_hull: null pointer");
  FP_REQUIRE(bl_dtype_ok(dtype) && (!remove || bl_dtype_ok(remove_dtype)) && (!keep || bl_dtype_ok(keep_dtype)),
             "fp_baseline_hull: dtype codes are 0 = uint8, 1 = float16, 2 = float32");
  hipStream_t s = (hipStream_t)stream;
  const int rows = B * H;
  const long long total = (long long)rows * W;
  int2* sp = reinterpret_cast<int2*>(spans);
  fp_launch(hull_rows_kernel, dim3((unsigned)fp_ceil_div(rows, BL_T / 64)), dim3(BL_T), 0, s, x, dtype, bl_threshold(dtype, threshold), rows, W, sp);
  fp_launch(hull_chain_kernel, dim3(B), dim3(BL_T), (unsigned)(4 * sizeof(int) * (2 * H + 1)), s, H, W, sp);
  fp_launch(hull_fill_kernel, dim3((unsigned)fp_ceil_div(total, BL_T * 4)), dim3(BL_T), 0, s, (const int2*)sp, remove, remove_dtype, keep, keep_dtype,
            bl_threshold(keep_dtype, keep_threshold), total, W, out);
  return fp_check_launch("fp_baseline_hull");
}

extern "C" int fp_baseline_mask_counts(const void* x, int32_t dtype, double threshold, int32_t B, int32_t H, int32_t W, int32_t* counts,
                                       fp_stream_t stream) {
  FP_REQUIRE(bl_shape_ok(B, H, W), BL_SHAPE_MSG, "fp_baseline_mask_counts", B, H, W);
  FP_REQUIRE(x && counts, "fp_baseline_mask_counts: null pointer");
  FP_REQUIRE(bl_dtype_ok(dtype), "fp_baseline_mask_counts: dtype codes are 0 = uint8, 1 = float16, 2 = float32");
  fp_launch(mask_counts_kernel, dim3(B), dim3(BL_BUILD_T), 0, (hipStream_t)stream, x, dtype, bl_threshold(dtype, threshold), H * W, counts);
  return fp_check_launch("fp_baseline_mask_counts");
}

extern "C" int fp_baseline_plane_fit(const float* depth, const double* inv_K, const void* mask, int32_t dtype, double threshold,
                                     const int32_t* samples, int32_t C, int32_t B, int32_t H, int32_t W, int32_t* sample_pix, double* planes,
                                     int32_t* counts, double* best_plane, int32_t* best, fp_stream_t stream) {
  FP_REQUIRE(bl_shape_ok(B, H, W), BL_SHAPE_MSG, "fp_baseline_plane_fit", B, H, W);
  FP_REQUIRE(C >= 1 && C <= BL_MAX_C, "fp_baseline_plane_fit: needs 1 <= C <= %d candidates (got %d)", BL_MAX_C, C);
  FP_REQUIRE(depth && inv_K && mask && samples && sample_pix && planes && counts && best_plane && best, "fp_baseline_plane_fit: null pointer");
  FP_REQUIRE(bl_dtype_ok(dtype), "fp_baseline_plane_fit: dtype codes are 0 = uint8, 1 = float16, 2 = float32");
  hipStream_t s = (hipStream_t)stream;
  const int HW = H * W;
  const float thr = bl_threshold(dtype, threshold);
  fp_launch(plane_build_kernel, dim3(B), dim3(BL_BUILD_T), 0, s, depth, inv_K, mask, dtype, thr, samples, C, HW, W, sample_pix, planes, counts);
  fp_launch(plane_score_kernel, dim3((unsigned)fp_ceil_div(HW, BL_T * BL_PTS), B), dim3(BL_T), 0, s, depth, inv_K, mask, dtype, thr,
            (const double*)planes, C, HW, W, counts);
  fp_launch(plane_select_kernel, dim3((unsigned)fp_ceil_div(B, 64)), dim3(64), 0, s, (const double*)planes, (const int*)counts, C, B, best_plane, best);
  return fp_check_launch("fp_baseline_plane_fit");
}

extern "C" int fp_baseline_plane_depth(const float* depth, const double* inv_K, const double* best_plane, const uint8_t* passthrough, int32_t B,
                                       int32_t H, int32_t W, double* out, fp_stream_t stream) {
  FP_REQUIRE(bl_shape_ok(B, H, W), BL_SHAPE_MSG, "fp_baseline_plane_depth", B, H, W);
  FP_REQUIRE(depth && inv_K && best_plane && out, "fp_baseline_plane_depth: null pointer");
  const int HW = H * W;
  fp_launch(plane_depth_kernel, dim3((unsigned)fp_ceil_div(HW, BL_T), B), dim3(BL_T), 0, (hipStream_t)stream, depth, inv_K, best_plane, passthrough, HW, W,
            out);
  return fp_check_launch("fp_baseline_plane_depth");
}
