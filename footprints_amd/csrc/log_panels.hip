// The TensorBoard pictures of the trainer's log event (reference training/logger.py:19-67) as bytes, on the device.
//
// Per logged sample the reference writes the image, six label maps and five prediction maps, every map but the image stretched to
// [0, 1] by its own minimum and maximum (utils.py:58-66, normalise_image), disparities as 1 / (d + 1e-7) * (d > 0) (utils.py:45-48,
// depth_to_disp), the predicted disparity through the plasma map; tensorboardX turns the floats into bytes by (x * 255).astype(uint8).
// The prediction maps are what LossManager's visualisation branch builds for scale 1/1 (training/losses.py:54-78), taken here from the
// raw [B][4][H][W] network output: sigmoid on channels 0 and 1, sigmoid_to_depth on channels 2 and 3, the masked ground depth by
// sigmoid(channel 1) > 0.5.
//
// Two launches on the caller's stream, no workgroup waits for another:
//   lp_reduce_kernel   every workgroup folds the minimum and maximum of the eleven maps over its 1024 pixels and writes them as one row of
//                      partials (min and max do not depend on the order they are folded in: the result is deterministic);
//   lp_map_kernel      every workgroup folds its sample's rows of partials (a few KB, from L2), then maps its 1024 pixels to bytes.
// Both evaluate a pixel's eleven pre-normalisation values through lp_values, with floating-point contraction off: the map sees the bits
// the reduction saw, so a map's minimum becomes byte 0 and its maximum byte 255, and every multiply followed by an add rounds twice as
// in the reference's float32 tensor arithmetic.  The file is built with -ffp-contract=off as well (Makefile).
//
// A thread owns four consecutive pixels: one 16-byte load per input plane and three dword stores per panel when H * W is a multiple of four
// and the planes are 16-byte aligned, scalar loads and byte stores otherwise.
#include <math.h>

#include "fp_common.h"

namespace {

constexpr int LP_THREADS = 256;
constexpr int LP_PX = 4;                          // pixels per thread
constexpr int LP_TILE = LP_THREADS * LP_PX;       // pixels per workgroup
constexpr int LP_K = 11;                          // normalised maps per sample (the moving-object map included, present or not)
constexpr int LP_ROW = 2 * LP_K;                  // floats of one row of partials: LP_K minima, then LP_K maxima
constexpr int LP_GROUPS = LP_THREADS / 32;        // the map kernel folds the rows in this many interleaved groups

// label planes in the order of the entry point's arguments
enum { LP_VISIBLE = 0, LP_DEPTH, LP_GROUND_DEPTH, LP_MOVING, LP_DEPTH_MASK, LP_ALL_GROUND, LP_LABELS };

struct LpArgs {
  const float* image;               // [B][3][HW]
  const float* label[LP_LABELS];    // [B][HW] each; label[LP_MOVING] may be null
  const float* pred;                // [B][4][HW]
  const unsigned char* lut;         // [256][3]
  unsigned char* out;               // [n][P][HW][3]
  float* part;                      // [n][nblk][LP_ROW]
  int32_t HW, nblk, P, vec;
  float min_disp, disp_range;       // sigmoid_to_depth's 1 / max_depth and 1 / min_depth - 1 / max_depth, rounded from double
};

__device__ __forceinline__ float lp_disp(float d) {
#pragma clang fp contract(off)
  return (1.0f / (d + 1e-7f)) * (d > 0.0f ? 1.0f : 0.0f);
}

__device__ __forceinline__ float lp_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

// the eleven values of one pixel before normalisation, in panel order (the image aside): t = the six labels, p = the four channels
__device__ __forceinline__ void lp_values(const LpArgs& a, const float t[LP_LABELS], const float p[4], float v[LP_K]) {
#pragma clang fp contract(off)
  v[0] = lp_disp(t[LP_DEPTH]);
  v[1] = t[LP_VISIBLE];
  v[2] = t[LP_ALL_GROUND];
  v[3] = t[LP_GROUND_DEPTH];
  v[4] = t[LP_DEPTH_MASK];
  v[5] = t[LP_MOVING];
  const float s0 = lp_sigmoid(p[0]), s1 = lp_sigmoid(p[1]);
  const float d2 = 1.0f / (a.min_disp + a.disp_range * p[2]);
  const float d3 = 1.0f / (a.min_disp + a.disp_range * p[3]);
  v[6] = lp_disp(d2);
  v[7] = s0;
  v[8] = s1;
  v[9] = lp_disp(d3);
  v[10] = lp_disp(d3 * (s1 > 0.5f ? 1.0f : 0.0f));
}

// four consecutive floats of a plane from pixel px0 on; pixels at or behind HW read as 0
__device__ __forceinline__ void lp_load4(const float* __restrict__ plane, int px0, int HW, int vec, float o[LP_PX]) {
  if (vec) {                                       // HW % 4 == 0: the four pixels are inside together or outside together
    if (px0 < HW) {
      const float4 q = *reinterpret_cast<const float4*>(plane + px0);
      o[0] = q.x; o[1] = q.y; o[2] = q.z; o[3] = q.w;
    } else {
      o[0] = o[1] = o[2] = o[3] = 0.0f;
    }
  } else {
#pragma unroll
    for (int j = 0; j < LP_PX; ++j) o[j] = px0 + j < HW ? plane[px0 + j] : 0.0f;
  }
}

// labels and channels of the thread's four pixels of sample s
__device__ __forceinline__ void lp_load_maps(const LpArgs& a, int s, int px0, float t[LP_PX][LP_LABELS], float p[LP_PX][4]) {
  float q[LP_PX];
#pragma unroll
  for (int m = 0; m < LP_LABELS; ++m) {
    if (a.label[m]) {
      lp_load4(a.label[m] + (size_t)s * a.HW, px0, a.HW, a.vec, q);
    } else {
      q[0] = q[1] = q[2] = q[3] = 0.0f;
    }
#pragma unroll
    for (int j = 0; j < LP_PX; ++j) t[j][m] = q[j];
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    lp_load4(a.pred + ((size_t)s * 4 + c) * a.HW, px0, a.HW, a.vec, q);
#pragma unroll
    for (int j = 0; j < LP_PX; ++j) p[j][c] = q[j];
  }
}

// grid = (nblk, n)
__global__ void __launch_bounds__(LP_THREADS) lp_reduce_kernel(LpArgs a) {
  const int s = blockIdx.y, px0 = (blockIdx.x * LP_THREADS + threadIdx.x) * LP_PX;
  float mn[LP_K], mx[LP_K];
#pragma unroll
  for (int k = 0; k < LP_K; ++k) {
    mn[k] = INFINITY;
    mx[k] = -INFINITY;
  }
  float t[LP_PX][LP_LABELS], p[LP_PX][4];
  lp_load_maps(a, s, px0, t, p);
#pragma unroll
  for (int j = 0; j < LP_PX; ++j) {
    if (px0 + j < a.HW) {
      float v[LP_K];
      lp_values(a, t[j], p[j], v);
#pragma unroll
      for (int k = 0; k < LP_K; ++k) {
        mn[k] = fminf(mn[k], v[k]);
        mx[k] = fmaxf(mx[k], v[k]);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < LP_K; ++k) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      mn[k] = fminf(mn[k], __shfl_xor(mn[k], o, 64));
      mx[k] = fmaxf(mx[k], __shfl_xor(mx[k], o, 64));
    }
  }
  __shared__ float sh[LP_THREADS / 64][LP_ROW];
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < LP_K; ++k) {
      sh[threadIdx.x >> 6][k] = mn[k];
      sh[threadIdx.x >> 6][LP_K + k] = mx[k];
    }
  }
  __syncthreads();
  if (threadIdx.x < LP_ROW) {
    const int k = threadIdx.x;
    float r = sh[0][k];
    for (int w = 1; w < LP_THREADS / 64; ++w) r = k < LP_K ? fminf(r, sh[w][k]) : fmaxf(r, sh[w][k]);
    a.part[((size_t)s * a.nblk + blockIdx.x) * LP_ROW + k] = r;
  }
}

__device__ __forceinline__ unsigned lp_byte(float x) {       // tensorboardX: (x * 255).astype(uint8), for x in [0, 1]
  const int i = (int)(x * 255.0f);
  return (unsigned)min(max(i, 0), 255);
}

// twelve bytes = four RGB pixels -> the panel's bytes from pixel px0 on
__device__ __forceinline__ void lp_store(unsigned char* __restrict__ panel, int px0, int HW, int vec, const unsigned c[LP_PX][3]) {
  if (vec) {
    if (px0 < HW) {
      unsigned* d = reinterpret_cast<unsigned*>(panel + (size_t)px0 * 3);
      d[0] = c[0][0] | c[0][1] << 8 | c[0][2] << 16 | c[1][0] << 24;
      d[1] = c[1][1] | c[1][2] << 8 | c[2][0] << 16 | c[2][1] << 24;
      d[2] = c[2][2] | c[3][0] << 8 | c[3][1] << 16 | c[3][2] << 24;
    }
  } else {
#pragma unroll
    for (int j = 0; j < LP_PX; ++j)
      if (px0 + j < HW) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) panel[(size_t)(px0 + j) * 3 + ch] = (unsigned char)c[j][ch];
      }
  }
}

// grid = (nblk, n)
__global__ void __launch_bounds__(LP_THREADS) lp_map_kernel(LpArgs a) {
  const int s = blockIdx.y, px0 = (blockIdx.x * LP_THREADS + threadIdx.x) * LP_PX;
  __shared__ float fold[LP_GROUPS][32];
  __shared__ float lo[LP_K], den[LP_K];
  __shared__ unsigned char lut[768];
  {
    // the sample's minima and maxima: group g folds rows g, g + LP_GROUPS, ...; then the groups are folded
    const int k = threadIdx.x & 31, g = threadIdx.x >> 5;
    if (k < LP_ROW) {
      float r = k < LP_K ? INFINITY : -INFINITY;
      const float* rows = a.part + (size_t)s * a.nblk * LP_ROW;
      for (int b = g; b < a.nblk; b += LP_GROUPS) {
        const float q = rows[(size_t)b * LP_ROW + k];
        r = k < LP_K ? fminf(r, q) : fmaxf(r, q);
      }
      fold[g][k] = r;
    }
    for (int i = threadIdx.x; i < 768; i += LP_THREADS) lut[i] = a.lut[i];
  }
  __syncthreads();
  if (threadIdx.x < LP_K) {
    const int k = threadIdx.x;
    float m0 = fold[0][k], m1 = fold[0][LP_K + k];
    for (int g = 1; g < LP_GROUPS; ++g) {
      m0 = fminf(m0, fold[g][k]);
      m1 = fmaxf(m1, fold[g][LP_K + k]);
    }
    lo[k] = m0;
    den[k] = m1 != m0 ? (float)((double)m1 - (double)m0) : 1e5f;       // normalise_image: the difference is taken in float64
  }
  __syncthreads();

  const bool moving = a.label[LP_MOVING] != nullptr;
  unsigned char* out = a.out + (size_t)s * a.P * a.HW * 3;
  unsigned c[LP_PX][3];
  {
    float im[3][LP_PX];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) lp_load4(a.image + ((size_t)s * 3 + ch) * a.HW, px0, a.HW, a.vec, im[ch]);
#pragma unroll
    for (int j = 0; j < LP_PX; ++j) {
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) c[j][ch] = lp_byte(im[ch][j]);
    }
    lp_store(out, px0, a.HW, a.vec, c);
  }
  float t[LP_PX][LP_LABELS], p[LP_PX][4];
  lp_load_maps(a, s, px0, t, p);
  float x[LP_PX][LP_K];
#pragma unroll
  for (int j = 0; j < LP_PX; ++j) {
    float v[LP_K];
    lp_values(a, t[j], p[j], v);
#pragma unroll
    for (int k = 0; k < LP_K; ++k) x[j][k] = (v[k] - lo[k]) / den[k];
  }
#pragma unroll
  for (int k = 0; k < LP_K; ++k) {
    if (k == 5 && !moving) continue;
    const int panel = 1 + k - (k > 5 && !moving ? 1 : 0);
#pragma unroll
    for (int j = 0; j < LP_PX; ++j) {
      if (k == 6) {                               // plt.cm.plasma of a float: x * 256 truncated, 256 -> 255
        const int idx = min(max((int)(x[j][k] * 256.0f), 0), 255);
        c[j][0] = lut[idx * 3];
        c[j][1] = lut[idx * 3 + 1];
        c[j][2] = lut[idx * 3 + 2];
      } else {
        c[j][0] = c[j][1] = c[j][2] = lp_byte(x[j][k]);
      }
    }
    lp_store(out + (size_t)panel * a.HW * 3, px0, a.HW, a.vec, c);
  }
}

bool lp_sizes_ok(int32_t n, int32_t H, int32_t W) {
  return n > 0 && n <= 65535 && H > 0 && W > 0 && (int64_t)H * W <= ((int64_t)1 << 28);
}

}  // namespace

extern "C" int64_t fp_log_panels_workspace(int32_t n, int32_t H, int32_t W) {
  if (!lp_sizes_ok(n, H, W)) return -1;
  return (int64_t)n * fp_ceil_div((int64_t)H * W, LP_TILE) * LP_ROW * (int64_t)sizeof(float);
}

extern "C" int fp_log_panels(const float* image, const float* visible_ground, const float* depth, const float* ground_depth,
                             const float* moving_object_mask, const float* depth_mask, const float* all_ground, const float* pred,
                             const uint8_t* lut, uint8_t* out, int32_t B, int32_t n, int32_t H, int32_t W, double min_depth, double max_depth,
                             void* workspace, int64_t workspace_bytes, fp_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  FP_REQUIRE(image && visible_ground && depth && ground_depth && depth_mask && all_ground && pred && lut && out,
             "fp_log_panels: a null operand (only the moving-object mask may be absent)");
  FP_REQUIRE(lp_sizes_ok(n, H, W) && n <= B, "fp_log_panels: bad sizes (1 <= n <= B, H * W <= 2^28)");
  FP_REQUIRE(min_depth > 0.0 && max_depth > min_depth, "fp_log_panels: bad depth range");
  const int64_t need = fp_log_panels_workspace(n, H, W);
  FP_REQUIRE(workspace && workspace_bytes >= need, "fp_log_panels: workspace too small (%lld < %lld bytes)", (long long)workspace_bytes,
             (long long)need);
  LpArgs a;
  a.image = image;
  a.label[LP_VISIBLE] = visible_ground;
  a.label[LP_DEPTH] = depth;
  a.label[LP_GROUND_DEPTH] = ground_depth;
  a.label[LP_MOVING] = moving_object_mask;
  a.label[LP_DEPTH_MASK] = depth_mask;
  a.label[LP_ALL_GROUND] = all_ground;
  a.pred = pred;
  a.lut = lut;
  a.out = out;
  a.part = (float*)workspace;
  a.HW = H * W;
  a.nblk = (int32_t)fp_ceil_div(a.HW, LP_TILE);
  a.P = moving_object_mask ? 12 : 11;
  // wide accesses: every plane starts at a multiple of HW floats behind its base, every panel at a multiple of HW * 3 bytes
  uintptr_t bits = (uintptr_t)image | (uintptr_t)pred | (uintptr_t)out;
  for (int m = 0; m < LP_LABELS; ++m) bits |= (uintptr_t)a.label[m];
  a.vec = (a.HW % 4 == 0 && bits % 16 == 0) ? 1 : 0;
  // sigmoid_to_depth (utils.py:36-42): Python floats, rounded to float32 where they meet the tensor
  const double min_disp = 1.0 / max_depth, max_disp = 1.0 / min_depth;
  a.min_disp = (float)min_disp;
  a.disp_range = (float)(max_disp - min_disp);
  const dim3 grid((unsigned)a.nblk, (unsigned)n);
  fp_launch(lp_reduce_kernel, grid, dim3(LP_THREADS), 0, stream, a);
  int rc = fp_check_launch("fp_log_panels(reduce)");
  if (rc != FP_OK) return rc;
  fp_launch(lp_map_kernel, grid, dim3(LP_THREADS), 0, stream, a);
  return fp_check_launch("fp_log_panels(map)");
}
