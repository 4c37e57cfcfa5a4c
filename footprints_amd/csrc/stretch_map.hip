// Pictures made by stretching a map to [0, 1] by its own minimum and maximum and reading a colour table, as bytes, on the device:
//   fp_seg_log_panels   the segmentation trainer's TensorBoard picture (reference preprocessing/segmentation/logger.py:28-42 followed by
//                       tensorboardX's (x.astype(float32) * 255).astype(uint8)): per logged sample [image | ground truth | prediction];
//   fp_stretch_colour   matplotlib's imsave of a 2-D array (the label generator's --save_visualisations): Normalize, then the colour map
//                       with bytes=True.
// Both are two launches on the caller's stream, the scheme of log_panels.hip; no workgroup waits for another:
//   *_reduce_kernel   every workgroup folds the minimum and maximum over its 1024 pixels and writes them as one row of partials (min and
//                     max do not depend on the order they are folded in: the result is deterministic);
//   *_map_kernel      every workgroup folds its sample's rows of partials (from L2), then maps its 1024 pixels to bytes.
// The values that are stretched are the inputs themselves, so the map sees the bits the reduction saw: a map's minimum becomes index 0 and
// its maximum the last index.  The file is built with -ffp-contract=off (Makefile): every operation rounds once, as in the reference's
// numpy arithmetic.  Finite inputs are the contract; a NaN gives some index inside the table, never an access outside it.
//
// A thread owns four consecutive pixels: one 16-byte load per float plane (one dword per byte plane) and three dword stores per panel
// where the sizes and the alignment keep the four pixels together, scalar loads and byte stores otherwise; the choice is made per launch
// for the loads and for the stores.
#include <math.h>

#include "fp_common.h"
#include "infer_out.h"      // sigmoid_exact, fp_store12

namespace {

constexpr int SM_THREADS = 256;
constexpr int SM_PX = 4;                          // pixels per thread
constexpr int SM_TILE = SM_THREADS * SM_PX;       // pixels per workgroup
constexpr int SM_WAVES = SM_THREADS / 64;

// four consecutive floats of a plane from pixel px0 on; pixels at or behind HW read as `fill`
__device__ __forceinline__ void sm_load4(const float* __restrict__ plane, int px0, int HW, int vec, float fill, float o[SM_PX]) {
  if (vec) {                                       // HW % 4 == 0: the four pixels are inside together or outside together
    if (px0 < HW) {
      const float4 q = *reinterpret_cast<const float4*>(plane + px0);
      o[0] = q.x; o[1] = q.y; o[2] = q.z; o[3] = q.w;
    } else {
      o[0] = o[1] = o[2] = o[3] = fill;
    }
  } else {
#pragma unroll
    for (int j = 0; j < SM_PX; ++j) o[j] = px0 + j < HW ? plane[px0 + j] : fill;
  }
}

// the same for a plane of bytes, as floats
__device__ __forceinline__ void sm_load4_u8(const unsigned char* __restrict__ plane, int px0, int HW, int vec, float fill, float o[SM_PX]) {
  if (vec) {
    if (px0 < HW) {
      const unsigned q = *reinterpret_cast<const unsigned*>(plane + px0);
      o[0] = (float)(q & 255u); o[1] = (float)((q >> 8) & 255u); o[2] = (float)((q >> 16) & 255u); o[3] = (float)(q >> 24);
    } else {
      o[0] = o[1] = o[2] = o[3] = fill;
    }
  } else {
#pragma unroll
    for (int j = 0; j < SM_PX; ++j) o[j] = px0 + j < HW ? (float)plane[px0 + j] : fill;
  }
}

// the workgroup's minimum and maximum -> part[0], part[1]
__device__ __forceinline__ void sm_block_minmax(float mn, float mx, float* __restrict__ part) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    mn = fminf(mn, __shfl_xor(mn, o, 64));
    mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  }
  __shared__ float sh[SM_WAVES][2];
  if ((threadIdx.x & 63) == 0) {
    sh[threadIdx.x >> 6][0] = mn;
    sh[threadIdx.x >> 6][1] = mx;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < SM_WAVES; ++w) {
      mn = fminf(mn, sh[w][0]);
      mx = fmaxf(mx, sh[w][1]);
    }
    part[0] = mn;
    part[1] = mx;
  }
}

// the sample's minimum and maximum out of its nblk rows of partials, in every thread; also loads the colour table (r | g << 8 | b << 16)
__device__ __forceinline__ void sm_fold(const float* __restrict__ rows, int nblk, const unsigned char* __restrict__ lut, unsigned colours[256],
                                        float& lo, float& hi) {
  float mn = INFINITY, mx = -INFINITY;
  for (int b = threadIdx.x; b < nblk; b += SM_THREADS) {
    mn = fminf(mn, rows[2 * (size_t)b]);
    mx = fmaxf(mx, rows[2 * (size_t)b + 1]);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    mn = fminf(mn, __shfl_xor(mn, o, 64));
    mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  }
  __shared__ float sh[SM_WAVES][2];
  if ((threadIdx.x & 63) == 0) {
    sh[threadIdx.x >> 6][0] = mn;
    sh[threadIdx.x >> 6][1] = mx;
  }
  {
    const int i = threadIdx.x;                     // SM_THREADS == 256 entries
    colours[i] = (unsigned)lut[3 * i] | ((unsigned)lut[3 * i + 1] << 8) | ((unsigned)lut[3 * i + 2] << 16);
  }
  __syncthreads();
  lo = sh[0][0];
  hi = sh[0][1];
#pragma unroll
  for (int w = 1; w < SM_WAVES; ++w) {
    lo = fminf(lo, sh[w][0]);
    hi = fmaxf(hi, sh[w][1]);
  }
}

__device__ __forceinline__ int sm_index(float x) {           // matplotlib's Colormap call on a float32 array: x * 256 truncated, 256 -> 255
  return min(max((int)(x * 256.0f), 0), 255);
}

// ---- the segmentation trainer's picture -------------------------------------------------------------------------------------------------
struct SegLogArgs {
  const float* image;               // [B][3][HW]
  const float* ground_mask;         // [B][HW]
  const float* logits;              // plane of sample s at logits + s * logit_stride
  int64_t logit_stride;
  const unsigned char* lut;         // [256][3]
  unsigned char* out;               // [n][H][3 W][3]
  float* part;                      // [n][nblk][2]
  int32_t HW, W, nblk, vec_in, vec_out;
};

// grid = (nblk, n)
__global__ void __launch_bounds__(SM_THREADS) seg_log_reduce_kernel(SegLogArgs a) {
  const int s = blockIdx.y, px0 = (blockIdx.x * SM_THREADS + threadIdx.x) * SM_PX;
  float mn = INFINITY, mx = -INFINITY;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    float v[SM_PX];
    sm_load4(a.image + ((size_t)s * 3 + ch) * a.HW, px0, a.HW, a.vec_in, 0.0f, v);
#pragma unroll
    for (int j = 0; j < SM_PX; ++j)
      if (px0 + j < a.HW) {
        mn = fminf(mn, v[j]);
        mx = fmaxf(mx, v[j]);
      }
  }
  sm_block_minmax(mn, mx, a.part + ((size_t)s * a.nblk + blockIdx.x) * 2);
}

// four pixels from flat pixel px0 on into panel `panel` of the sample's [H][3 W][3] picture
__device__ __forceinline__ void seg_log_store(const SegLogArgs& a, unsigned char* __restrict__ pic, int panel, int px0, const unsigned c[SM_PX]) {
  if (a.vec_out) {                                 // W % 4 == 0: the four pixels lie in one row
    if (px0 < a.HW) {
      const int y = px0 / a.W, x = px0 - y * a.W;
      fp_store12(pic + ((size_t)y * 3 * a.W + (size_t)panel * a.W + x) * 3, c, SM_PX, true);
    }
  } else {
#pragma unroll
    for (int j = 0; j < SM_PX; ++j)
      if (px0 + j < a.HW) {
        const int y = (px0 + j) / a.W, x = px0 + j - y * a.W;
        fp_store12(pic + ((size_t)y * 3 * a.W + (size_t)panel * a.W + x) * 3, c + j, 1, false);
      }
  }
}

// grid = (nblk, n)
__global__ void __launch_bounds__(SM_THREADS) seg_log_map_kernel(SegLogArgs a) {
  const int s = blockIdx.y, px0 = (blockIdx.x * SM_THREADS + threadIdx.x) * SM_PX;
  __shared__ unsigned colours[256];
  float lo, hi;
  sm_fold(a.part + (size_t)s * a.nblk * 2, a.nblk, a.lut, colours, lo, hi);
  const float den = hi != lo ? (float)((double)hi - (double)lo) : 1e5f;      // normalize_image: the difference is taken in float64
  unsigned char* pic = a.out + (size_t)s * a.HW * 9;
  unsigned c[SM_PX] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    float v[SM_PX];
    sm_load4(a.image + ((size_t)s * 3 + ch) * a.HW, px0, a.HW, a.vec_in, lo, v);
#pragma unroll
    for (int j = 0; j < SM_PX; ++j) {
      const float x = (v[j] - lo) / den;
      c[j] |= (unsigned)min(max((int)(x * 255.0f), 0), 255) << (8 * ch);
    }
  }
  seg_log_store(a, pic, 0, px0, c);
  float t[SM_PX];
  sm_load4(a.ground_mask + (size_t)s * a.HW, px0, a.HW, a.vec_in, 0.0f, t);
#pragma unroll
  for (int j = 0; j < SM_PX; ++j) c[j] = t[j] == 1.0f ? 255u : 0u;            // red alone
  seg_log_store(a, pic, 1, px0, c);
  sm_load4(a.logits + (size_t)s * a.logit_stride, px0, a.HW, a.vec_in, 0.0f, t);
#pragma unroll
  for (int j = 0; j < SM_PX; ++j) c[j] = colours[sm_index(sigmoid_exact(t[j]))];
  seg_log_store(a, pic, 2, px0, c);
}

// ---- imsave of a 2-D array --------------------------------------------------------------------------------------------------------------
struct StretchArgs {
  const void* maps;                 // [B][HW] float or uint8
  const unsigned char* lut;         // [256][3]
  unsigned char* out;               // [B][HW][3]
  float* part;                      // [B][nblk][2]
  int32_t HW, nblk, u8, vec_in, vec_out;
};

__device__ __forceinline__ void stretch_load(const StretchArgs& a, int s, int px0, float v[SM_PX]) {
  if (a.u8) sm_load4_u8((const unsigned char*)a.maps + (size_t)s * a.HW, px0, a.HW, a.vec_in, 0.0f, v);
  else sm_load4((const float*)a.maps + (size_t)s * a.HW, px0, a.HW, a.vec_in, 0.0f, v);
}

// grid = (nblk, B)
__global__ void __launch_bounds__(SM_THREADS) stretch_reduce_kernel(StretchArgs a) {
  const int s = blockIdx.y, px0 = (blockIdx.x * SM_THREADS + threadIdx.x) * SM_PX;
  float mn = INFINITY, mx = -INFINITY, v[SM_PX];
  stretch_load(a, s, px0, v);
#pragma unroll
  for (int j = 0; j < SM_PX; ++j)
    if (px0 + j < a.HW) {
      mn = fminf(mn, v[j]);
      mx = fmaxf(mx, v[j]);
    }
  sm_block_minmax(mn, mx, a.part + ((size_t)s * a.nblk + blockIdx.x) * 2);
}

// grid = (nblk, B)
__global__ void __launch_bounds__(SM_THREADS) stretch_map_kernel(StretchArgs a) {
  const int s = blockIdx.y, px0 = (blockIdx.x * SM_THREADS + threadIdx.x) * SM_PX;
  __shared__ unsigned colours[256];
  float lo, hi;
  sm_fold(a.part + (size_t)s * a.nblk * 2, a.nblk, a.lut, colours, lo, hi);
  const double range = (double)hi - (double)lo;
  float v[SM_PX];
  stretch_load(a, s, px0, v);
  unsigned c[SM_PX];
#pragma unroll
  for (int j = 0; j < SM_PX; ++j) {
    // Normalize: the subtraction in float32, the division in float64, rounded to float32; a constant map is 0 everywhere
    const float x = hi != lo ? (float)((double)(v[j] - lo) / range) : 0.0f;
    c[j] = colours[sm_index(x)];
  }
  unsigned char* pic = a.out + (size_t)s * a.HW * 3;
  if (a.vec_out) {
    if (px0 < a.HW) fp_store12(pic + (size_t)px0 * 3, c, SM_PX, true);
  } else if (px0 < a.HW) {
    fp_store12(pic + (size_t)px0 * 3, c, min(SM_PX, a.HW - px0), false);
  }
}

bool sm_sizes_ok(int32_t n, int32_t H, int32_t W) {
  return n > 0 && n <= 65535 && H > 0 && W > 0 && (int64_t)H * W <= ((int64_t)1 << 27);
}

int64_t sm_workspace(int32_t n, int32_t H, int32_t W) {
  if (!sm_sizes_ok(n, H, W)) return -1;
  return (int64_t)n * fp_ceil_div((int64_t)H * W, SM_TILE) * 2 * (int64_t)sizeof(float);
}

}  // namespace

extern "C" int64_t fp_seg_log_panels_workspace(int32_t n, int32_t H, int32_t W) { return sm_workspace(n, H, W); }

extern "C" int fp_seg_log_panels(const float* image, const float* ground_mask, const float* logits, int64_t logit_batch_stride, const uint8_t* lut,
                                 uint8_t* out, int32_t B, int32_t n, int32_t H, int32_t W, void* workspace, int64_t workspace_bytes,
                                 fp_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  FP_REQUIRE(image && ground_mask && logits && lut && out, "fp_seg_log_panels: a null operand");
  FP_REQUIRE(sm_sizes_ok(n, H, W) && n <= B, "fp_seg_log_panels: bad sizes (1 <= n <= B, H * W <= 2^27)");
  FP_REQUIRE(logit_batch_stride >= (int64_t)H * W && logit_batch_stride < ((int64_t)1 << 40),
             "fp_seg_log_panels: the sample stride of the logits is below H * W (or absurd)");
  FP_REQUIRE((((uintptr_t)image | (uintptr_t)ground_mask | (uintptr_t)logits) & 3) == 0, "fp_seg_log_panels: a pointer is not aligned to its element type");
  const int64_t need = sm_workspace(n, H, W);
  FP_REQUIRE(workspace && workspace_bytes >= need && ((uintptr_t)workspace & 3) == 0, "fp_seg_log_panels: workspace too small (%lld < %lld bytes)",
             (long long)workspace_bytes, (long long)need);
  SegLogArgs a;
  a.image = image;
  a.ground_mask = ground_mask;
  a.logits = logits;
  a.logit_stride = logit_batch_stride;
  a.lut = lut;
  a.out = out;
  a.part = (float*)workspace;
  a.HW = H * W;
  a.W = W;
  a.nblk = (int32_t)fp_ceil_div(a.HW, SM_TILE);
  // wide loads: every plane starts a multiple of HW floats (the logits: of the stride) behind its base
  const uintptr_t in_bits = (uintptr_t)image | (uintptr_t)ground_mask | (uintptr_t)logits;
  a.vec_in = (a.HW % 4 == 0 && in_bits % 16 == 0 && logit_batch_stride % 4 == 0) ? 1 : 0;
  // wide stores: with W % 4 == 0 four pixels share a row, and a picture starts 9 * HW bytes behind the last
  a.vec_out = (W % 4 == 0 && (uintptr_t)out % 4 == 0) ? 1 : 0;
  const dim3 grid((unsigned)a.nblk, (unsigned)n);
  fp_launch(seg_log_reduce_kernel, grid, dim3(SM_THREADS), 0, stream, a);
  int rc = fp_check_launch("fp_seg_log_panels(reduce)");
  if (rc != FP_OK) return rc;
  fp_launch(seg_log_map_kernel, grid, dim3(SM_THREADS), 0, stream, a);
  return fp_check_launch("fp_seg_log_panels(map)");
}

extern "C" int64_t fp_stretch_colour_workspace(int32_t B, int32_t H, int32_t W) { return sm_workspace(B, H, W); }

extern "C" int fp_stretch_colour(const void* maps, int32_t is_u8, const uint8_t* lut, uint8_t* out, int32_t B, int32_t H, int32_t W, void* workspace,
                                 int64_t workspace_bytes, fp_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  FP_REQUIRE(maps && lut && out, "fp_stretch_colour: a null operand");
  FP_REQUIRE(sm_sizes_ok(B, H, W), "fp_stretch_colour: bad sizes (1 <= B <= 65535, H * W <= 2^27)");
  FP_REQUIRE(is_u8 || ((uintptr_t)maps & 3) == 0, "fp_stretch_colour: a pointer is not aligned to its element type");
  const int64_t need = sm_workspace(B, H, W);
  FP_REQUIRE(workspace && workspace_bytes >= need && ((uintptr_t)workspace & 3) == 0, "fp_stretch_colour: workspace too small (%lld < %lld bytes)",
             (long long)workspace_bytes, (long long)need);
  StretchArgs a;
  a.maps = maps;
  a.lut = lut;
  a.out = out;
  a.part = (float*)workspace;
  a.HW = H * W;
  a.nblk = (int32_t)fp_ceil_div(a.HW, SM_TILE);
  a.u8 = is_u8 ? 1 : 0;
  a.vec_in = (a.HW % 4 == 0 && (uintptr_t)maps % (is_u8 ? 4 : 16) == 0) ? 1 : 0;
  a.vec_out = (a.HW % 4 == 0 && (uintptr_t)out % 4 == 0) ? 1 : 0;
  const dim3 grid((unsigned)a.nblk, (unsigned)B);
  fp_launch(stretch_reduce_kernel, grid, dim3(SM_THREADS), 0, stream, a);
  int rc = fp_check_launch("fp_stretch_colour(reduce)");
  if (rc != FP_OK) return rc;
  fp_launch(stretch_map_kernel, grid, dim3(SM_THREADS), 0, stream, a);
  return fp_check_launch("fp_stretch_colour(map)");
}
