// Device-side visualisations: what the reference's predict_simple.py and evaluation/inference.py do to a
// prediction on one host core before a picture is encoded.
//   reference: footprints/predict_simple.py:75-92 (resize of the hidden-ground logit and the hidden depth to the photo's size, mask, plasma
//              colour map over the depth normalised inside the mask, blend); footprints/evaluation/inference.py:114-118 (input image beside
//              the two-colour mask).
// (1) fp_vis_overlay restates footprints_amd.predict_simple.InferenceManager.visualise byte for byte.  That host path resizes with Pillow's
//     mode-"F" BILINEAR (libImaging/Resample.c: ImagingResampleHorizontal_32bpc / Vertical_32bpc) where the reference calls cv2.resize, so
//     the kernels restate Pillow: taps normalised in double on the host (fp_resize_coeffs_f64), `ss += double(pixel) * k` in tap order
//     from 0.0, one rounding to float at the store, horizontal pass into a float intermediate first, a pass whose sizes agree skipped.
//     This file is compiled with -ffp-contract=off.  The colour map is a 256 x 3 byte table the caller takes from matplotlib; the index
//     follows matplotlib's rule (x * 256, 256 -> 255, truncation) and `uint8((x / 255.0) * 255) == x` for every byte x, so the float64
//     blend of the host path is a selection between the table's bytes and the photo's.
//     Phases are separated by kernel boundaries (horizontal | vertical + mask + extrema | compose); no workgroup waits for another.  The
//     per-sample minimum and maximum of the depth inside the mask are folded with integer atomics on an order-preserving key of the float
//     bits, after a wave-level and a workgroup-level reduce: the result does not depend on scheduling.
// (2) fp_vis_side_by_side: left half uint8(image * 255.0f), right half one of two colours by `logit > 0`.  The reference thresholds
//     sigmoid(logit) > 0.5 in fp32; that is the same predicate except for the positive logits so small (below about 1.2e-7) that the fp32
//     sigmoid rounds to exactly 0.5, which the reference paints with colour 0 and this kernel with colour 1.
#include "fp_common.h"
#include "infer_out.h"

namespace {

struct VisTable {           // fp_resize_table over the 8-byte coefficient buffer
  int32_t in_size, out_size, ksize;
  int32_t bounds_off;       // in 8-byte elements: [out] pairs of int32 = first source index, tap count
  int32_t kk_off;           // in 8-byte elements: double [out][ksize]
};
struct VisSample {          // fp_resize_sample: the ORIGINAL (h, w) is the target here, the prediction (H, W) the source
  int64_t offset;           // of the original's first byte in the packed buffer, and of its overlay in the output
  int32_t h, w;
  int32_t table_h;          // index of the (W -> w) table, -1: w == W
  int32_t table_v;          // index of the (H -> h) table, -1: h == H
};

constexpr int NSUB = 16;            // sub-slots of one sample's minimum / maximum: workgroups spread over them, the compose kernel folds them
constexpr int SUB_STRIDE = 32;      // in uint32: one 128-byte line per sub-slot
constexpr int VROWS = 4;            // output rows per thread of the vertical pass

struct VisArgs {
  const float* pred;        // [B][4][H][W]
  const unsigned char* src; // packed originals
  int64_t bytes;            // of src and of out
  const VisSample* samples;
  const VisTable* tables;
  int32_t n_tables;
  const double* coeffs;
  int64_t coeffs_len;       // in 8-byte elements
  const unsigned char* lut; // [256][3]
  unsigned char* out;
  float* tmp;               // [B][2][H][max_w]: logit, depth after the horizontal pass
  float* depth;             // [B][max_h][max_w]: the resized depth
  unsigned char* mask;      // [B][max_h][max_w]
  unsigned int* kmin;       // [B][NSUB][SUB_STRIDE] keys
  unsigned int* kmax;
  int32_t* status;
  int32_t H, W, max_h, max_w;
};

// The status word is only ever set to 1, here and by the table guards in the passes, by plain stores without ordering: every lane that
// trips writes the same value, so which store lands last does not matter, and the host reads the word after the stream has drained.
__device__ __forceinline__ void reject(const VisArgs& a) {
  if (threadIdx.x == 0) *a.status = 1;
}
__device__ __forceinline__ bool table_ok(const VisArgs& a, const VisTable& t, int in_size, int out_size) {
  return t.in_size == in_size && t.out_size == out_size && t.ksize > 0 && t.bounds_off >= 0 && t.kk_off >= 0 &&
         (int64_t)t.bounds_off + (int64_t)out_size <= a.coeffs_len && (int64_t)t.kk_off + (int64_t)out_size * t.ksize <= a.coeffs_len;
}
// every kernel asks the same question, so a sample is drawn whole or left alone
__device__ __forceinline__ bool record_ok(const VisArgs& a, const VisSample& s) {
  if (s.h <= 0 || s.w <= 0 || s.h > a.max_h || s.w > a.max_w || s.offset < 0) return false;
  if (s.offset + (int64_t)s.h * s.w * 3 > a.bytes) return false;
  if (s.table_h < 0 ? s.w != a.W : s.table_h >= a.n_tables) return false;
  if (s.table_v < 0 ? s.h != a.H : s.table_v >= a.n_tables) return false;
  if (s.table_h >= 0 && !table_ok(a, a.tables[s.table_h], a.W, s.w)) return false;
  if (s.table_v >= 0 && !table_ok(a, a.tables[s.table_v], a.H, s.h)) return false;
  return true;
}

// sigmoid_to_depth as NumPy evaluates it on a float32 array: every operation rounded to float, the division correctly rounded
__device__ __forceinline__ float sigmoid_to_depth(float d) {
  const float scaled = 9.99f * d;
  const float den = 0.01f + scaled;
  return 1.0f / den;
}

// unsigned order of the keys = order of the floats
__device__ __forceinline__ unsigned int key_of(float v) {
  const unsigned int b = __float_as_uint(v);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float float_of(unsigned int k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// horizontal pass: one workgroup = one source row of one sample, both maps staged once through LDS (dynamic: 2 * W floats).
// grid = (H, B)
__global__ void __launch_bounds__(256) vis_horizontal_kernel(const VisArgs a) {
  extern __shared__ float rows[];
  const VisSample s = a.samples[blockIdx.y];
  const int y = blockIdx.x;
  if (!record_ok(a, s)) return reject(a);
  const float* p = a.pred + (size_t)blockIdx.y * 4 * a.H * a.W + (size_t)y * a.W;
  float* logit = rows;
  float* depth = rows + a.W;
  for (int x = threadIdx.x; x < a.W; x += 256) {
    logit[x] = p[(size_t)1 * a.H * a.W + x];
    depth[x] = sigmoid_to_depth(p[(size_t)3 * a.H * a.W + x]);
  }
  __syncthreads();
  float* o_logit = a.tmp + (((size_t)blockIdx.y * 2 + 0) * a.H + y) * a.max_w;
  float* o_depth = a.tmp + (((size_t)blockIdx.y * 2 + 1) * a.H + y) * a.max_w;
  if (s.table_h < 0) {
    for (int xx = threadIdx.x; xx < s.w; xx += 256) {
      o_logit[xx] = logit[xx];
      o_depth[xx] = depth[xx];
    }
    return;
  }
  const VisTable t = a.tables[s.table_h];
  const int2* bounds = reinterpret_cast<const int2*>(a.coeffs + t.bounds_off);
  const double* kk = a.coeffs + t.kk_off;
  for (int xx = threadIdx.x; xx < s.w; xx += 256) {
    const int2 bd = bounds[xx];
    const double* k = kk + (size_t)xx * t.ksize;
    double sl = 0.0, sd = 0.0;
    if (bd.x < 0 || bd.y < 0 || bd.y > t.ksize || bd.x > a.W - bd.y) *a.status = 1;       // never outside the row
    else
      for (int x = 0; x < bd.y; ++x) {
        const double w = k[x];
        sl += (double)logit[bd.x + x] * w;
        sd += (double)depth[bd.x + x] * w;
      }
    o_logit[xx] = (float)sl;
    o_depth[xx] = (float)sd;
  }
}

// vertical pass, mask and extrema: a thread owns one column of VROWS output rows.  grid = (ceil(max_w / 256), ceil(max_h / VROWS), B)
__global__ void __launch_bounds__(256) vis_vertical_kernel(const VisArgs a) {
  __shared__ unsigned int wave_min[4], wave_max[4];
  const VisSample s = a.samples[blockIdx.z];
  if (!record_ok(a, s)) return reject(a);
  const int x = blockIdx.x * 256 + threadIdx.x;
  const int y0 = blockIdx.y * VROWS;
  if (y0 >= s.h || blockIdx.x * 256 >= s.w) return;             // the whole workgroup is outside this sample
  const float* t_logit = a.tmp + ((size_t)blockIdx.z * 2 + 0) * a.H * a.max_w;
  const float* t_depth = a.tmp + ((size_t)blockIdx.z * 2 + 1) * a.H * a.max_w;
  VisTable t = {};
  const int2* bounds = nullptr;
  const double* kk = nullptr;
  if (s.table_v >= 0) {
    t = a.tables[s.table_v];
    bounds = reinterpret_cast<const int2*>(a.coeffs + t.bounds_off);
    kk = a.coeffs + t.kk_off;
  }
  unsigned int kmin = 0xffffffffu, kmax = 0u;
  if (x < s.w) {
    for (int i = 0; i < VROWS; ++i) {
      const int yy = y0 + i;
      if (yy >= s.h) break;
      float lr, dr;
      if (s.table_v < 0) {
        lr = t_logit[(size_t)yy * a.max_w + x];
        dr = t_depth[(size_t)yy * a.max_w + x];
      } else {
        const int2 bd = bounds[yy];
        const double* k = kk + (size_t)yy * t.ksize;
        double sl = 0.0, sd = 0.0;
        if (bd.x < 0 || bd.y < 0 || bd.y > t.ksize || bd.x > a.H - bd.y) *a.status = 1;       // never outside the intermediate
        else
          for (int r = 0; r < bd.y; ++r) {
            const double w = k[r];
            sl += (double)t_logit[(size_t)(bd.x + r) * a.max_w + x] * w;
            sd += (double)t_depth[(size_t)(bd.x + r) * a.max_w + x] * w;
          }
        lr = (float)sl;
        dr = (float)sd;
      }
      const bool m = lr > 0.5f;
      const size_t o = ((size_t)blockIdx.z * a.max_h + yy) * a.max_w + x;
      a.depth[o] = dr;
      a.mask[o] = m ? 1 : 0;
      if (m) {
        const unsigned int key = key_of(dr);
        kmin = min(kmin, key);
        kmax = max(kmax, key);
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    kmin = min(kmin, (unsigned int)__shfl_xor((int)kmin, o, 64));
    kmax = max(kmax, (unsigned int)__shfl_xor((int)kmax, o, 64));
  }
  if ((threadIdx.x & 63) == 0) {
    wave_min[threadIdx.x >> 6] = kmin;
    wave_max[threadIdx.x >> 6] = kmax;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < 4; ++i) {
      kmin = min(kmin, wave_min[i]);
      kmax = max(kmax, wave_max[i]);
    }
    if (kmin <= kmax) {          // some pixel of this workgroup is inside the mask
      const size_t slot = ((size_t)blockIdx.z * NSUB + (blockIdx.x + blockIdx.y) % NSUB) * SUB_STRIDE;
      atomicMin(a.kmin + slot, kmin);
      atomicMax(a.kmax + slot, kmax);
    }
  }
}

// compose: a thread owns one aligned dword of the output (a sample's first byte may sit at any address): the photo's bytes outside the mask,
// the table's inside.  grid = (ceil(ceil((max_h * max_w * 3 + 3) / 4) / 256), B): the dwords a sample of the largest size spans at the worst alignment
__global__ void __launch_bounds__(256) vis_compose_kernel(const VisArgs a) {
  __shared__ unsigned char lut[768];
  __shared__ unsigned int ext[2];
  const VisSample s = a.samples[blockIdx.y];
  if (!record_ok(a, s)) return reject(a);
  const int64_t n = (int64_t)s.h * s.w * 3;
  const int64_t first = s.offset & ~(int64_t)3;
  const int64_t p0 = first + 4 * ((int64_t)blockIdx.x * 256 + threadIdx.x);       // this thread's dword, as a byte position in the buffer
  if (first + 4 * (int64_t)blockIdx.x * 256 >= s.offset + n) return;              // the whole workgroup is behind this sample
  for (int i = threadIdx.x; i < 768; i += 256) lut[i] = a.lut[i];
  if (threadIdx.x < 64) {
    const int ln = threadIdx.x;
    unsigned int kmin = ln < NSUB ? a.kmin[((size_t)blockIdx.y * NSUB + ln) * SUB_STRIDE] : 0xffffffffu;
    unsigned int kmax = ln < NSUB ? a.kmax[((size_t)blockIdx.y * NSUB + ln) * SUB_STRIDE] : 0u;
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) {
      kmin = min(kmin, (unsigned int)__shfl_xor((int)kmin, o, 64));
      kmax = max(kmax, (unsigned int)__shfl_xor((int)kmax, o, 64));
    }
    if (ln == 0) {
      ext[0] = kmin;
      ext[1] = kmax;
    }
  }
  __syncthreads();
  const bool any = ext[0] <= ext[1];
  const float mn = float_of(ext[0]), mx = float_of(ext[1]);
  float den = mx - mn;
  if ((double)den < 1e-12) den = (float)1e-12;
  if (p0 >= s.offset + n) return;
  const bool whole = p0 >= s.offset && p0 + 4 <= s.offset + n;
  unsigned int v = 0;
  if (whole) v = *reinterpret_cast<const unsigned int*>(a.src + p0);
  else
    for (int j = 0; j < 4; ++j)
      if (p0 + j >= s.offset && p0 + j < s.offset + n) v |= (unsigned int)a.src[p0 + j] << (8 * j);
  // the 4 bytes touch at most 2 pixels
  const int64_t ifirst = max(p0, s.offset) - s.offset, ilast = min(p0 + 3, s.offset + n - 1) - s.offset;
  const int pix0 = (int)(ifirst / 3), pix1 = (int)(ilast / 3);
  int idx[2];
  bool in_mask[2];
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int pix = q == 0 ? pix0 : pix1;
    const size_t o = (size_t)blockIdx.y * a.max_h * a.max_w + (size_t)(pix / s.w) * a.max_w + (size_t)(pix % s.w);
    in_mask[q] = a.mask[o] != 0;
    float d = a.depth[o];
    if (any) {
      const float shifted = d - mn;
      d = shifted / den;
    }
    const float t = fminf(fmaxf(d, 0.0f), 1.0f) * 256.0f;
    const int i = t == 256.0f ? 255 : (int)t;
    idx[q] = min(max(i, 0), 255);        // a non-finite prediction gives some colour of the table, never a read outside it
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int64_t i = p0 + j - s.offset;
    if (i < 0 || i >= n) continue;
    const int pix = (int)(i / 3), c = (int)(i - 3 * (int64_t)pix);
    const int q = pix == pix0 ? 0 : 1;
    if (in_mask[q]) v = (v & ~(0xffu << (8 * j))) | ((unsigned int)lut[idx[q] * 3 + c] << (8 * j));
  }
  if (whole) *reinterpret_cast<unsigned int*>(a.out + p0) = v;
  else
    for (int j = 0; j < 4; ++j)
      if (p0 + j >= s.offset && p0 + j < s.offset + n) a.out[p0 + j] = (unsigned char)(v >> (8 * j));
}

// side by side: one thread per pixel of the input image writes its byte triple on the left and the mask's colour on the right.
// grid = (ceil(W / 256), H, B)
__global__ void __launch_bounds__(256) vis_side_by_side_kernel(const float* __restrict__ image, const float* __restrict__ pred,
                                                               unsigned char* __restrict__ out, int H, int W, unsigned int colour0,
                                                               unsigned int colour1) {
  const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, b = blockIdx.z;
  if (x >= W) return;
  const size_t hw = (size_t)H * W, at = (size_t)y * W + x;
  unsigned char* row = out + ((size_t)b * H + y) * 2 * W * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c) row[x * 3 + c] = (unsigned char)fp_sbs_image_byte(image[((size_t)b * 3 + c) * hw + at]);
  const unsigned int col = fp_sbs_colour(pred[((size_t)b * 4 + 1) * hw + at], colour0, colour1);
#pragma unroll
  for (int c = 0; c < 3; ++c) row[(W + x) * 3 + c] = (unsigned char)(col >> (8 * c));
}

// the workspace's parts, in bytes from its start; false when a part would not fit the kernels' 32-bit pixel indices
struct VisLayout {
  int64_t tmp, depth, mask, kmin, kmax, status, total;
};
bool layout_of(int32_t B, int32_t H, int32_t W, int32_t max_h, int32_t max_w, VisLayout* l) {
  if (B <= 0 || H <= 0 || W <= 0 || max_h <= 0 || max_w <= 0 || B > 65535 || H > 65535 || max_h > 65535 * VROWS) return false;
  if ((int64_t)max_h * max_w * 3 >= ((int64_t)1 << 31) || (int64_t)H * max_w >= ((int64_t)1 << 30) || (int64_t)H * W >= ((int64_t)1 << 29)) return false;
  const int64_t px = (int64_t)B * max_h * max_w;
  const int64_t slots = (int64_t)B * NSUB * SUB_STRIDE * 4;
  l->tmp = 0;
  l->depth = l->tmp + (int64_t)B * 2 * H * max_w * 4;
  l->mask = l->depth + px * 4;
  l->kmin = (l->mask + px + 127) & ~(int64_t)127;
  l->kmax = l->kmin + slots;
  l->status = l->kmax + slots;
  l->total = l->status + 16;
  return l->total < ((int64_t)1 << 40);
}

}  // namespace

extern "C" int64_t fp_vis_overlay_workspace(int32_t B, int32_t H, int32_t W, int32_t max_h, int32_t max_w) {
  VisLayout l;
  return layout_of(B, H, W, max_h, max_w, &l) ? l.total : -1;
}

extern "C" int64_t fp_vis_overlay_status_offset(int32_t B, int32_t H, int32_t W, int32_t max_h, int32_t max_w) {
  VisLayout l;
  return layout_of(B, H, W, max_h, max_w, &l) ? l.status : -1;
}

extern "C" int fp_vis_overlay(const float* pred, const uint8_t* src, int64_t bytes, const void* samples, const void* tables, int32_t n_tables,
                              const double* coeffs, int64_t coeffs_len, const uint8_t* lut, uint8_t* out, int32_t B, int32_t H, int32_t W,
                              int32_t max_h, int32_t max_w, void* workspace, int64_t workspace_bytes, fp_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  FP_REQUIRE(pred && src && samples && lut && out && bytes > 0, "fp_vis_overlay: bad arguments");
  FP_REQUIRE(n_tables == 0 || (tables && coeffs && coeffs_len > 0), "fp_vis_overlay: tables are missing");
  VisLayout l;
  FP_REQUIRE(layout_of(B, H, W, max_h, max_w, &l), "fp_vis_overlay: bad sizes or too large (fp_vis_overlay_workspace)");
  FP_REQUIRE(workspace && workspace_bytes >= l.total, "fp_vis_overlay: workspace too small (fp_vis_overlay_workspace)");
  FP_REQUIRE(((uintptr_t)workspace & 15) == 0, "fp_vis_overlay: the workspace must be 16-byte aligned");
  FP_REQUIRE(((uintptr_t)src & 3) == 0 && ((uintptr_t)out & 3) == 0, "fp_vis_overlay: the packed buffers must be 4-byte aligned");
  FP_REQUIRE((size_t)W * 2 * sizeof(float) <= 64 * 1024, "fp_vis_overlay: two prediction rows must fit 64 KiB of LDS (W <= 8192)");
  unsigned char* ws = (unsigned char*)workspace;
  VisArgs a;
  a.pred = pred; a.src = src; a.bytes = bytes; a.samples = (const VisSample*)samples; a.tables = (const VisTable*)tables; a.n_tables = n_tables;
  a.coeffs = coeffs; a.coeffs_len = coeffs_len; a.lut = lut; a.out = out; a.tmp = (float*)(ws + l.tmp); a.depth = (float*)(ws + l.depth);
  a.mask = ws + l.mask; a.kmin = (unsigned int*)(ws + l.kmin); a.kmax = (unsigned int*)(ws + l.kmax); a.status = (int32_t*)(ws + l.status);
  a.H = H; a.W = W; a.max_h = max_h; a.max_w = max_w;
  // the slots of this call: all ones under the minima, zeros under the maxima and the status word
  // (two fills, not launches through fp_launch: like the reader's, this call cannot be recorded into a launch plan -- a replay of the three
  // kernels alone would fold new extrema into the previous call's)
  hipError_t e = hipMemsetAsync(a.kmin, 0xff, (size_t)(l.kmax - l.kmin), stream);
  if (e == hipSuccess) e = hipMemsetAsync(a.kmax, 0, (size_t)(l.total - l.kmax), stream);
  if (e != hipSuccess) return fp_set_error((int)e, "fp_vis_overlay: %s", hipGetErrorString(e));
  // the sample records live on the device: every kernel is launched for the largest sample and leaves early where it has nothing to do
  fp_launch(vis_horizontal_kernel, dim3(H, B), dim3(256), (unsigned)((size_t)W * 2 * sizeof(float)), stream, a);
  int rc = fp_check_launch("fp_vis_overlay(horizontal)");
  if (rc) return rc;
  fp_launch(vis_vertical_kernel, dim3((unsigned)fp_ceil_div(max_w, 256), (unsigned)fp_ceil_div(max_h, VROWS), B), dim3(256), 0, stream, a);
  rc = fp_check_launch("fp_vis_overlay(vertical)");
  if (rc) return rc;
  const unsigned dwords = (unsigned)fp_ceil_div((int64_t)max_h * max_w * 3 + 3, 4);
  fp_launch(vis_compose_kernel, dim3((unsigned)fp_ceil_div(dwords, 256), B), dim3(256), 0, stream, a);
  return fp_check_launch("fp_vis_overlay(compose)");
}

extern "C" int fp_vis_side_by_side(const float* image, const float* pred, uint8_t* out, int32_t B, int32_t H, int32_t W, uint32_t colour0,
                                   uint32_t colour1, fp_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  FP_REQUIRE(image && pred && out && B > 0 && H > 0 && W > 0, "fp_vis_side_by_side: bad arguments");
  FP_REQUIRE(B <= 65535 && H <= 65535 && (int64_t)H * W * 6 < ((int64_t)1 << 31), "fp_vis_side_by_side: too large");
  fp_launch(vis_side_by_side_kernel, dim3((unsigned)fp_ceil_div(W, 256), H, B), dim3(256), 0, stream, image, pred, out, H, W, colour0, colour1);
  return fp_check_launch("fp_vis_side_by_side");
}
