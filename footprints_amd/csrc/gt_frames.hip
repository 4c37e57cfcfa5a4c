// Device-side loader work of the training-label generators: the cv2 resizes of the source frames and the
// per-target batch of a device-resident frame cache.
//   reference: footprints/preprocessing/ground_truth_generation/data_loader.py:109-174 (KITTILoader.load_frame_data: `disp *= width / w` in the
//              stored dtype, cv2.resize(x.astype(float), (width, height)) -- INTER_LINEAR -- of disparity, ground segmentation and flow, the
//              threshold, the flow's `* width / w`), :212-228 (MatterportLoader.load_frame_data: threshold + INTER_NEAREST, depth * 0.00025),
//              :91-98 (np.stack, .float(), depths = fx * baseline / disparities).
// fp_gt_frame_resize: one launch resizes every map of a list -- mixed native sizes, mixed stored dtypes -- each into its float32 [H][W] slot
// of a cache the caller owns.  OpenCV's arithmetic is restated operation by operation (imgproc/src/resize.cpp for double data, no SIMD:
// resizeNN, resizeAreaFast_ for the 2 x 2 case, HResizeLinear + VResizeLinear with float coefficients widened to double).  This file is
// compiled with -ffp-contract=off and spells every double product and sum as __dmul_rn / __dadd_rn: a fused multiply-add anywhere would
// change bits.  No atomics, no reductions: every output element is written once, by one thread.
// fp_gt_gather_frames: B cache slots -> depths [B][H][W] (fb / disparity, or the slot as it is) and ground_segs [B][H][W].
#include <math.h>

#include "fp_common.h"

namespace {

typedef fp_gt_frame Frame;
typedef fp_gt_table Table;

struct Bounds {
  int64_t src_bytes, cache_elems, words_len;
  int32_t n_tables, H, W;
};

struct ResizeArgs {
  const unsigned char* src;
  const Frame* records;       // device copy of the records the host half validated
  const Table* tables;
  const int32_t* words;       // the tables' offsets and coefficient bits
  float* cache;
  Bounds bounds;
};

__host__ __device__ __forceinline__ int elem_bytes(int dtype) { return dtype == FP_GT_F64 ? 8 : dtype == FP_GT_F32 ? 4 : 2; }

// The one rule of what a record may address, for the host half (which reports) and the kernel (which leaves a record it turns down
// unwritten: its device copy of records and tables need not be the copy the host validated)
enum { kOk = 0, kBadKind, kBadSource, kBadSlot, kBadArea2, kBadTable };

__host__ __device__ __forceinline__ int frame_fault(const Frame& r, const Table* tables, const Bounds& b) {
  if (r.dtype < FP_GT_F16 || r.dtype > FP_GT_U16 || r.method < FP_GT_LINEAR || r.method > FP_GT_AREA2) return kBadKind;
  if (r.h <= 0 || r.w <= 0 || r.offset < 0 || (r.offset & 7) != 0 || (int64_t)r.h * r.w > (b.src_bytes - r.offset) / elem_bytes(r.dtype)) return kBadSource;
  if (r.dst < 0 || r.dst > b.cache_elems - (int64_t)b.H * b.W) return kBadSlot;
  if (r.method == FP_GT_AREA2) return r.h == 2 * (int64_t)b.H && r.w == 2 * (int64_t)b.W ? kOk : kBadArea2;
  if (r.method == FP_GT_LINEAR) {
    if (r.table_x < 0 || r.table_x >= b.n_tables || r.table_y < 0 || r.table_y >= b.n_tables) return kBadTable;
    const Table tx = tables[r.table_x], ty = tables[r.table_y];
    if (tx.in_size != r.w || tx.out_size != b.W || tx.clamp != 1 || tx.offset < 0 || tx.offset > b.words_len - 3 * (int64_t)b.W) return kBadTable;
    if (ty.in_size != r.h || ty.out_size != b.H || ty.clamp != 0 || ty.offset < 0 || ty.offset > b.words_len - 3 * (int64_t)b.H) return kBadTable;
  }
  return kOk;
}

// one stored element: times `pre` in the stored dtype (numpy's in-place `disp *= scalar`; the host half hands `pre` over rounded to that
// dtype, so narrowing it here is exact), then widened to double (.astype(float))
__device__ __forceinline__ double load_elem(const unsigned char* base, int dtype, size_t i, double pre) {
  switch (dtype) {                      // wave-uniform: the record is the workgroup's
    case FP_GT_F16: {
      // the product of two halves is exact in float, so float product + one rounding to half = numpy's half multiply
      const float p = __fmul_rn((float)reinterpret_cast<const _Float16*>(base)[i], (float)pre);
      return (double)(_Float16)p;
    }
    case FP_GT_F32: return (double)__fmul_rn(reinterpret_cast<const float*>(base)[i], (float)pre);
    case FP_GT_F64: return __dmul_rn(reinterpret_cast<const double*>(base)[i], pre);
    default: return (double)reinterpret_cast<const unsigned short*>(base)[i];          // uint16: the host half admits pre == 1 only
  }
}

// one axis of the linear tables: (first source index, the two float coefficients) of output index d
__device__ __forceinline__ void linear_tap(const int32_t* words, const Table& t, int d, int& s, double& c0, double& c1) {
  s = words[t.offset + d];
  c0 = (double)__int_as_float(words[t.offset + t.out_size + 2 * d]);
  c1 = (double)__int_as_float(words[t.offset + t.out_size + 2 * d + 1]);
}

__device__ __forceinline__ int clip(int x, int n) { return x < 0 ? 0 : (x < n ? x : n - 1); }

// one thread = one output pixel.  grid = (ceil(H * W / 256), records); record r writes cache[r.dst .. r.dst + H * W)
__global__ void __launch_bounds__(256) gt_frame_resize_kernel(const ResizeArgs a) {
  const Frame r = a.records[blockIdx.y];                   // uniform address: scalar loads, the record lives in SGPRs
  const int H = a.bounds.H, W = a.bounds.W;
  if (frame_fault(r, a.tables, a.bounds) != kOk) return;   // wave-uniform
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= H * W) return;
  const int dy = i / W, dx = i - dy * W;
  const unsigned char* src = a.src + r.offset;
  const int h = r.h, w = r.w, dt = r.dtype;
  double v;
  if (r.method == FP_GT_NEAREST) {
    if (h == H && w == W) {                                                 // cv2's early copyTo
      v = load_elem(src, dt, (size_t)i, r.pre);
    } else {                                                                // resizeNN
      const double scale_x = __ddiv_rn(1.0, __ddiv_rn((double)W, (double)w)), scale_y = __ddiv_rn(1.0, __ddiv_rn((double)H, (double)h));
      const int sx = min((int)floor(__dmul_rn((double)dx, scale_x)), w - 1);
      const int sy = min((int)floor(__dmul_rn((double)dy, scale_y)), h - 1);
      v = load_elem(src, dt, (size_t)sy * w + sx, r.pre);
    }
  } else if (r.method == FP_GT_AREA2) {                                     // resizeAreaFast_ at 2 x 2: row-major sum, times float 1 / 4
    const size_t row = (size_t)(2 * dy) * w + 2 * dx;
    v = __dadd_rn(load_elem(src, dt, row, r.pre), load_elem(src, dt, row + 1, r.pre));
    v = __dadd_rn(v, load_elem(src, dt, row + w, r.pre));
    v = __dadd_rn(v, load_elem(src, dt, row + w + 1, r.pre));
    v = __dmul_rn(v, (double)__fdiv_rn(1.f, 4.f));
  } else {                                                                  // HResizeLinear of the two rows, then VResizeLinear
    int sx, sy;
    double c0, c1, b0, b1;
    linear_tap(a.words, a.tables[r.table_x], dx, sx, c0, c1);
    linear_tap(a.words, a.tables[r.table_y], dy, sy, b0, b1);
    sx = clip(sx, w);                                                       // the table's offsets are clamped already: a guard, not arithmetic
    const size_t row0 = (size_t)clip(sy, h) * w, row1 = (size_t)clip(sy + 1, h) * w;
    double h0, h1;
    if (sx == w - 1) {                                                      // dx >= xmax: S[sx] * 1
      h0 = __dmul_rn(load_elem(src, dt, row0 + sx, r.pre), 1.0);
      h1 = __dmul_rn(load_elem(src, dt, row1 + sx, r.pre), 1.0);
    } else {
      h0 = __dadd_rn(__dmul_rn(load_elem(src, dt, row0 + sx, r.pre), c0), __dmul_rn(load_elem(src, dt, row0 + sx + 1, r.pre), c1));
      h1 = __dadd_rn(__dmul_rn(load_elem(src, dt, row1 + sx, r.pre), c0), __dmul_rn(load_elem(src, dt, row1 + sx + 1, r.pre), c1));
    }
    v = __dadd_rn(__dmul_rn(h0, b0), __dmul_rn(h1, b1));
  }
  v = __ddiv_rn(__dmul_rn(v, r.post_num), r.post_den);
  if (r.threshold) v = v > r.thr ? 1.0 : 0.0;
  a.cache[r.dst + i] = __double2float_rn(v);
}

struct GatherArgs {
  const float* cache;
  const int32_t* slots;       // [2][B]: the slot behind depths[b], then the slot behind ground_segs[b]
  float* depths;
  float* ground_segs;
  int64_t n_slots;
  int32_t B, HW;
  int32_t divide;
  float fb;
};

// grid = (ceil(HW / (256 * V)), B, 2): plane z of frame b; V floats per thread (4 when HW is a multiple of 4: every slot is 16-byte aligned)
template <int V>
__global__ void __launch_bounds__(256) gt_gather_kernel(const GatherArgs a) {
  const int b = blockIdx.y, plane = blockIdx.z;
  const int64_t slot = a.slots[plane * a.B + b];
  if (slot < 0 || slot >= a.n_slots) return;                // the host half validated the host copy: a guard against a differing device copy
  const int i = (blockIdx.x * 256 + threadIdx.x) * V;
  if (i >= a.HW) return;
  const float* s = a.cache + slot * a.HW + i;
  float* o = (plane ? a.ground_segs : a.depths) + (int64_t)b * a.HW + i;
  const bool div = plane == 0 && a.divide;
  if (V == 4) {
    float4 v = *reinterpret_cast<const float4*>(s);
    if (div) v = make_float4(__fdiv_rn(a.fb, v.x), __fdiv_rn(a.fb, v.y), __fdiv_rn(a.fb, v.z), __fdiv_rn(a.fb, v.w));
    *reinterpret_cast<float4*>(o) = v;
  } else {
    *o = div ? __fdiv_rn(a.fb, *s) : *s;
  }
}

}  // namespace

extern "C" int32_t fp_gt_frame_bytes(void) { return (int32_t)sizeof(Frame); }
extern "C" int32_t fp_gt_table_bytes(void) { return (int32_t)sizeof(Table); }

// HOST: the offsets and coefficients of cv2's INTER_LINEAR for one axis
extern "C" int fp_linear_table(int32_t in_size, int32_t out_size, int32_t clamp, int32_t* offsets, float* coeffs) {
  FP_REQUIRE(in_size > 0 && out_size > 0 && offsets && coeffs, "fp_linear_table: sizes must be positive and the outputs given");
  const double inv = (double)out_size / (double)in_size, scale = 1.0 / inv;
  for (int d = 0; d < out_size; ++d) {
    float f = (float)((d + 0.5) * scale - 0.5);
    int s = (int)floorf(f);
    f -= (float)s;
    if (clamp) {
      if (s < 0) f = 0.f, s = 0;
      if (s >= in_size - 1) f = 0.f, s = in_size - 1;
    }
    offsets[d] = s;
    coeffs[2 * d] = 1.f - f;
    coeffs[2 * d + 1] = f;
  }
  return 0;
}

// HOST: every record against the buffers it will address; -> 0, or FP_EINVAL with the first bad record named
extern "C" int fp_gt_frame_check(const fp_gt_frame* records, int32_t n_records, int64_t src_bytes, const fp_gt_table* tables, int32_t n_tables,
                                 int64_t words_len, int64_t cache_elems, int32_t H, int32_t W) {
  FP_REQUIRE(records && n_records > 0 && n_records <= 65535 && src_bytes >= 0 && n_tables >= 0 && (tables || n_tables == 0) && words_len >= 0 &&
                 cache_elems >= 0 && H > 0 && W > 0 && (int64_t)H * W < ((int64_t)1 << 31) - 256,
             "fp_gt_frame_resize: bad arguments");
  const Bounds bounds{src_bytes, cache_elems, words_len, n_tables, H, W};
  for (int32_t j = 0; j < n_records; ++j) {
    const Frame& r = records[j];
    switch (frame_fault(r, tables, bounds)) {
      case kOk: break;
      case kBadKind: return fp_set_error(FP_EINVAL, "fp_gt_frame_resize: record %d: dtype %d, method %d", j, r.dtype, r.method);
      case kBadSource:
        return fp_set_error(FP_EINVAL, "fp_gt_frame_resize: record %d: a %d x %d map at byte %lld does not lie inside the %lld packed bytes (offsets "
                            "are multiples of 8)", j, r.h, r.w, (long long)r.offset, (long long)src_bytes);
      case kBadSlot:
        return fp_set_error(FP_EINVAL, "fp_gt_frame_resize: record %d: destination %lld does not lie inside the cache of %lld elements", j,
                            (long long)r.dst, (long long)cache_elems);
      case kBadArea2:
        return fp_set_error(FP_EINVAL, "fp_gt_frame_resize: record %d: area2 needs a %d x %d map, got %d x %d", j, 2 * H, 2 * W, r.h, r.w);
      default:
        return fp_set_error(FP_EINVAL, "fp_gt_frame_resize: record %d: tables %d and %d of %d (%lld words) do not fit %d x %d -> %d x %d", j, r.table_x,
                            r.table_y, n_tables, (long long)words_len, r.h, r.w, H, W);
    }
    // what cannot make the kernel leave its buffers, but would not be the reference's arithmetic
    FP_REQUIRE(r.dtype != FP_GT_U16 || r.pre == 1.0, "fp_gt_frame_resize: record %d: an integer map takes no pre-scale", j);
    FP_REQUIRE(r.dtype == FP_GT_F64 || r.dtype == FP_GT_U16 || (double)(float)r.pre == r.pre,
               "fp_gt_frame_resize: record %d: pre must arrive rounded to the stored dtype", j);
    FP_REQUIRE(r.post_den != 0.0, "fp_gt_frame_resize: record %d: post_den is 0", j);
  }
  return 0;
}

extern "C" int fp_gt_frame_resize(const void* src, int64_t src_bytes, const fp_gt_frame* records, const void* d_records, int32_t n_records,
                                  const fp_gt_table* tables, const void* d_tables, int32_t n_tables, const int32_t* d_words, int64_t words_len,
                                  float* cache, int64_t cache_elems, int32_t H, int32_t W, fp_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  FP_REQUIRE(src && d_records && cache && (n_tables == 0 || (d_tables && d_words)), "fp_gt_frame_resize: bad arguments");
  const int rc = fp_gt_frame_check(records, n_records, src_bytes, tables, n_tables, words_len, cache_elems, H, W);
  if (rc != 0) return rc;
  ResizeArgs a;
  a.src = (const unsigned char*)src; a.records = (const Frame*)d_records; a.tables = (const Table*)d_tables; a.words = d_words; a.cache = cache;
  a.bounds = Bounds{src_bytes, cache_elems, words_len, n_tables, H, W};
  fp_launch(gt_frame_resize_kernel, dim3((unsigned)fp_ceil_div((int64_t)H * W, 256), n_records), dim3(256), 0, stream, a);
  return fp_check_launch("fp_gt_frame_resize");
}

extern "C" int fp_gt_gather_frames(const float* cache, int64_t n_slots, const int32_t* slots, const int32_t* d_slots, int32_t B, int32_t H, int32_t W,
                                   int32_t divide, float fb, float* depths, float* ground_segs, fp_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  FP_REQUIRE(cache && slots && d_slots && depths && ground_segs && n_slots > 0 && B > 0 && B <= 65535 && H > 0 && W > 0 &&
                 (int64_t)H * W < ((int64_t)1 << 31) - 1024,
             "fp_gt_gather_frames: bad arguments");
  for (int32_t j = 0; j < 2 * B; ++j)
    FP_REQUIRE(slots[j] >= 0 && slots[j] < n_slots, "fp_gt_gather_frames: slot %d (entry %d) does not lie inside the cache of %lld slots", slots[j], j,
               (long long)n_slots);
  GatherArgs a;
  a.cache = cache; a.slots = d_slots; a.depths = depths; a.ground_segs = ground_segs; a.n_slots = n_slots; a.B = B; a.HW = H * W; a.divide = divide;
  a.fb = fb;
  const bool vec = a.HW % 4 == 0 && ((uintptr_t)cache | (uintptr_t)depths | (uintptr_t)ground_segs) % 16 == 0;
  if (vec) fp_launch(gt_gather_kernel<4>, dim3((unsigned)fp_ceil_div(a.HW, 1024), B, 2), dim3(256), 0, stream, a);
  else fp_launch(gt_gather_kernel<1>, dim3((unsigned)fp_ceil_div(a.HW, 256), B, 2), dim3(256), 0, stream, a);
  return fp_check_launch("fp_gt_gather_frames");
}
