// Device-side reader work of the Footprints trainer: the cv2 resizes of the label maps.
//   reference: footprints/datasets/footprint_dataset.py:82-94 (load_and_resize_npy: .astype(float), np.fliplr, cv2.resize with INTER_AREA or
//              INTER_NEAREST on float64, times the disparity multiplier), kitti_dataset.py:65-105, matterport_dataset.py:55-89;
//              footprint_dataset.py:73-80 (load_and_resize_image: Pillow's resize(NEAREST) of Matterport's 16-bit depth PNG, then the transpose).
// fp_label_resize: one launch resizes every map of a batch -- mixed native sizes, mixed stored dtypes -- into the float64 [K][B][H][W] buffer
// that fp_filter_depth_mask and fp_assemble_labels read.  OpenCV's arithmetic is restated operation by operation (imgproc/src/resize.cpp:
// resizeNN, resizeAreaFast_, computeResizeAreaTab + resizeArea_ for double data): float weights widened to double, products and sums in
// double in OpenCV's order.  This file is compiled with -ffp-contract=off and spells every product and sum as __dmul_rn / __dadd_rn: a fused
// multiply-add anywhere would change bits.  No atomics, no reductions: every output element is written once, by one thread.
// FP_LABEL_PIL_NEAREST is Pillow's NEAREST instead of cv2's: a plain gather of src = min(floor((dst + 0.5) * in / out), in - 1) per axis, in
// integers ((2 * dst + 1) * in / (2 * out)); it enlarges as well as shrinks.  Its flip differs from the cv2 methods': the reference flips
// the .npy maps FIRST and resizes them then (source column w - 1 - index[x] lands at final column x), but resizes the depth PNG first and
// transposes it THEN (final column x holds source column index[W - 1 - x]).  The two orders differ wherever (x + 0.5) * w / W is a whole
// number -- floor(w - t) is w - 1 - floor(t) for every other t -- which is every column at an even ratio such as Matterport's 1280 -> 640,
// and no column at 53 -> 32.  So a flipped PIL_NEAREST record reads the source unmirrored: stored column c -- which fp_assemble_labels
// moves to W - 1 - c -- holds source column index[c].
#include <float.h>
#include <math.h>

#include "fp_common.h"

namespace {

constexpr int kMaxEntries = FP_LABEL_MAX_ENTRIES;      // most table entries per output index that a launch can be asked to stage

struct LabelSample {        // fp_label_sample
  int64_t offset;           // of the map's first byte in the packed source buffer, a multiple of 8; dense [h][w] of `dtype`
  int32_t h, w;
  int32_t dtype;            // FP_LABEL_U8 / F16 / F32 / F64 / U16
  int32_t method;           // FP_LABEL_ZERO / NEAREST / AREA / PIL_NEAREST
  int32_t flip;             // read the source mirrored and store mirrored: cv2.resize(np.fliplr(m)) once fp_assemble_labels has flipped
  int32_t table_x, table_y; // (w -> W) and (h -> H) area tables; read only on INTER_AREA's general path
  int32_t pad;
  double multiplier;        // applied to the resized value (the KITTI disparity: W / w)
};

struct LabelTable {         // fp_label_table
  int32_t in_size, out_size;
  int32_t max_count;        // most entries of one output index
  int32_t n_entries;
  int32_t bounds_off;       // 8-byte element offsets into the entry buffer: [out_size] x (first entry, count) ...
  int32_t entries_off;      // ... and [n_entries] x (source index, float weight)
};

struct Entry {
  int32_t s;
  float w;
};

struct Args {
  const unsigned char* src;
  int64_t src_bytes;
  const LabelSample* samples;
  const LabelTable* tables;
  int32_t n_tables;
  const int2* entries;
  int64_t entries_len;
  double* out;
  int32_t* status;
  int32_t H, W;
  int32_t max_entries;      // entries per output index the launch's LDS holds, per axis and thread
};

template <typename T>
__device__ __forceinline__ double load_as_double(const unsigned char* base, size_t i) {       // .astype(float): exact for every stored type
  return (double)reinterpret_cast<const T*>(base)[i];
}

__device__ __forceinline__ double load_elem(const unsigned char* base, int dtype, size_t i) {
  switch (dtype) {                    // wave-uniform: the record is the workgroup's
    case FP_LABEL_U8: return load_as_double<unsigned char>(base, i);
    case FP_LABEL_F16: return load_as_double<_Float16>(base, i);
    case FP_LABEL_F32: return load_as_double<float>(base, i);
    case FP_LABEL_U16: return load_as_double<unsigned short>(base, i);
    default: return load_as_double<double>(base, i);
  }
}

__device__ __forceinline__ int elem_bytes(int dtype) {
  return dtype == FP_LABEL_U8 ? 1 : dtype == FP_LABEL_F16 || dtype == FP_LABEL_U16 ? 2 : dtype == FP_LABEL_F32 ? 4 : 8;
}

// Pillow's NEAREST source index of output index d: floor((d + 0.5) * in / out), clamped
__device__ __forceinline__ int pil_nearest(int d, int in_size, int out_size) {
  const int64_t s = ((int64_t)(2 * d + 1) * in_size) / ((int64_t)2 * out_size);
  return (int)(s < in_size - 1 ? s : in_size - 1);
}

__device__ __forceinline__ bool table_ok(const Args& a, int t, int in_size, int out_size) {
  if (t < 0 || t >= a.n_tables) return false;
  const LabelTable tb = a.tables[t];
  if (tb.in_size != in_size || tb.out_size != out_size || tb.max_count < 1 || tb.max_count > a.max_entries || tb.n_entries < out_size) return false;
  if (tb.bounds_off < 0 || tb.entries_off < 0) return false;
  return (int64_t)tb.bounds_off + out_size <= a.entries_len && (int64_t)tb.entries_off + tb.n_entries <= a.entries_len;
}

// the entries of output index d into the thread's column of `lds` ([k][thread]: a wave reads and writes consecutive 8-byte words);
// -> their count, 0 when the table points outside itself or outside the source
__device__ __forceinline__ int stage_entries(const Args& a, const LabelTable& tb, int d, int in_size, Entry* lds) {
  const int2 b = a.entries[tb.bounds_off + d];
  if (b.x < 0 || b.y < 1 || b.y > a.max_entries || (int64_t)b.x + b.y > tb.n_entries) return 0;
  for (int k = 0; k < b.y; ++k) {
    const int2 e = a.entries[tb.entries_off + b.x + k];
    if (e.x < 0 || e.x >= in_size) return 0;
    lds[k * 256 + threadIdx.x] = Entry{e.x, __int_as_float(e.y)};
  }
  return b.y;
}

// one thread = one output pixel.  grid = (ceil(H * W / 256), records); record r writes out[r][H][W].  Dynamic LDS: 2 * max_entries * 256
// entries -- sized by the longest table row of the launch (3 for a KITTI map: 12 KB), none at all when no record walks a table
__global__ void __launch_bounds__(256) label_resize_kernel(const Args a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  Entry* const lds_x = reinterpret_cast<Entry*>(lds_raw);
  Entry* const lds_y = lds_x + a.max_entries * 256;
  const LabelSample r = a.samples[blockIdx.y];             // uniform address: scalar loads, the record lives in SGPRs
  const int H = a.H, W = a.W;
  const bool zero = r.method == FP_LABEL_ZERO;
  const bool pil = r.method == FP_LABEL_PIL_NEAREST;
  bool ok = r.method == FP_LABEL_ZERO || r.method == FP_LABEL_NEAREST || r.method == FP_LABEL_AREA || pil;
  if (ok && !zero) {
    ok = r.h > 0 && r.w > 0 && r.dtype >= FP_LABEL_U8 && r.dtype <= FP_LABEL_U16 && r.offset >= 0 && (r.offset & 7) == 0 &&
         r.offset + (int64_t)r.h * r.w * elem_bytes(r.dtype) <= a.src_bytes;
  }
  // cv2::resize: inv_scale = dsize / ssize in double, scale = 1 / inv_scale
  const bool same = !zero && r.h == H && r.w == W;
  double scale_x = 1.0, scale_y = 1.0;
  int ix = 1, iy = 1;
  bool fast = false;
  if (ok && !zero && !same && !pil) {
    scale_x = __ddiv_rn(1.0, __ddiv_rn((double)W, (double)r.w));
    scale_y = __ddiv_rn(1.0, __ddiv_rn((double)H, (double)r.h));
    if (r.method == FP_LABEL_AREA) {
      ok = scale_x >= 1.0 && scale_y >= 1.0;                // below 1 cv2 switches to a linear kernel: not provided
      const double rx = rint(scale_x), ry = rint(scale_y);
      fast = ok && fabs(__dsub_rn(scale_x, rx)) < DBL_EPSILON && fabs(__dsub_rn(scale_y, ry)) < DBL_EPSILON;
      if (fast) {
        ix = (int)rx;
        iy = (int)ry;
        ok = (int64_t)ix * W <= r.w && (int64_t)iy * H <= r.h;
      } else if (ok) {
        ok = table_ok(a, r.table_x, r.w, W) && table_ok(a, r.table_y, r.h, H);
      }
    }
  }
  if (!ok) {
    if (threadIdx.x == 0) *a.status = 1;
    return;
  }
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= H * W) return;
  const int dy = i / W, dx = i - dy * W;
  double* o = a.out + (size_t)blockIdx.y * H * W + (size_t)dy * W + (r.flip && !zero ? W - 1 - dx : dx);
  if (zero) {
    *o = 0.0;
    return;
  }
  const unsigned char* src = a.src + r.offset;
  const int w = r.w, dt = r.dtype;
  const int mirror = r.flip ? w - 1 : 0, step = r.flip ? -1 : 1;       // source column of the flipped map: mirror + step * sx
  double v;
  if (pil) {                                                              // Image.resize(NEAREST); flipped AFTER the resize (see the top)
    const int c = r.flip ? W - 1 - dx : dx;                               // the column this thread stores
    v = load_elem(src, dt, (size_t)pil_nearest(dy, r.h, H) * w + pil_nearest(c, w, W));
  } else if (same) {                                                             // cv2's early copyTo
    v = load_elem(src, dt, (size_t)dy * w + mirror + step * dx);
  } else if (r.method == FP_LABEL_NEAREST) {                              // resizeNN
    const int sx = min((int)floor(__dmul_rn((double)dx, scale_x)), w - 1);
    const int sy = min((int)floor(__dmul_rn((double)dy, scale_y)), r.h - 1);
    v = load_elem(src, dt, (size_t)sy * w + mirror + step * sx);
  } else if (fast) {                                                      // resizeAreaFast_: the block in row-major order, times float 1 / area
    v = 0.0;
    for (int ky = 0; ky < iy; ++ky) {
      const size_t row = (size_t)(dy * iy + ky) * w;
      for (int kx = 0; kx < ix; ++kx) {
        const double s = load_elem(src, dt, row + mirror + step * (dx * ix + kx));
        v = (ky | kx) == 0 ? s : __dadd_rn(v, s);
      }
    }
    v = __dmul_rn(v, (double)__fdiv_rn(1.f, (float)(ix * iy)));
  } else {                                                                // resizeArea_ over computeResizeAreaTab's entries
    const LabelTable tx = a.tables[r.table_x], ty = a.tables[r.table_y];
    const int nx = stage_entries(a, tx, dx, w, lds_x), ny = stage_entries(a, ty, dy, r.h, lds_y);
    if (nx == 0 || ny == 0) {
      *a.status = 1;
      return;
    }
    v = 0.0;
    for (int ky = 0; ky < ny; ++ky) {
      const Entry ey = lds_y[ky * 256 + threadIdx.x];
      const size_t row = (size_t)ey.s * w;
      double buf = 0.0;
      for (int kx = 0; kx < nx; ++kx) {
        const Entry ex = lds_x[kx * 256 + threadIdx.x];
        buf = __dadd_rn(buf, __dmul_rn(load_elem(src, dt, row + mirror + step * ex.s), (double)ex.w));
      }
      const double t = __dmul_rn((double)ey.w, buf);
      v = ky == 0 ? t : __dadd_rn(v, t);
    }
  }
  *o = __dmul_rn(v, r.multiplier);
}

}  // namespace

extern "C" int32_t fp_label_sample_bytes(void) { return (int32_t)sizeof(LabelSample); }
extern "C" int32_t fp_label_table_bytes(void) { return (int32_t)sizeof(LabelTable); }
extern "C" int32_t fp_label_max_entries(void) { return kMaxEntries; }

// HOST: cv2's computeResizeAreaTab for one axis
extern "C" int32_t fp_area_table(int32_t in_size, int32_t out_size, int32_t* bounds, int32_t* index, float* weight, int32_t capacity) {
  if (in_size <= 0 || out_size <= 0 || out_size > in_size) {
    fp_set_error(FP_EINVAL, "fp_area_table: sizes must be positive and out_size <= in_size (INTER_AREA's upscaling branch is not provided)");
    return -1;
  }
  const bool write = bounds && index && weight;
  const double scale = 1.0 / ((double)out_size / (double)in_size);
  int64_t k = 0;
  for (int d = 0; d < out_size; ++d) {
    const double f1 = d * scale, f2 = f1 + scale, cw = fmin(scale, in_size - f1);
    int s1 = (int)ceil(f1), s2 = (int)floor(f2);
    s2 = s2 < in_size - 1 ? s2 : in_size - 1;
    s1 = s1 < s2 ? s1 : s2;
    const int64_t first = k;
    auto put = [&](int s, float wgt) {
      if (write && k < capacity) {
        index[k] = s;
        weight[k] = wgt;
      }
      ++k;
    };
    if (s1 - f1 > 1e-3) put(s1 - 1, (float)((s1 - f1) / cw));
    for (int s = s1; s < s2; ++s) put(s, (float)(1.0 / cw));
    if (f2 - s2 > 1e-3) put(s2, (float)(fmin(fmin(f2 - s2, 1.0), cw) / cw));
    if (write) {
      bounds[2 * d] = (int32_t)first;
      bounds[2 * d + 1] = (int32_t)(k - first);
    }
  }
  if (k > INT32_MAX || (write && k > capacity)) {
    fp_set_error(FP_EINVAL, "fp_area_table: %lld entries do not fit the capacity of %d", (long long)k, capacity);
    return -1;
  }
  return (int32_t)k;
}

extern "C" int fp_label_resize(const void* src, int64_t src_bytes, const void* samples, int32_t n_records, const void* tables, int32_t n_tables,
                               const void* entries, int64_t entries_len, int32_t max_entries, double* out, int32_t H, int32_t W, int32_t* status,
                               fp_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  FP_REQUIRE(samples && out && status && n_records > 0 && H > 0 && W > 0 && src_bytes >= 0 && (src || src_bytes == 0),
             "fp_label_resize: bad arguments");
  FP_REQUIRE(n_tables >= 0 && entries_len >= 0 && (n_tables == 0 || (tables && entries)), "fp_label_resize: bad tables");
  FP_REQUIRE(max_entries >= 0 && max_entries <= kMaxEntries && (n_tables == 0 || max_entries >= 1), "fp_label_resize: max_entries must be 0 .. %d", kMaxEntries);
  FP_REQUIRE(n_records <= 65535 && (int64_t)H * W < ((int64_t)1 << 31) - 256, "fp_label_resize: too large");
  Args a;
  a.src = (const unsigned char*)src; a.src_bytes = src_bytes; a.samples = (const LabelSample*)samples; a.tables = (const LabelTable*)tables;
  a.n_tables = n_tables; a.entries = (const int2*)entries; a.entries_len = entries_len; a.out = out; a.status = status; a.H = H; a.W = W;
  a.max_entries = n_tables ? max_entries : 0;
  hipError_t e = hipMemsetAsync(status, 0, sizeof(int32_t), stream);
  if (e != hipSuccess) return fp_set_error((int)e, "fp_label_resize: %s", hipGetErrorString(e));
  fp_launch(label_resize_kernel, dim3((unsigned)fp_ceil_div((int64_t)H * W, 256), n_records), dim3(256),
            (unsigned)(2 * a.max_entries * 256 * sizeof(Entry)), stream, a);
  return fp_check_launch("fp_label_resize");
}
