// Device-side file-reader work: what the reference's dataset classes do to a decoded frame and to a depth mask
// before the augmentation of data_path.hip sees them.
//   reference: footprints/datasets/footprint_dataset.py:73-80 (Image.resize(LANCZOS)), :96-105 (filter_depth_mask: skimage.measure.label
//              + a loop over the components); the same resize in datasets/inference_dataset.py:26,48 and predict_simple.py:41,55.
// (1) Pillow's 8-bit resample (libImaging/Resample.c: ImagingResampleHorizontal_8bpc / Vertical_8bpc): a separable filter whose
//     coefficients are normalised in double on the host and quantised to 22 fractional bits; the image passes are pure int32 arithmetic
//     with a uint8 intermediate between the horizontal and the vertical pass.  The tables are built here on the HOST (fp_resize_coeffs;
//     this file is compiled with -ffp-contract=off, and sin() is the C library's, as in Pillow); the kernels use no float operation.
// (2) filter_depth_mask: connected components (8-connectivity) by label equivalence -- union-find with integer atomicMin on the parent
//     array and integer atomicAdd on per-root counters, so the result does not depend on the order in which threads arrive.  Phases are
//     separated by kernel boundaries (tile-local labelling in LDS | merge across tile borders | flatten + count | threshold); no
//     workgroup ever waits for another.
#include <math.h>

#include "fp_common.h"

namespace {

constexpr int PRECISION_BITS = 32 - 8 - 2;      // Resample.c

// ---- host: coefficient tables --------------------------------------------------------------------------------------------------------
double box_filter(double x) { return (x > -0.5 && x <= 0.5) ? 1.0 : 0.0; }
double bilinear_filter(double x) {
  if (x < 0.0) x = -x;
  return x < 1.0 ? 1.0 - x : 0.0;
}
double bicubic_filter(double x) {
  const double a = -0.5;
  if (x < 0.0) x = -x;
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
  if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
  return 0.0;
}
double sinc_filter(double x) {
  if (x == 0.0) return 1.0;
  x = x * M_PI;
  return sin(x) / x;
}
double lanczos_filter(double x) { return (-3.0 <= x && x < 3.0) ? sinc_filter(x) * sinc_filter(x / 3) : 0.0; }

bool filter_of(int id, double (**fn)(double), double* support) {
  switch (id) {
    case FP_RESIZE_LANCZOS: *fn = lanczos_filter; *support = 3.0; return true;
    case FP_RESIZE_BILINEAR: *fn = bilinear_filter; *support = 1.0; return true;
    case FP_RESIZE_BICUBIC: *fn = bicubic_filter; *support = 2.0; return true;
    case FP_RESIZE_BOX: *fn = box_filter; *support = 0.5; return true;
    default: return false;
  }
}

// ---- device: resample ----------------------------------------------------------------------------------------------------------------
struct ResizeTable {        // fp_resize_table
  int32_t in_size, out_size, ksize;
  int32_t bounds_off;       // into the int32 table buffer: [out][2] = first source index, tap count
  int32_t kk_off;           // [out][ksize]
};
struct ResizeSample {       // fp_resize_sample
  int64_t offset;           // of the sample's first byte in the packed source buffer
  int32_t h, w;
  int32_t table_h;          // index of the (w -> W) table, -1: w == W, the horizontal pass is skipped
  int32_t table_v;          // index of the (h -> H) table, -1: h == H
};

struct ResizeArgs {
  const unsigned char* src;
  int64_t src_bytes;
  const ResizeSample* samples;
  const ResizeTable* tables;
  int32_t n_tables;
  const int32_t* coeffs;
  int64_t coeffs_len;
  unsigned char* tmp;       // [B][max_h][W][C]
  unsigned char* out;       // [B][H][W][C]
  int32_t* status;          // the workspace's last word: cleared by every call, 1 once a kernel turned a record down
  int32_t H, W, max_h, max_w;
};

// a sample record the kernels may follow without leaving any buffer; everything else leaves the sample's output untouched and is
// reported in the status word (every rejecting workgroup stores the same 1)
__device__ __forceinline__ void reject(const ResizeArgs& a) {
  if (threadIdx.x == 0) *a.status = 1;
}
__device__ __forceinline__ bool sample_ok(const ResizeArgs& a, const ResizeSample& s, int C) {
  if (s.h <= 0 || s.w <= 0 || s.h > a.max_h || s.w > a.max_w || s.offset < 0) return false;
  if (s.offset + (int64_t)s.h * s.w * C > a.src_bytes) return false;
  if (s.table_h < 0 ? s.w != a.W : s.table_h >= a.n_tables) return false;
  if (s.table_v < 0 ? s.h != a.H : s.table_v >= a.n_tables) return false;
  return true;
}
__device__ __forceinline__ bool table_ok(const ResizeArgs& a, const ResizeTable& t, int in_size, int out_size) {
  return t.in_size == in_size && t.out_size == out_size && t.ksize > 0 && t.bounds_off >= 0 && t.kk_off >= 0 &&
         (int64_t)t.bounds_off + 2 * (int64_t)out_size <= a.coeffs_len && (int64_t)t.kk_off + (int64_t)out_size * t.ksize <= a.coeffs_len;
}

// both passes ask the same question, so a sample is resized whole or left alone
__device__ __forceinline__ bool record_ok(const ResizeArgs& a, const ResizeSample& s, int C) {
  if (!sample_ok(a, s, C)) return false;
  if (s.table_h >= 0 && !table_ok(a, a.tables[s.table_h], s.w, a.W)) return false;
  if (s.table_v >= 0 && !table_ok(a, a.tables[s.table_v], s.h, a.H)) return false;
  return true;
}

__device__ __forceinline__ unsigned char clip8(int v) { return (unsigned char)min(max(v >> PRECISION_BITS, 0), 255); }

// horizontal pass: one workgroup = one source row of one sample, staged once through LDS (dynamic: max_w * C bytes rounded up to 4 + 4);
// a thread owns whole output pixels, so a coefficient is loaded once for the C channels.  grid = (max_h, B)
template <int C>
__global__ void __launch_bounds__(256) resize_horizontal_kernel(const ResizeArgs a) {
  extern __shared__ unsigned int row_words[];
  const ResizeSample s = a.samples[blockIdx.y];
  const int y = blockIdx.x;
  if (!record_ok(a, s, C)) return reject(a);
  if (s.table_h < 0 || y >= s.h) return;
  const ResizeTable t = a.tables[s.table_h];
  // the row starts at any byte address: whole aligned words where the buffer holds them, bytes at its very end
  const int64_t first = s.offset + (int64_t)y * s.w * C;
  const int shift = (int)(first & 3);
  const int64_t word0 = first - shift;
  const int n_words = (shift + s.w * C + 3) >> 2;
  for (int i = threadIdx.x; i < n_words; i += 256) {
    const int64_t p = word0 + 4 * (int64_t)i;
    unsigned int v = 0;
    if (p + 4 <= a.src_bytes) v = *reinterpret_cast<const unsigned int*>(a.src + p);
    else
      for (int j = 0; j < 4; ++j)
        if (p + j < a.src_bytes) v |= (unsigned int)a.src[p + j] << (8 * j);
    row_words[i] = v;
  }
  __syncthreads();
  const unsigned char* row = reinterpret_cast<const unsigned char*>(row_words) + shift;
  const int32_t* bounds = a.coeffs + t.bounds_off;
  const int32_t* kk = a.coeffs + t.kk_off;
  // without a vertical pass this IS the output row
  unsigned char* dst = s.table_v < 0 ? a.out + ((size_t)blockIdx.y * a.H + y) * a.W * C : a.tmp + ((size_t)blockIdx.y * a.max_h + y) * a.W * C;
  for (int xx = threadIdx.x; xx < a.W; xx += 256) {
    const int xmin = bounds[2 * xx], n = bounds[2 * xx + 1];
    const int32_t* k = kk + (size_t)xx * t.ksize;
    int acc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = 1 << (PRECISION_BITS - 1);
    if (xmin < 0 || n > t.ksize || xmin + n > s.w) *a.status = 1;       // never outside the row
    else
      for (int x = 0; x < n; ++x) {
        const int w = k[x];
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] += w * (int)row[(xmin + x) * C + c];
      }
#pragma unroll
    for (int c = 0; c < C; ++c) dst[xx * C + c] = clip8(acc[c]);
  }
}

// vertical pass over rows of W * C bytes (the channel layout does not matter to it): a thread owns 4 consecutive bytes of VT output rows and
// walks the source rows those outputs need once, so a source byte is loaded once per tile of VT output rows; the coefficients and bounds
// are uniform over the workgroup.  grid = (strips of 1024 bytes, ceil(H / VT), B)
constexpr int VT = 8;
__global__ void __launch_bounds__(256) resize_vertical_kernel(const ResizeArgs a, int C) {
  const ResizeSample s = a.samples[blockIdx.z];
  if (!record_ok(a, s, C)) return reject(a);
  if (s.table_v < 0) return;
  const ResizeTable t = a.tables[s.table_v];
  const int row_bytes = a.W * C;
  const unsigned char* in = s.table_h < 0 ? a.src + s.offset : a.tmp + (size_t)blockIdx.z * a.max_h * row_bytes;
  const int32_t* bounds = a.coeffs + t.bounds_off;
  const int32_t* kk = a.coeffs + t.kk_off;
  const int y0 = blockIdx.y * VT;
  const int j = (blockIdx.x * 256 + threadIdx.x) * 4;
  if (j >= row_bytes) return;
  const int nb = min(4, row_bytes - j);
  int ymin[VT], cnt[VT], acc[VT][4];
  int lo = s.h, hi = 0;
#pragma unroll
  for (int i = 0; i < VT; ++i) {
    const bool live = y0 + i < a.H;
    ymin[i] = live ? bounds[2 * (y0 + i)] : 0;
    cnt[i] = live ? bounds[2 * (y0 + i) + 1] : 0;
    if (ymin[i] < 0 || cnt[i] > t.ksize || ymin[i] + cnt[i] > s.h) { cnt[i] = 0; reject(a); }       // never outside the source
    if (cnt[i] > 0) { lo = min(lo, ymin[i]); hi = max(hi, ymin[i] + cnt[i]); }
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[i][b] = 1 << (PRECISION_BITS - 1);
  }
  for (int r = lo; r < hi; ++r) {
    const unsigned char* p = in + (size_t)r * row_bytes + j;
    unsigned int v = 0;
    if (nb == 4) __builtin_memcpy(&v, p, 4);
    else
      for (int b = 0; b < nb; ++b) v |= (unsigned int)p[b] << (8 * b);
#pragma unroll
    for (int i = 0; i < VT; ++i) {
      const int x = r - ymin[i];
      if (x >= 0 && x < cnt[i]) {
        const int w = kk[(size_t)(y0 + i) * t.ksize + x];
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[i][b] += w * (int)((v >> (8 * b)) & 0xffu);
      }
    }
  }
#pragma unroll
  for (int i = 0; i < VT; ++i) {
    if (y0 + i >= a.H) break;
    unsigned char* o = a.out + ((size_t)blockIdx.z * a.H + y0 + i) * row_bytes + j;
    for (int b = 0; b < nb; ++b) o[b] = clip8(acc[i][b]);
  }
}

// a sample that already has the target size is copied.  grid = (blocks, B)
__global__ void __launch_bounds__(256) resize_copy_kernel(const ResizeArgs a, int C) {
  const ResizeSample s = a.samples[blockIdx.y];
  if (!sample_ok(a, s, C) || s.table_h >= 0 || s.table_v >= 0) return;
  const size_t n = (size_t)a.H * a.W * C;
  unsigned char* o = a.out + (size_t)blockIdx.y * n;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) o[i] = a.src[s.offset + i];
}

// ---- device: depth-mask filter -------------------------------------------------------------------------------------------------------
constexpr int TW = 32, TH = 8;        // tile of the local labelling: one workgroup of 256 threads

__device__ __forceinline__ int uf_find(int* L, int x) {       // parents only ever decrease, so the walk ends at the current root
  int p;
  while ((p = __hip_atomic_load(&L[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) != x) x = p;
  return x;
}
// label equivalence (Komura 2015 / Playne & Hawick 2018): hang the larger root under the smaller with atomicMin; when the larger one
// stopped being a root in the meantime, carry on with the parent it had.  The final partition, and the root of every set (its smallest
// index), do not depend on the interleaving.
__device__ __forceinline__ void uf_union(int* L, int x, int y) {
  for (;;) {
    x = uf_find(L, x);
    y = uf_find(L, y);
    if (x == y) return;
    if (x < y) { const int t = x; x = y; y = t; }
    const int old = atomicMin(&L[x], y);
    if (old == x) return;
    x = old;
  }
}

template <typename T>
__global__ void __launch_bounds__(256) cc_local_kernel(const T* __restrict__ mask, int* __restrict__ labels, int* __restrict__ counts, int H, int W) {
  __shared__ int L[TW * TH];
  const int lx = threadIdx.x & (TW - 1), ly = threadIdx.x / TW;
  const int x = blockIdx.x * TW + lx, y = blockIdx.y * TH + ly;
  const bool inside = x < W && y < H;
  const size_t g = ((size_t)blockIdx.z * H + y) * W + x;
  const bool fg = inside && mask[g] == (T)1;
  const int me = (int)threadIdx.x;
  L[me] = fg ? me : -1;
  __syncthreads();
  if (fg) {                                                 // the four neighbours that come earlier in raster order, inside the tile
    if (lx > 0 && L[me - 1] >= 0) uf_union(L, me, me - 1);
    if (ly > 0) {
      if (L[me - TW] >= 0) uf_union(L, me, me - TW);
      if (lx > 0 && L[me - TW - 1] >= 0) uf_union(L, me, me - TW - 1);
      if (lx < TW - 1 && L[me - TW + 1] >= 0) uf_union(L, me, me - TW + 1);
    }
  }
  __syncthreads();
  if (inside) {
    int lab = -1;
    if (fg) {
      const int r = uf_find(L, me);
      lab = (blockIdx.y * TH + r / TW) * W + blockIdx.x * TW + (r & (TW - 1));      // the root's pixel index in its image
    }
    labels[g] = lab;
    counts[g] = 0;
  }
}

// unions across tile borders, on the global parent array of each image.  One thread per pixel; only border pixels have work
__global__ void __launch_bounds__(256) cc_border_kernel(int* __restrict__ labels, int H, int W) {
  const int x = blockIdx.x * TW + (threadIdx.x & (TW - 1)), y = blockIdx.y * TH + threadIdx.x / TW;
  if (x >= W || y >= H) return;
  const int lx = x & (TW - 1), ly = y & (TH - 1);
  if (lx != 0 && ly != 0 && lx != TW - 1) return;
  int* L = labels + (size_t)blockIdx.z * H * W;
  const int me = y * W + x;
  if (L[me] < 0) return;
  if (lx == 0 && x > 0 && L[me - 1] >= 0) uf_union(L, me, me - 1);
  if (y > 0) {
    if (ly == 0 && L[me - W] >= 0) uf_union(L, me, me - W);
    if ((lx == 0 || ly == 0) && x > 0 && L[me - W - 1] >= 0) uf_union(L, me, me - W - 1);
    if ((lx == TW - 1 || ly == 0) && x < W - 1 && L[me - W + 1] >= 0) uf_union(L, me, me - W + 1);
  }
}

// every foreground pixel finds its root, remembers it and counts itself there
__global__ void __launch_bounds__(256) cc_count_kernel(int* __restrict__ labels, int* __restrict__ counts, int HW) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= HW) return;
  int* L = labels + (size_t)blockIdx.y * HW;
  if (__hip_atomic_load(&L[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < 0) return;
  const int r = uf_find(L, i);
  // a root keeps pointing at itself; any other pixel now points straight at its root, which is still an ancestor for concurrent walks
  if (r != i) __hip_atomic_store(&L[i], r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  atomicAdd(&counts[(size_t)blockIdx.y * HW + r], 1);
}

// `size < self.width * self.height / 100` (footprint_dataset.py:102): an integer against a Python float, strictly less
template <typename T>
__global__ void __launch_bounds__(256) cc_threshold_kernel(const int* __restrict__ labels, const int* __restrict__ counts, T* __restrict__ out, int HW,
                                                           double limit) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= HW) return;
  const size_t g = (size_t)blockIdx.y * HW + i;
  const int r = labels[g];
  out[g] = (r >= 0 && (double)counts[(size_t)blockIdx.y * HW + r] < limit) ? (T)1 : (T)0;
}

}  // namespace

extern "C" int32_t fp_resize_ksize(int32_t in_size, int32_t out_size, int32_t filter) {
  double (*fn)(double);
  double support;
  if (in_size <= 0 || out_size <= 0 || !filter_of(filter, &fn, &support)) return -1;
  double filterscale = (double)in_size / out_size;
  if (filterscale < 1.0) filterscale = 1.0;
  const double ks = ceil(support * filterscale) * 2 + 1;
  return ks < (double)(1 << 30) ? (int32_t)ks : -1;
}

// Resample.c precompute_coeffs: the double stage both table forms share.  kk double [out][ksize] = the taps normalised by their running
// sum, rows padded with zeros; bounds [out][2] = first source index, tap count.  Pillow computes every output index on its own, so the
// rows of output indices first .. first + count - 1 alone are the same rows of the whole table.  The caller has checked the arguments.
static void precompute_coeffs(int32_t in_size, int32_t out_size, double (*fn)(double), double support, int32_t first, int32_t count,
                              int32_t* bounds, double* kk, int32_t ksize) {
  const double scale = (double)in_size / out_size;
  const double filterscale = scale < 1.0 ? 1.0 : scale;
  support = support * filterscale;
  const double ss = 1.0 / filterscale;
  for (int xx = first; xx < first + count; ++xx) {
    const double center = 0.0 + (xx + 0.5) * scale;
    double ww = 0.0;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in_size) xmax = in_size;
    xmax -= xmin;
    double* k = kk + (size_t)(xx - first) * ksize;
    for (int x = 0; x < xmax; ++x) {
      const double w = fn((x + xmin - center + 0.5) * ss);
      k[x] = w;
      ww += w;
    }
    for (int x = 0; x < xmax; ++x)
      if (ww != 0.0) k[x] /= ww;
    for (int x = xmax; x < ksize; ++x) k[x] = 0;
    bounds[(xx - first) * 2 + 0] = xmin;
    bounds[(xx - first) * 2 + 1] = xmax;
  }
}

// the taps as Pillow's 32-bit-per-channel passes (mode "F") use them: normalised, not quantised
extern "C" int fp_resize_coeffs_f64(int32_t in_size, int32_t out_size, int32_t filter, int32_t* bounds, double* kk, int32_t ksize) {
  double (*fn)(double);
  double support;
  FP_REQUIRE(bounds && kk && in_size > 0 && out_size > 0, "fp_resize_coeffs_f64: bad arguments");
  FP_REQUIRE(filter_of(filter, &fn, &support), "fp_resize_coeffs_f64: filter must be FP_RESIZE_LANCZOS, _BILINEAR, _BICUBIC or _BOX");
  FP_REQUIRE(ksize == fp_resize_ksize(in_size, out_size, filter), "fp_resize_coeffs_f64: ksize differs from fp_resize_ksize");
  precompute_coeffs(in_size, out_size, fn, support, 0, out_size, bounds, kk, ksize);
  return 0;
}

// Resample.c precompute_coeffs + normalize_coeffs_8bpc for the output indices first .. first + count - 1: work and memory of `count` rows
extern "C" int fp_resize_coeffs_range(int32_t in_size, int32_t out_size, int32_t filter, int32_t first, int32_t count, int32_t* bounds, int32_t* kk,
                                      int32_t ksize) {
  double (*fn)(double);
  double support;
  FP_REQUIRE(bounds && kk && in_size > 0 && out_size > 0, "fp_resize_coeffs: bad arguments");
  FP_REQUIRE(filter_of(filter, &fn, &support), "fp_resize_coeffs: filter must be FP_RESIZE_LANCZOS, _BILINEAR, _BICUBIC or _BOX");
  FP_REQUIRE(ksize == fp_resize_ksize(in_size, out_size, filter), "fp_resize_coeffs: ksize differs from fp_resize_ksize");
  FP_REQUIRE(first >= 0 && count > 0 && count <= out_size - first, "fp_resize_coeffs_range: first .. first + count - 1 must lie inside the output");
  // Pillow keeps the double weights in the table and quantises afterwards
  double* w = (double*)malloc(sizeof(double) * (size_t)count * (size_t)ksize);
  FP_REQUIRE(w, "fp_resize_coeffs: out of memory");
  precompute_coeffs(in_size, out_size, fn, support, first, count, bounds, w, ksize);
  for (size_t i = 0, n = (size_t)count * (size_t)ksize; i < n; ++i)
    kk[i] = w[i] < 0 ? (int)(-0.5 + w[i] * (1 << PRECISION_BITS)) : (int)(0.5 + w[i] * (1 << PRECISION_BITS));
  free(w);
  return 0;
}

extern "C" int fp_resize_coeffs(int32_t in_size, int32_t out_size, int32_t filter, int32_t* bounds, int32_t* kk, int32_t ksize) {
  FP_REQUIRE(out_size > 0, "fp_resize_coeffs: bad arguments");
  return fp_resize_coeffs_range(in_size, out_size, filter, 0, out_size, bounds, kk, ksize);
}

// Pillow's NEAREST resize of one axis (libImaging Geometry.c, ImagingScaleAffine with the scale in / out and the offset of half a step): the
// source coordinate is ACCUMULATED in double, one addition per output index, and truncated
extern "C" int fp_nearest_index(int32_t in_size, int32_t out_size, int32_t* idx) {
  FP_REQUIRE(idx && in_size > 0 && out_size > 0, "fp_nearest_index: bad arguments");
  const double step = (double)in_size / out_size;
  double o = step * 0.5;
  for (int x = 0; x < out_size; ++x) {
    const int i = (int)o;
    idx[x] = i < in_size ? i : in_size - 1;
    o += step;
  }
  return 0;
}

extern "C" int32_t fp_resize_sample_bytes(void) { return (int32_t)sizeof(ResizeSample); }
extern "C" int32_t fp_resize_table_bytes(void) { return (int32_t)sizeof(ResizeTable); }

extern "C" int64_t fp_resize_workspace(int32_t B, int32_t max_h, int32_t W, int32_t C) {
  if (B <= 0 || max_h <= 0 || W <= 0 || (C != 1 && C != 3)) return -1;
  return (((int64_t)B * max_h * W * C + 15) & ~(int64_t)15) + 16;       // the intermediate, then the status word
}

extern "C" int64_t fp_resize_status_offset(int32_t B, int32_t max_h, int32_t W, int32_t C) {
  const int64_t n = fp_resize_workspace(B, max_h, W, C);
  return n < 0 ? -1 : n - 16;
}

extern "C" int fp_resize_u8(const uint8_t* src, int64_t src_bytes, const void* samples, const void* tables, int32_t n_tables, const int32_t* coeffs,
                            int64_t coeffs_len, uint8_t* out, int32_t B, int32_t H, int32_t W, int32_t C, int32_t max_h, int32_t max_w,
                            void* workspace, int64_t workspace_bytes, fp_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  FP_REQUIRE(src && samples && out && B > 0 && H > 0 && W > 0 && max_h > 0 && max_w > 0 && src_bytes > 0, "fp_resize_u8: bad arguments");
  FP_REQUIRE(C == 1 || C == 3, "fp_resize_u8: C must be 1 or 3");
  FP_REQUIRE(n_tables == 0 || (tables && coeffs && coeffs_len > 0), "fp_resize_u8: tables are missing");
  FP_REQUIRE(B <= 65535 && (int64_t)H * W * C < ((int64_t)1 << 31) && (int64_t)max_h * max_w * C < ((int64_t)1 << 31), "fp_resize_u8: too large");
  FP_REQUIRE(((uintptr_t)src & 3) == 0, "fp_resize_u8: the source buffer must be 4-byte aligned");
  const size_t lds = (((size_t)max_w * C + 3) & ~(size_t)3) + 4;
  FP_REQUIRE(lds <= 64 * 1024, "fp_resize_u8: a source row must fit 64 KiB of LDS (max_w * C <= 65528)");
  FP_REQUIRE(workspace && workspace_bytes >= fp_resize_workspace(B, max_h, W, C), "fp_resize_u8: workspace too small (fp_resize_workspace)");
  FP_REQUIRE(((uintptr_t)workspace & 3) == 0, "fp_resize_u8: the workspace must be 4-byte aligned");
  ResizeArgs a;
  a.src = src; a.src_bytes = src_bytes; a.samples = (const ResizeSample*)samples; a.tables = (const ResizeTable*)tables; a.n_tables = n_tables;
  a.coeffs = coeffs; a.coeffs_len = coeffs_len; a.tmp = (unsigned char*)workspace; a.out = out; a.H = H; a.W = W; a.max_h = max_h; a.max_w = max_w;
  a.status = (int32_t*)((unsigned char*)workspace + fp_resize_status_offset(B, max_h, W, C));
  hipError_t e = hipMemsetAsync(a.status, 0, sizeof(int32_t), stream);
  if (e != hipSuccess) return fp_set_error((int)e, "fp_resize_u8: %s", hipGetErrorString(e));
  // the sample records live on the device: every kernel is launched for the largest sample and leaves early where it has nothing to do
  if (C == 3) fp_launch(resize_horizontal_kernel<3>, dim3(max_h, B), dim3(256), (unsigned)lds, stream, a);
  else fp_launch(resize_horizontal_kernel<1>, dim3(max_h, B), dim3(256), (unsigned)lds, stream, a);
  int rc = fp_check_launch("fp_resize_u8(horizontal)");
  if (rc) return rc;
  fp_launch(resize_vertical_kernel, dim3((unsigned)fp_ceil_div((int64_t)W * C, 1024), (unsigned)fp_ceil_div(H, VT), B), dim3(256), 0, stream, a, C);
  rc = fp_check_launch("fp_resize_u8(vertical)");
  if (rc) return rc;
  if (max_h >= H && max_w >= W) {
    int bx = (int)fp_ceil_div((int64_t)H * W * C, 256 * 16);
    fp_launch(resize_copy_kernel, dim3(bx, B), dim3(256), 0, stream, a, C);
    rc = fp_check_launch("fp_resize_u8(copy)");
  }
  return rc;
}

extern "C" int64_t fp_filter_depth_mask_workspace(int32_t B, int32_t H, int32_t W) {
  if (B <= 0 || H <= 0 || W <= 0 || (int64_t)H * W >= ((int64_t)1 << 31) || B > 65535) return -1;
  return (int64_t)B * H * W * 2 * (int64_t)sizeof(int32_t);
}

extern "C" int fp_filter_depth_mask(const void* mask, int32_t is_double, void* out, int32_t B, int32_t H, int32_t W, void* workspace,
                                    int64_t workspace_bytes, fp_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  FP_REQUIRE(mask && out && B > 0 && H > 0 && W > 0, "fp_filter_depth_mask: bad arguments");
  const int64_t need = fp_filter_depth_mask_workspace(B, H, W);
  FP_REQUIRE(need > 0, "fp_filter_depth_mask: too large");
  FP_REQUIRE(workspace && workspace_bytes >= need, "fp_filter_depth_mask: workspace too small (fp_filter_depth_mask_workspace)");
  const int HW = H * W;
  int* labels = (int*)workspace;
  int* counts = labels + (size_t)B * HW;
  const dim3 tiles((unsigned)fp_ceil_div(W, TW), (unsigned)fp_ceil_div(H, TH), B);
  FP_REQUIRE(tiles.y <= 65535, "fp_filter_depth_mask: too many rows");
  const double limit = (double)((int64_t)W * H) / 100;
  if (is_double) fp_launch(cc_local_kernel<double>, tiles, dim3(256), 0, stream, (const double*)mask, labels, counts, H, W);
  else fp_launch(cc_local_kernel<float>, tiles, dim3(256), 0, stream, (const float*)mask, labels, counts, H, W);
  int rc = fp_check_launch("fp_filter_depth_mask(local)");
  if (rc) return rc;
  fp_launch(cc_border_kernel, tiles, dim3(256), 0, stream, labels, H, W);
  rc = fp_check_launch("fp_filter_depth_mask(border)");
  if (rc) return rc;
  const dim3 flat((unsigned)fp_ceil_div(HW, 256), B);
  fp_launch(cc_count_kernel, flat, dim3(256), 0, stream, labels, counts, HW);
  rc = fp_check_launch("fp_filter_depth_mask(count)");
  if (rc) return rc;
  if (is_double) fp_launch(cc_threshold_kernel<double>, flat, dim3(256), 0, stream, (const int*)labels, (const int*)counts, (double*)out, HW, limit);
  else fp_launch(cc_threshold_kernel<float>, flat, dim3(256), 0, stream, (const int*)labels, (const int*)counts, (float*)out, HW, limit);
  return fp_check_launch("fp_filter_depth_mask");
}
