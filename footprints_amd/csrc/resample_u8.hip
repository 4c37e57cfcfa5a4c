// Pillow's 8-bit resample on the device: everything that restates libImaging/Resample.c for 8-bit images.
//   reference: footprints/datasets/footprint_dataset.py:73-80 (Image.resize(LANCZOS)), datasets/inference_dataset.py:26,48, predict_simple.py:41,55;
//              footprints/preprocessing/segmentation/datasets/dataset_utils.py:24-91 (prepare_size: resize_all + crop_all).
// A separable filter (ImagingResampleHorizontal_8bpc / Vertical_8bpc) whose coefficients are normalised in double on the host and quantised
// to 22 fractional bits; the image passes are pure int32 arithmetic with a uint8 intermediate between the horizontal and the vertical pass.
// The tables are built here on the HOST (fp_resize_coeffs; this file is compiled with -ffp-contract=off, and sin() is the C library's, as
// in Pillow); the kernels use no float operation, no atomics and no reductions: every output byte is written once, by one thread.
// There is ONE pair of passes.  fp_resize_window_u8 gives every sample its own target size and produces only a WINDOW of it from a staged
// rectangle of the source (the reference resizes the whole frame and crop_all keeps 192 x 640 of it, while the crop offsets are known
// before any pixel is touched); fp_resize_u8, whole frames to one target size, is the same with window = target and rectangle = source.
// Each entry point has its own record layout and acceptance rule; a decoder turns a record into the View the passes are written against.
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

// ---- device: the records of the two entry points, and the view of one sample that the passes work from -------------------------------
// one axis of a sample: its table rows and the source indices their taps reach
struct Axis {
  const int32_t* bounds;    // [out][2] = first source index, tap count, from the pass's first output index on; null: the pass is skipped
  const int32_t* kk;        // [out][ksize], likewise
  int ksize;
  int lo, hi;               // the taps reach the source indices [lo, hi) of the full source image
};
// filled once per workgroup, in registers; nothing in it says which record kind it came from
struct View {
  int64_t src_off;          // of staged row 0's first byte in the source buffer
  int src_pitch;            // bytes from one staged row to the next
  int rows;                 // staged rows
  int y0, x0;               // where staged row 0 sits in the full source image
  Axis h, v;
  int out_w, out_h, top;    // the sample's output, and the target row of its row 0
  unsigned char* out;
  unsigned char* tmp;       // the sample's intermediate: row r = staged row r
  int tmp_pitch;
  bool direct;              // the vertical pass reads the staged rows themselves: no horizontal pass runs
};

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

  // one axis of a record: no table and the size is the target's already, or a table of the library's for exactly this pair of sizes
  __device__ __forceinline__ bool axis(int table, int in_size, int out_size, Axis* ax) const {
    *ax = Axis{nullptr, nullptr, 0, 0, in_size};
    if (table < 0) return in_size == out_size;
    if (table >= n_tables) return false;
    const ResizeTable t = tables[table];
    if (!(t.in_size == in_size && t.out_size == out_size && t.ksize > 0 && t.bounds_off >= 0 && t.kk_off >= 0 &&
          (int64_t)t.bounds_off + 2 * (int64_t)out_size <= coeffs_len && (int64_t)t.kk_off + (int64_t)out_size * t.ksize <= coeffs_len))
      return false;
    ax->bounds = coeffs + t.bounds_off;
    ax->kk = coeffs + t.kk_off;
    ax->ksize = t.ksize;
    return true;
  }
  // a sample record the kernels may follow without leaving any buffer; everything else leaves the sample's output untouched and is
  // reported in the status word.  Both passes ask the same question, so a sample is resized whole or left alone
  __device__ __forceinline__ bool view(int sample, int C, View* v) const {
    const ResizeSample s = samples[sample];
    if (s.h <= 0 || s.w <= 0 || s.h > max_h || s.w > max_w || s.offset < 0) return false;
    if (s.offset + (int64_t)s.h * s.w * C > src_bytes) return false;
    if (!axis(s.table_h, s.w, W, &v->h) || !axis(s.table_v, s.h, H, &v->v)) return false;
    v->src_off = s.offset; v->src_pitch = s.w * C; v->rows = s.h; v->y0 = 0; v->x0 = 0;
    v->out_w = W; v->out_h = H; v->top = 0;
    v->out = out + (size_t)sample * H * W * C;
    v->tmp_pitch = W * C;
    v->tmp = tmp + (size_t)sample * max_h * v->tmp_pitch;
    v->direct = s.table_h < 0 && s.table_v >= 0;      // the source rows have the output's width already
    return true;
  }
};

struct WinTable {           // fp_resize_window_table
  int32_t in_size, out_size, ksize;
  int32_t first, count;     // the rows describe the output indices first .. first + count - 1
  int32_t bounds_off;       // into the int32 table buffer: [count][2] = first source index, tap count
  int32_t kk_off;           // [count][ksize]
};
struct WinSample {          // fp_resize_window_sample
  int64_t src_offset;       // of the staged rectangle's first byte in the source buffer; dense uint8 [src_h][src_w][C]
  int64_t out_offset;       // of the window's first byte in the output buffer; dense uint8 [win_h][win_w][C]
  int32_t src_h, src_w;
  int32_t src_y0, src_x0;   // where the rectangle sits in the full source image
  int32_t table_h, table_v; // -1: the pass is skipped (the target size of that axis is the source's)
  int32_t top, left, win_h, win_w;
};

struct WinArgs {
  const unsigned char* src;
  int64_t src_bytes;
  const WinSample* samples;
  const WinTable* tables;
  int32_t n_tables;
  const int32_t* coeffs;
  int64_t coeffs_len;
  unsigned char* tmp;       // [B][max_src_h][max_win_w][C]
  unsigned char* out;
  int64_t out_bytes;
  int32_t* status;
  int32_t max_src_h, max_src_w, max_win_h, max_win_w;

  // one axis of a record: the window [lo, lo + n) lies inside the target, the table (when there is one) describes it, and the rectangle
  // [r0, r0 + rn) covers every source index the window's taps reach.  Pillow's bounds never decrease along a table, so the first row's
  // first tap and the last row's last tap span them all; the passes check every row's taps again before they follow them.
  __device__ __forceinline__ bool axis(int table, int lo, int n, int r0, int rn, Axis* ax) const {
    *ax = Axis{nullptr, nullptr, 0, lo, lo + n};
    if (table < 0) return lo >= r0 && (int64_t)lo + n <= (int64_t)r0 + rn;
    if (table >= n_tables) return false;
    const WinTable t = tables[table];
    if (t.in_size <= 0 || t.out_size <= 0 || t.ksize <= 0 || t.first < 0 || t.count <= 0 || (int64_t)t.first + t.count > t.out_size) return false;
    if (t.bounds_off < 0 || t.kk_off < 0 || (int64_t)t.bounds_off + 2 * (int64_t)t.count > coeffs_len ||
        (int64_t)t.kk_off + (int64_t)t.count * t.ksize > coeffs_len)
      return false;
    if (lo < t.first || (int64_t)lo + n > (int64_t)t.first + t.count) return false;
    if ((int64_t)r0 + rn > t.in_size) return false;
    ax->bounds = coeffs + t.bounds_off + 2 * (size_t)(lo - t.first);
    ax->kk = coeffs + t.kk_off + (size_t)(lo - t.first) * t.ksize;
    ax->ksize = t.ksize;
    const int first = ax->bounds[0];
    const int last_min = ax->bounds[2 * (n - 1)], last_n = ax->bounds[2 * (n - 1) + 1];
    if (first < 0 || last_min < first || last_n < 0 || last_n > t.ksize) return false;
    ax->lo = first;
    ax->hi = last_min + last_n;
    return first >= r0 && (int64_t)last_min + last_n <= (int64_t)r0 + rn;
  }
  // a record the kernels may follow without leaving any buffer; every pass asks the same question, so a sample is written whole or not at all
  __device__ __forceinline__ bool view(int sample, int C, View* v) const {
    const WinSample s = samples[sample];
    if (s.src_h <= 0 || s.src_w <= 0 || s.src_h > max_src_h || s.src_w > max_src_w || s.src_offset < 0 || s.src_y0 < 0 || s.src_x0 < 0) return false;
    if (s.src_offset + (int64_t)s.src_h * s.src_w * C > src_bytes) return false;
    if (s.win_h <= 0 || s.win_w <= 0 || s.win_h > max_win_h || s.win_w > max_win_w || s.top < 0 || s.left < 0 || s.out_offset < 0) return false;
    if (s.out_offset + (int64_t)s.win_h * s.win_w * C > out_bytes) return false;
    if (!axis(s.table_h, s.left, s.win_w, s.src_x0, s.src_w, &v->h)) return false;
    if (!axis(s.table_v, s.top, s.win_h, s.src_y0, s.src_h, &v->v)) return false;
    v->src_off = s.src_offset; v->src_pitch = s.src_w * C; v->rows = s.src_h; v->y0 = s.src_y0; v->x0 = s.src_x0;
    v->out_w = s.win_w; v->out_h = s.win_h; v->top = s.top;
    v->out = out + s.out_offset;
    v->tmp_pitch = max_win_w * C;
    v->tmp = tmp + (size_t)sample * max_src_h * v->tmp_pitch;
    v->direct = false;                                // without a table the horizontal pass copies the window's columns
    return true;
  }
};

__device__ __forceinline__ void reject(int32_t* status) {       // every rejecting workgroup stores the same 1
  if (threadIdx.x == 0) *status = 1;
}
__device__ __forceinline__ unsigned char clip8(int v) { return (unsigned char)min(max(v >> PRECISION_BITS, 0), 255); }

// horizontal pass: one workgroup = one staged row of one sample; rows outside the span of the vertical taps leave at once.  Only the column
// span the horizontal taps reach is staged through LDS (dynamic: the widest staged row's bytes rounded up to 4, + 4); a thread owns whole
// output pixels, so a coefficient is loaded once for the C channels.  Without a table the pass copies the output's columns.
// grid = (most staged rows, B)
template <typename Args, int C>
__global__ void __launch_bounds__(256) resample_horizontal_kernel(const Args a) {
  extern __shared__ unsigned int row_words[];
  View v;
  if (!a.view(blockIdx.y, C, &v)) return reject(a.status);
  const int y = blockIdx.x;
  if (v.direct || y >= v.rows || y + v.y0 < v.v.lo || y + v.y0 >= v.v.hi) return;
  // the span starts at any byte address: whole aligned words where the buffer holds them, bytes at its very end
  const int64_t first = v.src_off + (int64_t)y * v.src_pitch + (v.h.lo - v.x0) * C;
  const int shift = (int)(first & 3);
  const int64_t word0 = first - shift;
  const int n_words = (shift + (v.h.hi - v.h.lo) * C + 3) >> 2;
  for (int i = threadIdx.x; i < n_words; i += 256) {
    const int64_t p = word0 + 4 * (int64_t)i;
    unsigned int w = 0;
    if (p + 4 <= a.src_bytes) w = *reinterpret_cast<const unsigned int*>(a.src + p);
    else
      for (int j = 0; j < 4; ++j)
        if (p + j < a.src_bytes) w |= (unsigned int)a.src[p + j] << (8 * j);
    row_words[i] = w;
  }
  __syncthreads();
  const unsigned char* row = reinterpret_cast<const unsigned char*>(row_words) + shift;       // row[0] = source column h.lo
  // without a vertical pass this IS the output row: source row = target row
  unsigned char* dst = v.v.bounds ? v.tmp + (size_t)y * v.tmp_pitch : v.out + (size_t)(y + v.y0 - v.top) * v.out_w * C;
  if (!v.h.bounds) {
    for (int i = threadIdx.x; i < v.out_w * C; i += 256) dst[i] = row[i];
    return;
  }
  for (int xx = threadIdx.x; xx < v.out_w; xx += 256) {
    const int xmin = v.h.bounds[2 * xx], n = v.h.bounds[2 * xx + 1];
    const int32_t* k = v.h.kk + (size_t)xx * v.h.ksize;
    int acc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = 1 << (PRECISION_BITS - 1);
    if (xmin < v.h.lo || n < 0 || n > v.h.ksize || xmin + n > v.h.hi) *a.status = 1;       // never outside the staged span
    else
      for (int x = 0; x < n; ++x) {
        const int w = k[x];
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] += w * (int)row[(xmin - v.h.lo + x) * C + c];
      }
#pragma unroll
    for (int c = 0; c < C; ++c) dst[xx * C + c] = clip8(acc[c]);
  }
}

// vertical pass over rows of out_w * C bytes (the channel layout does not matter to it): a thread owns 4 consecutive bytes of VT output rows
// and walks the source rows those outputs need once, so a source byte is loaded once per tile of VT output rows; the coefficients and
// bounds are uniform over the workgroup.  grid = (strips of 1024 bytes of the widest output, ceil(tallest output / VT), B)
constexpr int VT = 8;
template <typename Args>
__global__ void __launch_bounds__(256) resample_vertical_kernel(const Args a, int C) {
  View v;
  if (!a.view(blockIdx.z, C, &v)) return reject(a.status);
  if (!v.v.bounds) return;
  const int row_bytes = v.out_w * C;
  const unsigned char* in = v.direct ? a.src + v.src_off : v.tmp;       // row r of it = source row r + y0
  const size_t pitch = v.direct ? v.src_pitch : v.tmp_pitch;
  const int y0 = blockIdx.y * VT;
  const int j = (blockIdx.x * 256 + threadIdx.x) * 4;
  if (j >= row_bytes || y0 >= v.out_h) return;
  const int nb = min(4, row_bytes - j);
  int ymin[VT], cnt[VT], acc[VT][4];
  int lo = v.v.hi, hi = v.v.lo;
#pragma unroll
  for (int i = 0; i < VT; ++i) {
    const bool live = y0 + i < v.out_h;
    ymin[i] = live ? v.v.bounds[2 * (y0 + i)] : v.v.lo;
    cnt[i] = live ? v.v.bounds[2 * (y0 + i) + 1] : 0;
    // never outside the rows the horizontal pass has written
    if (ymin[i] < v.v.lo || cnt[i] < 0 || cnt[i] > v.v.ksize || ymin[i] + cnt[i] > v.v.hi) { cnt[i] = 0; *a.status = 1; }
    if (cnt[i] > 0) { lo = min(lo, ymin[i]); hi = max(hi, ymin[i] + cnt[i]); }
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[i][b] = 1 << (PRECISION_BITS - 1);
  }
  for (int r = lo; r < hi; ++r) {
    const unsigned char* p = in + (size_t)(r - v.y0) * pitch + j;
    unsigned int w4 = 0;
    if (nb == 4) __builtin_memcpy(&w4, p, 4);
    else
      for (int b = 0; b < nb; ++b) w4 |= (unsigned int)p[b] << (8 * b);
#pragma unroll
    for (int i = 0; i < VT; ++i) {
      const int x = r - ymin[i];
      if (x >= 0 && x < cnt[i]) {
        const int w = v.v.kk[(size_t)(y0 + i) * v.v.ksize + x];
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[i][b] += w * (int)((w4 >> (8 * b)) & 0xffu);
      }
    }
  }
#pragma unroll
  for (int i = 0; i < VT; ++i) {
    if (y0 + i >= v.out_h) break;
    unsigned char* o = v.out + (size_t)(y0 + i) * row_bytes + j;
    for (int b = 0; b < nb; ++b) o[b] = clip8(acc[i][b]);
  }
}

// ---- host: what the two entry points share -------------------------------------------------------------------------------------------
// the intermediate rounded up to 16 bytes, then the status word
int64_t workspace_bytes_of(int32_t B, int32_t rows, int32_t w, int32_t C) {
  if (B <= 0 || rows <= 0 || w <= 0 || (C != 1 && C != 3)) return -1;
  return (((int64_t)B * rows * w * C + 15) & ~(int64_t)15) + 16;
}
int64_t status_offset_of(int32_t B, int32_t rows, int32_t w, int32_t C) {
  const int64_t n = workspace_bytes_of(B, rows, w, C);
  return n < 0 ? -1 : n - 16;
}

// the argument checks of `fn`; `need` is what its workspace function `ws_fn` asks for
int check_args(const char* fn, const char* ws_fn, const void* src, int32_t C, const void* tables, int32_t n_tables, const int32_t* coeffs,
               int64_t coeffs_len, const void* workspace, int64_t workspace_bytes, int64_t need) {
  FP_REQUIRE(C == 1 || C == 3, "%s: C must be 1 or 3", fn);
  FP_REQUIRE(n_tables == 0 || (tables && coeffs && coeffs_len > 0), "%s: tables are missing", fn);
  FP_REQUIRE(((uintptr_t)src & 3) == 0, "%s: the source buffer must be 4-byte aligned", fn);
  FP_REQUIRE(workspace && workspace_bytes >= need, "%s: workspace too small (%s)", fn, ws_fn);
  FP_REQUIRE(((uintptr_t)workspace & 3) == 0, "%s: the workspace must be 4-byte aligned", fn);
  return 0;
}

// clears the status word, then the two passes over `rows` staged rows and an output of out_h rows of out_row_bytes.  The records live on
// the device: every kernel is launched for the largest sample and leaves early where it has nothing to do
template <typename Args>
int run_passes(const char* fn, const Args& a, int32_t B, int32_t C, int32_t rows, size_t lds, int64_t out_row_bytes, int32_t out_h,
               hipStream_t stream) {
  hipError_t e = hipMemsetAsync(a.status, 0, sizeof(int32_t), stream);
  if (e != hipSuccess) return fp_set_error((int)e, "%s: %s", fn, hipGetErrorString(e));
  if (C == 3) fp_launch(resample_horizontal_kernel<Args, 3>, dim3(rows, B), dim3(256), (unsigned)lds, stream, a);
  else fp_launch(resample_horizontal_kernel<Args, 1>, dim3(rows, B), dim3(256), (unsigned)lds, stream, a);
  const auto check = [fn](const char* pass) {
    const int rc = fp_check_launch(fn);
    return rc ? fp_set_error(rc, "%s(%s): %s", fn, pass, hipGetErrorString((hipError_t)rc)) : 0;
  };
  if (const int rc = check("horizontal")) return rc;
  fp_launch(resample_vertical_kernel<Args>, dim3((unsigned)fp_ceil_div(out_row_bytes, 1024), (unsigned)fp_ceil_div(out_h, VT), B), dim3(256), 0,
            stream, a, C);
  return check("vertical");
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
extern "C" int32_t fp_resize_window_sample_bytes(void) { return (int32_t)sizeof(WinSample); }
extern "C" int32_t fp_resize_window_table_bytes(void) { return (int32_t)sizeof(WinTable); }

extern "C" int64_t fp_resize_workspace(int32_t B, int32_t max_h, int32_t W, int32_t C) { return workspace_bytes_of(B, max_h, W, C); }
extern "C" int64_t fp_resize_status_offset(int32_t B, int32_t max_h, int32_t W, int32_t C) { return status_offset_of(B, max_h, W, C); }
extern "C" int64_t fp_resize_window_workspace(int32_t B, int32_t max_src_h, int32_t max_win_w, int32_t C) {
  return workspace_bytes_of(B, max_src_h, max_win_w, C);
}
extern "C" int64_t fp_resize_window_status_offset(int32_t B, int32_t max_src_h, int32_t max_win_w, int32_t C) {
  return status_offset_of(B, max_src_h, max_win_w, C);
}

extern "C" int fp_resize_u8(const uint8_t* src, int64_t src_bytes, const void* samples, const void* tables, int32_t n_tables, const int32_t* coeffs,
                            int64_t coeffs_len, uint8_t* out, int32_t B, int32_t H, int32_t W, int32_t C, int32_t max_h, int32_t max_w,
                            void* workspace, int64_t workspace_bytes, fp_stream_t stream_) {
  FP_REQUIRE(src && samples && out && B > 0 && H > 0 && W > 0 && max_h > 0 && max_w > 0 && src_bytes > 0, "fp_resize_u8: bad arguments");
  const int rc = check_args("fp_resize_u8", "fp_resize_workspace", src, C, tables, n_tables, coeffs, coeffs_len, workspace, workspace_bytes,
                            workspace_bytes_of(B, max_h, W, C));
  if (rc) return rc;
  FP_REQUIRE(B <= 65535 && (int64_t)H * W * C < ((int64_t)1 << 31) && (int64_t)max_h * max_w * C < ((int64_t)1 << 31), "fp_resize_u8: too large");
  const size_t lds = (((size_t)max_w * C + 3) & ~(size_t)3) + 4;
  FP_REQUIRE(lds <= 64 * 1024, "fp_resize_u8: a source row must fit 64 KiB of LDS (max_w * C <= 65528)");
  ResizeArgs a;
  a.src = src; a.src_bytes = src_bytes; a.samples = (const ResizeSample*)samples; a.tables = (const ResizeTable*)tables; a.n_tables = n_tables;
  a.coeffs = coeffs; a.coeffs_len = coeffs_len; a.tmp = (unsigned char*)workspace; a.out = out; a.H = H; a.W = W; a.max_h = max_h; a.max_w = max_w;
  a.status = (int32_t*)((unsigned char*)workspace + status_offset_of(B, max_h, W, C));
  return run_passes("fp_resize_u8", a, B, C, max_h, lds, (int64_t)W * C, H, (hipStream_t)stream_);
}

extern "C" int fp_resize_window_u8(const uint8_t* src, int64_t src_bytes, const void* samples, const void* tables, int32_t n_tables,
                                   const int32_t* coeffs, int64_t coeffs_len, uint8_t* out, int64_t out_bytes, int32_t B, int32_t C,
                                   int32_t max_src_h, int32_t max_src_w, int32_t max_win_h, int32_t max_win_w, void* workspace,
                                   int64_t workspace_bytes, fp_stream_t stream_) {
  FP_REQUIRE(src && samples && out && B > 0 && max_src_h > 0 && max_src_w > 0 && max_win_h > 0 && max_win_w > 0 && src_bytes > 0 && out_bytes > 0,
             "fp_resize_window_u8: bad arguments");
  const int rc = check_args("fp_resize_window_u8", "fp_resize_window_workspace", src, C, tables, n_tables, coeffs, coeffs_len, workspace,
                            workspace_bytes, workspace_bytes_of(B, max_src_h, max_win_w, C));
  if (rc) return rc;
  FP_REQUIRE(n_tables >= 0 && B <= 65535 && (int64_t)max_win_h * max_win_w * C < ((int64_t)1 << 31) &&
                 (int64_t)max_src_h * max_src_w * C < ((int64_t)1 << 31) && (int64_t)max_src_h * max_win_w * C < ((int64_t)1 << 31),
             "fp_resize_window_u8: too large");
  const size_t lds = (((size_t)max_src_w * C + 3) & ~(size_t)3) + 4;
  FP_REQUIRE(lds <= 64 * 1024, "fp_resize_window_u8: a staged row must fit 64 KiB of LDS (max_src_w * C <= 65528)");
  FP_REQUIRE(fp_ceil_div(max_win_h, VT) <= 65535, "fp_resize_window_u8: too many window rows");
  WinArgs a;
  a.src = src; a.src_bytes = src_bytes; a.samples = (const WinSample*)samples; a.tables = (const WinTable*)tables; a.n_tables = n_tables;
  a.coeffs = coeffs; a.coeffs_len = coeffs_len; a.tmp = (unsigned char*)workspace; a.out = out; a.out_bytes = out_bytes;
  a.max_src_h = max_src_h; a.max_src_w = max_src_w; a.max_win_h = max_win_h; a.max_win_w = max_win_w;
  a.status = (int32_t*)((unsigned char*)workspace + status_offset_of(B, max_src_h, max_win_w, C));
  return run_passes("fp_resize_window_u8", a, B, C, max_src_h, lds, (int64_t)max_win_w * C, max_win_h, (hipStream_t)stream_);
}
