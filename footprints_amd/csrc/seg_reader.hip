// Device-side reader work of the ground-segmentation trainer: what the reference's segmentation datasets do to a
// decoded frame and its label image before the network sees them.
//   reference: footprints/preprocessing/segmentation/datasets/dataset_utils.py:24-91 (prepare_size: resize_all + crop_all),
//              cityscapes_dataset.py:46-71, matterport_dataset.py:44-64, ade20k_dataset.py:49-59, base_dataset.py:57-60 (in1d).
// (1) fp_resize_window_u8: Pillow's 8-bit resample as in reader.hip (22-bit fixed point, int32 accumulation, uint8 intermediate, horizontal
//     pass first), but every sample has its OWN target size and only a WINDOW of the target is produced: the reference resizes the whole
//     frame and crop_all keeps 192 x 640 of it, while the crop offsets are known before any pixel is touched.  The horizontal pass runs over
//     the source rows the window's vertical taps reach and over the window's columns only; the vertical pass produces the window.  The
//     source may be a staged rectangle of the frame (its origin is part of the record), so the host uploads only what the taps reach.
// (2) fp_seg_labels: NEAREST resizes, crops and the flip of a label image are index maps; the host composes them into one row table and one
//     column table per sample, and one kernel gathers, decodes the label id and looks it up in the sample's ground-id set.
// No float operation, no atomics, no reductions: every output element is written once, by one thread.
#include "fp_common.h"

namespace {

constexpr int PRECISION_BITS = 32 - 8 - 2;      // Resample.c

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
};

__device__ __forceinline__ void reject(const WinArgs& a) {
  if (threadIdx.x == 0) *a.status = 1;
}

// one axis of a record: the window [lo, lo + n) lies inside the target, the table (when there is one) describes it, and the rectangle
// [r0, r0 + rn) covers every source index the window's taps reach.  Pillow's bounds never decrease along a table, so the first row's
// first tap and the last row's last tap span them all; the passes check every row's taps again before they follow them.
__device__ __forceinline__ bool axis_ok(const WinArgs& a, int table, int lo, int n, int r0, int rn, int* span_lo, int* span_hi) {
  if (table < 0) {
    *span_lo = lo;
    *span_hi = lo + n;
    return lo >= r0 && (int64_t)lo + n <= (int64_t)r0 + rn;
  }
  if (table >= a.n_tables) return false;
  const WinTable t = a.tables[table];
  if (t.in_size <= 0 || t.out_size <= 0 || t.ksize <= 0 || t.first < 0 || t.count <= 0 || (int64_t)t.first + t.count > t.out_size) return false;
  if (t.bounds_off < 0 || t.kk_off < 0 || (int64_t)t.bounds_off + 2 * (int64_t)t.count > a.coeffs_len ||
      (int64_t)t.kk_off + (int64_t)t.count * t.ksize > a.coeffs_len)
    return false;
  if (lo < t.first || (int64_t)lo + n > (int64_t)t.first + t.count) return false;
  if ((int64_t)r0 + rn > t.in_size) return false;
  const int32_t* bounds = a.coeffs + t.bounds_off;
  const int first = bounds[2 * (lo - t.first)];
  const int last_min = bounds[2 * (lo + n - 1 - t.first)], last_n = bounds[2 * (lo + n - 1 - t.first) + 1];
  if (first < 0 || last_min < first || last_n < 0 || last_n > t.ksize) return false;
  *span_lo = first;
  *span_hi = last_min + last_n;
  return first >= r0 && (int64_t)last_min + last_n <= (int64_t)r0 + rn;
}

struct Spans {
  int x_lo, x_hi, y_lo, y_hi;       // the source columns and rows the window needs, in the full source image
};

// a record the kernels may follow without leaving any buffer; every pass asks the same question, so a sample is written whole or not at all
__device__ __forceinline__ bool record_ok(const WinArgs& a, const WinSample& s, int C, Spans* sp) {
  if (s.src_h <= 0 || s.src_w <= 0 || s.src_h > a.max_src_h || s.src_w > a.max_src_w || s.src_offset < 0 || s.src_y0 < 0 || s.src_x0 < 0) return false;
  if (s.src_offset + (int64_t)s.src_h * s.src_w * C > a.src_bytes) return false;
  if (s.win_h <= 0 || s.win_w <= 0 || s.win_h > a.max_win_h || s.win_w > a.max_win_w || s.top < 0 || s.left < 0 || s.out_offset < 0) return false;
  if (s.out_offset + (int64_t)s.win_h * s.win_w * C > a.out_bytes) return false;
  if (!axis_ok(a, s.table_h, s.left, s.win_w, s.src_x0, s.src_w, &sp->x_lo, &sp->x_hi)) return false;
  if (!axis_ok(a, s.table_v, s.top, s.win_h, s.src_y0, s.src_h, &sp->y_lo, &sp->y_hi)) return false;
  return true;
}

__device__ __forceinline__ unsigned char clip8(int v) { return (unsigned char)min(max(v >> PRECISION_BITS, 0), 255); }

// horizontal pass: one workgroup = one row of one sample's staged rectangle; rows outside the span of the window's vertical taps leave at
// once.  Only the column span the window's taps reach is staged through LDS (dynamic: max_src_w * C bytes rounded up to 4 + 4).  Without
// a table the pass copies the window's columns.  grid = (max_src_h, B)
template <int C>
__global__ void __launch_bounds__(256) window_horizontal_kernel(const WinArgs a) {
  extern __shared__ unsigned int row_words[];
  const WinSample s = a.samples[blockIdx.y];
  const int y = blockIdx.x;
  Spans sp;
  if (!record_ok(a, s, C, &sp)) return reject(a);
  if (y >= s.src_h || y + s.src_y0 < sp.y_lo || y + s.src_y0 >= sp.y_hi) return;
  // the span starts at any byte address: whole aligned words where the buffer holds them, bytes at its very end
  const int64_t first = s.src_offset + ((int64_t)y * s.src_w + (sp.x_lo - s.src_x0)) * C;
  const int shift = (int)(first & 3);
  const int64_t word0 = first - shift;
  const int n_words = (shift + (sp.x_hi - sp.x_lo) * C + 3) >> 2;
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
  const unsigned char* row = reinterpret_cast<const unsigned char*>(row_words) + shift;       // row[0] = source column sp.x_lo
  // without a vertical pass this IS the output row: source row = target row
  unsigned char* dst = s.table_v < 0 ? a.out + s.out_offset + (size_t)(y + s.src_y0 - s.top) * s.win_w * C
                                     : a.tmp + ((size_t)blockIdx.y * a.max_src_h + y) * a.max_win_w * C;
  if (s.table_h < 0) {
    for (int i = threadIdx.x; i < s.win_w * C; i += 256) dst[i] = row[i];
    return;
  }
  const WinTable t = a.tables[s.table_h];
  const int32_t* bounds = a.coeffs + t.bounds_off + 2 * (size_t)(s.left - t.first);
  const int32_t* kk = a.coeffs + t.kk_off + (size_t)(s.left - t.first) * t.ksize;
  for (int xx = threadIdx.x; xx < s.win_w; xx += 256) {
    const int xmin = bounds[2 * xx], n = bounds[2 * xx + 1];
    const int32_t* k = kk + (size_t)xx * t.ksize;
    int acc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = 1 << (PRECISION_BITS - 1);
    if (xmin < sp.x_lo || n < 0 || n > t.ksize || xmin + n > sp.x_hi) *a.status = 1;       // never outside the staged span
    else
      for (int x = 0; x < n; ++x) {
        const int w = k[x];
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] += w * (int)row[(xmin - sp.x_lo + x) * C + c];
      }
#pragma unroll
    for (int c = 0; c < C; ++c) dst[xx * C + c] = clip8(acc[c]);
  }
}

// vertical pass over the intermediate's rows of win_w * C bytes: a thread owns 4 consecutive bytes of VT window rows and walks the source rows
// those need once.  grid = (strips of 1024 bytes, ceil(max_win_h / VT), B)
constexpr int VT = 8;
__global__ void __launch_bounds__(256) window_vertical_kernel(const WinArgs a, int C) {
  const WinSample s = a.samples[blockIdx.z];
  Spans sp;
  if (!record_ok(a, s, C, &sp)) return reject(a);
  if (s.table_v < 0) return;
  const WinTable t = a.tables[s.table_v];
  const int row_bytes = s.win_w * C;
  const size_t tmp_stride = (size_t)a.max_win_w * C;
  const unsigned char* in = a.tmp + (size_t)blockIdx.z * a.max_src_h * tmp_stride;           // row r of it = source row r + src_y0
  const int32_t* bounds = a.coeffs + t.bounds_off + 2 * (size_t)(s.top - t.first);
  const int32_t* kk = a.coeffs + t.kk_off + (size_t)(s.top - t.first) * t.ksize;
  const int y0 = blockIdx.y * VT;
  const int j = (blockIdx.x * 256 + threadIdx.x) * 4;
  if (j >= row_bytes || y0 >= s.win_h) return;
  const int nb = min(4, row_bytes - j);
  int ymin[VT], cnt[VT], acc[VT][4];
  int lo = sp.y_hi, hi = sp.y_lo;
#pragma unroll
  for (int i = 0; i < VT; ++i) {
    const bool live = y0 + i < s.win_h;
    ymin[i] = live ? bounds[2 * (y0 + i)] : sp.y_lo;
    cnt[i] = live ? bounds[2 * (y0 + i) + 1] : 0;
    // never outside the rows the horizontal pass has written
    if (ymin[i] < sp.y_lo || cnt[i] < 0 || cnt[i] > t.ksize || ymin[i] + cnt[i] > sp.y_hi) { cnt[i] = 0; *a.status = 1; }
    if (cnt[i] > 0) { lo = min(lo, ymin[i]); hi = max(hi, ymin[i] + cnt[i]); }
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[i][b] = 1 << (PRECISION_BITS - 1);
  }
  for (int r = lo; r < hi; ++r) {
    const unsigned char* p = in + (size_t)(r - s.src_y0) * tmp_stride + j;
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
    if (y0 + i >= s.win_h) break;
    unsigned char* o = a.out + s.out_offset + (size_t)(y0 + i) * row_bytes + j;
    for (int b = 0; b < nb; ++b) o[b] = clip8(acc[i][b]);
  }
}

// ---- labels --------------------------------------------------------------------------------------------------------------------------
struct LabelSample {        // fp_seg_label_sample
  int64_t src_offset;       // of the staged label rectangle in the source buffer; dense uint8 [h][w][C]
  int32_t h, w, C;          // C = 1 or 3
  int32_t rows_off;         // into the int32 index buffer: [H] source row of every output row, relative to the rectangle
  int32_t cols_off;         // [W] source column of every output column (the flip is part of it)
  int32_t decode;           // FP_SEG_DECODE_*
  int32_t labelled;         // FP_SEG_LABELLED_*
  int32_t ground_set;       // index of its ground-id set
};

struct LabelArgs {
  const unsigned char* src;
  int64_t src_bytes;
  const LabelSample* samples;
  const int32_t* index;
  int64_t index_len;
  const int32_t* ground_ids;      // the sets one after the other, each sorted
  const int32_t* set_offsets;     // [n_sets + 1]
  int32_t n_sets;
  int64_t ground_len;
  float* ground_mask;
  float* labelled_pix;
  int32_t* status;
  int32_t H, W;
};

__device__ __forceinline__ bool label_record_ok(const LabelArgs& a, const LabelSample& s) {
  if (s.h <= 0 || s.w <= 0 || (s.C != 1 && s.C != 3) || s.src_offset < 0) return false;
  if (s.src_offset + (int64_t)s.h * s.w * s.C > a.src_bytes) return false;
  if (s.rows_off < 0 || s.cols_off < 0 || (int64_t)s.rows_off + a.H > a.index_len || (int64_t)s.cols_off + a.W > a.index_len) return false;
  if (s.decode != FP_SEG_DECODE_CHANNEL0 && s.decode != FP_SEG_DECODE_ADE20K) return false;
  if (s.decode == FP_SEG_DECODE_ADE20K && s.C != 3) return false;
  if (s.labelled != FP_SEG_LABELLED_ONES && s.labelled != FP_SEG_LABELLED_NONZERO) return false;
  if (s.ground_set < 0 || s.ground_set >= a.n_sets) return false;
  const int lo = a.set_offsets[s.ground_set], hi = a.set_offsets[s.ground_set + 1];
  return lo >= 0 && hi >= lo && hi <= a.ground_len;
}

// one thread = one output pixel.  grid = (ceil(H * W / 256), B)
__global__ void __launch_bounds__(256) seg_labels_kernel(const LabelArgs a) {
  const LabelSample s = a.samples[blockIdx.y];
  if (!label_record_ok(a, s)) {
    if (threadIdx.x == 0) *a.status = 1;
    return;
  }
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.H * a.W) return;
  const int y = i / a.W, x = i - y * a.W;
  const int sy = a.index[s.rows_off + y], sx = a.index[s.cols_off + x];
  if (sy < 0 || sy >= s.h || sx < 0 || sx >= s.w) {        // never outside the rectangle
    *a.status = 1;
    return;
  }
  const unsigned char* p = a.src + s.src_offset + ((size_t)sy * s.w + sx) * s.C;
  const int id = s.decode == FP_SEG_DECODE_ADE20K ? (int)p[0] / 10 * 256 + (int)p[1] : (int)p[0];
  bool ground = false;
  for (int k = a.set_offsets[s.ground_set], e = a.set_offsets[s.ground_set + 1]; k < e; ++k) ground |= a.ground_ids[k] == id;
  const size_t o = (size_t)blockIdx.y * a.H * a.W + i;
  a.ground_mask[o] = ground ? 1.0f : 0.0f;
  a.labelled_pix[o] = (s.labelled == FP_SEG_LABELLED_ONES || id != 0) ? 1.0f : 0.0f;
}

}  // namespace

extern "C" int32_t fp_resize_window_sample_bytes(void) { return (int32_t)sizeof(WinSample); }
extern "C" int32_t fp_resize_window_table_bytes(void) { return (int32_t)sizeof(WinTable); }
extern "C" int32_t fp_seg_label_sample_bytes(void) { return (int32_t)sizeof(LabelSample); }

extern "C" int64_t fp_resize_window_workspace(int32_t B, int32_t max_src_h, int32_t max_win_w, int32_t C) {
  if (B <= 0 || max_src_h <= 0 || max_win_w <= 0 || (C != 1 && C != 3)) return -1;
  return (((int64_t)B * max_src_h * max_win_w * C + 15) & ~(int64_t)15) + 16;       // the intermediate, then the status word
}

extern "C" int64_t fp_resize_window_status_offset(int32_t B, int32_t max_src_h, int32_t max_win_w, int32_t C) {
  const int64_t n = fp_resize_window_workspace(B, max_src_h, max_win_w, C);
  return n < 0 ? -1 : n - 16;
}

extern "C" int fp_resize_window_u8(const uint8_t* src, int64_t src_bytes, const void* samples, const void* tables, int32_t n_tables,
                                   const int32_t* coeffs, int64_t coeffs_len, uint8_t* out, int64_t out_bytes, int32_t B, int32_t C,
                                   int32_t max_src_h, int32_t max_src_w, int32_t max_win_h, int32_t max_win_w, void* workspace,
                                   int64_t workspace_bytes, fp_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  FP_REQUIRE(src && samples && out && B > 0 && max_src_h > 0 && max_src_w > 0 && max_win_h > 0 && max_win_w > 0 && src_bytes > 0 && out_bytes > 0,
             "fp_resize_window_u8: bad arguments");
  FP_REQUIRE(C == 1 || C == 3, "fp_resize_window_u8: C must be 1 or 3");
  FP_REQUIRE(n_tables == 0 || (tables && coeffs && coeffs_len > 0), "fp_resize_window_u8: tables are missing");
  FP_REQUIRE(n_tables >= 0 && B <= 65535 && (int64_t)max_win_h * max_win_w * C < ((int64_t)1 << 31) &&
                 (int64_t)max_src_h * max_src_w * C < ((int64_t)1 << 31) && (int64_t)max_src_h * max_win_w * C < ((int64_t)1 << 31),
             "fp_resize_window_u8: too large");
  FP_REQUIRE(((uintptr_t)src & 3) == 0, "fp_resize_window_u8: the source buffer must be 4-byte aligned");
  const size_t lds = (((size_t)max_src_w * C + 3) & ~(size_t)3) + 4;
  FP_REQUIRE(lds <= 64 * 1024, "fp_resize_window_u8: a staged row must fit 64 KiB of LDS (max_src_w * C <= 65528)");
  FP_REQUIRE(workspace && workspace_bytes >= fp_resize_window_workspace(B, max_src_h, max_win_w, C),
             "fp_resize_window_u8: workspace too small (fp_resize_window_workspace)");
  FP_REQUIRE(((uintptr_t)workspace & 3) == 0, "fp_resize_window_u8: the workspace must be 4-byte aligned");
  const int64_t vy = fp_ceil_div(max_win_h, VT);
  FP_REQUIRE(vy <= 65535, "fp_resize_window_u8: too many window rows");
  WinArgs a;
  a.src = src; a.src_bytes = src_bytes; a.samples = (const WinSample*)samples; a.tables = (const WinTable*)tables; a.n_tables = n_tables;
  a.coeffs = coeffs; a.coeffs_len = coeffs_len; a.tmp = (unsigned char*)workspace; a.out = out; a.out_bytes = out_bytes;
  a.max_src_h = max_src_h; a.max_src_w = max_src_w; a.max_win_h = max_win_h; a.max_win_w = max_win_w;
  a.status = (int32_t*)((unsigned char*)workspace + fp_resize_window_status_offset(B, max_src_h, max_win_w, C));
  hipError_t e = hipMemsetAsync(a.status, 0, sizeof(int32_t), stream);
  if (e != hipSuccess) return fp_set_error((int)e, "fp_resize_window_u8: %s", hipGetErrorString(e));
  // the records live on the device: every kernel is launched for the largest sample and leaves early where it has nothing to do
  if (C == 3) fp_launch(window_horizontal_kernel<3>, dim3(max_src_h, B), dim3(256), (unsigned)lds, stream, a);
  else fp_launch(window_horizontal_kernel<1>, dim3(max_src_h, B), dim3(256), (unsigned)lds, stream, a);
  int rc = fp_check_launch("fp_resize_window_u8(horizontal)");
  if (rc) return rc;
  fp_launch(window_vertical_kernel, dim3((unsigned)fp_ceil_div((int64_t)max_win_w * C, 1024), (unsigned)vy, B), dim3(256), 0, stream, a, C);
  return fp_check_launch("fp_resize_window_u8(vertical)");
}

extern "C" int fp_seg_labels(const uint8_t* src, int64_t src_bytes, const void* samples, const int32_t* index, int64_t index_len,
                             const int32_t* ground_ids, int64_t ground_len, const int32_t* set_offsets, int32_t n_sets, float* ground_mask,
                             float* labelled_pix, int32_t* status, int32_t B, int32_t H, int32_t W, fp_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  FP_REQUIRE(src && samples && index && ground_ids && set_offsets && ground_mask && labelled_pix && status, "fp_seg_labels: bad arguments");
  FP_REQUIRE(B > 0 && H > 0 && W > 0 && src_bytes > 0 && index_len > 0 && ground_len >= 0 && n_sets > 0, "fp_seg_labels: bad arguments");
  FP_REQUIRE(B <= 65535 && (int64_t)H * W < ((int64_t)1 << 31) - 256, "fp_seg_labels: too large");
  LabelArgs a;
  a.src = src; a.src_bytes = src_bytes; a.samples = (const LabelSample*)samples; a.index = index; a.index_len = index_len;
  a.ground_ids = ground_ids; a.set_offsets = set_offsets; a.n_sets = n_sets; a.ground_len = ground_len; a.ground_mask = ground_mask;
  a.labelled_pix = labelled_pix; a.status = status; a.H = H; a.W = W;
  hipError_t e = hipMemsetAsync(status, 0, sizeof(int32_t), stream);
  if (e != hipSuccess) return fp_set_error((int)e, "fp_seg_labels: %s", hipGetErrorString(e));
  fp_launch(seg_labels_kernel, dim3((unsigned)fp_ceil_div((int64_t)H * W, 256), B), dim3(256), 0, stream, a);
  return fp_check_launch("fp_seg_labels");
}
