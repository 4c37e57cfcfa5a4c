// Device-side reader work of the ground-segmentation trainer: what the reference's segmentation datasets do to a
// label image before the network sees it.  (The frame's windowed resize, fp_resize_window_u8, is resample_u8.hip.)
//   reference: footprints/preprocessing/segmentation/datasets/dataset_utils.py:24-91 (prepare_size: resize_all + crop_all),
//              cityscapes_dataset.py:46-71, matterport_dataset.py:44-64, ade20k_dataset.py:49-59, base_dataset.py:57-60 (in1d).
// fp_seg_labels: NEAREST resizes, crops and the flip of a label image are index maps; the host composes them into one row table and one
// column table per sample, and one kernel gathers, decodes the label id and looks it up in the sample's ground-id set.
// No float operation, no atomics, no reductions: every output element is written once, by one thread.
#include "fp_common.h"

namespace {

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

extern "C" int32_t fp_seg_label_sample_bytes(void) { return (int32_t)sizeof(LabelSample); }

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
