// Output stage of the ground-segmentation network's inference mode: what the reference's Tester.test_batch and
// KITTIInferenceDataset.save_result do to the full-resolution logit map on one host core.
//   reference: footprints/preprocessing/segmentation/inference.py:80-90 (sigmoid, copy to the host, the input image beside the plasma
//              colour map of the prediction), datasets/inference_dataset.py:39-50 (astype(float16) into the .npy file, plt.imsave).
// fp_seg_pack is ONE launch: it reads the logit plane once (channel 0 of the engine's [B][2][H][W] head buffer, addressed by a base pointer
// and a per-sample stride: nothing is sliced into a copy first) and, when the picture is wanted, the network input once.
//   p        = 1 / (1 + expf(-x)): the accurate exponential and a correctly rounded division (this file is built without fast-math and with
//              -ffp-contract=off; no __expf, no __fdividef)
//   half     = __float2half_rn(p), float16 subnormals included
//   picture  = left half (uint8)((double)image * 255.0) -- matplotlib's float image path promotes to float64 and truncates; values outside
//              [0, 1], where matplotlib raises, are clamped -- right half lut[min((int)(p * 256.0f), 255)]: matplotlib scales a float32
//              array in float32, truncates and maps p == 1 to the last entry.  The 256 x 3 byte table is the caller's (ops.vis_colour_table).
// The kernel is bandwidth-bound (4 B read and 2 B written per pixel; 12 B and 6 B more with the picture).  A thread owns four consecutive
// pixels of one row.  Where W is a multiple of 4 every such quad is whole, and each operand whose base pointer (and, for the logits, sample
// stride) keeps the quads aligned moves as one wide access: 16-byte loads of the logits and of each image plane, a 16-byte store of the
// float32 sigmoid, an 8-byte store of the halves, and the 12 bytes a quad takes in each half of the picture as three dwords.  Every other
// operand -- and everything when W is not a multiple of 4, where every second row starts off the grid -- takes the scalar path element by
// element; the choice is per operand and uniform over the launch.
#include <hip/hip_fp16.h>

#include "fp_common.h"
#include "infer_out.h"      // sigmoid_exact; fp_pack12 / fp_store12: 4 pixels -> the 12 bytes of an [..][3] row

namespace {

enum : unsigned { SP_VEC_LOGIT = 1, SP_VEC_HALF = 2, SP_VEC_F32 = 4, SP_VEC_IMAGE = 8, SP_VEC_PICTURE = 16 };

struct SegPackArgs {
  const float* logits;
  int64_t logit_stride;     // elements between two samples' planes
  const float* image;       // [B][3][H][W] or null
  __half* prob_half;        // [B][H][W]
  float* prob_f32;          // [B][H][W] or null
  unsigned char* picture;   // [B][H][2W][3] or null
  const unsigned char* lut; // [256][3]
  int32_t H, W, quads;      // quads = ceil(W / 4)
  unsigned vec;             // SP_VEC_*
};

__device__ __forceinline__ unsigned int image_byte(float v) {
  const float c = fminf(fmaxf(v, 0.0f), 1.0f);      // a NaN gives 0
  return (unsigned int)(int)((double)c * 255.0);
}

// grid = (ceil(H * quads / 256), B)
__global__ void __launch_bounds__(256) seg_pack_kernel(const SegPackArgs a) {
  __shared__ unsigned int colours[256];
  const bool draw = a.picture != nullptr;
  if (draw) {
    const int i = threadIdx.x;
    colours[i] = (unsigned int)a.lut[3 * i] | ((unsigned int)a.lut[3 * i + 1] << 8) | ((unsigned int)a.lut[3 * i + 2] << 16);
    __syncthreads();
  }
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= (int64_t)a.H * a.quads) return;
  const int b = blockIdx.y;
  const int y = (int)(q / a.quads), x0 = 4 * (int)(q - (int64_t)y * a.quads);
  const int n = min(4, a.W - x0);             // always 4 on a vector path: those need W % 4 == 0
  const int64_t hw = (int64_t)a.H * a.W;
  const int64_t at = (int64_t)y * a.W + x0;   // inside a plane

  float x[4] = {0.f, 0.f, 0.f, 0.f};
  const float* lp = a.logits + (int64_t)b * a.logit_stride + at;
  if (a.vec & SP_VEC_LOGIT) {
    const float4 v = *reinterpret_cast<const float4*>(lp);
    x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
  } else {
    for (int j = 0; j < n; ++j) x[j] = lp[j];
  }
  float p[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) p[j] = sigmoid_exact(x[j]);

  __half* hp = a.prob_half + (int64_t)b * hw + at;
  if (a.vec & SP_VEC_HALF) {
    uint2 h;
    h.x = (unsigned int)__half_as_ushort(__float2half_rn(p[0])) | ((unsigned int)__half_as_ushort(__float2half_rn(p[1])) << 16);
    h.y = (unsigned int)__half_as_ushort(__float2half_rn(p[2])) | ((unsigned int)__half_as_ushort(__float2half_rn(p[3])) << 16);
    *reinterpret_cast<uint2*>(hp) = h;
  } else {
    for (int j = 0; j < n; ++j) hp[j] = __float2half_rn(p[j]);
  }
  if (a.prob_f32) {
    float* fp = a.prob_f32 + (int64_t)b * hw + at;
    if (a.vec & SP_VEC_F32) *reinterpret_cast<float4*>(fp) = make_float4(p[0], p[1], p[2], p[3]);
    else
      for (int j = 0; j < n; ++j) fp[j] = p[j];
  }
  if (!draw) return;

  unsigned int left[4] = {0u, 0u, 0u, 0u}, right[4];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float* ip = a.image + ((int64_t)b * 3 + c) * hw + at;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (a.vec & SP_VEC_IMAGE) {
      const float4 u = *reinterpret_cast<const float4*>(ip);
      v[0] = u.x; v[1] = u.y; v[2] = u.z; v[3] = u.w;
    } else {
      for (int j = 0; j < n; ++j) v[j] = ip[j];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) left[j] |= image_byte(v[j]) << (8 * c);
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int idx = (int)(p[j] * 256.0f);
    right[j] = colours[min(max(idx, 0), 255)];      // p is in [0, 1] (NaN logits convert to some index): never a read outside the table
  }
  unsigned char* row = a.picture + ((int64_t)b * a.H + y) * ((int64_t)a.W * 6);
  fp_store12(row + (int64_t)x0 * 3, left, n, (a.vec & SP_VEC_PICTURE) != 0);
  fp_store12(row + ((int64_t)a.W + x0) * 3, right, n, (a.vec & SP_VEC_PICTURE) != 0);
}

}  // namespace

extern "C" int fp_seg_pack(const float* logits, int64_t logit_batch_stride, const float* image, void* prob_half, float* prob_f32, uint8_t* picture,
                           const uint8_t* lut, int32_t B, int32_t H, int32_t W, fp_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  FP_REQUIRE(logits && prob_half && B > 0 && H > 0 && W > 0, "fp_seg_pack: bad arguments");
  FP_REQUIRE(B <= 65535 && H <= 65535 && (int64_t)H * W * 6 < ((int64_t)1 << 31), "fp_seg_pack: too large");
  FP_REQUIRE(logit_batch_stride >= (int64_t)H * W && logit_batch_stride < ((int64_t)1 << 40), "fp_seg_pack: the sample stride is below H * W (or absurd)");
  FP_REQUIRE(!picture || (image && lut), "fp_seg_pack: the picture needs the image and the colour table");
  FP_REQUIRE(((uintptr_t)logits & 3) == 0 && ((uintptr_t)prob_half & 1) == 0 && ((uintptr_t)prob_f32 & 3) == 0 && ((uintptr_t)image & 3) == 0,
             "fp_seg_pack: a pointer is not aligned to its element type");
  SegPackArgs a;
  a.logits = logits; a.logit_stride = logit_batch_stride; a.image = picture ? image : nullptr; a.prob_half = (__half*)prob_half;
  a.prob_f32 = prob_f32; a.picture = picture; a.lut = lut; a.H = H; a.W = W; a.quads = (int32_t)fp_ceil_div(W, 4);
  a.vec = 0;
  if (W % 4 == 0) {           // then H * W is a multiple of 4 too: a quad's alignment is that of the base pointer (and of the stride)
    if (((uintptr_t)logits & 15) == 0 && logit_batch_stride % 4 == 0) a.vec |= SP_VEC_LOGIT;
    if (((uintptr_t)prob_half & 7) == 0) a.vec |= SP_VEC_HALF;
    if (prob_f32 && ((uintptr_t)prob_f32 & 15) == 0) a.vec |= SP_VEC_F32;
    if (picture && ((uintptr_t)image & 15) == 0) a.vec |= SP_VEC_IMAGE;
    if (picture && ((uintptr_t)picture & 3) == 0) a.vec |= SP_VEC_PICTURE;
  }
  fp_launch(seg_pack_kernel, dim3((unsigned)fp_ceil_div((int64_t)H * a.quads, 256), B), dim3(256), 0, stream, a);
  return fp_check_launch("fp_seg_pack");
}
