// Output stage of the main network's test-set inference: the counterpart of fp_seg_pack for the four-channel
// network.
//   reference: footprints/evaluation/inference.py:105-119 (sigmoid on the two mask channels, copy to the host, the input image beside the
//              two-colour hidden-ground mask), datasets/inference_dataset.py:35-43 (astype(float16) into the .npy file).
// fp_infer_pack is ONE launch that reads the logits once and writes what fp_pack_pred_fp16 and fp_vis_side_by_side write in two:
//   out_half = fp_pred_half(pred, channel)                 -- bit-equal to fp_pack_pred_fp16
//   picture  = left half fp_sbs_image_byte(image), right half fp_sbs_colour(pred[:, 1])       -- byte-equal to fp_vis_side_by_side
// through the same device functions (infer_out.h): the arithmetic is stated once.
// The kernel is bandwidth-bound (16 B read and 8 B written per pixel; 12 B and 6 B more with the picture).  A thread owns four
// consecutive pixels of one row of one channel plane.  Where W is a multiple of 4 every such quad is whole, and each operand whose base
// pointer keeps the quads aligned moves as one wide access: 16-byte loads of the logit and image planes, 8-byte stores of the halves, and
// the 12 bytes a quad takes in each half of the picture as three dwords.  Every other operand -- and everything when W is not a multiple
// of 4 -- takes the scalar path element by element; the choice is per operand and uniform over the launch.
// A thread owns the quad of ONE channel plane (the grid's y is the channel: uniform over a workgroup), and the picture is shared out:
// the workgroups of channel 1 paint the right half from the logits they hold anyway, those of channel 0 convert the image.
// The scalar paths are unrolled and predicated (`if (j < n)`), not loops to a run-time bound: such a loop indexes the thread's quad
// dynamically, the compiler then keeps the quad in LDS, and together with a 64-bit division for the row that form of this kernel took
// 31 - 34 us at 12 x 192 x 640 where this one takes 9.4 us (14.3 us with the picture; profiles/infer_decode_notes.md).  The index math
// is 32-bit: H * quads < 2^31 / 6 by the host's size check.
#include <hip/hip_fp16.h>

#include "fp_common.h"
#include "infer_out.h"

namespace {

enum : unsigned { IP_VEC_PRED = 1, IP_VEC_HALF = 2, IP_VEC_IMAGE = 4, IP_VEC_PICTURE = 8 };

struct InferPackArgs {
  const float* pred;        // [B][4][H][W]
  const float* image;       // [B][3][H][W] or null
  __half* out_half;         // [B][4][H][W]
  unsigned char* picture;   // [B][H][2W][3] or null
  unsigned int colour0, colour1;
  int32_t H, W, quads;      // quads = ceil(W / 4)
  unsigned vec;             // IP_VEC_*
};

__device__ __forceinline__ void load4(const float* p, float v[4], int n, bool vec) {
  if (vec) {
    const float4 u = *reinterpret_cast<const float4*>(p);
    v[0] = u.x; v[1] = u.y; v[2] = u.z; v[3] = u.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < n) v[j] = p[j];
  }
}

// grid = (ceil(H * quads / 256), 4, B): a workgroup works on one channel plane of one sample, so the channel is uniform over it
__global__ void __launch_bounds__(256) infer_pack_kernel(const InferPackArgs a) {
  const unsigned int q = blockIdx.x * 256u + threadIdx.x;           // H * quads <= H * W < 2^31 / 6 (checked by the host): 32-bit index math
  if (q >= (unsigned int)a.H * (unsigned int)a.quads) return;
  const int c = blockIdx.y, b = blockIdx.z;
  const int y = (int)(q / (unsigned int)a.quads), x0 = 4 * (int)(q - (unsigned int)y * (unsigned int)a.quads);
  const int n = min(4, a.W - x0);             // always 4 on a vector path: those need W % 4 == 0
  const int64_t hw = (int64_t)a.H * a.W;
  const int64_t at = (int64_t)y * a.W + x0;   // inside a plane

  float x[4] = {0.f, 0.f, 0.f, 0.f};
  load4(a.pred + ((int64_t)b * 4 + c) * hw + at, x, n, (a.vec & IP_VEC_PRED) != 0);
  __half h[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) h[j] = fp_pred_half(x[j], c);
  __half* hp = a.out_half + ((int64_t)b * 4 + c) * hw + at;
  if (a.vec & IP_VEC_HALF) {
    uint2 w;
    w.x = (unsigned int)__half_as_ushort(h[0]) | ((unsigned int)__half_as_ushort(h[1]) << 16);
    w.y = (unsigned int)__half_as_ushort(h[2]) | ((unsigned int)__half_as_ushort(h[3]) << 16);
    *reinterpret_cast<uint2*>(hp) = w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < n) hp[j] = h[j];
  }
  if (!a.picture || c > 1) return;

  // the picture is shared out between two of the four planes' workgroups: channel 1's, which hold the hidden-ground logits, paint the
  // right half; channel 0's convert the image for the left half
  unsigned int px[4] = {0u, 0u, 0u, 0u};
  unsigned char* row = a.picture + ((int64_t)b * a.H + y) * ((int64_t)a.W * 6);
  if (c == 1) {
#pragma unroll
    for (int j = 0; j < 4; ++j) px[j] = fp_sbs_colour(x[j], a.colour0, a.colour1) & 0xffffffu;
    fp_store12(row + ((int64_t)a.W + x0) * 3, px, n, (a.vec & IP_VEC_PICTURE) != 0);
    return;
  }
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    load4(a.image + ((int64_t)b * 3 + ch) * hw + at, v, n, (a.vec & IP_VEC_IMAGE) != 0);
#pragma unroll
    for (int j = 0; j < 4; ++j) px[j] |= fp_sbs_image_byte(v[j]) << (8 * ch);
  }
  fp_store12(row + (int64_t)x0 * 3, px, n, (a.vec & IP_VEC_PICTURE) != 0);
}

}  // namespace

extern "C" int fp_infer_pack(const float* pred, const float* image, void* out_half, uint8_t* picture, uint32_t colour0, uint32_t colour1,
                             int32_t B, int32_t H, int32_t W, fp_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  FP_REQUIRE(pred && out_half && B > 0 && H > 0 && W > 0, "fp_infer_pack: bad arguments");
  FP_REQUIRE(B <= 65535 && H <= 65535 && (int64_t)H * W * 6 < ((int64_t)1 << 31), "fp_infer_pack: too large");
  FP_REQUIRE(!picture || image, "fp_infer_pack: the picture needs the image");
  FP_REQUIRE(((uintptr_t)pred & 3) == 0 && ((uintptr_t)out_half & 1) == 0 && ((uintptr_t)image & 3) == 0,
             "fp_infer_pack: a pointer is not aligned to its element type");
  InferPackArgs a;
  a.pred = pred; a.image = picture ? image : nullptr; a.out_half = (__half*)out_half; a.picture = picture;
  a.colour0 = colour0; a.colour1 = colour1; a.H = H; a.W = W; a.quads = (int32_t)fp_ceil_div(W, 4);
  a.vec = 0;
  if (W % 4 == 0) {           // then H * W is a multiple of 4 too: a quad's alignment is that of the base pointer
    if (((uintptr_t)pred & 15) == 0) a.vec |= IP_VEC_PRED;
    if (((uintptr_t)out_half & 7) == 0) a.vec |= IP_VEC_HALF;
    if (picture && ((uintptr_t)image & 15) == 0) a.vec |= IP_VEC_IMAGE;
    if (picture && ((uintptr_t)picture & 3) == 0) a.vec |= IP_VEC_PICTURE;
  }
  fp_launch(infer_pack_kernel, dim3((unsigned)fp_ceil_div((int64_t)H * a.quads, 256), 4, B), dim3(256), 0, stream, a);
  return fp_check_launch("fp_infer_pack");
}
