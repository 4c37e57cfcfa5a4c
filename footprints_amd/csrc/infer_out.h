// Device functions of the inference output stages, shared so that every kernel that writes a test-set file rounds the same way:
//   pack_pred_fp16_kernel (loss_adam_misc.hip), vis_side_by_side_kernel (visualise.hip), seg_pack_kernel (seg_infer.hip),
//   infer_pack_kernel (infer_pack.hip), and the picture kernels of stretch_map.hip, which share the sigmoid and the 12-byte stores.
// Nothing here holds a multiply next to an add, so the functions give the same bits with and without -ffp-contract=off; the division
// is the correctly rounded one (no fast-math anywhere in this library).
#pragma once
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

// the segmentation network's probability: the accurate exponential and a correctly rounded division (seg_pack_kernel, the log's prediction panel)
__device__ __forceinline__ float sigmoid_exact(float x) {
  const float e = expf(-x);
  const float den = 1.0f + e;
  return 1.0f / den;
}

// one element of the test-set .npy file: sigmoid on the two mask channels (0, 1), depth channels (2, 3) unchanged, rounded to float16
// to nearest even (numpy's astype), subnormals kept
__device__ __forceinline__ __half fp_pred_half(float v, int channel) {
  if (channel < 2) v = 1.f / (1.f + expf(-v));
  return __float2half_rn(v);
}

// one byte of the left half of the test-set picture: uint8(image * 255.0f), clamped
__device__ __forceinline__ unsigned int fp_sbs_image_byte(float v) {
  const float s = v * 255.0f;
  return (unsigned int)min(max((int)s, 0), 255);
}

// the right half: one of two colours (r | g << 8 | b << 16) by the sign of the hidden-ground logit
__device__ __forceinline__ unsigned int fp_sbs_colour(float logit, unsigned int colour0, unsigned int colour1) {
  return logit > 0.0f ? colour1 : colour0;
}

// 4 pixels of 24 bits (r | g << 8 | b << 16) -> the 12 bytes they take in an [..][3] byte row
__device__ __forceinline__ void fp_pack12(const unsigned int c[4], unsigned int d[3]) {
  d[0] = c[0] | (c[1] << 24);
  d[1] = (c[1] >> 8) | (c[2] << 16);
  d[2] = (c[2] >> 16) | (c[3] << 8);
}

// vec: `at` is 4-byte aligned and n == 4 -> three dword stores; otherwise n pixels byte by byte
__device__ __forceinline__ void fp_store12(unsigned char* at, const unsigned int c[4], int n, bool vec) {
  if (vec) {
    unsigned int d[3];
    fp_pack12(c, d);
    unsigned int* o = reinterpret_cast<unsigned int*>(at);
    o[0] = d[0];
    o[1] = d[1];
    o[2] = d[2];
  } else {
    for (int j = 0; j < n; ++j) {
      at[3 * j + 0] = (unsigned char)(c[j]);
      at[3 * j + 1] = (unsigned char)(c[j] >> 8);
      at[3 * j + 2] = (unsigned char)(c[j] >> 16);
    }
  }
}
