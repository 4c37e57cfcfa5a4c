// Backward of a BatchNorm that normalises with its RUNNING statistics (nn.BatchNorm2d in eval mode inside a network that is being trained:
// fine-tuning with frozen statistics).  The statistics do not depend on the batch, so the layer is an affine map per channel:
//   g = dy * (relu_out > 0),  dz = g * (gamma * invstd),  dbeta = sum g,  dgamma = sum g * (z - mean) * invstd
// -- no second pass over the activation as in fp_bn_bwd (bn_pool.hip), whose dz needs the two sums first.  NHWC [M][C], a channel is a column:
// float4 (4 channels) per thread, R = 256 / (C / 4) rows per workgroup, rows strided across a capped grid (the grid rule of the reductions in
// bn_pool.hip, read off fp_bn_workspace), partial sums per workgroup combined in a fixed order by a second small launch: deterministic, no atomics.
#include "fp_common.h"

namespace {

// SUMS: also partial[block][c][2] = (sum g, sum g * xhat) over the block's rows; without them z, mean and the partials are never touched
template <bool SUMS>
__global__ void __launch_bounds__(256) bn_frozen_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ ro,
                                                            const float* __restrict__ z, const float* __restrict__ mean,
                                                            const float* __restrict__ invstd, const float* __restrict__ gamma,
                                                            float* __restrict__ dz, float* __restrict__ gout, int M, int C,
                                                            float* __restrict__ part, unsigned* amax_out) {
  __shared__ float sm[SUMS ? 2 * 256 * 4 : 1];
  const int C4 = C >> 2, R = 256 / C4;
  const int cq = threadIdx.x % C4, rr = threadIdx.x / C4;
  const float4 is = reinterpret_cast<const float4*>(invstd)[cq];
  const float4 ga = reinterpret_cast<const float4*>(gamma)[cq];
  const float4 a = make_float4(ga.x * is.x, ga.y * is.y, ga.z * is.z, ga.w * is.w);
  float4 mu = make_float4(0.f, 0.f, 0.f, 0.f);
  if (SUMS) mu = reinterpret_cast<const float4*>(mean)[cq];
  float s1[4] = {0, 0, 0, 0}, s2[4] = {0, 0, 0, 0};
  float ymax = 0.f;
  for (int m = blockIdx.x * R + rr; m < M; m += gridDim.x * R) {
    const size_t o = (size_t)m * C + cq * 4;
    float4 g = *reinterpret_cast<const float4*>(dy + o);
    if (ro) {
      const float4 r = *reinterpret_cast<const float4*>(ro + o);
      g.x = r.x > 0.f ? g.x : 0.f; g.y = r.y > 0.f ? g.y : 0.f; g.z = r.z > 0.f ? g.z : 0.f; g.w = r.w > 0.f ? g.w : 0.f;
    }
    if (gout) *reinterpret_cast<float4*>(gout + o) = g;
    const float4 d = make_float4(g.x * a.x, g.y * a.y, g.z * a.z, g.w * a.w);
    *reinterpret_cast<float4*>(dz + o) = d;
    ymax = fp_amax4(ymax, d);
    if (SUMS) {
      const float4 v = *reinterpret_cast<const float4*>(z + o);
      s1[0] += g.x; s2[0] += g.x * ((v.x - mu.x) * is.x);
      s1[1] += g.y; s2[1] += g.y * ((v.y - mu.y) * is.y);
      s1[2] += g.z; s2[2] += g.z * ((v.z - mu.z) * is.z);
      s1[3] += g.w; s2[3] += g.w * ((v.w - mu.w) * is.w);
    }
  }
  if (SUMS) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      sm[(0 * 256 + threadIdx.x) * 4 + j] = s1[j];
      sm[(1 * 256 + threadIdx.x) * 4 + j] = s2[j];
    }
    __syncthreads();
    if (rr == 0) {
      for (int r = 1; r < R; ++r) {
        const int tt = r * C4 + cq;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          s1[j] += sm[(0 * 256 + tt) * 4 + j];
          s2[j] += sm[(1 * 256 + tt) * 4 + j];
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float* p = part + ((size_t)blockIdx.x * C + cq * 4 + j) * 2;
        p[0] = s1[j]; p[1] = s2[j];
      }
    }
  }
  if (amax_out) fp_amax_publish_block(amax_out, ymax);      // (every thread of the block arrives here: no early return above)
}

// dbeta (+)= sum over the blocks of part[b][c][0], dgamma (+)= ... of part[b][c][1].  One wave per channel: lane l adds partials l, l + 64, ...
// in order, then a fixed shuffle tree -- in double, like bn_bwd_final_kernel
__global__ void __launch_bounds__(256) bn_frozen_final_kernel(const float* __restrict__ part, int nblk, int C, float* dgamma, float* dbeta,
                                                              int accumulate) {
  const int lane = threadIdx.x & 63;
  const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= C) return;
  double d1 = 0.0, d2 = 0.0;
  for (int b = lane; b < nblk; b += 64) {
    const float* p = part + ((size_t)b * C + c) * 2;
    d1 += (double)p[0]; d2 += (double)p[1];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    d1 += __shfl_down(d1, o, 64);
    d2 += __shfl_down(d2, o, 64);
  }
  if (lane != 0) return;
  const float s1 = (float)d1, s2 = (float)d2;
  if (dgamma) dgamma[c] = accumulate ? dgamma[c] + s2 : s2;
  if (dbeta) dbeta[c] = accumulate ? dbeta[c] + s1 : s1;
}

// dz = g * (gamma * invstd) on an already masked g (the producing data gradient's epilogue applied the ReLU mask)
__global__ void __launch_bounds__(256) bn_frozen_scale_kernel(const float* __restrict__ g, const float* __restrict__ invstd,
                                                              const float* __restrict__ gamma, float* __restrict__ dz, size_t total4,
                                                              int C4, unsigned* amax_out) {
  float ymax = 0.f;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total4; e += (size_t)gridDim.x * 256) {
    const int cq = (int)(e % C4);
    const float4 v = reinterpret_cast<const float4*>(g)[e];
    const float4 is = reinterpret_cast<const float4*>(invstd)[cq];
    const float4 ga = reinterpret_cast<const float4*>(gamma)[cq];
    const float4 o = make_float4(v.x * (ga.x * is.x), v.y * (ga.y * is.y), v.z * (ga.z * is.z), v.w * (ga.w * is.w));
    reinterpret_cast<float4*>(dz)[e] = o;
    ymax = fp_amax4(ymax, o);
  }
  if (amax_out) fp_amax_publish_block(amax_out, ymax);
}

// eval-mode coefficients that also leave the statistics where the backward reads them: mean = running_mean, invstd = 1 / sqrt(running_var +
// eps), and scale = gamma * invstd from THAT float32 invstd (dz = g * gamma * invstd is then the exact derivative of the forward's scale)
__global__ void __launch_bounds__(256) bn_frozen_coeffs_kernel(const float* gamma, const float* beta, const float* rm, const float* rv,
                                                               float eps, int C, float* scale, float* shift, float* mean, float* invstd) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  const float is = 1.f / sqrtf(rv[c] + eps);
  const float sc = gamma[c] * is;
  mean[c] = rm[c];
  invstd[c] = is;
  scale[c] = sc;
  shift[c] = beta[c] - rm[c] * sc;
}

bool frozen_c_ok(int C) { return C >= 4 && C % 4 == 0 && 256 % (C / 4) == 0 && C / 4 <= 256; }

// workgroups of the row-strided launch: the grid of the BatchNorm reductions (bn_pool.hip bn_blocks), read off the workspace rule they publish
int frozen_blocks(int64_t M, int C) {
  return (int)((fp_bn_workspace(M, C) - (int64_t)C * 2 * (int64_t)sizeof(float)) / ((int64_t)C * 3 * (int64_t)sizeof(float)));
}

}  // namespace

extern "C" int fp_bn_eval_coeffs_saved(const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                                       float eps, int32_t C, float* scale, float* shift, float* save_mean, float* save_invstd,
                                       fp_stream_t stream) {
  FP_REQUIRE(gamma && beta && running_mean && running_var && scale && shift && save_mean && save_invstd,
             "fp_bn_eval_coeffs_saved: null pointer");
  FP_REQUIRE(C > 0, "fp_bn_eval_coeffs_saved: empty problem");
  fp_launch(bn_frozen_coeffs_kernel, dim3((C + 255) / 256), dim3(256), 0, (hipStream_t)stream, gamma, beta, running_mean, running_var, eps,
            C, scale, shift, save_mean, save_invstd);
  return fp_check_launch("fp_bn_eval_coeffs_saved");
}

extern "C" int fp_bn_bwd_frozen(const float* dy, const float* relu_out, const float* z, const float* mean, const float* invstd,
                                const float* gamma, float* dz, float* dgamma, float* dbeta, float* g_out, int accumulate, int64_t M,
                                int32_t C, void* workspace, int64_t workspace_bytes, uint32_t* amax_out, fp_stream_t stream) {
  const bool sums = dgamma || dbeta;
  FP_REQUIRE(dy && invstd && gamma && dz, "fp_bn_bwd_frozen: null pointer");
  FP_REQUIRE(frozen_c_ok(C) && M > 0 && M < ((int64_t)1 << 31), "fp_bn_bwd_frozen: unsupported C=%d", C);
  const int nblk = frozen_blocks(M, C);
  FP_REQUIRE(nblk >= 1, "fp_bn_bwd_frozen: empty grid");
  if (!sums) {
    fp_launch(bn_frozen_bwd_kernel<false>, dim3(nblk), dim3(256), 0, (hipStream_t)stream, dy, relu_out, (const float*)nullptr,
              (const float*)nullptr, invstd, gamma, dz, g_out, (int)M, C, (float*)nullptr, amax_out);
    return fp_check_launch("fp_bn_bwd_frozen");
  }
  FP_REQUIRE(z && mean && workspace, "fp_bn_bwd_frozen: the sums need z, mean and a workspace");
  FP_REQUIRE(workspace_bytes >= fp_bn_workspace(M, C), "fp_bn_bwd_frozen: workspace too small");
  float* part = (float*)workspace;            // nblk * C * 2 floats of the nblk * C * 3 + 2 C the query asks for
  fp_launch(bn_frozen_bwd_kernel<true>, dim3(nblk), dim3(256), 0, (hipStream_t)stream, dy, relu_out, z, mean, invstd, gamma, dz, g_out,
            (int)M, C, part, amax_out);
  fp_launch(bn_frozen_final_kernel, dim3((C + 3) / 4), dim3(256), 0, (hipStream_t)stream, (const float*)part, nblk, C, dgamma, dbeta,
            accumulate);
  return fp_check_launch("fp_bn_bwd_frozen");
}

extern "C" int fp_bn_bwd_frozen_partials(const float* g, const float* invstd, const float* gamma, float* dz, float* dgamma, float* dbeta,
                                         int accumulate, int64_t M, int32_t C, const float* part, int32_t nblk, uint32_t* amax_out,
                                         fp_stream_t stream) {
  FP_REQUIRE(g && invstd && gamma && dz, "fp_bn_bwd_frozen_partials: null pointer");
  FP_REQUIRE(C >= 4 && C % 4 == 0 && M > 0 && M < ((int64_t)1 << 31), "fp_bn_bwd_frozen_partials: unsupported C=%d", C);
  if (dgamma || dbeta) {
    FP_REQUIRE(part && nblk > 0, "fp_bn_bwd_frozen_partials: the sums need the partials (nblk=%d)", nblk);
    fp_launch(bn_frozen_final_kernel, dim3((C + 3) / 4), dim3(256), 0, (hipStream_t)stream, part, (int)nblk, C, dgamma, dbeta, accumulate);
  }
  const size_t total4 = (size_t)M * (C / 4);
  size_t grid = (total4 + 255) / 256;
  if (grid > 8192) grid = 8192;
  fp_launch(bn_frozen_scale_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, g, invstd, gamma, dz, total4, C / 4, amax_out);
  return fp_check_launch("fp_bn_bwd_frozen_partials");
}
