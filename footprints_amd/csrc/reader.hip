// Device-side file-reader work: what the reference's dataset class does to a depth mask before the augmentation of
// data_path.hip sees it.  (The frame's Image.resize(LANCZOS) is resample_u8.hip.)
//   reference: footprints/datasets/footprint_dataset.py:96-105 (filter_depth_mask: skimage.measure.label + a loop over the components).
// filter_depth_mask: connected components (8-connectivity) by label equivalence -- union-find with integer atomicMin on the parent array
// and integer atomicAdd on per-root counters, so the result does not depend on the order in which threads arrive.  Phases are separated
// by kernel boundaries (tile-local labelling in LDS | merge across tile borders | flatten + count | threshold); no workgroup ever waits
// for another.
#include "fp_common.h"

namespace {

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
