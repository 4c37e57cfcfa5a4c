/*
 * footprints_hip.h -- flat C ABI of libfootprints_hip.so (gfx950 / MI355X).
 *
 * The reference (nianticlabs/footprints) has no FFI: its hot path is implicit
 * ATen/cuDNN ops behind nn.Modules.  Each entry point below replaces the ATen op
 * family named in its comment (reference file:line = where the op is issued).
 * Conventions:
 *   - raw device pointers (tensor.data_ptr()), explicit int32 dims, fp32 only;
 *   - activations NHWC [N][H][W][C]; network input image and the four network
 *     outputs NCHW (the reference's layout at the nn.Module boundary);
 *   - the caller (PyTorch) owns every buffer, workspace included; the library
 *     never allocates or frees device memory and keeps no pointer after return;
 *   - every function returns 0 on success, else a negative FP_E* code or a
 *     positive hipError_t; fp_last_error_string() describes the last failure of
 *     the calling thread; nothing throws or aborts across the ABI;
 *   - kernels are asynchronous on the hipStream_t passed as the last argument
 *     (torch.cuda.current_stream().cuda_stream), so calls are graph-capturable.
 */
#ifndef FOOTPRINTS_HIP_H
#define FOOTPRINTS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* fp_stream_t; /* hipStream_t */

#define FP_OK 0
#define FP_EINVAL (-1)     /* bad descriptor / unsupported shape */
#define FP_EWORKSPACE (-2) /* workspace too small */

/* ---- implicit-GEMM convolution family ---------------------------------- */

/* how the GEMM A-operand (one row per output pixel, one K-slice per tap) is gathered */
enum fp_gather {
  FP_GATHER_FWD_ZERO = 0,        /* conv fwd, zero padding, any stride  (torchvision resnet convs; network.py:38-44) */
  FP_GATHER_FWD_REFLECT = 1,     /* conv fwd, ReflectionPad2d(1), stride 1 (network.py:115,126,132) */
  FP_GATHER_FWD_REFLECT_UP2 = 2, /* same, input = cat[nearest_x2(src0), src1] never materialised (network.py:154-155,98) */
  FP_GATHER_DGRAD_ZERO = 3,      /* data-gradient of FWD_ZERO (gather form, stride parity skipped) */
  FP_GATHER_DGRAD_REFLECT = 4,   /* data-gradient of FWD_REFLECT: halo gradients folded back onto rows/cols 1 and H-2 */
  FP_GATHER_STEM = 5             /* 7x7/2 pad 3 on the NCHW image with (x-0.45)/0.225 folded into the load (network.py:50) */
};

enum fp_act { FP_ACT_NONE = 0, FP_ACT_ELU = 1, FP_ACT_RELU = 2 };

/* epilogue: v = acc + bias[n] + addend[m][n]*(addend_mask>0) ; v *= actgrad(actsrc[m][n]) ; v = act(v) ; y = v (+ y) */
#define FP_EPI_BIAS 1u
#define FP_EPI_ADDEND 2u
#define FP_EPI_ADDEND_MASK 4u  /* addend is multiplied by (addend_mask[m][n] > 0) */
#define FP_EPI_ACTGRAD_ELU 8u  /* v *= (s > 0 ? 1 : s + 1), s = actsrc = saved ELU OUTPUT (nn.ELU(inplace=True), network.py:118) */
#define FP_EPI_ACTGRAD_RELU 16u /* v *= (actsrc > 0) */
#define FP_EPI_ACCUM 32u       /* y += v (second decoder / second consumer accumulating into the same gradient) */
#define FP_EPI_BF16X2 64u      /* fp_conv3x3_bf3 forward only, opt-in INFERENCE mode: operands rounded to two bf16 terms (16 significant
                                  bits), three MFMA products instead of six; not exact -- never set by the training path */

typedef struct fp_conv_desc {
  int32_t N;          /* batch */
  int32_t OH, OW;     /* spatial domain of the GEMM rows (fwd: conv output; dgrad: conv input) */
  int32_t IH, IW;     /* spatial dims of the gathered tensor's virtual domain (fwd: conv input, hi-res for UP2; dgrad: dZ) */
  int32_t C0, C1;     /* K channels per tap taken from src0 / src1 (C1 = 0 unless UP2 concat); multiples of 4 */
  int32_t Nout;       /* GEMM N (fwd: Cout; dgrad: Cin) */
  int32_t KH, KW, stride, pad;
  int32_t gather;     /* enum fp_gather */
  int32_t act;        /* enum fp_act */
  uint32_t epi;       /* FP_EPI_* */
} fp_conv_desc;

/* Optional side outputs of ONE launch (round 6; replaces the per-thread fp_amax_out_next / fp_bn_stats_out_next / fp_bn_bwd_out_next sinks of
 * rounds 3-5: the library holds no state between calls besides the calling thread's last error string).  Passed as `const fp_aux* aux` right
 * before the stream argument of the entry points that can produce them; NULL = none; fields that an entry point cannot serve are ignored.
 * The struct is read during the call only.
 *   amax_out   amax slot (see "fp16-pair operands" below; zeroed by the caller) that also receives max |output| of the launch:
 *              fp_bn_apply, fp_bn_bwd / fp_bn_bwd_partials (their dz), fp_maxpool_fwd, fp_up2_fold_bwd, fp_head_dgrad,
 *              fp_conv_up2_phase_fwd_bf3, fp_conv_stem_hp.
 *   bn_part    BatchNorm partials out of a convolution's epilogue -- fp_conv3x3_bf3 / fp_conv3x3_hp, fp_conv_igemm_bf3 / _hp (split grids: from
 *              their reduce launch), fp_conv_stem_hp, fp_conv_igemm (stem gather):
 *                bnb_z == NULL: a plain forward launch (no bias / addend / activation) in front of a train-mode BatchNorm writes Welford partials
 *                  bn_part[pixel tile][Nout] = (count, mean, M2) of what it stores -> fp_bn_train_stats_partials;
 *                bnb_z != NULL: a data gradient whose stored output IS g = dy * (relu_out > 0) of a train-mode BatchNorm (mask applied by its own
 *                  FP_EPI_ACTGRAD_RELU epilogue, no FP_EPI_ACCUM) writes bn_part[pixel tile][Nout] = (sum g, sum g * xhat), xhat = (bnb_z - bnb_mean)
 *                  * bnb_invstd of THAT BatchNorm -> fp_bn_bwd_partials.
 *              *bn_nblk_out (host memory) = number of pixel tiles written, set before the call returns; 0 = nothing emitted (launch form cannot
 *              emit, bn_capacity_floats too small): the caller then runs the BatchNorm's own reduction pass. */
typedef struct fp_aux {
  uint32_t* amax_out;
  float* bn_part;
  int64_t bn_capacity_floats;
  int32_t* bn_nblk_out;
  const float* bnb_z;
  const float* bnb_mean;
  const float* bnb_invstd;
} fp_aux;

/* Y[m][n] = epilogue( sum_{tap,k} A[m][tap,k] * Wp[tap][k][n] ).
 * Wp is the packed weight produced by fp_pack_conv_weight (fwd) / fp_pack_conv_weight_dgrad.
 * Replaces aten::convolution (+reflection_pad2d, upsample_nearest2d, cat, elu_) and the
 * data-gradient half of aten::convolution_backward (+elu_backward, relu mask, residual add).
 * Small problems (few output tiles) are split along K across workgroups when `workspace` (>=
 * fp_conv_igemm_workspace(d) bytes; may be NULL = never split) is given; partials are summed in a fixed order. */
int64_t fp_conv_igemm_workspace(const fp_conv_desc* d);
int fp_conv_igemm(const fp_conv_desc* d, const float* src0, const float* src1, const float* wpacked,
                  const float* bias, const float* addend, const float* addend_mask, const float* actsrc,
                  float* y, void* workspace, int64_t workspace_bytes, const fp_aux* aux, fp_stream_t stream);

/* Weight gradient: dW (OIHW [Nout][C0+C1][KH][KW]) = sum_m A[m][tap,k] * dZ[m][n]; A gathered as the
 * matching forward conv (desc.gather is a FWD_* / STEM mode, desc.OH/OW = conv output dims).
 * Deterministic two-stage reduction through `workspace` (>= fp_conv_wgrad_workspace(d) bytes).
 * accumulate != 0 => dW += result.  Replaces the weight half of aten::convolution_backward. */
int64_t fp_conv_wgrad_workspace(const fp_conv_desc* d);
/* fp_conv_wgrad_slice: same, but the C0+C1 input channels of `d` are the slice [k_begin, k_begin+C0+C1) of a wider
 * gradient dw_oihw[Nout][kc_total][KH][KW] (the skip half of a concat conv). */
int fp_conv_wgrad_slice(const fp_conv_desc* d, const float* src0, const float* src1, const float* dz, float* dw_oihw,
                        int32_t kc_total, int32_t k_begin, int accumulate, void* workspace, int64_t workspace_bytes,
                        fp_stream_t stream);
int fp_conv_wgrad(const fp_conv_desc* d, const float* src0, const float* src1, const float* dz,
                  float* dw_oihw, int accumulate, void* workspace, int64_t workspace_bytes, fp_stream_t stream);

/* One repacking job of fp_pack_weights_batched: every convolution's packed copies are refreshed by ONE launch after the
 * optimizer step (the table lives in device memory and is built once: parameter and packed buffers never move). */
enum { FP_PACK_FWD = 0, FP_PACK_DGRAD = 1, FP_PACK_STEM = 2, FP_PACK_UP2_FWD = 3, FP_PACK_UP2_DGRAD = 4,
       FP_PACK_FWD_BF3 = 5, FP_PACK_DGRAD_BF3 = 6, FP_PACK_UP2_FWD_BF3 = 7, FP_PACK_UP2_DGRAD_BF3 = 8, /* bf16x3 split planes, see fp_conv3x3_bf3 */
       FP_PACK_FWD_HP = 9, FP_PACK_DGRAD_HP = 10, FP_PACK_UP2_FWD_HP = 11, FP_PACK_UP2_DGRAD_HP = 12, /* scaled fp16 pairs, see fp_conv3x3_hp */
       FP_PACK_STEM_HP = 13 /* the 7x7x3 stem as fp16 pairs, K = 7 rows x 24 (21 taps + 3 zeros): [11 K-steps][2 planes][64][16], see fp_conv_stem_hp */ };
typedef struct fp_pack_job {
  const float* w;  /* [Cout][Cin][KH][KW] */
  float* wp;       /* packed destination */
  int32_t Cout, Cin, KH, KW;
  int32_t kind;             /* FP_PACK_* */
  int32_t c_begin, c_count; /* input-channel slice (whole tensor: 0, Cin) */
  int32_t block_begin, block_count; /* this job's contiguous range of workgroups in the batched launch */
  uint32_t* amax;           /* *_HP kinds: the weight tensor's amax slot (FP_AMAX_ELEMS uint32, shared by all jobs of the tensor) */
} fp_pack_job;
int32_t fp_pack_job_blocks(int32_t kind, int32_t Cout, int32_t KH, int32_t KW, int32_t c_count);
int fp_pack_weights_batched(const fp_pack_job* jobs_dev, const int32_t* blk2job_dev, int32_t nblocks, fp_stream_t stream);
/* the same launch, persistent: at most `max_wgs` workgroups (> 0) walk the nblocks virtual blocks -- a repack on a side stream must not take
 * the wave slots of the chain it runs beside (Engine.refresh_packed; 0 = one workgroup per virtual block) */
int fp_pack_weights_batched_capped(const fp_pack_job* jobs_dev, const int32_t* blk2job_dev, int32_t nblocks, int32_t max_wgs,
                                   fp_stream_t stream);

/* packed-weight sizes (floats) and packers; w_oihw is the torch Conv2d.weight [Cout][Cin][KH][KW] */
int64_t fp_packed_weight_elems(int32_t Cout, int32_t Cin, int32_t KH, int32_t KW, int32_t for_dgrad, int32_t stem);
int fp_pack_conv_weight(const float* w_oihw, float* wp, int32_t Cout, int32_t Cin, int32_t KH, int32_t KW,
                        int32_t stem, fp_stream_t stream);
int fp_pack_conv_weight_dgrad(const float* w_oihw, float* wp, int32_t Cout, int32_t Cin, int32_t KH, int32_t KW,
                              fp_stream_t stream);

/* ---- 3x3 stride-1 convolution with exactly split operands (conv3x3_tile_bf3.hip).
 * Every fp32 operand is split into three bf16 terms whose sum is exact (8+8+8 significant bits); six of the nine bf16 x bf16
 * products (all those >= 2^-16 of the leading one) are accumulated in fp32 by v_mfma_f32_32x32x16_bf16.  The result is
 * closer to the exact dot product than the fp32 MFMA path (the dropped terms are <= 2^-24 relative, below fp32 rounding) and
 * runs at up to 2.7x its MFMA rate.  Same operation, arguments and epilogue flags as fp_conv_igemm for
 * FP_GATHER_{FWD_ZERO, FWD_REFLECT, DGRAD_ZERO, DGRAD_REFLECT} (C1 = 0, src1 = NULL) and FP_GATHER_FWD_REFLECT_UP2 (src = the
 * half-resolution tensor with C0 % 16 == 0 channels, src1 = the skip tensor with C1 channels), for the shapes fp_conv3x3_bf3_supported accepts
 * (3x3 / stride 1 / pad 1; 8x16- or 6x20-pixel tiles with <= 25 % padding; small grids are split along the input
 * channels into raw partials in `workspace`, summed in a fixed order before the epilogue); weights packed by
 * fp_pack_conv_weight_bf3 (fp_packed_weight_elems_bf3 floats of storage) or FP_PACK_{FWD,DGRAD}_BF3 jobs. */
int fp_conv3x3_bf3_supported(const fp_conv_desc* d);
int64_t fp_conv3x3_bf3_workspace(const fp_conv_desc* d);   /* split-K scratch for small grids (0 = none) */
int fp_conv3x3_bf3(const fp_conv_desc* d, const float* src, const float* src1, const void* wpacked_bf3, const float* bias,
                   const float* addend, const float* addend_mask, const float* actsrc, float* y, void* workspace,
                   int64_t workspace_bytes, const fp_aux* aux, fp_stream_t stream);
int64_t fp_packed_weight_elems_bf3(int32_t Cout, int32_t Cin, int32_t KH, int32_t KW, int32_t for_dgrad);
int fp_pack_conv_weight_bf3(const float* w_oihw, void* wp, int32_t Cout, int32_t Cin, int32_t KH, int32_t KW,
                            int32_t for_dgrad, fp_stream_t stream);

/* ---- fp16-pair operands ("hp"): x * 2^k = h + m, h = fp16(x * 2^k), m = fp16(x * 2^k - h) -- 22 significant bits after a per-tensor
 * power-of-two scaling taken from the tensor's largest magnitude; three fp16 products (hh + hm + mh; mm is <= 2^-22 of a product and left out; each exact in the fp32
 * accumulator of v_mfma_f32_32x32x16_f16) instead of the six of the exact split and two operand planes instead of three.
 * An "amax slot" is FP_AMAX_SLOTS = 16 uint32 (FP_AMAX_STRIDE apart) holding float bit patterns of |x| (combined with max): zero it (fp_zero_u32), then
 * either reduce a tensor into it (fp_amax_f32) or let the kernel that produces the tensor publish into it (`amax_out`). */
#define FP_AMAX_SLOTS 16                 /* sub-slots per amax slot */
#ifndef FP_AMAX_STRIDE
#define FP_AMAX_STRIDE 32                /* uint32 elements between consecutive sub-slots: one 128-byte line each */
#endif
#define FP_AMAX_ELEMS (FP_AMAX_SLOTS * FP_AMAX_STRIDE)     /* uint32 elements of storage per slot */
int32_t fp_amax_slot_elems(void);        /* = FP_AMAX_ELEMS of the loaded build */
int fp_zero_u32(uint32_t* p, int64_t n, fp_stream_t stream);
int fp_amax_f32(const float* x, int64_t n, uint32_t* slot, fp_stream_t stream);          /* x 16-byte aligned; slot zeroed by the caller */
int fp_weight_amax(const float* w, int64_t n, uint32_t* amax_slot, fp_stream_t stream);  /* zero + reduce */
int64_t fp_packed_weight_elems_hp(int32_t Cout, int32_t Cin, int32_t KH, int32_t KW, int32_t for_dgrad);   /* floats of storage */
int fp_pack_conv_weight_hp(const float* w_oihw, void* wp, int32_t Cout, int32_t Cin, int32_t KH, int32_t KW, int32_t for_dgrad,
                           uint32_t* amax_slot, int32_t amax_ready, fp_stream_t stream);
int fp_pack_weights_amax(const fp_pack_job* jobs_dev, const int32_t* blk2job_dev, int32_t nblocks, fp_stream_t stream);
/* fp_conv3x3_bf3 with fp16-pair operands: same shapes, gathers and epilogue flags; weights from fp_pack_conv_weight_hp /
 * FP_PACK_{FWD,DGRAD}_HP jobs together with the slot they were scaled by (`amax_w`); `amax_src` (and `amax_src1` for the skip tensor
 * of FP_GATHER_FWD_REFLECT_UP2) = max |x| of the source tensor(s); `amax_out` (optional, zeroed by the caller) receives max |y|. */
int fp_conv3x3_hp(const fp_conv_desc* d, const float* src, const float* src1, const void* wpacked_hp, const float* bias,
                  const float* addend, const float* addend_mask, const float* actsrc, float* y, void* workspace,
                  int64_t workspace_bytes, const uint32_t* amax_src, const uint32_t* amax_src1, const uint32_t* amax_w,
                  uint32_t* amax_out, const fp_aux* aux, fp_stream_t stream);

/* nearest-x2 phase kernels (conv_up2_phase.hip) with fp16-pair operands: weights from FP_PACK_UP2_FWD_HP / FP_PACK_UP2_DGRAD_HP jobs */
int fp_conv_up2_phase_fwd_hp(const float* low, const void* wphase_hp, const float* bias, const float* addend, float* y, int32_t N,
                             int32_t h, int32_t w, int32_t C0, int32_t Nout, int32_t act, const uint32_t* amax_low,
                             const uint32_t* amax_w, uint32_t* amax_out, fp_stream_t stream);
int fp_conv_up2_phase_dgrad_hp(const float* dz, const void* wpacked_hp, float* ext, int32_t N, int32_t h, int32_t w, int32_t Cout,
                               int32_t C0, const uint32_t* amax_dz, const uint32_t* amax_w, fp_stream_t stream);

/* weight gradients with fp16-pair operands: fp_conv_wgrad_bf3 / fp_conv_up2_phase_wgrad_bf3 with the amax slots of their two tensors */
int fp_conv_wgrad_hp(const fp_conv_desc* d, const float* x, const float* dz, float* dw_oihw, float* db, int32_t kc_total,
                     int32_t k_begin, int accumulate, void* workspace, int64_t workspace_bytes, const uint32_t* amax_x,
                     const uint32_t* amax_dz, fp_stream_t stream);
int fp_conv_up2_phase_wgrad_hp(const float* low, const float* dz, float* dw_oihw, float* db, int32_t N, int32_t h, int32_t w,
                               int32_t C0, int32_t Nout, int32_t kc_total, int32_t k_begin, int accumulate, void* workspace,
                               int64_t workspace_bytes, const uint32_t* amax_low, const uint32_t* amax_dz, fp_stream_t stream);

/* Weight gradient with the same exactly split operands (wgrad3x3_bf3.hip): 3x3 / stride 1 / pad 1, FWD_ZERO, FWD_REFLECT or
 * FWD_REFLECT_UP2 gather (then x is the half-resolution tensor [N][OH/2][OW/2][C0]: the upsampled half of a concat conv), C1 = 0, C0 and Nout multiples of 32; fp_conv_wgrad_bf3_workspace returns -1 for anything else (use fp_conv_wgrad).
 * dw_oihw is [Nout][kc_total][3][3]; the C0 input channels of `d` are its slice [k_begin, k_begin + C0).
 * db (optional, [Nout]): the bias gradient = column sums of dz, produced from the dz tiles the kernel stages anyway
 * (replaces a separate fp_colsum pass over dz); (+)= like dw_oihw. */
int64_t fp_conv_wgrad_bf3_workspace(const fp_conv_desc* d);
int fp_conv_wgrad_bf3(const fp_conv_desc* d, const float* x, const float* dz, float* dw_oihw, float* db, int32_t kc_total,
                      int32_t k_begin, int accumulate, void* workspace, int64_t workspace_bytes, fp_stream_t stream);

/* ---- nearest-x2 phase decomposition (reference footprints/network.py:98,126-134,154: upsample -> [cat skip] ->
 * ReflectionPad2d(1) -> Conv2d 3x3).  A 3x3 conv over the x2-upsampled `low` equals four 2x2 convs (one per output
 * parity phase) over `low` itself with row/column-collapsed weights and replicate padding: 2.25x fewer MACs and no
 * upsampled temporary.  fp_pack_up2_weight collapses input channels [c_begin, c_begin+c_count) of w_oihw
 * [Cout][Cin][3][3] into wp[phase 4][tap 4][ceil(c_count/16)][Cout][16]; fp_pack_conv_weight_slice packs the remaining
 * (skip) channels in the ordinary fp_pack_conv_weight layout.  fp_conv_up2_phase_fwd:
 *   y[n][2y+dy][2x+dx][:] = act( sum_taps Wc . low + bias + addend )      (addend may alias y: skip-half partial sums) */
int64_t fp_up2_packed_weight_elems(int32_t Cout, int32_t c_count);
int fp_pack_up2_weight(const float* w_oihw, float* wp, int32_t Cout, int32_t Cin, int32_t c_begin, int32_t c_count,
                       fp_stream_t stream);
int fp_pack_conv_weight_slice(const float* w_oihw, float* wp, int32_t Cout, int32_t Cin, int32_t c_begin,
                              int32_t c_count, fp_stream_t stream);
int fp_conv_up2_phase_fwd(const float* low, const float* wphase, const float* bias, const float* addend, float* y,
                          int32_t N, int32_t h, int32_t w, int32_t C0, int32_t Nout, int32_t act, fp_stream_t stream);
/* bf16x3-split variant (see fp_conv3x3_bf3): same operation, weights from fp_pack_up2_weight_bf3 / FP_PACK_UP2_FWD_BF3
 * (fp_up2_packed_weight_elems(Cout, c_count) * 3 / 2 floats of storage). */
int fp_pack_up2_weight_bf3(const float* w_oihw, void* wp, int32_t Cout, int32_t Cin, int32_t c_begin, int32_t c_count,
                           fp_stream_t stream);
int fp_conv_up2_phase_fwd_bf3(const float* low, const void* wphase_bf3, const float* bias, const float* addend, float* y,
                              int32_t N, int32_t h, int32_t w, int32_t C0, int32_t Nout, int32_t act, const fp_aux* aux,
                              fp_stream_t stream);
/* Backward (the upsample_nearest2d_backward + reflection_pad2d_backward + convolution_backward(data) chain): d(low) is a
 * 4x4 stride-2 convolution over dZ.  Pack with fp_pack_up2_weight_dgrad (fp_up2_packed_weight_elems(c_count, Cout)
 * floats), run fp_conv_igemm{FWD_ZERO, K=4, stride 2, pad 3, IH=2h, OH=h+2} into ext[N][h+2][w+2][c_count], then
 * fp_up2_fold_bwd folds the replicate-padding border back:  dlow = (fold(ext) + addend) * ELU'(ylow_elu)  (both optional).
 * The skip half of a concat conv takes the ordinary DGRAD_REFLECT path with fp_pack_conv_weight_dgrad_slice weights. */
int fp_pack_up2_weight_dgrad(const float* w_oihw, float* wp, int32_t Cout, int32_t Cin, int32_t c_begin, int32_t c_count,
                             fp_stream_t stream);
int fp_pack_conv_weight_dgrad_slice(const float* w_oihw, float* wp, int32_t Cout, int32_t Cin, int32_t c_begin,
                                    int32_t c_count, fp_stream_t stream);
/* bf16x3 variant of the 4x4 stride-2 data-gradient convolution: writes the same ext[N][h+2][w+2][C0] as fp_conv_igemm would;
 * weights from fp_pack_up2_weight_dgrad_bf3 / FP_PACK_UP2_DGRAD_BF3 (fp_up2_packed_weight_elems(c_count, Cout) * 3 / 2 floats). */
int fp_pack_up2_weight_dgrad_bf3(const float* w_oihw, void* wp, int32_t Cout, int32_t Cin, int32_t c_begin,
                                 int32_t c_count, fp_stream_t stream);
int fp_conv_up2_phase_dgrad_bf3(const float* dz, const void* wpacked_bf3, float* ext, int32_t N, int32_t h, int32_t w,
                                int32_t Cout, int32_t C0, fp_stream_t stream);
int fp_up2_fold_bwd(const float* ext, int32_t N, int32_t h, int32_t w, int32_t C, const float* addend,
                    const float* ylow_elu, float* dlow, const fp_aux* aux, fp_stream_t stream);
/* Weight gradient of the upsampled half: dw_oihw[:, k_begin:k_begin+C0] (+)= un-collapse of the 16 per-phase products
 * (dw_oihw is [Nout][kc_total][3][3]).  fp_conv_up2_phase_wgrad_workspace returns -1 for shapes it does not take
 * (C0, Nout multiples of 32; <= 30 % padded 2x16 chunks) -- use fp_conv_wgrad{FWD_REFLECT_UP2} there.  The skip half is
 * fp_conv_wgrad_slice{FWD_REFLECT} into dw_oihw[:, C0:]. */
int64_t fp_conv_up2_phase_wgrad_workspace(int32_t N, int32_t h, int32_t w, int32_t C0, int32_t Nout);
int fp_conv_up2_phase_wgrad(const float* low, const float* dz, float* dw_oihw, int32_t N, int32_t h, int32_t w, int32_t C0,
                            int32_t Nout, int32_t kc_total, int32_t k_begin, int accumulate, void* workspace,
                            int64_t workspace_bytes, fp_stream_t stream);
/* same contract and workspace; fp32 operands split exactly into three bf16 terms, six bf16 MFMA products (error below the fp32 MFMA's);
 * db (optional, [Nout]) (+)= the bias gradient = column sums of dz, from the dz tiles the kernel stages anyway */
int fp_conv_up2_phase_wgrad_bf3(const float* low, const float* dz, float* dw_oihw, float* db, int32_t N, int32_t h, int32_t w, int32_t C0,
                                int32_t Nout, int32_t kc_total, int32_t k_begin, int accumulate, void* workspace,
                                int64_t workspace_bytes, fp_stream_t stream);

/* column sums: out[c] (+)= sum_m x[m][c]  -- conv bias gradient (weight half of convolution_backward) */
int64_t fp_colsum_workspace(int64_t M, int32_t C);
int fp_colsum(const float* x, int64_t M, int32_t C, float* out, int accumulate, void* workspace,
              int64_t workspace_bytes, fp_stream_t stream);

/* backward of cat[nearest_x2(low), skip] feeding a conv: dxv is the conv's input gradient at hi-res
 * [N][2h][2w][C0+C1]; dlow[N][h][w][C0] = (sum2x2(dxv[..:C0]) + addend) * elu'(ylow) ; dskip (+)= dxv[..C0:].
 * Replaces upsample_nearest2d_backward + cat backward + elu_backward (network.py:154-155,98). */
int fp_up2cat_bwd(const float* dxv, int32_t N, int32_t h, int32_t w, int32_t C0, int32_t C1,
                  const float* addend, const float* ylow_elu, float* dlow, float* dskip, int accumulate_skip,
                  fp_stream_t stream);

/* ---- 2-channel output heads (OutConvBlock, network.py:161-183) --------- */
/* low[N][h][w][2] = [sigmoid](reflect-pad 3x3 conv Cin->2 + bias); w_oihw [2][Cin][3][3] */
int fp_head_fwd(const float* x, const float* w_oihw, const float* bias, float* low, int32_t N, int32_t h, int32_t w,
                int32_t Cin, int32_t apply_sigmoid, fp_stream_t stream);
/* out[N][out_channels][H][W] channels c0,c0+1 = bilinear_xS(low), align_corners=False (S=1: copy) */
int fp_head_upsample(const float* low, float* out_nchw, int32_t N, int32_t h, int32_t w, int32_t scale,
                     int32_t out_channels, int32_t c0, fp_stream_t stream);
/* dzlow[N][h][w][2] = bilinear^T(dout[:, c0:c0+2]) [* s(1-s), s = low when apply_sigmoid] */
int fp_head_upsample_bwd(const float* dout_nchw, const float* low, float* dzlow, int32_t N, int32_t h, int32_t w,
                         int32_t scale, int32_t out_channels, int32_t c0, int32_t apply_sigmoid, fp_stream_t stream);
/* dx[N][h][w][Cin] = conv^T(dzlow) with the reflection halo folded back (plain store);
 * elu_src != NULL: dx *= elu'(elu_src) (the head is the only consumer of an ELU output: outconv4, network.py:78-80) */
int fp_head_dgrad(const float* dzlow, const float* w_oihw, const float* elu_src, float* dx, int32_t N, int32_t h, int32_t w,
                  int32_t Cin, const fp_aux* aux, fp_stream_t stream);
/* host-only query: the workgroup mapping of fp_head_fwd / fp_head_dgrad, out = (column blocks, rows per workgroup, row groups per image) */
int fp_head_grid(int32_t N, int32_t h, int32_t w, int32_t Cin, int32_t out[3]);
/* dw_oihw[2][Cin][3][3], db[2] (+)= ... ; deterministic two-stage */
int64_t fp_head_wgrad_workspace(int32_t N, int32_t h, int32_t w, int32_t Cin);
int fp_head_wgrad(const float* x, const float* dzlow, float* dw_oihw, float* db, int32_t N, int32_t h, int32_t w,
                  int32_t Cin, int accumulate, void* workspace, int64_t workspace_bytes, fp_stream_t stream);

/* The stem (7x7 / stride 2 / pad 3 on the NCHW image, (x - 0.45) / 0.225 applied before the zero padding; network.py:48-52) with fp16-pair
 * operands: the image patch of an 8 x 16 output tile is normalised, scaled by 2^12 (|x| <= 2.45) and split into its two fp16 planes once in
 * LDS; weights from an FP_PACK_STEM_HP job with the slot they were scaled by.  Same desc / epilogue rules as fp_conv_igemm's STEM gather
 * (bias flag, act); honors the statistics and amax sinks.  fp_conv_stem_hp_supported: Nout == 64, IH == 2 OH, IW == 2 OW. */
int fp_conv_stem_hp_supported(const fp_conv_desc* d);
int fp_conv_stem_hp(const fp_conv_desc* d, const float* img_nchw, const void* wpacked_hp, const float* bias, float* y,
                    const uint32_t* amax_w, const fp_aux* aux, fp_stream_t stream);

/* ... and the stem's weight gradient likewise (dW [64][3][7][7] (+)= ...; desc / workspace of fp_conv_wgrad on the STEM gather): the image
 * patch and the dZ tile are split into fp16 pairs in LDS, fragments by gfx950's transposing LDS read; `amax_dz` = amax slot of dz */
int fp_conv_stem_wgrad_hp(const fp_conv_desc* d, const float* img_nchw, const float* dz, float* dw_oihw, int accumulate, void* workspace,
                          int64_t workspace_bytes, const uint32_t* amax_dz, fp_stream_t stream);

/* ---- BatchNorm (train-mode batch statistics; torchvision BN in the encoder) ---- */
/* stats over z[M][C]: save_mean, save_invstd, fused scale = gamma*invstd, shift = beta - mean*scale;
 * running stats updated in place with momentum (unbiased var), num_batches_tracked += 1 (int64).
 * Replaces aten::native_batch_norm (training=True). workspace >= fp_bn_workspace(M, C). */
int64_t fp_bn_workspace(int64_t M, int32_t C);
int fp_bn_train_stats(const float* z, int64_t M, int32_t C, const float* gamma, const float* beta, float eps,
                      float momentum, float* running_mean, float* running_var, int64_t* num_batches_tracked,
                      float* save_mean, float* save_invstd, float* scale, float* shift, void* workspace,
                      int64_t workspace_bytes, fp_stream_t stream);
/* fp_bn_train_stats's second launch on Welford partials that the producing convolution's epilogue wrote (fp_aux.bn_part, bnb_z == NULL): same
 * outputs, the activation is not read for its statistics (torchvision BatchNorm2d behind footprints/network.py:38-44). */
int fp_bn_train_stats_partials(const float* part, int32_t nblk, int32_t C, const float* gamma, const float* beta, float eps,
                               float momentum, float* running_mean, float* running_var, int64_t* num_batches_tracked,
                               float* save_mean, float* save_invstd, float* scale, float* shift, fp_stream_t stream);
/* The backward counterpart (round 4): fp_bn_bwd's combination + apply launches on partial sums (sum g, sum g * xhat) that a data gradient's
 * epilogue wrote (fp_aux.bn_part with bnb_z / bnb_mean / bnb_invstd): fp_bn_bwd's reduction pass over (dy, relu_out, z) and its launch are gone
 * (the backward of torchvision BatchNorm2d behind footprints/network.py:38-44; coef = 2 C floats of scratch). */
int fp_bn_bwd_partials(const float* g, const float* z, const float* save_mean, const float* save_invstd, const float* gamma, float* dz,
                       float* dgamma, float* dbeta, int accumulate, int64_t M, int32_t C, const float* part, int32_t nblk, float* coef,
                       const fp_aux* aux, fp_stream_t stream);
/* eval mode: scale/shift from running statistics */
int fp_bn_eval_coeffs(const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                      float eps, int32_t C, float* scale, float* shift, fp_stream_t stream);
/* ... and for a backward pass through the layer (fine-tuning with frozen statistics): the same coefficients, with save_mean = running_mean and
 * save_invstd = 1 / sqrt(running_var + eps) left where fp_bn_bwd_frozen and the data gradients' epilogue sinks (fp_aux.bnb_*) read them;
 * scale = gamma * save_invstd is built from that float32 value. */
int fp_bn_eval_coeffs_saved(const float* gamma, const float* beta, const float* running_mean, const float* running_var, float eps,
                            int32_t C, float* scale, float* shift, float* save_mean, float* save_invstd, fp_stream_t stream);
/* Backward of nn.BatchNorm2d in eval mode (aten::native_batch_norm_backward with train=False; torchvision BatchNorm2d behind
 * footprints/network.py:38-44 with frozen statistics): g = dy * (relu_out > 0 if relu_out); dz = g * gamma * invstd; g_out (optional) = g;
 * dbeta (+)= sum g; dgamma (+)= sum g * (z - mean) * invstd.  One pass; with dgamma == dbeta == NULL a single launch that never reads z /
 * mean (both may be NULL, workspace too); otherwise per-workgroup partial sums + a small combining launch (double, fixed order, no atomics),
 * workspace >= fp_bn_workspace(M, C).  amax_out (optional): the amax slot that receives max |dz|, published like fp_bn_bwd's (the slot
 * itself is the argument: these two launches have no other side output to ask for). */
int fp_bn_bwd_frozen(const float* dy, const float* relu_out, const float* z, const float* mean, const float* invstd, const float* gamma,
                     float* dz, float* dgamma, float* dbeta, float* g_out, int accumulate, int64_t M, int32_t C, void* workspace,
                     int64_t workspace_bytes, uint32_t* amax_out, fp_stream_t stream);
/* ... on a masked g and the partial sums (sum g, sum g * xhat) that the producing data gradient's epilogue wrote (fp_aux.bn_part with bnb_mean /
 * bnb_invstd = the running statistics): they ARE dbeta / dgamma; only their combination (skipped with dgamma == dbeta == NULL) and the
 * element-wise dz remain. */
int fp_bn_bwd_frozen_partials(const float* g, const float* invstd, const float* gamma, float* dz, float* dgamma, float* dbeta, int accumulate,
                              int64_t M, int32_t C, const float* part, int32_t nblk, uint32_t* amax_out, fp_stream_t stream);
/* out[r][:] = w[r][:] * scale[r]: folds the eval-mode scale into the preceding conv's OIHW weights (the shift becomes the
 * conv's bias), so inference runs conv + bias + ReLU (+ residual) in one launch -- SURVEY.md section 8(f) N1. */
int fp_scale_rows(const float* w, const float* scale, float* out, int64_t rows, int64_t inner, fp_stream_t stream);
/* y = [relu](z*scale + shift [+ residual]) */
/* fp16-pair operands for the flattened implicit GEMM (round 3): the 3x3 stride-2 and 1x1 convolutions of torchvision's BasicBlocks
 * (footprints/network.py:38-44) and their data gradients -- everything fp_conv3x3_hp does not take -- on the fp16 matrix path instead of
 * the fp32 one.  Same operation / epilogue flags / split-K workspace as fp_conv_igemm for zero-padding gathers of one source tensor
 * (FP_GATHER_FWD_ZERO, FP_GATHER_DGRAD_ZERO; C1 = 0); weights from FP_PACK_FWD_HP / FP_PACK_DGRAD_HP jobs (any kernel size) with the
 * slot `amax_w` they were scaled by; `amax_src` holds max |src| (fp_amax_f32 or a producer's publication). */
int fp_conv_igemm_hp_supported(const fp_conv_desc* d);
int fp_conv_igemm_hp(const fp_conv_desc* d, const float* src, const void* wpacked_hp, const float* bias, const float* addend,
                     const float* addend_mask, const float* actsrc, float* y, void* workspace, int64_t workspace_bytes,
                     const uint32_t* amax_src, const uint32_t* amax_w, const fp_aux* aux, fp_stream_t stream);
/* ... and with EXACTLY split bf16x3 operands (round 5): the default operand format's path for the same convolutions -- x = h + m + l in
 * bf16, six MFMA products, no operand bit of fp32 dropped, no amax slots.  Weights from FP_PACK_FWD_BF3 / FP_PACK_DGRAD_BF3 jobs (any
 * kernel size; fp_packed_weight_elems_bf3 floats).  Shapes: fp_conv_igemm_hp_supported.  Replaces aten::convolution /
 * convolution_backward(data) of the stride-2 BasicBlock convs and the 1x1 downsample convs (footprints/network.py:38-44). */
int fp_conv_igemm_bf3(const fp_conv_desc* d, const float* src, const void* wpacked_bf3, const float* bias, const float* addend,
                      const float* addend_mask, const float* actsrc, float* y, void* workspace, int64_t workspace_bytes, const fp_aux* aux,
                      fp_stream_t stream);

int fp_bn_apply(const float* z, const float* scale, const float* shift, const float* residual, float* y, int64_t M,
                int32_t C, int32_t relu, const fp_aux* aux, fp_stream_t stream);
/* backward: g = dy * (relu_out > 0 if relu_out) ; dgamma (+)= sum g*xhat ; dbeta (+)= sum g ;
 * dz = gamma*invstd*(g - mean(g) - xhat*mean(g*xhat)) ; g_out (optional) = g. */
int fp_bn_bwd(const float* dy, const float* relu_out, const float* z, const float* save_mean, const float* save_invstd,
              const float* gamma, float* dz, float* g_out, float* dgamma, float* dbeta, int accumulate, int64_t M,
              int32_t C, void* workspace, int64_t workspace_bytes, const fp_aux* aux, fp_stream_t stream);

/* ---- test-set inference output: [B][4][H][W] fp32 predictions -> float16 with sigmoid on channels 0, 1
 * (reference evaluation/inference.py:105-108, datasets/inference_dataset.py:35-38) ---- */
int fp_pack_pred_fp16(const float* pred_nchw, void* out_half, int32_t B, int32_t H, int32_t W, fp_stream_t stream);

/* ---- test-set metrics (reference evaluation/evaluate_model.py:50-99 evaluate_depth / evaluate_mask, :160-177 call sites).
 * pred: float32 or float16 (pred_is_half) images, image b at pred + b * pred_stride elements; gt: float32 [B][pixels];
 * region: optional uint8 [B][pixels] (pixels with 0 are skipped); invert = 1 evaluates (1 - gt, 1 - pred) like the footprint score.
 * counts: int64 [B][4] = n_true, tp, fp, fn.   sums: float64 [B][5] = n, n(thresh < 1.25), sum sq, sum abs_rel, sum sq_rel over gt > 0. */
int fp_eval_mask_counts(const void* pred, int32_t pred_is_half, const float* gt, const uint8_t* region, int32_t invert, int32_t B,
                        int64_t pixels, int64_t pred_stride, int64_t* counts, fp_stream_t stream);
int fp_eval_depth_sums(const void* pred_disp, int32_t pred_is_half, const float* gt, int32_t B, int64_t pixels, int64_t pred_stride,
                       double min_depth, double max_depth, double clip_min, double clip_max, double* sums, fp_stream_t stream);

/* ---- training-label generation (reference preprocessing/ground_truth_generation/{geometry,ground_truth_generator}.py) -------------
 * Matrices are row-major fp32 4 x 4 per frame ([B][16]); depths fp32 [B][H*W]; cam_pix fp32 [B][4][H*W] = u, v, z, c3.
 * Warp: w = (invK[:3,:3] . (x, y, 1)) * d, m = (d > 0); c = K . (T . (w, m)); u = c0 / (c2 + 1e-7f), v = c1 / (c2 + 1e-7f), z = c2.  An
 * infinite depth is not special-cased: it gives NaN coordinates and an invalid point.
 * Splat: a point is valid when u > 0 && u < W && v > 0 && v < H && z > 0 && c3 > 0; it writes z to pixel (trunc(v), trunc(u)) of its
 * frame, and of several valid points in one pixel the one with the HIGHEST source index wins.  `keys` is the device-only plane that
 * decides this: uint64 [B][H*W], (source_index + 1) << 32 | float_bits(z), fp_gt_workspace(B, H, W) bytes; the splats clear it first.
 * Aggregate: n = frames with depth > 0 at the pixel; 0 unless n > 2 (robust) / n > 0, else (s[(n-1)/2] + s[n/2]) * 0.5f of the sorted
 * positive depths (= numpy.ma.median(...).filled(0)); `projections` (optional) receives the per-frame depths [B][H*W].
 * All of them refuse B > 512 and H * W * 64 >= 2^32 - 1 (the source index of the depth mask's 64 offset copies).
 * fp_gt_workspace is host-only: bytes of key plane, or -1 with the error string set. */
int64_t fp_gt_workspace(int32_t B, int32_t H, int32_t W);
int fp_gt_project(const float* depths, const float* inv_intrinsics, const float* poses, const float* intrinsics, int32_t B, int32_t H,
                  int32_t W, float* cam_pix, fp_stream_t stream);
/* the two halves of the warp on their own (BatchProjector.project_to_world / project_to_camera): world fp32 [B][4][points] = x, y, z, m */
int fp_gt_project_to_world(const float* depths, const float* inv_intrinsics, int32_t B, int32_t H, int32_t W, float* world,
                           fp_stream_t stream);
int fp_gt_project_to_camera(const float* world, const float* poses, const float* intrinsics, int32_t B, int64_t points, float* cam_pix,
                            fp_stream_t stream);
int fp_gt_splat(const float* cam_pix, int32_t B, int32_t H, int32_t W, uint64_t* keys, int64_t keys_bytes, fp_stream_t stream);
int fp_gt_warp_splat(const float* depths, const float* inv_intrinsics, const float* poses, const float* intrinsics, int32_t B, int32_t H,
                     int32_t W, uint64_t* keys, int64_t keys_bytes, fp_stream_t stream);
int fp_gt_aggregate(const uint64_t* keys, int32_t B, int32_t H, int32_t W, int32_t robust, float* median, float* projections,
                    fp_stream_t stream);
/* moving-object mask of one frame: depth = (float)fx_baseline / disparity, warp by `pose`, induced flow (u - x, v - y) against
 * flow fp32 [2][H*W]; mask uint8 [H*W] = sqrt(d0^2 + d1^2) > 3 (float64 on the fp32 differences; NaN compares false) */
int fp_gt_moving_mask(const float* disparity, const float* flow, const float* inv_intrinsics, const float* pose, const float* intrinsics,
                      double fx_baseline, int32_t H, int32_t W, uint8_t* mask, fp_stream_t stream);
/* depth mask, on the back-projected frame `world` (fp32 [4][H*W] of fp_gt_project_to_world).  fp_gt_ground_count: count[0] = pixels with ground_seg > threshold.  fp_gt_plane_score: `samples` int32 [C][3] index the
 * ground pixels in raster order (the host draws them); sample_pix [C][3] receives their pixel indices, planes float64 [C][4] the planes
 * (p1 - p0) x (p2 - p0), d = -n . p0 through the sampled world points (all zero for a degenerate sample, which scores 0), counts [C]
 * the ground points with |distance| < 0.05 in float64, best_plane [4] / best [2] = {index, count} the first candidate with the strictly
 * largest count ({-1, 0} when every count is 0), inlier_mask (optional) uint8 [H*W] its inliers.  fp_gt_flatten_splat: every non-ground
 * point moved onto `plane` (device pointer, 4 float64), copied to the 8 x 8 offsets numpy.arange(-0.1, 0.1, 0.025) along n x (0,0,1) and
 * n x (n x (0,0,1)), projected with K and splatted with source index k * H*W + p into keys [H*W]; cam_pix (optional, for tests) fp32
 * [4][64 * H*W] receives the copies' coordinates (NaN for ground pixels).  fp_gt_depth_mask: mask uint8 [H*W] = projection > 0 &&
 * ground_seg < 0.5 && |projection - depth| / (depth + 1e-7) < 0.10 && projection < 30 && depth > 0; projection (optional) fp32 [H*W]. */
int fp_gt_ground_count(const float* ground_seg, double threshold, int32_t H, int32_t W, int32_t* count, fp_stream_t stream);
int fp_gt_plane_score(const float* world, const float* ground_seg, double threshold, const int32_t* samples, int32_t C, int32_t H, int32_t W, int32_t* sample_pix, double* planes, int32_t* counts, double* best_plane,
                      int32_t* best, uint8_t* inlier_mask, fp_stream_t stream);
int fp_gt_flatten_splat(const float* world, const float* ground_seg, double threshold, const float* intrinsics, const double* plane, int32_t H, int32_t W, uint64_t* keys, int64_t keys_bytes, float* cam_pix, fp_stream_t stream);
int fp_gt_depth_mask(const uint64_t* keys, const float* depth, const float* ground_seg, int32_t H, int32_t W, uint8_t* mask,
                     float* projection, fp_stream_t stream);

/* ---- the paper's comparison baselines (csrc/baselines.hip; reference footprints/baselines/) ----------
 * A mask argument is a pointer with a dtype code: 0 = uint8 (non-zero is set), 1 = float16, 2 = float32 (value > threshold, compared
 * in the mask's own dtype as numpy compares an array with a Python scalar).  All arrays are [B][H][W] unless stated.
 * fp_baseline_hull: out uint8 = skimage.morphology.convex_hull_image(mask) with its defaults for every frame (zeros for an empty mask),
 * in exact integer arithmetic on doubled coordinates; then, in the same pass, pixels with remove < 0.5 (optional, any dtype code) are
 * cleared and pixels set in keep (optional mask with its own threshold) are set -- BoundingBox.frame_predict's order.  spans int32
 * [B][H][2] is caller-owned scratch that receives each row's inclusive column span {lo, hi} of the hull (lo > hi: empty row).
 * H <= 2040, W <= 32768.  Three launches for any B.
 * fp_baseline_mask_counts: counts int32 [B] = set pixels per frame.
 * fp_baseline_plane_fit: points are depth * (inv_K . (x, y, 1)) in float64 (depth fp32, inv_K float64 [B][3][3]); samples int32
 * [B][C][3], C <= 100, are ranks into the frame's masked pixels in raster order (the host draws them); sample_pix [B][C][3] receives
 * their pixel indices (-1: out of range), planes float64 [B][C][4] the unit 4-vectors spanning the null space of the three augmented
 * sample points (ransac.estimate up to sign; all zero for a sample that repeats a rank, has a rank out of range or whose minors are
 * all zero -- such a candidate scores 0), counts [B][C] the masked points with |m . (p, 1)| < 0.05, best [B][2] = {index, count} of the
 * first candidate with the strictly largest count ({-1, 0} when every count is 0) and best_plane [B][4] its vector.  Three launches.
 * fp_baseline_plane_depth: out float64 = depth - (m . (p, 1)) / (rhat . m[:3]) at EVERY pixel, rhat the normalised ray, m =
 * best_plane[b]; a frame with passthrough[b] != 0 (optional uint8 [B]; the host sets it for fewer than 20 masked pixels) gets its depth. */
int fp_baseline_hull(const void* x, int32_t dtype, double threshold, const void* remove, int32_t remove_dtype, const void* keep,
                     int32_t keep_dtype, double keep_threshold, int32_t B, int32_t H, int32_t W, int32_t* spans, uint8_t* out,
                     fp_stream_t stream);
int fp_baseline_mask_counts(const void* x, int32_t dtype, double threshold, int32_t B, int32_t H, int32_t W, int32_t* counts,
                            fp_stream_t stream);
int fp_baseline_plane_fit(const float* depth, const double* inv_K, const void* mask, int32_t dtype, double threshold,
                          const int32_t* samples, int32_t C, int32_t B, int32_t H, int32_t W, int32_t* sample_pix, double* planes,
                          int32_t* counts, double* best_plane, int32_t* best, fp_stream_t stream);
int fp_baseline_plane_depth(const float* depth, const double* inv_K, const double* best_plane, const uint8_t* passthrough, int32_t B,
                            int32_t H, int32_t W, double* out, fp_stream_t stream);

/* ---- maxpool 3x3 stride 2 pad 1 (encoder.maxpool, network.py:41) ---------- */
int fp_maxpool_fwd(const float* x, float* y, uint8_t* argmax, int32_t N, int32_t H, int32_t W, int32_t C,
                   const fp_aux* aux, fp_stream_t stream);
int fp_maxpool_bwd(const float* dy, const uint8_t* argmax, float* dx, int32_t N, int32_t H, int32_t W, int32_t C,
                   int accumulate, fp_stream_t stream);

/* ---- fused multi-head loss, forward + backward (training/losses.py:31-152) ---- */
/* preds[4]: '1/8','1/4','1/2','1/1' each [B][4][H][W]; targets [B][H][W];
 * losses_out[21] in the order of LossManager's dict (5 per scale: visible_ground, all_ground, depth,
 * ground_depth, loss; then total 'loss'); dpreds[4] = d(total loss)/d(pred) (may be NULL => forward only). */
int64_t fp_loss_workspace(int32_t B, int32_t H, int32_t W);
int fp_loss_fwd_bwd(const float* const preds[4], const float* visible_ground, const float* all_ground,
                    const float* depth, const float* ground_depth, const float* moving_object_mask,
                    const float* depth_mask, float min_depth, float max_depth, float prior_weight,
                    float* const dpreds[4], float* losses_out, int32_t B, int32_t H, int32_t W, void* workspace,
                    int64_t workspace_bytes, fp_stream_t stream);

/* ---- fused Adam over a flat parameter buffer (torch.optim.Adam, model_manager.py:27) ---- */
/* hyper-parameters are doubles (python floats) like torch's; gradients are multiplied by grad_scale (1/world under DP) */
int fp_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, double lr, double beta1,
                 double beta2, double eps, int32_t step, double grad_scale, fp_stream_t stream);
/* Graph-replay variant: the seven per-step scalars (fp_adam_hyper fills them on the host exactly as fp_adam_step derives
 * them) live in device memory, so a captured launch stays valid across steps; n must be a multiple of 4. */
int fp_adam_hyper(double lr, double beta1, double beta2, double eps, int32_t step, double grad_scale, float* hyper7_host);
int fp_adam_step_dev(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                     const float* hyper7_dev, fp_stream_t stream);

/* ---- recorded launch plans: replay a whole training step (~740 launches on five streams) from C ------------------------------ */
/* While a plan records (thread local) every kernel launch of this library and every fp_event_record / fp_event_wait is executed AND
 * appended to the plan with a private copy of its arguments; fp_plan_replay re-issues nodes [begin, end) (end < 0: to the last node)
 * with the same streams.  Valid as long as every pointer argument stays valid (static arena, workspaces and tables).
 * fp_plan_mark returns the current node count (stage boundaries for a replay in pieces, e.g. around gradient all-reduces). */
void* fp_plan_begin(void);
int32_t fp_plan_mark(void* plan);
int32_t fp_plan_end(void* plan);
int fp_plan_replay(void* plan, int32_t begin, int32_t end);
void fp_plan_destroy(void* plan);
/* stream-to-stream ordering used by the engine (instead of framework events, so that a recording sees it): record returns an event
 * id >= 0 (valid for fp_event_wait until ~4000 further records, or -- inside a recording -- until the recording ends) */
int64_t fp_event_record(fp_stream_t stream);
int fp_event_wait(fp_stream_t stream, int64_t event_id);

/* ---- device-side data path (footprints/datasets/footprint_dataset.py:55-65,73-85; kitti_dataset.py:66-112; matterport_dataset.py:69-97) ---- */
/* one per sample; fp_aug_params_bytes() == sizeof(fp_aug_params) */
typedef struct fp_aug_params {
  int32_t flip;        /* horizontal flip of the image and every label map (footprint_dataset.py:73-75,84-85) */
  int32_t n_ops;       /* 0 = no colour jitter, 4 = torchvision ColorJitter's four ops */
  int32_t ops[4];      /* application order (random.shuffle in ColorJitter.get_params): 0 brightness, 1 contrast, 2 saturation, 3 hue */
  float factor[4];     /* indexed by op id: ImageEnhance factors (float, as libImaging's Image.blend takes them) */
  int32_t hue_shift;   /* np.uint8(hue_factor * 255) of torchvision's adjust_hue */
  int32_t pad;
} fp_aug_params;
int32_t fp_aug_params_bytes(void);
/* images_hwc uint8 [B][H][W][3] (as PIL delivers them after the resize, not flipped) -> out_nchw float [B][3][H][W] in [0,1]:
 * flip, ColorJitter (bit-exact with Pillow 12's ImageEnhance / convert arithmetic), ToTensor.  luma_sums: B uint64 scratch
 * (the contrast op needs the mean grey level of the image as it stands before that op: one integer reduction pass). */
int fp_assemble_images(const uint8_t* images_hwc, const void* aug_params, uint64_t* luma_sums, float* out_nchw, int32_t B, int32_t H,
                       int32_t W, fp_stream_t stream);
/* label maps [B][H][W] (float32 or float64 as they leave the resize, not flipped) -> the six float32 maps of the batch schema.
 * dataset 0 = KITTI (aux = resized pixel disparity before the -1.25; fxb = focal * baseline; moving may be NULL when !use_moving),
 * 1 = Matterport (aux = raw 16-bit depth, depth_scaling = metres per unit).  Arithmetic in float64 like numpy in the reference. */
int fp_assemble_labels(const void* visible_ground, const void* ground_depth, const void* depth_mask, const void* aux, const void* moving,
                       int32_t is_double, const void* aug_params, float* o_visible_ground, float* o_depth, float* o_ground_depth,
                       float* o_moving, float* o_depth_mask, float* o_all_ground, int32_t B, int32_t H, int32_t W, int32_t dataset,
                       int32_t no_depth_mask, int32_t project_down_baseline, int32_t use_moving, double threshold, double fxb,
                       double depth_scaling, fp_stream_t stream);

/* ---- device-side reader work: Pillow's 8-bit Image.resize and filter_depth_mask (footprint_dataset.py:73-80, :96-105;
 * csrc/resample_u8.hip, csrc/reader.hip) ---- */
/* Resample filters, numbered like Pillow's Image.Resampling.  NEAREST (0) is not provided; of the mode-"F" (float) paths only
 * what the overlay below needs: the double tables as an entry point of their own, the float passes inside the overlay. */
#define FP_RESIZE_LANCZOS 1
#define FP_RESIZE_BILINEAR 2
#define FP_RESIZE_BICUBIC 3
#define FP_RESIZE_BOX 4
/* HOST functions (no GPU needed): Resample.c's coefficient tables of one axis.  ksize = 2 * ceil(support * max(in / out, 1)) + 1 (-1 on bad
 * arguments); bounds int32 [out][2] = first source index and tap count, kk int32 [out][ksize] = the taps in 22-bit fixed point, rows padded
 * with zeros.  Built in double exactly as Pillow builds them. */
int32_t fp_resize_ksize(int32_t in_size, int32_t out_size, int32_t filter);
int fp_resize_coeffs(int32_t in_size, int32_t out_size, int32_t filter, int32_t* bounds, int32_t* kk, int32_t ksize);
/* one axis table inside the int32 coefficient buffer on the device; fp_resize_table_bytes() == sizeof(fp_resize_table) */
typedef struct fp_resize_table {
  int32_t in_size, out_size, ksize;
  int32_t bounds_off; /* element offsets into the coefficient buffer */
  int32_t kk_off;
} fp_resize_table;
/* one source image of the batch; fp_resize_sample_bytes() == sizeof(fp_resize_sample) */
typedef struct fp_resize_sample {
  int64_t offset;  /* of its first byte in the packed source buffer; the image is uint8 [h][w][C], dense */
  int32_t h, w;
  int32_t table_h; /* index of its (w -> W) table; -1 = w == W, no horizontal pass */
  int32_t table_v; /* index of its (h -> H) table; -1 = h == H, no vertical pass */
} fp_resize_sample;
int32_t fp_resize_table_bytes(void);
int32_t fp_resize_sample_bytes(void);
/* bytes of the workspace: the uint8 intermediate between the horizontal and the vertical pass (B * max_h * W * C) and, at
 * fp_resize_status_offset, one int32 status word (-1 on bad arguments) */
int64_t fp_resize_workspace(int32_t B, int32_t max_h, int32_t W, int32_t C);
int64_t fp_resize_status_offset(int32_t B, int32_t max_h, int32_t W, int32_t C);
/* B source images of different sizes (all h <= max_h, w <= max_w; C = 1 or 3), packed in `src` (4-byte aligned, src_bytes long) and
 * described by `samples` (device, B records), -> out uint8 [B][H][W][C], byte for byte what PIL.Image.resize((W, H), filter) gives:
 * horizontal pass into the uint8 workspace, then the vertical pass, a pass whose sizes agree skipped, int32 arithmetic throughout.  It is
 * fp_resize_window_u8 (below) with window = target and rectangle = source: the same two kernels, two launches.
 * tables: n_tables device records over `coeffs` (device int32, coeffs_len elements).  A record that points outside a buffer, or whose
 * table does not fit its sizes, leaves that sample's output unwritten and sets the workspace's status word to 1 (every call clears it
 * first; read it after the stream has finished).  max_w * C <= 65528 (a source row is staged in LDS). */
int fp_resize_u8(const uint8_t* src, int64_t src_bytes, const void* samples, const void* tables, int32_t n_tables, const int32_t* coeffs,
                 int64_t coeffs_len, uint8_t* out, int32_t B, int32_t H, int32_t W, int32_t C, int32_t max_h, int32_t max_w, void* workspace,
                 int64_t workspace_bytes, fp_stream_t stream);
/* filter_depth_mask: mask [B][H][W] (float32, or float64 when is_double; values 0 / 1) -> out, same type: 1 on every 8-connected component
 * of ones with fewer than W * H / 100 pixels (compared in double, strictly), 0 elsewhere.  out may be the mask itself.  Integer atomics
 * only: the result does not depend on scheduling.  workspace >= fp_filter_depth_mask_workspace(B, H, W) bytes (-1: too large). */
int64_t fp_filter_depth_mask_workspace(int32_t B, int32_t H, int32_t W);
int fp_filter_depth_mask(const void* mask, int32_t is_double, void* out, int32_t B, int32_t H, int32_t W, void* workspace,
                         int64_t workspace_bytes, fp_stream_t stream);

/* ---- device-side reader work: the cv2 resizes of the label maps (footprint_dataset.py:82-94; csrc/label_resize.hip) ---- */
#define FP_LABEL_U8 0 /* stored dtype of a map: uint8 or bool */
#define FP_LABEL_F16 1
#define FP_LABEL_F32 2
#define FP_LABEL_F64 3
#define FP_LABEL_U16 4 /* uint16: Matterport's depth PNG (mode I;16) */
#define FP_LABEL_ZERO 0    /* the map is 0.0 everywhere (a missing depth mask); nothing is read */
#define FP_LABEL_NEAREST 1 /* cv2.INTER_NEAREST */
#define FP_LABEL_AREA 2    /* cv2.INTER_AREA, shrinking or equal on both axes; its upscaling branch (a linear kernel) is not provided */
#define FP_LABEL_PIL_NEAREST 3 /* Pillow's Image.resize(NEAREST): src = min(floor((dst + 0.5) * in / out), in - 1) per axis, any ratio;
                                * a flipped record is resized first and flipped then, so it reads the source unmirrored */
#define FP_LABEL_MAX_ENTRIES 12 /* most entries of one output index in an area table that a launch stages: non-integer shrink factors up to 10 */
/* one map of the batch; fp_label_sample_bytes() == sizeof(fp_label_sample) */
typedef struct fp_label_sample {
  int64_t offset;  /* of its first byte in the packed source buffer, a multiple of 8; the map is dense [h][w] of `dtype` */
  int32_t h, w;
  int32_t dtype;   /* FP_LABEL_U8 .. FP_LABEL_U16 */
  int32_t method;  /* FP_LABEL_ZERO / NEAREST / AREA / PIL_NEAREST */
  int32_t flip;    /* read the source mirrored and store mirrored (PIL_NEAREST: read unmirrored, store mirrored) */
  int32_t table_x; /* index of its (w -> W) area table; read only on INTER_AREA's general path */
  int32_t table_y; /* index of its (h -> H) area table */
  int32_t pad;
  double multiplier; /* the resized value is multiplied by it (the KITTI disparity: W / w; 1.0 elsewhere) */
} fp_label_sample;
/* one axis table of INTER_AREA inside the entry buffer (8-byte elements; offsets count elements): bounds = one element per output index
 * (two int32: first entry relative to the table's entries, entry count), entries = (int32 source index, float weight);
 * fp_label_table_bytes() == sizeof(fp_label_table) */
typedef struct fp_label_table {
  int32_t in_size, out_size;
  int32_t max_count; /* most entries of one output index, <= FP_LABEL_MAX_ENTRIES */
  int32_t n_entries;
  int32_t bounds_off;
  int32_t entries_off;
} fp_label_table;
int32_t fp_label_sample_bytes(void);
int32_t fp_label_table_bytes(void);
int32_t fp_label_max_entries(void);
/* HOST function (no GPU needed): OpenCV's computeResizeAreaTab of one axis, out_size <= in_size.  With scale = 1 / ((double)out / in), for
 * every output index d: f1 = d * scale, f2 = f1 + scale, cw = min(scale, in - f1), s1 = ceil(f1), s2 = min(floor(f2), in - 1), s1 = min(s1, s2);
 * a leading partial cell (s1 - 1, (s1 - f1) / cw) when s1 - f1 > 1e-3, whole cells (s, 1 / cw) for s1 <= s < s2, a trailing partial cell
 * (s2, min(min(f2 - s2, 1), cw) / cw) when f2 - s2 > 1e-3; every weight rounded to float.  bounds int32 [out][2] = first entry and count,
 * index int32 / weight float [capacity].  Returns the number of entries (at most in + 2 * out), -1 on bad arguments or when they do not
 * fit; with bounds, index and weight NULL it only counts. */
int32_t fp_area_table(int32_t in_size, int32_t out_size, int32_t* bounds, int32_t* index, float* weight, int32_t capacity);
/* n_records maps of mixed sizes and stored dtypes, packed in `src` (device, 8-byte aligned, src_bytes long) and described by `samples`
 * (device, n_records fp_label_sample), -> out double [n_records][H][W], bit for bit what
 * cv2.resize(m.astype(float), (W, H), interpolation) * multiplier gives on float64 data, restated from OpenCV's algorithm: equal sizes are
 * copied; NEAREST reads min(floor(d * scale), in - 1) per axis with scale = 1 / ((double)out / in); AREA with both scales integer (within
 * DBL_EPSILON) sums the block in row-major order in double and multiplies by (double)(1.f / (float)area); AREA otherwise walks the two
 * axis tables: per y entry buf = 0.0, buf = buf + S[sy][sx] * alpha over the x entries, sum = beta * buf for the first y entry and
 * sum = sum + beta * buf after it, the float weights widened to double, no fused multiply-add.  A flipped record gives
 * cv2.resize(np.fliplr(m)) mirrored, so that the flip of fp_assemble_labels undoes the mirroring.  PIL_NEAREST gathers
 * S[min(((2 * y + 1) * h) / (2 * H), h - 1)][min(((2 * x + 1) * w) / (2 * W), w - 1)] in integers, flipped or not.  tables: n_tables fp_label_table records
 * over `entries` (device, entries_len 8-byte elements).  A record that points outside the packed buffer, asks AREA to enlarge, or whose
 * table does not fit its sizes leaves that map unwritten and sets *status (one int32 on the device) to 1; every call clears it first; read
 * it after the stream has finished.  max_entries: the largest max_count of the tables (0 without tables, at most FP_LABEL_MAX_ENTRIES); it
 * sizes the launch's LDS (2 * max_entries * 2 KiB per workgroup), and a table with a longer row is turned down like any other that does not
 * fit.  One kernel, one thread per output element, no workspace. */
int fp_label_resize(const void* src, int64_t src_bytes, const void* samples, int32_t n_records, const void* tables, int32_t n_tables,
                    const void* entries, int64_t entries_len, int32_t max_entries, double* out, int32_t H, int32_t W, int32_t* status,
                    fp_stream_t stream);

/* ---- device-side loader work of the training-label generators (preprocessing/ground_truth_generation/data_loader.py;
 * csrc/gt_frames.hip) ---- */
#define FP_GT_F16 0 /* stored dtype of a source map */
#define FP_GT_F32 1
#define FP_GT_F64 2
#define FP_GT_U16 3    /* Matterport's 16-bit depth; takes no pre-scale */
#define FP_GT_LINEAR 0  /* cv2.resize's default INTER_LINEAR on float64, enlarging as well as shrinking, through two axis tables */
#define FP_GT_NEAREST 1 /* cv2.INTER_NEAREST; equal sizes are a copy */
#define FP_GT_AREA2 2   /* what cv::resize makes of INTER_LINEAR when both scales are exactly 2: the fast INTER_AREA path, h == 2 H and w == 2 W */
/* one map of a launch; fp_gt_frame_bytes() == sizeof(fp_gt_frame).  Per output element, in this order: the stored element times `pre` in the
 * stored dtype (pre arrives rounded to that dtype; 1 = none), widened to double, resized by `method`, v = (v * post_num) / post_den in double
 * (two rounded operations), v = v > thr ? 1 : 0 when `threshold`, rounded to float32 (nearest even). */
typedef struct fp_gt_frame {
  int64_t offset; /* of the map's first byte in the packed source buffer, a multiple of 8; dense [h][w] of `dtype` */
  int64_t dst;    /* of its [H][W] float32 slot in the cache, in elements */
  int32_t h, w;
  int32_t dtype;  /* FP_GT_F16 .. FP_GT_U16 */
  int32_t method; /* FP_GT_LINEAR / NEAREST / AREA2 */
  int32_t table_x; /* index of the clamped (w -> W) table; read by FP_GT_LINEAR only */
  int32_t table_y; /* index of the unclamped (h -> H) table */
  int32_t threshold;
  int32_t pad;
  double pre, post_num, post_den, thr;
} fp_gt_frame;
/* one axis table of INTER_LINEAR inside the word buffer (int32 words): [out_size] first source indices, then [out_size][2] float
 * coefficient bits; fp_gt_table_bytes() == sizeof(fp_gt_table) */
typedef struct fp_gt_table {
  int32_t in_size, out_size;
  int32_t clamp;  /* 1: the horizontal form, 0: the vertical form (fp_linear_table) */
  int32_t offset; /* of the table in the word buffer, in words */
} fp_gt_table;
int32_t fp_gt_frame_bytes(void);
int32_t fp_gt_table_bytes(void);
/* HOST function (no GPU needed): cv2's INTER_LINEAR offsets and coefficients of one axis, a reading of OpenCV's portable C++ path
 * (imgproc/src/resize.cpp).  With scale = 1 / ((double)out / in), for every output index d: f = (float)((d + 0.5) * scale - 0.5),
 * s = floor(f), f -= s; with `clamp` (the horizontal pass) s < 0 gives f = 0, s = 0 and s >= in - 1 gives f = 0, s = in - 1; without (the
 * vertical pass) s and f stay, and the reader clips the row indices s and s + 1 into [0, in - 1].  offsets int32 [out] = s, coeffs float
 * [out][2] = (1.f - f, f). */
int fp_linear_table(int32_t in_size, int32_t out_size, int32_t clamp, int32_t* offsets, float* coeffs);
/* HOST function (no GPU needed): what fp_gt_frame_resize checks before it launches -- every record's source extent inside the src_bytes
 * packed bytes at a multiple of 8, its destination slot inside the cache_elems elements of the cache, dtype and method known, an integer map
 * without pre-scale, area2 at exactly twice the target, and for linear records two tables (host records; words_len = length of the word
 * buffer) that fit the record's sizes and lie inside the word buffer.  0, or FP_EINVAL with the first bad record in the error string. */
int fp_gt_frame_check(const fp_gt_frame* records, int32_t n_records, int64_t src_bytes, const fp_gt_table* tables, int32_t n_tables,
                      int64_t words_len, int64_t cache_elems, int32_t H, int32_t W);
/* n_records maps of mixed native sizes and stored dtypes, packed in `src` (device, src_bytes long), each resized into its float32 [H][W]
 * slot of `cache` (device, cache_elems elements) as fp_gt_frame states, bit for bit what the reference's loader computes on float64 before
 * its .float(): linear = HResizeLinear (out = S[s] * c0 + S[s + 1] * c1, S[in - 1] * 1.0 at the right clamp) of the two rows, then
 * VResizeLinear (h0 * b0 + h1 * b1), float coefficients widened to double, every product and sum rounded; nearest reads
 * min(floor(d * scale), in - 1) per axis; area2 sums the 2 x 2 block in row-major order and multiplies by (double)(1.f / 4.f).
 * `records` / `tables` are HOST arrays and are validated (fp_gt_frame_check) before anything is launched; d_records / d_tables are the same
 * bytes on the device, d_words the tables' word buffer; the kernel applies the same rule of what a record may address to its device copies
 * and leaves the slot of a record it turns down unwritten.  One kernel, one thread per output element, no workspace, no atomics. */
int fp_gt_frame_resize(const void* src, int64_t src_bytes, const fp_gt_frame* records, const void* d_records, int32_t n_records,
                       const fp_gt_table* tables, const void* d_tables, int32_t n_tables, const int32_t* d_words, int64_t words_len, float* cache,
                       int64_t cache_elems, int32_t H, int32_t W, fp_stream_t stream);
/* The batch of one target frame out of the cache (n_slots slots of [H][W] float32): slots (HOST, validated) / d_slots (the same on the
 * device) = int32 [2][B], the slot behind depths[b] and the slot behind ground_segs[b]; repeats and any order are fine.
 * depths[b] = fb / slot (IEEE float32 division) when `divide` (KITTI caches disparity), the slot itself otherwise (Matterport caches
 * depth); ground_segs[b] = its slot. */
int fp_gt_gather_frames(const float* cache, int64_t n_slots, const int32_t* slots, const int32_t* d_slots, int32_t B, int32_t H, int32_t W,
                        int32_t divide, float fb, float* depths, float* ground_segs, fp_stream_t stream);

/* ---- device-side reader work of the segmentation trainer (footprints/preprocessing/segmentation/datasets;
 * csrc/resample_u8.hip, csrc/seg_reader.hip) ---- */
/* HOST function (no GPU needed): rows first .. first + count - 1 of fp_resize_coeffs' tables (bounds int32 [count][2], kk int32
 * [count][ksize]).  Pillow computes every output index on its own, so the rows are identical; work and memory are those of `count` rows. */
int fp_resize_coeffs_range(int32_t in_size, int32_t out_size, int32_t filter, int32_t first, int32_t count, int32_t* bounds, int32_t* kk,
                           int32_t ksize);
/* HOST function: the source index of every output index of Pillow's NEAREST resize of one axis (idx int32 [out_size]); the source
 * coordinate starts at in / out / 2 and is accumulated in double, one addition of in / out per index, as libImaging does. */
int fp_nearest_index(int32_t in_size, int32_t out_size, int32_t* idx);
/* one axis table of the windowed resize: like fp_resize_table, but its rows describe the output indices first .. first + count - 1 only
 * (first = 0, count = out_size: a whole table).  fp_resize_window_table_bytes() == sizeof(fp_resize_window_table) */
typedef struct fp_resize_window_table {
  int32_t in_size, out_size, ksize;
  int32_t first, count;
  int32_t bounds_off; /* element offsets into the coefficient buffer */
  int32_t kk_off;
} fp_resize_window_table;
/* one sample of the windowed resize; fp_resize_window_sample_bytes() == sizeof(fp_resize_window_sample) */
typedef struct fp_resize_window_sample {
  int64_t src_offset; /* of the staged source rectangle's first byte in `src`; dense uint8 [src_h][src_w][C] */
  int64_t out_offset; /* of the window's first byte in `out`; dense uint8 [win_h][win_w][C] */
  int32_t src_h, src_w;
  int32_t src_y0, src_x0; /* where the rectangle sits in the full source image: a table's source indices minus the origin address it */
  int32_t table_h, table_v; /* index of the sample's (source width -> target width) / (height -> height) table; -1 = equal sizes, pass skipped */
  int32_t top, left, win_h, win_w; /* the window of the target image that is produced */
} fp_resize_window_sample;
int32_t fp_resize_window_table_bytes(void);
int32_t fp_resize_window_sample_bytes(void);
/* bytes of the workspace: the uint8 intermediate (B * max_src_h * max_win_w * C) and, at fp_resize_window_status_offset, one int32 status
 * word (-1 on bad arguments) */
int64_t fp_resize_window_workspace(int32_t B, int32_t max_src_h, int32_t max_win_w, int32_t C);
int64_t fp_resize_window_status_offset(int32_t B, int32_t max_src_h, int32_t max_win_w, int32_t C);
/* Per sample, the bytes of PIL.Image.resize((tw, th), filter).crop((left, top, left + win_w, top + win_h)), where (tw, th) is the sample's
 * OWN target size (the out_size of its tables): Pillow's 8-bit arithmetic and the two kernels of fp_resize_u8, but the horizontal pass runs only over the
 * source rows the window's vertical taps reach and over the window's columns, and the vertical pass produces only the window.  With both
 * tables -1 the window is copied.  `src` (device, 4-byte aligned, src_bytes long) holds each sample's staged rectangle -- at least the rows
 * and columns the window's taps reach, at most the whole image (origin 0, 0); it may be the `out` of an earlier call, which chains two
 * resizes.  Tables may describe the window's output indices only (fp_resize_coeffs_range); their bounds must not decrease along a table, as
 * Pillow's never do.  A record whose window leaves its target, whose rectangle does not cover the taps, that exceeds the stated maxima or
 * points outside a buffer leaves its output unwritten and sets the workspace's status word to 1 (every call clears it first; read it after
 * the stream has finished); the other samples are not affected.  max_src_w * C <= 65528 (the staged part of a row lives in LDS). */
int fp_resize_window_u8(const uint8_t* src, int64_t src_bytes, const void* samples, const void* tables, int32_t n_tables, const int32_t* coeffs,
                        int64_t coeffs_len, uint8_t* out, int64_t out_bytes, int32_t B, int32_t C, int32_t max_src_h, int32_t max_src_w,
                        int32_t max_win_h, int32_t max_win_w, void* workspace, int64_t workspace_bytes, fp_stream_t stream);
#define FP_SEG_DECODE_CHANNEL0 0 /* label id = channel 0 (Cityscapes, Matterport) */
#define FP_SEG_DECODE_ADE20K 1   /* label id = R / 10 * 256 + G in integers (ade20k_dataset.py:51), 0 .. 6655 */
#define FP_SEG_LABELLED_ONES 0    /* labelled_pix = 1 everywhere (ADE20K, Matterport) */
#define FP_SEG_LABELLED_NONZERO 1 /* labelled_pix = id != 0 (cityscapes_dataset.py:69) */
/* one label image of the batch; fp_seg_label_sample_bytes() == sizeof(fp_seg_label_sample) */
typedef struct fp_seg_label_sample {
  int64_t src_offset; /* of the staged label rectangle in `src`; dense uint8 [h][w][C] */
  int32_t h, w, C;    /* C = 1 or 3 */
  int32_t rows_off;   /* into `index`: [H] source row of every output row, relative to the rectangle */
  int32_t cols_off;   /* into `index`: [W] source column of every output column */
  int32_t decode;     /* FP_SEG_DECODE_* */
  int32_t labelled;   /* FP_SEG_LABELLED_* */
  int32_t ground_set; /* index of its ground-id set */
} fp_seg_label_sample;
int32_t fp_seg_label_sample_bytes(void);
/* The label half of a segmentation batch (_process_labels of the three datasets): the NEAREST resizes, crops and the flip of a label
 * image are index maps, composed by the host into one row and one column table per sample.  ground_mask[b][y][x] = id is in the sample's
 * ground-id set (np.in1d), labelled_pix per the sample's mode; float32 [B][H][W] each.  ground_ids: the sets one after the other
 * (ground_len int32), set s = ground_ids[set_offsets[s] .. set_offsets[s + 1]); one batch may mix datasets.  status: one int32 on the device,
 * cleared by the call and set to 1 when a record or a table entry points outside a buffer (those outputs stay unwritten). */
int fp_seg_labels(const uint8_t* src, int64_t src_bytes, const void* samples, const int32_t* index, int64_t index_len, const int32_t* ground_ids,
                  int64_t ground_len, const int32_t* set_offsets, int32_t n_sets, float* ground_mask, float* labelled_pix, int32_t* status,
                  int32_t B, int32_t H, int32_t W, fp_stream_t stream);

/* ---- device-side visualisations (footprints/predict_simple.py:75-92, footprints/evaluation/inference.py:114-118; csrc/visualise.hip) ---- */
/* HOST function (no GPU needed): the tables of fp_resize_coeffs before the quantisation -- kk double [out][ksize] = the taps normalised in
 * double, as Pillow's mode-"F" passes use them; bounds as there.  Both functions share the double stage. */
int fp_resize_coeffs_f64(int32_t in_size, int32_t out_size, int32_t filter, int32_t* bounds, double* kk, int32_t ksize);
/* The overlay of footprints_amd.predict_simple.InferenceManager.visualise for B predictions, byte for byte: pred float [B][4][H][W]
 * (channel 1 = hidden-ground logit, channel 3 = hidden-depth sigmoid).  The B photos are dense uint8 [h][w][3] at any byte offsets of `src`
 * (4-byte aligned, `bytes` long); `out` has the same length and layout.  samples: B fp_resize_sample records on the device, here with
 * (h, w) = the photo's size, table_h = index of its (W -> w) table and table_v = index of its (H -> h) table (-1 = equal sizes).  tables:
 * n_tables fp_resize_table records over `coeffs`, a device buffer of coeffs_len 8-BYTE elements in which offsets count: a table's bounds are
 * one element per output index (two int32: first source index, tap count), its kk the doubles of fp_resize_coeffs_f64.  lut: uint8
 * [256][3].  Per sample: both maps through Pillow's float resample (double accumulation in tap order, float store, horizontal pass first,
 * a pass whose sizes agree skipped), the depth as float 1 / (0.01 + 9.99 d) first; mask = logit > 0.5; where the mask is not empty the
 * depth is normalised by its minimum and maximum inside the mask (float; a range below 1e-12 counts as 1e-12); index = the clipped depth
 * times 256, 256 -> 255, truncated, clamped to 0..255; out = lut[index] inside the mask, the photo's bytes outside.  Integer atomics only:
 * the result does not depend on scheduling.  A record that points outside a buffer, or whose table does not fit its sizes, leaves that
 * sample's output unwritten and sets the int32 status word of the workspace (at the status offset; every call clears it first; read it
 * after the stream has finished).  The workspace query returns -1 on bad arguments or when the sizes are too large. */
int64_t fp_vis_overlay_workspace(int32_t B, int32_t H, int32_t W, int32_t max_h, int32_t max_w);
int64_t fp_vis_overlay_status_offset(int32_t B, int32_t H, int32_t W, int32_t max_h, int32_t max_w);
int fp_vis_overlay(const float* pred, const uint8_t* src, int64_t bytes, const void* samples, const void* tables, int32_t n_tables,
                   const double* coeffs, int64_t coeffs_len, const uint8_t* lut, uint8_t* out, int32_t B, int32_t H, int32_t W, int32_t max_h,
                   int32_t max_w, void* workspace, int64_t workspace_bytes, fp_stream_t stream);
/* image float [B][3][H][W] in [0,1], pred logits float [B][4][H][W] -> out uint8 [B][H][2W][3]: left half uint8(image * 255.0f), right half
 * colour1 where pred[:,1] > 0 and colour0 elsewhere (a colour = r | g << 8 | b << 16).  The reference tests sigmoid > 0.5 in fp32, which
 * differs only for positive logits so small that the fp32 sigmoid rounds to exactly 0.5. */
int fp_vis_side_by_side(const float* image, const float* pred, uint8_t* out, int32_t B, int32_t H, int32_t W, uint32_t colour0,
                        uint32_t colour1, fp_stream_t stream);

/* ---- the trainer's TensorBoard pictures (footprints/training/logger.py:19-67, training/losses.py:54-78; csrc/log_panels.hip) ---- */
/* The twelve pictures the reference logs for each of the first n samples of a batch, as bytes: out uint8 [n][P][H][W][3] with P = 12, or 11
 * when moving_object_mask is NULL.  Panel order: the image; then target_disp, target_visible_ground, target_all_ground, target_ground_depth,
 * depth_mask, moving_pixels (when present); then from pred, the raw float [B][4][H][W] output of scale 1/1: pred_disp through lut (uint8
 * [256][3], the plasma table; index min(int(x * 256), 255)), pred_ground_visible, pred_ground_all, pred_ground_disp and
 * pred_ground_disp_masked.  image float [B][3][H][W] is written as uint8(x * 255.0f) (clamped to 0..255); every other panel is
 * (v - min) / float(double(max) - double(min)) over its own H * W values (1e5 when they are equal), then uint8(x * 255.0f), replicated to
 * three channels; disparities are (1 / (d + 1e-7f)) * (d > 0), predicted depths 1 / (1 / max_depth + (1 / min_depth - 1 / max_depth) * p),
 * all in float32 without fused multiply-adds.  Labels are float [B][H][W].  Two launches (block partials of the minima and maxima, then
 * combine and map): deterministic.  The workspace query returns the bytes needed, -1 on bad sizes (n >= 1, H * W <= 2^28). */
int64_t fp_log_panels_workspace(int32_t n, int32_t H, int32_t W);
int fp_log_panels(const float* image, const float* visible_ground, const float* depth, const float* ground_depth,
                  const float* moving_object_mask, const float* depth_mask, const float* all_ground, const float* pred, const uint8_t* lut,
                  uint8_t* out, int32_t B, int32_t n, int32_t H, int32_t W, double min_depth, double max_depth, void* workspace,
                  int64_t workspace_bytes, fp_stream_t stream);
/* ---- stretched maps as pictures (csrc/stretch_map.hip) ---- */
/* The segmentation trainer's TensorBoard picture (footprints/preprocessing/segmentation/logger.py:28-42, then tensorboardX's
 * (x.astype(float32) * 255).astype(uint8)) for the first n samples of a batch: out uint8 [n][H][3 W][3] = image | ground truth | prediction.
 * image float [B][3][H][W]: (x - min) / float(double(max) - double(min)) over the sample's three channels together (1e5 when they are
 * equal), then (int)(v * 255.0f).  ground_mask float [B][H][W]: red 255 where it is 1, else 0; green and blue 0.  logits: the
 * full-resolution logit plane of sample s at logits + s * logit_batch_stride (channel 0 of the [B][2][H][W] head buffer, as fp_seg_pack takes
 * it); p = the sigmoid of fp_seg_pack, colour lut[min((int)(p * 256.0f), 255)] with lut uint8 [256][3] from the caller.  Two launches
 * (block partials of the minimum and maximum, then combine and map): deterministic.  The workspace query returns the bytes needed, -1 on
 * bad sizes (1 <= n <= 65535, H * W <= 2^27). */
int64_t fp_seg_log_panels_workspace(int32_t n, int32_t H, int32_t W);
int fp_seg_log_panels(const float* image, const float* ground_mask, const float* logits, int64_t logit_batch_stride, const uint8_t* lut,
                      uint8_t* out, int32_t B, int32_t n, int32_t H, int32_t W, void* workspace, int64_t workspace_bytes, fp_stream_t stream);
/* matplotlib's imsave of 2-D arrays: maps [B][H][W], float (is_u8 = 0) or uint8 (is_u8 = 1; booleans as bytes), finite -> out uint8
 * [B][H][W][3].  Per map: n = float(double(float(x - min)) / (double(max) - double(min))), 0 everywhere when max == min; colour
 * lut[min((int)(n * 256.0f), 255)] with lut uint8 [256][3] from the caller.  Two launches, as above; same workspace rule. */
int64_t fp_stretch_colour_workspace(int32_t B, int32_t H, int32_t W);
int fp_stretch_colour(const void* maps, int32_t is_u8, const uint8_t* lut, uint8_t* out, int32_t B, int32_t H, int32_t W, void* workspace,
                      int64_t workspace_bytes, fp_stream_t stream);
/* Host only: CRC-32C (Castagnoli, reflected polynomial 0x82F63B78) of `bytes` bytes at data, continuing from crc (0 at the start) -- the
 * checksum of the event files' record framing (training/summary.py). */
uint32_t fp_crc32c(uint32_t crc, const void* data, int64_t bytes);

/* ---- output stage of the ground-segmentation network's inference mode (footprints/preprocessing/segmentation/inference.py:80-90,
 * datasets/inference_dataset.py:39-50; csrc/seg_infer.hip) ---- */
/* One launch over the full-resolution logit planes: sample b's plane is the H * W floats at logits + b * logit_batch_stride (any stride >=
 * H * W: channel 0 of the engine's [B][2][H][W] head buffer is stride 2 * H * W).  prob_half: float16 [B][1][H][W] = __float2half_rn(p)
 * with p = 1 / (1 + expf(-x)) (accurate exponential, correctly rounded division; float16 subnormals kept) -- the .npy file's contents.
 * prob_f32 (NULL ok): float [B][1][H][W] = p.  picture (NULL ok; needs image and lut): uint8 [B][H][2W][3], left half
 * (uint8)((double)image * 255.0) of image float [B][3][H][W] (values outside [0, 1] clamped), right half lut[min((int)(p * 256.0f), 255)]
 * with lut uint8 [256][3] -- matplotlib's imsave of the reference's visualisation, byte for byte.  Any H, W, B >= 1; operands that are
 * not aligned for wide accesses (W % 4 != 0, an odd stride, an offset base pointer) take a scalar path. */
int fp_seg_pack(const float* logits, int64_t logit_batch_stride, const float* image, void* prob_half, float* prob_f32, uint8_t* picture,
                const uint8_t* lut, int32_t B, int32_t H, int32_t W, fp_stream_t stream);

/* ---- output stage of the main network's test-set inference (footprints/evaluation/inference.py:105-119; csrc/infer_pack.hip) ---- */
/* One launch over the logits pred float [B][4][H][W] that writes what fp_pack_pred_fp16 and fp_vis_side_by_side write in two, through the
 * same device functions: out_half float16 [B][4][H][W], bit-equal to fp_pack_pred_fp16 (sigmoid on channels 0 and 1); picture (NULL ok;
 * needs image float [B][3][H][W]) uint8 [B][H][2W][3], byte-equal to fp_vis_side_by_side (left half uint8(image * 255.0f), right half
 * colour1 where pred[:,1] > 0, colour0 elsewhere; a colour = r | g << 8 | b << 16).  image may be NULL without a picture.  Any H, W,
 * B >= 1; operands that are not aligned for wide accesses (W % 4 != 0, an offset base pointer) take a scalar path. */
int fp_infer_pack(const float* pred, const float* image, void* out_half, uint8_t* picture, uint32_t colour0, uint32_t colour1, int32_t B,
                  int32_t H, int32_t W, fp_stream_t stream);

/* ---- baseline JPEG encoder (csrc/jpeg.hip): the scan Pillow's Image.save(quality=q) writes for an RGB picture, byte for byte ---- */
typedef struct fp_jpeg_sample {
  int64_t offset; /* of the picture's first byte in `src`; dense uint8 [h][w][3] */
  int32_t h, w;   /* 1 .. 65535 each, and within the call's max_h, max_w */
} fp_jpeg_sample;
int32_t fp_jpeg_sample_bytes(void);
/* uint32 words of the code table the caller builds from a header of its own JPEG library: [2][64] quantisation values in zigzag order
 * (luma, chroma: as the DQT segments hold them), [2][16] DC categories and [2][256] AC run / size symbols as code | length << 16
 * (length 0 = no such symbol), luma before chroma. */
int32_t fp_jpeg_table_words(void);
/* Scratch of one call over B pictures of at most max_h x max_w, from the worst case of one block -- 20 DC bits and 63 AC terms of 26
 * bits -- for the unstuffed streams; int16 coefficients and a bit offset per block beside them.  -1 on bad arguments or when a stream
 * could pass 2^31 bits.  The second query is the largest output the B scans can need: that worst case doubled for byte stuffing. */
int64_t fp_jpeg_workspace_bytes(int32_t B, int32_t max_h, int32_t max_w);
int64_t fp_jpeg_max_scan_bytes(int32_t B, int32_t max_h, int32_t max_w);
/* Encodes B pictures of mixed sizes in one call: baseline sequential DCT, YCbCr 4:2:0 (luma 2x2, one interleaved scan), no restart
 * markers, the code table's Huffman codes as they are; libjpeg's integer colour conversion, h2v2 downsample with its alternating bias,
 * edge replication, jfdctint, quantiser and dummy blocks.  samples: B fp_jpeg_sample records on the device; tables: the code table on the
 * device.  out receives the entropy-coded scans of the accepted samples back to back (FF bytes stuffed, the last byte filled with
 * one-bits), neither header nor EOI; table: int64 [B + 1][2] on the device, row b = byte offset and length of sample b's scan in out, row
 * B = the bytes written in all and the status.  The status is cleared by the call and set to 1 when a record was turned down -- h or w
 * outside 1 .. 65535 or beyond max_h / max_w, an offset outside `src` -- or a scan did not fit into out_bytes; such a sample has length 0
 * and nothing of it is written.  Nothing waits for the device: read the table after the stream has finished. */
int fp_jpeg_encode(const uint8_t* src, int64_t src_bytes, const void* samples, const uint32_t* tables, uint8_t* out, int64_t out_bytes,
                   int64_t* table, int32_t B, int32_t max_h, int32_t max_w, void* workspace, int64_t workspace_bytes, fp_stream_t stream);

/* ---- baseline JPEG decoder (csrc/jpeg_decode.hip): PIL.Image.open(f).convert("RGB") of a baseline file, byte for byte ---- */
typedef struct fp_jpeg_decode_sample {
  int64_t scan_offset; /* of the entropy-coded segment (behind the SOS header, up to the EOI marker) in the scans buffer */
  int64_t out_offset;  /* of the picture's first byte in the output; dense uint8 [h][w][3] */
  int32_t scan_bytes;  /* of the segment, stuffed zero bytes included */
  int32_t h, w;
  int32_t ncomp;       /* 1: grey (the value three times), 3: YCbCr */
  int32_t hs, vs;      /* luma sampling factors: 1x1, 2x1 or 2x2; the chroma components are 1x1 */
  int32_t table_set;   /* index of the table block */
  int32_t reserved;
} fp_jpeg_decode_sample;
int32_t fp_jpeg_decode_sample_bytes(void);
/* words of one table block (uint32): [3][4] per component the quantisation table, the DC and the AC Huffman table it uses; at 16 [4][64]
 * quantisation values in natural order; at 272 four Huffman tables (DC 0, DC 1, AC 0, AC 1) of 356 words: [256] length << 8 | symbol of
 * the code 8 bits begin with (0: longer), [18] maxcode per length (-1: none), [18] valptr - mincode per length, [64] the symbols, four
 * to a word.  Built by the caller from the file's own DQT / DHT segments; nothing of a table is compiled in. */
int32_t fp_jpeg_decode_table_words(void);
int64_t fp_jpeg_decode_workspace_bytes(int32_t B, int32_t max_h, int32_t max_w, int32_t max_scan_bytes, int32_t subseq_bits);
/* Decodes B baseline scans (SOF0, 8 bits, one interleaved scan, no restart markers) into `out`, the packed layout fp_resize_u8,
 * fp_vis_overlay and fp_jpeg_encode read.  samples: B records on the device; tables: n_table_sets table blocks on the device.  A scan is
 * cut into subsequences of subseq_bits bits (32..2^20), one thread each, whose entry states are iterated to the serial decode's; the
 * synchronisation kernel is launched max_rounds times (64 hops inside each launch; a launch is a no-op for a settled sample).
 * status: int32 [B + 1] on the device, one per sample and their maximum: 0 decoded; 1 record turned down (sizes, an offset outside a
 * buffer, an unknown table set, an output that does not fit); 2 not settled within max_rounds; 3 corrupt stream.  A sample with a
 * non-zero status writes nothing into out.  The workspace begins with int32 [B][8] per sample: destuffed bytes, 1 + the last launch that
 * moved an entry state (so the launches the sample needed), the most hops of a launch, blocks found.  Does not wait for the device. */
int fp_jpeg_decode(const uint8_t* scans, int64_t scan_bytes, const void* samples, const uint32_t* tables, int32_t n_table_sets, uint8_t* out,
                   int64_t out_bytes, int32_t* status, int32_t B, int32_t max_h, int32_t max_w, int32_t max_scan_bytes, int32_t subseq_bits,
                   int32_t max_rounds, void* workspace, int64_t workspace_bytes, fp_stream_t stream);
/* One rectangle of a picture: fp_jpeg_decode_sample's fields, then the rectangle. */
typedef struct fp_jpeg_decode_window_sample {
  int64_t scan_offset;
  int64_t out_offset;  /* of the WINDOW's first byte in the output; dense uint8 [rh][rw][3] */
  int32_t scan_bytes;
  int32_t h, w;        /* of the picture */
  int32_t ncomp;
  int32_t hs, vs;
  int32_t table_set;
  int32_t reserved;
  int32_t y0, x0;      /* the rectangle's first row and column in the picture */
  int32_t rh, rw;      /* its size: 1 <= rh <= h - y0, 1 <= rw <= w - x0 */
} fp_jpeg_decode_window_sample;
int32_t fp_jpeg_decode_window_sample_bytes(void);
/* fp_jpeg_decode for one rectangle per sample: writes the bytes fp_jpeg_decode's picture has at [y0 : y0 + rh, x0 : x0 + rw], densely at
 * out_offset, and nothing else.  samples: B fp_jpeg_decode_window_sample records on the device.  The entropy half is fp_jpeg_decode's (a scan
 * has no random access); the inverse DCT runs on the blocks the rectangle needs -- the luma blocks that intersect it, the chroma blocks
 * that intersect its chroma footprint grown by one sample on every side -- and the colour pass on the rectangle's pixels: both grids are
 * sized by max_win_h x max_win_w (1..max_h, 1..max_w), the largest rectangle of the call.  The upsampler's edge rules are the picture's.
 * The workspace is fp_jpeg_decode_workspace_bytes' (the component planes stay frame-sized) and begins with the same counters.  status as
 * fp_jpeg_decode; 1 also for a rectangle that is empty, reaches outside its picture or is larger than max_win_h x max_win_w.  A sample
 * with a non-zero status writes nothing, and the other samples are unaffected.  Does not wait for the device. */
int fp_jpeg_decode_window(const uint8_t* scans, int64_t scan_bytes, const void* samples, const uint32_t* tables, int32_t n_table_sets,
                          uint8_t* out, int64_t out_bytes, int32_t* status, int32_t B, int32_t max_h, int32_t max_w, int32_t max_win_h,
                          int32_t max_win_w, int32_t max_scan_bytes, int32_t subseq_bits, int32_t max_rounds, void* workspace,
                          int64_t workspace_bytes, fp_stream_t stream);

/* ---- pyramid pooling of the ground-segmentation network (footprints/preprocessing/segmentation/network.py:174-207) ---- */
/* nn.AdaptiveAvgPool2d(P) (network.py:180,188): y[N][P][P][C] = window means of x[N][H][W][C]; windows floor(i*H/P) .. ceil((i+1)*H/P) */
int fp_adaptive_avgpool_fwd(const float* x, float* y, int32_t N, int32_t H, int32_t W, int32_t C, int32_t P, fp_stream_t stream);
/* its gradient: dx[N][H][W][C] (+)= sum over the windows containing the pixel of dy / window area */
int fp_adaptive_avgpool_bwd(const float* dy, float* dx, int32_t N, int32_t H, int32_t W, int32_t C, int32_t P, int accumulate,
                            fp_stream_t stream);
/* F.interpolate(size=(H,W), mode='bilinear', align_corners=True) (network.py:189) of src[N][P][P][C], written into channels
 * [c_off, c_off + C) of dst[N][H][W][dstC]: the torch.cat of network.py:207 is this channel offset */
int fp_bilinear_ac_fwd(const float* src, float* dst, int32_t N, int32_t P, int32_t C, int32_t H, int32_t W, int32_t dstC, int32_t c_off,
                       fp_stream_t stream);
/* its transpose: dsrc[N][P][P][C] = sum of weight * ddst[N][H][W][c_off + c] (plain store) */
int fp_bilinear_ac_bwd(const float* ddst, float* dsrc, int32_t N, int32_t P, int32_t C, int32_t H, int32_t W, int32_t dstC, int32_t c_off,
                       fp_stream_t stream);
/* dst[M][dst_off + c] (+)= src[M][src_off + c], c < C: channel-slice copy / add (the identity branch of the concatenation and its gradient) */
int fp_copy_channels(const float* src, float* dst, int64_t M, int32_t C, int32_t srcC, int32_t src_off, int32_t dstC, int32_t dst_off,
                     int accumulate, fp_stream_t stream);

/* ---- misc ---- */
int fp_nchw_to_nhwc(const float* x, float* y, int32_t N, int32_t C, int32_t H, int32_t W, fp_stream_t stream);
int fp_nhwc_to_nchw(const float* x, float* y, int32_t N, int32_t C, int32_t H, int32_t W, fp_stream_t stream);
int fp_fill(float* x, int64_t n, float value, fp_stream_t stream);

/* ---- loss of the ground-segmentation trainer (footprints/preprocessing/segmentation/train.py:184-193, evaluation.py:39-58) ----------
 * Forward and gradient in one call: preds[s] = logit map of scale s ([B][h_s][w_s], batch stride bstrides[s] elements -- a channel slice
 * of a wider tensor is fine), up-sized bilinearly (align_corners = False) to H x W, per-image masked BCE-with-logits means, averaged over
 * the four scales and the batch.  losses: 5 B + 1 floats = per image the four per-scale means [s * B + b], their average [4 B + b], and
 * the batch mean [5 B]; dpreds (nullable): d losses[5 B] / d preds[s], same addressing.  workspace >= fp_seg_loss_workspace(B, H, W). */
int64_t fp_seg_loss_workspace(int32_t B, int32_t H, int32_t W);
int fp_seg_loss_fwd_bwd(const float* const* preds, float* const* dpreds, const int32_t* hs, const int32_t* ws, const int64_t* bstrides,
                        const float* ground_mask, const float* loss_mask, int32_t B, int32_t H, int32_t W, float* losses, void* workspace,
                        int64_t workspace_bytes, fp_stream_t stream);

/* ---- data-parallel gradient exchange: RCCL over xGMI (the reference is single-GPU, README.md:128,136) -- */
/* One process per GPU.  Rank 0 obtains a unique id (fp_comm_unique_id_bytes() bytes, ncclUniqueId) and hands it to every rank by
 * any host transport; every rank then calls fp_comm_init on its own device (collective: returns when all `world` ranks called it).
 * fp_comm_allreduce_async sums `count` floats in place across the ranks, asynchronously on `stream` -- the caller orders that
 * stream behind the kernels that write the buffer (fp_event_record / fp_event_wait) -- and, while a launch plan records, is also
 * appended to the plan (fp_plan_replay re-issues it).  fp_comm_wait makes `consumer` wait for everything queued on `comm_stream`
 * so far.  RCCL is resolved at run time (dlopen); a box without librccl.so gets FP_EINVAL from these calls and nothing else of
 * the library is affected.  Errors: -100 - ncclResult_t. */
int32_t fp_comm_unique_id_bytes(void);
int fp_comm_unique_id(void* id_out, int32_t cap);
int fp_comm_init(const void* id_bytes, int32_t rank, int32_t world, void** comm_out);
int32_t fp_comm_version(void); /* ncclGetVersion, or -1 */
int32_t fp_comm_count(void* comm); /* ranks of the communicator as RCCL counts them (ncclCommCount) */
int fp_comm_allreduce_async(void* comm, float* buf, int64_t count, fp_stream_t stream);
int fp_comm_broadcast(void* comm, float* buf, int64_t count, int32_t root, fp_stream_t stream);
int fp_comm_wait(void* comm, fp_stream_t comm_stream, fp_stream_t consumer);
int fp_comm_destroy(void* comm);

/* ---- per-kernel timing: HIP events on the launch stream around every kernel launch of the library (bench.py roofline leg) ------ */
/* fp_ktime_begin starts collecting (eager launches and plan replays alike); fp_ktime_end stops, synchronises the device and
 * returns the number of distinct kernel symbols seen; fp_ktime_row(i) gives a symbol's demangled name, launch count and summed
 * event-to-event milliseconds -- the per-kernel quantity of `rocprofv3 --kernel-trace --stats`.  Single host thread. */
int fp_ktime_begin(void);
int32_t fp_ktime_end(void);
int fp_ktime_row(int32_t i, char* name, int32_t name_cap, int64_t* launches, double* total_ms);

/* measurement aid (bench.py --sustain): (shader cycles, constant-rate ticks) of each of the 8 XCDs into out16[xcc * 2 + {0, 1}] (device memory,
 * 16 uint64); the difference of two probes on one stream gives the shader clock the chip sustained in between: d cycles / d ticks x
 * fp_wall_clock_khz().  fp_wall_clock_khz: hipDeviceAttributeWallClockRate of the current device, -1 on error. */
int fp_clock_probe(uint64_t* out16, fp_stream_t stream);
int fp_wall_clock_khz(void);
/* Matrix-pipe probe (round 6; bench.py's roofline leg): ONE launch of 768 workgroups x 4 waves x iters x 24 v_mfma_f32_32x32x16_bf16 and nothing
 * else -- mode 0 constant operands, mode 1 pseudo-random bf16 operands (the operand buses toggle like on real activations).  out: 768 * 256
 * floats of scratch; clk2 (optional): {shader cycles, constant-rate ticks} of workgroup 0 across the launch (clock = cycles / ticks x
 * fp_wall_clock_khz).  fp_mfma_probe_flop(iters) = the FLOPs of one launch.  What it showed: 2.46 PFLOP/s at 2.39 GHz on constant data,
 * 1.85 PFLOP/s at 1.81 GHz on random data (profiles/round6_mfma_sustained_clock.txt) -- the chip's dense bf16 peak is a constant-data figure. */
int fp_mfma_probe(float* out, uint64_t* clk2, int32_t iters, int32_t mode, fp_stream_t stream);
double fp_mfma_probe_flop(int32_t iters);
int fp_version(void);
const char* fp_last_error_string(void);

#ifdef __cplusplus
}
#endif
#endif /* FOOTPRINTS_HIP_H */
