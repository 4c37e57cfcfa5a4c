// What the forward / data-gradient convolution files share on the host: the epilogue operands as one value, and every host function
// one of these files defines for another.  (The rule for BatchNorm side outputs sits next to FpBnSink in fp_common.h.)
#pragma once
#include "fp_common.h"

// the optional operands of a convolution's epilogue (FP_EPI_* / FP_ACT_* of the header) and its output
struct FpConvEpilogue {
  const float* bias;
  const float* addend;
  const float* addend_mask;
  const float* actsrc;
  float* y;
  int act;
  unsigned epi;
};

// (a null descriptor, which the entry point rejects next, gives no flags)
static inline FpConvEpilogue fp_conv_epilogue_of(const fp_conv_desc* d, const float* bias, const float* addend, const float* addend_mask,
                                                 const float* actsrc, float* y) {
  return FpConvEpilogue{bias, addend, addend_mask, actsrc, y, d ? d->act : 0, d ? d->epi : 0u};
}

// every epilogue flag of the descriptor has its operand
static inline int fp_conv_check_epilogue(const char* who, const fp_conv_desc* d, const FpConvEpilogue& e) {
  FP_REQUIRE(!(d->epi & FP_EPI_BIAS) || e.bias, "%s: bias flag without pointer", who);
  FP_REQUIRE(!(d->epi & FP_EPI_ADDEND) || e.addend, "%s: addend flag without pointer", who);
  FP_REQUIRE(!(d->epi & FP_EPI_ADDEND_MASK) || e.addend_mask, "%s: addend_mask flag without pointer", who);
  FP_REQUIRE(!(d->epi & (FP_EPI_ACTGRAD_ELU | FP_EPI_ACTGRAD_RELU)) || e.actsrc, "%s: actgrad flag without pointer", who);
  return FP_OK;
}

// conv_igemm.hip: the one finish of a split grid, y = epilogue(sum over the SK raw partial copies part[SK][M][Nout]) in a fixed order, by
// exactly one reduce launch.  `sink` (null: this site never emits) is offered the BatchNorm partials of y: the backward sums where
// fp_bn_sink_bwd_ok, else the statistics where fp_bn_sink_fwd_ok -- one block of partials per block of the reduce grid, claimed with
// fp_bn_sink_claim -- and the plain reduce runs where neither holds, the shape has no such grid or the capacity is too small.  `amax_out`
// (or null) receives max |y|.  Returns the launch status.
int fp_splitk_finish(const char* who, const float* part, int SK, int64_t M, int Nout, const FpConvEpilogue& e, int gather, unsigned* amax_out,
                     const FpBnSink* sink, hipStream_t stream);

// stem_tile.hip / conv3x3_tile.hip: the kernels fp_conv_igemm hands a problem to first; -1000 = not handled (it runs the flattened kernel)
int fp_stem_tile_dispatch(const fp_conv_desc* d, const float* img, const float* wpacked, const float* bias, float* y, hipStream_t stream,
                          const FpBnSink& sink);
int fp_conv3x3_tile_dispatch(const fp_conv_desc* d, const float* src0, const float* src1, const float* wpacked, const float* bias,
                             const float* addend, const float* addend_mask, const float* actsrc, float* y, hipStream_t stream);
