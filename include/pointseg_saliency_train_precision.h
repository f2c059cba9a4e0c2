/* include/pointseg_saliency_train_precision.h -- a choice of arithmetic for the two gradients of the saliency attention network's 3-D
 * convolution: the fp32 matrix pipe (what pointseg_saliency_train.h's entries run; csrc/conv3d_train.hip), exact three-way bfloat16 splits on
 * the bf16 matrix pipe, or one plane of rounded bfloat16 (csrc/conv3d_bf16.hip's kernel with its gather policy for the data gradient,
 * csrc/conv3d_train_bf16.hip for the weight gradient).  The values of `precision` are pointseg_saliency_precision.h's PS_PREC_*.
 *
 * Same conventions as pointseg_saliency_train.h, whose ps_conv3d_bwd_data and ps_conv3d_bwd_weight these two entries extend: every argument
 * before `precision` is theirs, with their limits, their checks, their two-call scratch protocol and their scratch SIZE (the same number of
 * bytes in every mode).  ps_conv3d_bwd_data is ps_conv3d_bwd_data_prec(..., PS_PREC_FP32) and ps_conv3d_bwd_weight is
 * ps_conv3d_bwd_weight_prec(..., PS_PREC_FP32): one body each, the same bytes as before this header.  Any other value than the three
 * returns PS_EINVAL before anything is enqueued, also in the call that only sizes the scratch (*scratch_bytes is then left alone).
 * The instance norm's gradient stays fp32.  The one-call training step takes one precision per role: pointseg_saliency_step_precision.h.
 *
 * The rule
 * --------
 * An operand element is split (PS_PREC_BF16X3: the exact truncating three-way split, the six piece products with piece indices i + j <= 4,
 * fp32 accumulation) or rounded once to bfloat16, round to nearest even (PS_PREC_BF16: exact products of the rounded elements, fp32
 * accumulation), as pointseg_saliency_precision.h defines both.  Under PS_PREC_BF16X3 the promise is the accuracy class (the error bars of
 * pointseg_saliency_train.h's entries), not the kernel: a layer form may run on the fp32 kernel where the split form is measured slower.
 * Under PS_PREC_BF16 every form runs the rounded arithmetic, the stride-2 data gradient included, because the result differs.
 *
 * Data gradient.  The operands are dy as the gather fetches it and the kernel w as given; an absent term (an o that is no whole number or
 * lies outside the output) stays 0.  The sum over a source voxel's up^3 virtual voxels and the column split at C1 stay fp32, in the fp32
 * entry's fixed order.
 * Weight and bias gradient.  The operands are `in` as ps_conv3d fetches it (the concat and the up-sampling copy values and so commute with
 * the rounding; a padding tap is 0) and dy.  dbias is still the product with the row of ones: under PS_PREC_BF16 it is therefore the sum of
 * the ROUNDED dy; under PS_PREC_BF16X3 it is the sum of dy itself, because 1 is one piece and the split of dy is exact.  The slab partials
 * stay float32 per slab of 4096 output voxels and are added in one fixed order in float64, by the fp32 entry's reduction.
 * Both.  A chunk of 32 k is summed in a fresh accumulator that is then added to the running one; nothing uses a float atomic: two runs of
 * any mode give the same bytes, and the data gradient at B = 2 gives what two B = 1 calls give.
 */
#ifndef POINTSEG_SALIENCY_TRAIN_PRECISION_H
#define POINTSEG_SALIENCY_TRAIN_PRECISION_H

#include "pointseg_saliency_precision.h"
#include "pointseg_saliency_train.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ps_conv3d_bwd_data (pointseg_saliency_train.h) at the given precision.  The 16-byte fetch of dy is taken where C_out is a multiple of 4
 * and dy is 16-byte aligned; every other case takes the 4-byte fetch under PS_PREC_BF16, with the same result, and the fp32 kernel under
 * PS_PREC_BF16X3 (measured faster there than the split form; the weight gradient likewise runs the fp32 kernel under PS_PREC_BF16X3 below
 * 64 input or 32 output channels). */
int ps_conv3d_bwd_data_prec(ps_context* ctx, const void* dy, const void* w, int64_t B, int64_t Ds, int64_t Hs, int64_t Ws, int64_t C1, int64_t C2,
                            int32_t up, int32_t kd, int32_t kh, int32_t kw, int64_t C_out, int32_t stride, int32_t dilation, void* dx, void* dx2,
                            void* scratch, int64_t* scratch_bytes, int32_t precision);

/* ps_conv3d_bwd_weight (pointseg_saliency_train.h) at the given precision. */
int ps_conv3d_bwd_weight_prec(ps_context* ctx, const void* x, const void* x2, const void* dy, int64_t B, int64_t Ds, int64_t Hs, int64_t Ws, int64_t C1,
                              int64_t C2, int32_t up, int32_t kd, int32_t kh, int32_t kw, int64_t C_out, int32_t stride, int32_t dilation, void* dw,
                              void* dbias, void* scratch, int64_t* scratch_bytes, int32_t precision);

#ifdef __cplusplus
}
#endif

#endif /* POINTSEG_SALIENCY_TRAIN_PRECISION_H */
