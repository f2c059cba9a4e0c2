/* include/pointseg_saliency_precision.h -- a choice of arithmetic for the saliency attention network's INFERENCE convolutions: the fp32
 * matrix pipe (what pointseg_saliency.h's entries run), exact three-way bfloat16 splits on the bf16 matrix pipe, or one plane of rounded
 * bfloat16 (csrc/conv3d_bf16.hip; the fp32 kernel stays csrc/conv3d.hip).  Same conventions as pointseg_saliency.h, whose ps_conv3d and
 * ps_saliency_forward these two entries extend: every argument before `precision` is theirs, with their limits, their checks, their
 * two-call scratch protocol and their scratch SIZE (the same number of bytes in every mode).  ps_conv3d is ps_conv3d_prec(..., PS_PREC_FP32)
 * and ps_saliency_forward is ps_saliency_forward_prec(..., PS_PREC_FP32): one body each.  In training, the convolution's two
 * gradients take the same choice op by op (pointseg_saliency_train_precision.h), the one-call step per role (pointseg_saliency_step_precision.h).
 *
 * The rule, for every convolution of the call
 * -------------------------------------------
 *   PS_PREC_FP32    what the library did before this header: the fp32 kernel, the same bytes.
 *   PS_PREC_BF16X3  an fp32-level result.  Both operands are split EXACTLY into three bfloat16 pieces by truncation (x1 = x with its low 16
 *                   bits cleared, x2 = (x - x1) likewise, x3 = x - x1 - x2; x1 + x2 + x3 == x), and of the nine piece products the six
 *                   with piece indices i + j <= 4 are multiplied on the bf16 matrix pipe and accumulated in fp32 -- the dropped ones are
 *                   below 2^-25 of the product.  The promise is the accuracy class (the error bars of pointseg_saliency.h's entries), not
 *                   the kernel: a layer may run on the fp32 kernel under this value where the split form is slower.
 *   PS_PREC_BF16    every operand element is rounded ONCE to bfloat16, round to nearest even; the products of the rounded elements are
 *                   exact, the accumulation is fp32, the bias is added in fp32.
 * Any other value returns PS_EINVAL before anything is enqueued (also in the call that only sizes the scratch).
 *
 * The operand elements that are split or rounded:
 *   the activation as the convolution fetches it -- through the fused channel concat and the nearest up-sampling, which copy values and so
 *   commute with the rounding; a tap in the SAME padding stays 0;
 *   the kernel as the convolution receives it.  For C345_conv that is the PER-SAMPLE kernel into which the channel attention has folded its
 *   scale, fl32(scale[b, ci] * w[ci, co]): formed in fp32, then split or rounded.  A float64 restatement of PS_PREC_BF16 must round the same
 *   two things -- C345's activation and that fp32 product -- and not the scaled activation.
 * Everything else keeps its arithmetic in every mode: activations stay float32 in memory, the instance norm's float64 fixed-order sums, the
 * channel attention's two dense layers, the spatial gate, the softmax, the window average.
 * A chunk of 32 k is summed in a fresh accumulator that is then added to the running one, as in the fp32 kernel; nothing uses a float atomic:
 * two runs of any mode give the same bytes, and B = 2 gives what two B = 1 calls give.
 */
#ifndef POINTSEG_SALIENCY_PRECISION_H
#define POINTSEG_SALIENCY_PRECISION_H

#include "pointseg_saliency.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { PS_PREC_FP32 = 0, PS_PREC_BF16X3 = 1, PS_PREC_BF16 = 2 };

/* ps_conv3d (pointseg_saliency.h) at the given precision.  No scratch.  The 16-byte activation fetch is taken where C1 and C2 are multiples
 * of 4 and x, x2 are 16-byte aligned; every other case takes the 4-byte fetch, with the same result. */
int ps_conv3d_prec(ps_context* ctx, const void* x, const void* x2, int64_t B, int64_t Ds, int64_t Hs, int64_t Ws, int64_t C1, int64_t C2, int32_t up,
                   const void* w, const void* bias, int32_t kd, int32_t kh, int32_t kw, int64_t C_out, int32_t stride, int32_t dilation, void* y,
                   int32_t precision);

/* ps_saliency_forward (pointseg_saliency.h) with every convolution at the given precision. */
int ps_saliency_forward_prec(ps_context* ctx, const void* x, int64_t B, int64_t D, int64_t H, int64_t W, int64_t C_in, int64_t num_classes,
                             const void* weights, int64_t weight_count, void* logits, void* probs, const ps_saliency_taps* taps, void* scratch,
                             int64_t* scratch_bytes, int32_t precision);

#ifdef __cplusplus
}
#endif

#endif /* POINTSEG_SALIENCY_PRECISION_H */
