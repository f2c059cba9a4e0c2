/* include/pointseg_forward_precision.h -- a choice of arithmetic for the matrix products of the point network's INFERENCE forward
 * (ps_randla_forward, pointseg.h; csrc/randla.hip), per network.  The values are pointseg_saliency_precision.h's PS_PREC_* (one definition):
 *
 *   PS_PREC_BF16X3  the default: what ps_randla_forward ran before this header, the same dispatch and the same bytes.  Its matrix products at
 *                   d_out >= 64 run on the bf16 matrix pipe over exact three-way bfloat16 splits (fp32-level error) or, with the context's
 *                   ps_set_att_bf16x3(ctx, 0), on the fp32 matrix pipe.
 *   PS_PREC_BF16    the products named below take BOTH operands rounded ONCE to bfloat16, round to nearest even; products of the rounded
 *                   elements are exact, the accumulation is fp32.  The context's att_bf16x3 switch has no say at this value.
 *   PS_PREC_FP32 and any other value: PS_EINVAL (the fp32 MFMA forms stay a switch of the context: ps_set_att_bf16x3).
 *
 * The rule of PS_PREC_BF16 is one on shapes, never on the row count or on which kernel takes a product:
 *   dense layers and 1x1 convolutions outside the attention kernels (mlp1, the two att_pooling mlps, [mlp2 ; shortcut], decoder_0, the
 *     decoder steps, fc1, fc2, fc): rounded iff the K axis -- for a concatenated input the summed width -- is a multiple of 16 and at
 *     least 32.  fc0 never.
 *   inside an attention stage (LFA mlp2 h -> h; the score product, both halves: the pre-product G = f . Wfc[:h] that the layer in front
 *     computes, and f_xyz . Wfc[h:] in the kernel): rounded iff the 32x32 attention kernels serve the level (d_out 64 .. 512, K 16 or 32,
 *     rows below 2^24 and below 4 GiB of [f | G]); any other stage, its G included, runs as at the default.
 *   never rounded: the LocSE convolution (10 -> h: positions at 8 bits would quantise the volume; it stays on the exact split), bias,
 *     LeakyReLU, softmax, the value side of the weighted sum (fp32 features), max-pool, gathers.  Every stored activation stays float32.
 * The weight element that is rounded is the float32 the default images hold: the BatchNorm-folded weight; for Wfc[h:] the fold times log2(e)
 * (the kernels' softmax is exp2), for Wfc[:h] the weight itself.
 * Two forwards give the same bytes; B = 2 gives what two B = 1 forwards give up to the summation order of the deep dense layers, whose K
 * split follows the row count (as at the default); setting PS_PREC_BF16X3 again gives the default's bytes.
 *
 * The one-plane weight images of PS_PREC_BF16 are packed by the first forward at that value (2 bytes per weight and image), live next to the
 * default ones, are dropped by ps_randla_set_weights (and packed again on demand) and freed by ps_randla_destroy.
 */
#ifndef POINTSEG_FORWARD_PRECISION_H
#define POINTSEG_FORWARD_PRECISION_H

#include "pointseg.h"
#include "pointseg_saliency_precision.h" /* PS_PREC_FP32 / PS_PREC_BF16X3 / PS_PREC_BF16 */

#ifdef __cplusplus
extern "C" {
#endif

/* precision: PS_PREC_BF16X3 or PS_PREC_BF16; anything else returns PS_EINVAL and leaves the network as it was.  Takes effect with the next
 * ps_randla_forward; may be called before or after ps_randla_set_weights. */
int ps_randla_set_precision(ps_randla* net, int32_t precision);
int ps_randla_get_precision(const ps_randla* net, int32_t* precision);

#ifdef __cplusplus
}
#endif

#endif /* POINTSEG_FORWARD_PRECISION_H */
