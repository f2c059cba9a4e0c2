/* include/pointseg_saliency_train.h -- the gradients of the two layers that hold almost all of the saliency attention network's
 * arithmetic: the 3-D convolution (data, weight and bias gradient) and instance norm + ReLU (csrc/conv3d_train.hip, csrc/saliency_train.hip).  Same conventions as
 * pointseg_saliency.h (status codes, ps_last_error, caller-owned device buffers, the context's stream, the two-call scratch protocol);
 * kept out of it because a host that only runs the network never needs them.  All citations are relative to the reference repository root.
 *
 * What each entry point replaces
 * ------------------------------
 * The reference never writes these gradients down: SaliencyAttention/train.py:50-56, 83-110 returns total_cost and a
 * tf.train.MomentumOptimizer, and TensorFlow differentiates the graph -- tf.gradients through every tf.layers.conv3d and InstanceNorm5d
 * of SaliencyAttention/model.py:139-174, 356-386 and custom_ops.py:29-82.
 *   ps_conv3d_bwd_data        the gradient tf.gradients sends through tf.layers.conv3d to its input, behind the tf.concat and the
 *                             UpSampling3D that ps_conv3d fuses (their gradients: the channel split and the sum over the repeated voxels)
 *   ps_conv3d_bwd_weight      the gradients of the layer's `kernel` and `bias` variables
 *   ps_instance_norm_relu_bwd the gradients through tf.nn.relu and InstanceNorm5d (tf.nn.moments, gamma, beta) of BN_Relu
 *
 * Common to all.  Tensors, layouts, SAME padding, limits and the scratch protocol are pointseg_saliency.h's: scratch == NULL only fills
 * *scratch_bytes, from the shapes alone (the tensor pointers and the context are not looked at and may be NULL); the second call takes
 * device memory of at least that size, 256-byte aligned.  Asynchronous on the context's stream, no synchronisation, no host read, no
 * allocation.  Every argument error returns PS_EINVAL, with ps_last_error naming the function, before anything is enqueued.  Results
 * are overwritten, never accumulated.  Products run on the fp32 matrix pipe (exact fp32 operands, fp32 accumulation, a fresh accumulator
 * per chunk of 32 products added to the running one); every sum over voxels, slabs and samples is made in one fixed order, the norm's
 * in float64; nothing uses a float atomic: two runs give the same bytes.
 */
#ifndef POINTSEG_SALIENCY_TRAIN_H
#define POINTSEG_SALIENCY_TRAIN_H

#include "pointseg_saliency.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the convolution's data gradient ---------------------------------------------------------------------------------------------------------
 * The geometry is ps_conv3d's: the convolution's input is the channel concat of x [B, Ds, Hs, Ws, C1] and x2 [.., C2] up-sampled `up`
 * times by repetition (extents D = Ds * up, ...), its output [B, Do, Ho, Wo, C_out] with Do = ceil(D / stride), ...
 *   dy       [B, Do, Ho, Wo, C_out];  w: the forward's kernel [kd, kh, kw, C1 + C2, C_out]
 *   dx       [B, Ds, Hs, Ws, C1];  dx2: [B, Ds, Hs, Ws, C2].  With C2 == 0 dx2 must be NULL (and dx given); otherwise either may be NULL,
 *            not both.  Neither may overlap dy.
 * For a voxel i of the virtual (concatenated, up-sampled) input and its channel ci
 *   g[i, ci] = sum over taps t and co of dy[o, co] . w[t, ci, co]   with i = o * stride - pad_before + t * dilation on every axis;
 * terms whose o is no whole number or lies outside the output are absent.  A source voxel gets the sum of g over its up^3 virtual voxels,
 * added in one fixed order; channels below C1 go to dx, the others to dx2.
 * Scratch: a transposed copy of the kernel (kd * kh * kw * C_in * C_out floats) and, with up > 1, g (B * D * H * W * C_in floats). */
int ps_conv3d_bwd_data(ps_context* ctx, const void* dy, const void* w, int64_t B, int64_t Ds, int64_t Hs, int64_t Ws, int64_t C1, int64_t C2, int32_t up,
                       int32_t kd, int32_t kh, int32_t kw, int64_t C_out, int32_t stride, int32_t dilation, void* dx, void* dx2, void* scratch,
                       int64_t* scratch_bytes);

/* ---- the convolution's weight and bias gradient ----------------------------------------------------------------------------------------------
 *   dw[t, ci, co] = sum over b and output voxels o of in[b, o * stride - pad_before + t * dilation, ci] . dy[b, o, co]
 *   dbias[co]     = sum over b and o of dy[b, o, co]
 * with `in` fetched exactly as ps_conv3d fetches it (x and x2 concatenated, coordinate / up, 0 in the padding; never materialised).
 *   x, x2    as ps_conv3d's (x2 given exactly when C2 > 0);  dy: [B, Do, Ho, Wo, C_out]
 *   dw       [kd, kh, kw, C1 + C2, C_out] or NULL;  dbias: [C_out] or NULL; not both NULL
 * The sum runs over slabs of 4096 output voxels of one sample; the slabs' partial sums (float32) are added in one fixed order in float64.
 * Scratch: those partials, B * ceil(Do * Ho * Wo / 4096) * (kd * kh * kw * C_in + 1) * C_out floats. */
int ps_conv3d_bwd_weight(ps_context* ctx, const void* x, const void* x2, const void* dy, int64_t B, int64_t Ds, int64_t Hs, int64_t Ws, int64_t C1, int64_t C2,
                         int32_t up, int32_t kd, int32_t kh, int32_t kw, int64_t C_out, int32_t stride, int32_t dilation, void* dw, void* dbias,
                         void* scratch, int64_t* scratch_bytes);

/* ---- instance norm + ReLU ----------------------------------------------------------------------------------------------------------------------
 *   x        [B, V, C], the layer's input;  y: [B, V, C], ps_instance_norm_relu's output, used only as the ReLU mask y > 0 (a trainer keeps y
 *            anyway, it is the next layer's input; and the mask is then an input, not something that depends on rounding)
 *   dy       [B, V, C];  gamma: [C];  eps > 0
 * With g = dy where y > 0 and 0 elsewhere, and xhat = (x - mean) * rsqrt(var + eps) from x's own mean and BIASED variance per (sample, channel):
 *   dbeta[c]  = sum over b and v of g
 *   dgamma[c] = sum over b and v of g . xhat
 *   dx        = gamma * rsqrt(var + eps) * (g - mean_v(g) - xhat * mean_v(g . xhat))      per (sample, channel)
 * All five sums (x, x^2, g, g . xhat over the voxels, and the two over the samples) are float64 partials added in one fixed order.
 * dx: [B, V, C], may be dy (in place), must not be x or y;  dgamma, dbeta: [C].  Each result may be NULL, not all three.
 * At V == 1 the variance is 0 and dx is exactly 0.  Limits as ps_instance_norm_relu.
 * Scratch: 16 bytes per (slab of 4096 voxels, sample, channel) and three totals of that size per (sample, channel). */
int ps_instance_norm_relu_bwd(ps_context* ctx, const void* x, const void* y, const void* dy, int64_t B, int64_t V, int64_t C, const void* gamma, float eps,
                              void* dx, void* dgamma, void* dbeta, void* scratch, int64_t* scratch_bytes);

#ifdef __cplusplus
}
#endif

#endif /* POINTSEG_SALIENCY_TRAIN_H */
