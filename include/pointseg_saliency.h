/* include/pointseg_saliency.h -- the saliency attention map in front of ps_volume_sample: the inference forward of the reference's
 * `unet3d_attention` network (dense 3-D convolutions, instance norm, channel and spatial attention) and the sliding-window average around
 * it (csrc/conv3d.hip, csrc/saliency.hip).  Same conventions as pointseg.h, pointseg_prepare.h and pointseg_postprocess.h (status codes,
 * ps_last_error, caller-owned device buffers, the context's stream); kept out of pointseg.h because a host that is handed its attention
 * volume never needs it.  All citations are relative to the reference repository root.
 *
 * What each entry point replaces
 * ------------------------------
 *   ps_conv3d                 tf.layers.conv3d(inputs, filters, kernel_size, strides, dilation_rate, padding="SAME", use_bias,
 *                             data_format="channels_last") without its activation, SaliencyAttention/model.py:139-174, 182-307, 356-386 and
 *                             attention.py:82-141; optionally behind tf.concat([a, b], axis=-1) (model.py:251, 280, 298) and / or
 *                             tf.keras.layers.UpSampling3D(size) (model.py:316-317) of its input, neither of them materialised
 *   ps_instance_norm_relu     BN_Relu with config.INSTANCE_NORM: InstanceNorm5d then tf.nn.relu, SaliencyAttention/model.py:366-372,
 *                             custom_ops.py:29-82
 *   ps_saliency_weight_count  (the length of the weight buffer below)
 *   ps_saliency_forward       unet3d_attention(inputs) and final_probs = tf.nn.softmax(logits), SaliencyAttention/model.py:176-314,
 *                             attention.py:79-174, train.py:116
 *   ps_saliency_accumulate    `whole_pred[window] += pred[0, inside]; count_used[window] += 1`, SaliencyAttention/eval.py:168-174
 *   ps_saliency_finish        `whole_pred / count_used`, SaliencyAttention/eval.py:176-177
 *
 * Common to all.  Every tensor is device memory, float32, dense and row-major.  An activation is [B, D, H, W, C] (channels last, the
 * reference's DATA_FORMAT), a kernel is TensorFlow's [kd, kh, kw, C_in, C_out].
 * padding="SAME", per axis: out = ceil(in / stride); pad_total = max((out - 1) * stride + (k - 1) * dilation + 1 - in, 0);
 * pad_before = pad_total / 2 (rounded down), the rest behind -- a stride-2 convolution of an even extent pads 0 in front and 1 behind.
 * Scratch: the two-call protocol of ps_volume_zoom -- scratch == NULL only fills *scratch_bytes, from the shapes alone: the tensor pointers
 * and the context are not looked at and may be NULL, every other argument is checked as in the second call.  The second call takes device
 * memory of at least that size, 256-byte aligned, valid until the stream has passed the call.
 * Asynchronous on the context's stream, no synchronisation, no host read, no allocation.  Every argument error returns PS_EINVAL before
 * anything is enqueued.  Products run on the fp32 matrix pipe (exact fp32 operands, fp32 accumulation); the instance-norm statistics are
 * float64 partial sums added in one fixed order; nothing uses a float atomic: two runs give the same bytes.
 */
#ifndef POINTSEG_SALIENCY_H
#define POINTSEG_SALIENCY_H

#include "pointseg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- one 3-D convolution -------------------------------------------------------------------------------------------------------------------
 * y[b, od, oh, ow, :] = bias + sum over taps and input channels of in[b, od * stride - pad + t * dilation, ..., :] . w[t, :, :]
 * with taps outside the input reading 0 (no padded copy is made).
 *   x        [B, Ds, Hs, Ws, C1]; x2: NULL (C2 == 0) or [B, Ds, Hs, Ws, C2], the second part of a channel concat: C_in = C1 + C2
 *   up       >= 1: the convolution's input is x (and x2) up-sampled `up` times per axis by repetition -- its extents are
 *            D = Ds * up, H = Hs * up, W = Ws * up, and input voxel (d, h, w) is read from (d / up, h / up, w / up)
 *   w        [kd, kh, kw, C_in, C_out], every kernel extent one of 1, 3, 9;  bias: [C_out] or NULL
 *   stride   1 or 2 (all three axes);  dilation: 1, 3, 5 or 7 (all three axes)
 *   y        [B, ceil(D / stride), ceil(H / stride), ceil(W / stride), C_out]; must not overlap x or x2
 * 1 <= C_in <= 384, 1 <= C_out <= 256, every extent >= 1, and every tensor below 2^31 elements per sample.  No scratch. */
int ps_conv3d(ps_context* ctx, const void* x, const void* x2, int64_t B, int64_t Ds, int64_t Hs, int64_t Ws, int64_t C1, int64_t C2, int32_t up,
              const void* w, const void* bias, int32_t kd, int32_t kh, int32_t kw, int64_t C_out, int32_t stride, int32_t dilation, void* y);

/* ---- instance norm + ReLU ------------------------------------------------------------------------------------------------------------------
 * y[b, v, c] = max(0, (x[b, v, c] - mean[b, c]) * rsqrt(var[b, c] + eps) * gamma[c] + beta[c]), mean and the BIASED variance (tf.nn.moments)
 * per sample and channel over the V voxels.  x, y: [B, V, C]; y may be x (in place).  gamma, beta: [C].  eps > 0 (the reference: 1e-5).
 * V < 2^31, 1 <= C <= 1024.  The sums are float64, so the variance survives a mean far larger than the deviation.
 * Scratch: the per-workgroup partial sums, 16 bytes per (slab of 4096 voxels, sample, channel), and the totals. */
int ps_instance_norm_relu(ps_context* ctx, const void* x, int64_t B, int64_t V, int64_t C, const void* gamma, const void* beta, float eps, void* y,
                          void* scratch, int64_t* scratch_bytes);

/* ---- the whole network -----------------------------------------------------------------------------------------------------------------------
 * The weight buffer: float32, ps_saliency_weight_count(C_in, num_classes) values, the layers below in this order; per layer the kernel
 * [kd, kh, kw, cin, cout], then the bias [cout] where the layer has one, then gamma [cout] and beta [cout] where it has the norm.
 * (name under unet3d_attention/, kernel extents, cin -> cout, B = bias, N = instance norm + ReLU)
 *   init_conv                        3 3 3  C_in -> 16   B N
 *   for d = 0 .. 4, w = 16 << d:
 *     down{d}_conv_0, down{d}_conv_1 3 3 3  w -> w       B N      (the block's input is added after the second one's norm + ReLU)
 *     stride2conv{d}   (d < 4)       3 3 3  w -> 2w      B N      stride 2
 *   C1_conv                          3 3 3  16 -> 64     B N      on down_list[0]
 *   C2_conv                          3 3 3  32 -> 64     B N      on down_list[1]
 *   for p, cin in (C3_cfe, 64), (C4_cfe, 128), (C5_cfe, 256), on down_list[2], [3], [4]:
 *     {p}_cfe0                       1 1 1  cin -> 32      N
 *     {p}_cfe1_dilation, _cfe2_, _cfe3_   3 3 3  cin -> 32   N      dilation 3, 5, 7     (concatenated in this order: 128 channels)
 *   up_conv1_C5_cfe_up4              3 3 3  128 -> 128   B N      on C5_cfe up-sampled x 4
 *   up_conv1_C4_cfe_up2              3 3 3  128 -> 128   B N      on C4_cfe up-sampled x 2     (C345 = [C3_cfe, C4, C5]: 384 channels)
 *   C345_ChannelWiseAttention_withcpfe_dense_1   kernel [384, 96], bias [96]     ReLU, on the mean over the voxels
 *   C345_ChannelWiseAttention_withcpfe_dense_2   kernel [96, 384], bias [384]    sigmoid; scales the channels of C345
 *   C345_conv                        1 1 1  384 -> 64    B N
 *   up_conv1_C345_up4                3 3 3  64 -> 64     B N      on that, up-sampled x 4 (full resolution)
 *   for i = 1, 2, 3, (a, b) = ((1,9,9), (9,1,1)), ((9,1,9), (1,9,1)), ((9,9,1), (1,1,9)):
 *     spatial_attention_{i}_conv1    a      64 -> 32     B N
 *     spatial_attention_{i}_conv2    b      32 -> 1      B N      (SA = sigmoid of the sum of the three)
 *   up_conv1_C2_up2                  3 3 3  64 -> 64     B N      on C2 up-sampled x 2
 *   C12_conv                         3 3 3  128 -> 64    B N      on [C1, C2]; its result is multiplied by SA
 *   final                            3 3 3  128 -> num_classes  B     on [C12, C345]: the logits
 */
int64_t ps_saliency_weight_count(int64_t C_in, int64_t num_classes); /* -1 on a bad argument */

/* Activations a caller may ask for next to the result (tests); each pointer NULL or a dense tensor of the stated shape. */
typedef struct ps_saliency_taps {
    void* down4;  /* [B, D/16, H/16, W/16, 256]  down_list[4] */
    void* c345;   /* [B, D, H, W, 64]            C345 behind up_conv1_C345_up4 */
    void* sa;     /* [B, D, H, W]                the spatial attention (one channel; the reference tiles it over 64) */
    void* c12;    /* [B, D, H, W, 64]            C12 behind the multiplication */
} ps_saliency_taps;

/* x [B, D, H, W, C_in] -> logits and / or probs (softmax over the classes), each [B, D, H, W, num_classes] or NULL (at least one of them is given).
 * D, H and W must be multiples of 16 (four stride-2 convolutions, whose results are up-sampled back by 2 and 4), 1 <= C_in <= 16,
 * 2 <= num_classes <= 16, and per sample D * H * W * 128 < 2^31.  taps may be NULL.
 * With instance norm the samples of a batch do not see each other: B = 2 gives what two B = 1 calls give.
 * Scratch: every activation of the graph (about 340 floats per full-resolution voxel: 2.2 GB for one [64, 160, 160] patch). */
int ps_saliency_forward(ps_context* ctx, const void* x, int64_t B, int64_t D, int64_t H, int64_t W, int64_t C_in, int64_t num_classes,
                        const void* weights, int64_t weight_count, void* logits, void* probs, const ps_saliency_taps* taps, void* scratch,
                        int64_t* scratch_bytes);

/* ---- the window average ----------------------------------------------------------------------------------------------------------------------
 * ps_saliency_accumulate: sum[o0 + i, o1 + j, o2 + k, :] += probs[i, j, k, :] and count[o0 + i, o1 + j, o2 + k] += 1 for the part of the
 * window inside the volume (eval.py:168-174).  probs: [p0, p1, p2, C] float32; sum: [D, H, W, C] float32; count: [D, H, W] int32; the
 * caller zeroes sum and count before the first window.  0 <= o < extent per axis, 1 <= C <= 16.  No scratch.
 * ps_saliency_finish: out[v, :] = sum[v, :] / count[v] (eval.py:176-177); out may be sum.  A voxel no window covered (count 0) gives 0.
 * The window loop around these two has an entry of its own: ps_saliency_map (pointseg_saliency_map.h), with the views, the flip and the fusion. */
int ps_saliency_accumulate(ps_context* ctx, const void* probs, int64_t p0, int64_t p1, int64_t p2, int64_t C, int64_t o0, int64_t o1, int64_t o2,
                           int64_t D, int64_t H, int64_t W, void* sum, void* count);
int ps_saliency_finish(ps_context* ctx, const void* sum, const void* count, int64_t D, int64_t H, int64_t W, int64_t C, void* out);

#ifdef __cplusplus
}
#endif

#endif /* POINTSEG_SALIENCY_H */
