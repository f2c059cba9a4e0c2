/* include/pointseg_saliency_step.h -- the training step of the saliency attention network behind one call (csrc/saliency_step.hip): the
 * training-mode forward of unet3d_attention, softmax + weighted Dice, the whole backward, an optional gradient all-reduce through the
 * host's callback, and the momentum update -- no Python, no torch and no tape in the loop.  The step is a graph walker over the ops of
 * pointseg_saliency.h, pointseg_saliency_train.h and pointseg_saliency_attention.h: the kernels are theirs, what is new is the copy /
 * add kernel that builds and splits the concats and sums the gradients of a tensor several layers read, and the update.
 * All citations are relative to the reference repository root.
 *
 * What each entry point replaces
 * ------------------------------
 *   ps_saliency_backward      unet3d_attention(inputs) in training mode, Loss and dice, and what tf.gradients makes of them:
 *                             SaliencyAttention/model.py:176-314, 491-548, 592-618 under train.py:83-110
 *   ps_saliency_sgd_update    tf.train.MomentumOptimizer(lr, 0.9) on the loss plus tensorpack's l2_regularizer(1e-5) of every `kernel`
 *                             variable, SaliencyAttention/train.py:50-56, 83-110
 *   ps_saliency_train_step    one step of the trainer's loop: the two above around the gradient all-reduce, train.py:50-56, 83-110 with
 *                             model.py:176-314, 491-548, 592-618
 *
 * Common to all.  Conventions are pointseg_saliency.h's: status codes and ps_last_error, caller-owned device buffers, the two-call scratch
 * protocol (scratch == NULL only fills *scratch_bytes, from the shapes alone; the second call takes device memory of at least that size,
 * 256-byte aligned), everything asynchronous on the context's stream, no host read, no allocation, no synchronisation.  Every argument
 * error returns PS_EINVAL before anything is enqueued.  Results are overwritten, never accumulated.  Nothing uses a float atomic: two runs
 * give the same bytes.  The flat buffers `weights` / `params`, `grads` and `accum` hold ps_saliency_weight_count(C_in, num_classes)
 * floats in the order pointseg_saliency.h lists.
 */
#ifndef POINTSEG_SALIENCY_STEP_H
#define POINTSEG_SALIENCY_STEP_H

#include "pointseg.h" /* ps_allreduce_fn */
#include "pointseg_saliency.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- forward, loss and every gradient -------------------------------------------------------------------------------------------------------
 *   x        [B, D, H, W, C_in] float32;  labels: [B, D, H, W] int32;  weight: [B, D, H, W] float32 or NULL (ones)
 *   weights  the flat weight buffer (read only);  weight_count: its length, checked
 *   grads    a flat buffer of the same length and order: d loss / d weights of THIS rank; must not overlap weights
 *   loss     one device float: ps_softmax_dice_loss of the logits
 *   logits   [B, D, H, W, num_classes] or NULL
 * D, H and W multiples of 16; 1 <= C_in <= 16; 2 <= num_classes <= 16; B * D * H * W * 128 < 2^31.
 *
 * The forward is the graph of ps_saliency_forward in its training form, op for op what a host composes from ps_conv3d,
 * ps_instance_norm_relu, ps_channel_attention (the scale applied to the 384-channel tensor: the backward needs it), ps_spatial_gate and
 * ps_softmax_dice_loss: loss and logits come out byte-equal to that composition.  Every layer keeps its convolution's output and its
 * norm's output for the backward.  The gradient kernels read dense tensors, so a concat is assembled, and its gradient split, by a
 * strided copy (16 bytes per lane along the channel axis where the pitches and pointers allow, a float elsewhere; the same values).
 *
 * The order of every sum of gradients.  A tensor that several layers read receives the gradients of its readers in the REVERSE of the
 * layer order of pointseg_saliency.h: the first one is written, each later one is added to it in float32 (one rounding per addition):
 *   down_list[4]   C5_cfe_cfe3_dilation, then + _cfe2_, + _cfe1_, + _cfe0
 *   down_list[3]   C4_cfe_cfe3_dilation, + _cfe2_, + _cfe1_, + _cfe0, + stride2conv3
 *   down_list[2]   C3_cfe_cfe3_dilation, + _cfe2_, + _cfe1_, + _cfe0, + stride2conv2
 *   down_list[1]   C2_conv, + stride2conv1            down_list[0]   C1_conv, + stride2conv0
 *   C345 at full resolution   final, + spatial_attention_3_conv1, + spatial_attention_2_conv1, + spatial_attention_1_conv1
 *   a residual block's input  the gradient of the block's output (the residual add passes it on unchanged), + down{d}_conv_0
 * C12 has one reader behind the gate.  Weight, bias, gamma and beta gradients go straight to their offsets in `grads`.
 * Scratch: every kept activation, the gradient workspaces (reused level by level; DESIGN.md 4.13 has the plan) and the largest scratch
 * of any op: about 1 380 floats per full-resolution voxel (16.8 GB for two [64, 160, 160] patches). */
int ps_saliency_backward(ps_context* ctx, const void* x, const void* labels, const void* weight, int64_t B, int64_t D, int64_t H, int64_t W, int64_t C_in,
                         int64_t num_classes, const void* weights, int64_t weight_count, void* grads, void* loss, void* logits, void* scratch,
                         int64_t* scratch_bytes);

/* ---- the update -------------------------------------------------------------------------------------------------------------------------------
 * Per element e of the three flat buffers, in float32, every product and every sum rounded on its own (no fused multiply-add):
 *   g        = grads[e] * grad_scale
 *   g        = g + l2 * params[e]                 only where e lies in a `/kernel` tensor (every layer's, the two dense kernels included)
 *   accum[e] = momentum * accum[e] + g
 *   params[e] = params[e] - learning_rate * accum[e]
 * Which elements decay follows from C_in and num_classes through the layer table; the caller passes no mask.  grads is read only.  One
 * launch for the whole buffer, 16 bytes per lane where the three buffers are 16-byte aligned.  The three buffers must not overlap.
 * No scratch. */
int ps_saliency_sgd_update(ps_context* ctx, void* params, const void* grads, void* accum, int64_t C_in, int64_t num_classes, int64_t weight_count,
                           float learning_rate, float momentum, float l2, float grad_scale);

/* ---- one training step ------------------------------------------------------------------------------------------------------------------------
 * ps_saliency_backward into `grads`; then, with a callback and world_size > 1, ONE call fn(user, grads, weight_count, 0, stream) -- the
 * in-place sum over the ranks, dtype 0 = float32, ordered on the context's stream; then ps_saliency_sgd_update with
 * grad_scale = 1 / world_size.  With fn == NULL or world_size == 1 the callback is not called and grad_scale is 1.  A callback that
 * returns non-zero ends the step with PS_ESTATE before the update: the parameters are unchanged.  options == NULL: one rank, momentum 0.9,
 * l2 1e-5 (the reference's).  The learning rate is an argument of every call: the reference changes it by schedule. */
typedef struct ps_saliency_step_options {
    ps_allreduce_fn allreduce; /* NULL: one rank */
    void* user;
    int32_t world_size;        /* >= 1 */
    float momentum;            /* the reference: 0.9 */
    float l2;                  /* the reference: 1e-5 */
} ps_saliency_step_options;

int ps_saliency_train_step(ps_context* ctx, const void* x, const void* labels, const void* weight, int64_t B, int64_t D, int64_t H, int64_t W, int64_t C_in,
                           int64_t num_classes, void* params, int64_t weight_count, void* grads, void* accum, float learning_rate,
                           const ps_saliency_step_options* options, void* loss, void* logits, void* scratch, int64_t* scratch_bytes);

#ifdef __cplusplus
}
#endif

#endif /* POINTSEG_SALIENCY_STEP_H */
