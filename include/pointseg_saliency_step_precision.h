/* include/pointseg_saliency_step_precision.h -- a choice of arithmetic for the convolutions of the saliency attention network's one-call
 * training step (csrc/saliency_step.hip's walker): one precision for each of the three ROLES a convolution plays in a step -- the forward,
 * the data gradient, the weight gradient -- because they cost and gain differently.  The values are
 * pointseg_saliency_precision.h's PS_PREC_*; what each means for an operand element is written there (the forward) and in
 * pointseg_saliency_train_precision.h (the two gradients).  The walker adds no kernel: it calls ps_conv3d_prec, ps_conv3d_bwd_data_prec and
 * ps_conv3d_bwd_weight_prec where it called ps_conv3d, ps_conv3d_bwd_data and ps_conv3d_bwd_weight.
 *
 * What each entry point replaces
 * ------------------------------
 *   ps_saliency_backward_prec     ps_saliency_backward and ps_saliency_backward_soft (pointseg_saliency_step.h, pointseg_saliency_mixup.h)
 *   ps_saliency_train_step_prec   ps_saliency_train_step and ps_saliency_train_step_soft
 * Every argument before `soft_labels` is theirs, in their order, with their limits, their checks, their two-call scratch protocol and their
 * scratch SIZE: the same number of bytes in every combination of the three precisions (the op entries promise it, and the step's plan is a
 * function of the shapes alone), so a host sizes its scratch once.  The four older entries are calls of these two with PS_PREC_FP32 three
 * times: one body each, the same bytes as before this header, and an error message names the entry that was called.
 *
 * The rule
 * --------
 *   soft_labels           0: `labels` is [B, D, H, W] int32.  1: `labels` is the float32 [B, D, H, W, num_classes] rows of
 *                         pointseg_saliency_mixup.h.  The kind of the loss node and of its gradient; nothing else depends on it.
 *   precision_forward     every ps_conv3d of the training-mode forward
 *   precision_data_grad   every ps_conv3d_bwd_data of the backward (init_conv has none: the patch wants no gradient)
 *   precision_weight_grad every ps_conv3d_bwd_weight of the backward, the bias gradients with them
 * Any other value of any of the four returns PS_EINVAL before anything is enqueued, also in the call that only sizes the scratch
 * (*scratch_bytes is then left alone).
 *
 * Everything else keeps its arithmetic in every combination: the instance norm and its gradient (float64 fixed-order sums), the channel
 * attention and its two dense layers, the spatial gate, softmax + Dice and their gradients, the strided copy / add, the order of every sum
 * of gradients that pointseg_saliency_step.h lists (float32, one rounding per addition), the all-reduce and the update.  Kept activations
 * stay float32 in memory.  Nothing uses a float atomic: two runs of any combination give the same bytes.
 *
 * C345_conv.  The training graph applies the channel attention's scale to the 384-channel ACTIVATION in front of C345_conv (the backward
 * needs the scaled tensor), where ps_saliency_forward_prec folds the scale into that layer's kernel.  Under PS_PREC_BF16 the step therefore
 * rounds the scaled activation and the plain kernel, inference the activation and the scaled kernel: the two differ by roundings, as the
 * op-by-op training graph does from inference.
 *
 * What the step owes.  It runs the same op entries on the same operands in the same order as a host that composes the graph op by op at the
 * same three precisions: loss and logits come out byte-equal to that composition, and a gradient can differ from it only through the order
 * of the float32 sums of gradients above.
 */
#ifndef POINTSEG_SALIENCY_STEP_PRECISION_H
#define POINTSEG_SALIENCY_STEP_PRECISION_H

#include "pointseg_saliency_mixup.h"
#include "pointseg_saliency_step.h"
#include "pointseg_saliency_train_precision.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ps_saliency_backward (soft_labels == 0) or ps_saliency_backward_soft (soft_labels == 1) with the convolutions of each role at its own
 * precision. */
int ps_saliency_backward_prec(ps_context* ctx, const void* x, const void* labels, const void* weight, int64_t B, int64_t D, int64_t H, int64_t W,
                              int64_t C_in, int64_t num_classes, const void* weights, int64_t weight_count, void* grads, void* loss, void* logits,
                              void* scratch, int64_t* scratch_bytes, int32_t soft_labels, int32_t precision_forward, int32_t precision_data_grad,
                              int32_t precision_weight_grad);

/* ps_saliency_train_step (soft_labels == 0) or ps_saliency_train_step_soft (soft_labels == 1): ps_saliency_backward_prec into `grads`, the
 * all-reduce through the host's callback and the update, both as pointseg_saliency_step.h states them. */
int ps_saliency_train_step_prec(ps_context* ctx, const void* x, const void* labels, const void* weight, int64_t B, int64_t D, int64_t H, int64_t W,
                                int64_t C_in, int64_t num_classes, void* params, int64_t weight_count, void* grads, void* accum, float learning_rate,
                                const ps_saliency_step_options* options, void* loss, void* logits, void* scratch, int64_t* scratch_bytes,
                                int32_t soft_labels, int32_t precision_forward, int32_t precision_data_grad, int32_t precision_weight_grad);

#ifdef __cplusplus
}
#endif

#endif /* POINTSEG_SALIENCY_STEP_PRECISION_H */
