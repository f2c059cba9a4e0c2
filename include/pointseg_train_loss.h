/* include/pointseg_train_loss.h -- the objective of the point network's training step (pointseg_train_ops.h: ps_randla_train_step), chosen
 * per call, and the accuracy the reference's step returns next to the loss.
 *
 *   PS_LOSS_CE             the class-weighted cross-entropy (ps_op_weighted_ce; PointSegment/RandLANet.py:267-274): what the step minimised
 *                          before this header, the same launches and the same bytes
 *   PS_LOSS_DICE           dice_loss (RandLANet.py:276-291)
 *   PS_LOSS_DICE_WEIGHTED  get_loss_dice_weight (RandLANet.py:293-312) with u = class_weights; the reference hard-codes [4, 1, 1, 1] there,
 *                          the value to pass for BraTS
 *
 * The Dice is taken on the RAW logits, as the reference writes it (there is no softmax in RandLANet.py:276-312).  z f32 [R, C]; y i32 [R],
 * the labels after the trainer's label map, a label outside [0, C) is an ignored row as for the cross-entropy; V the rows not ignored;
 * u_c = 1 for PS_LOSS_DICE, class_weights[c] for PS_LOSS_DICE_WEIGHTED:
 *
 *   S0_c = sum_{i in V} [y_i = c] z_ic      S1_c = sum_{i in V} z_ic^2      S2_c = sum_{i in V} [y_i = c]     (unweighted, as :307)
 *   D_c  = u_c S1_c + S2_c + 1e-5           s_c  = 2 u_c S0_c / D_c         loss = 1 - (1 / C) sum_c s_c
 *   dloss/dz_ic = g (b_c z_ic - a_c [y_i = c]) for i in V, 0 for an ignored row;   a_c = 2 u_c / (C D_c),  b_c = a_c s_c,  g = grad_scale
 *
 * The sums are float64, added in one fixed order (no float atomics: two runs give the same bytes); a_c, b_c and the loss are formed in float64
 * from the sums and rounded once, a gradient element in float64 from the float32 logit and rounded once.  With nothing valid the loss is 1 and
 * every gradient 0; a class no valid row carries has s_c = 0.
 *
 * Accuracy (tf.nn.in_top_k(valid_logits, valid_labels, 1), then the mean; RandLANet.py:93-94): a valid row is correct iff its target logit
 * is finite and no class has a strictly larger logit (a tie is correct, as in TensorFlow); accuracy = float32(n_correct / n_valid) from integer
 * counts, and 0 when nothing is valid (the reference's mean over nothing is NaN).
 *
 * Limits of the Dice kinds: 1 <= C <= 16, 1 <= R < 2^31.  A bad shape, kind or NULL pointer returns PS_EINVAL before anything is enqueued.
 * Device time shows under the "train_loss" stage.  All pointers but the context and the trainer are device pointers.
 */
#ifndef POINTSEG_TRAIN_LOSS_H
#define POINTSEG_TRAIN_LOSS_H

#include "pointseg_train_ops.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { PS_LOSS_CE = 0, PS_LOSS_DICE = 1, PS_LOSS_DICE_WEIGHTED = 2 };

/* sums f64 [3 C + 2]: per class (S0_c, S1_c, S2_c), then n_valid, n_correct (exact integers).  One read of the logits and labels. */
int ps_op_dice_sums(ps_context* ctx, const float* logits, const int32_t* labels, int64_t R, int64_t C, double* sums);

/* From the first 3 C doubles of sums (this call's rows', or those of several calls added up: the loss and the gradient are then those of
 * the ONE Dice over all their rows, the gradient times grad_scale): loss f32 [1] and / or dlogits f32 [R, C].  kind: PS_LOSS_DICE
 * (class_weights is not read, may be NULL) or PS_LOSS_DICE_WEIGHTED (class_weights f32 [C]).  loss or dlogits may be NULL, not both;
 * dlogits may be logits. */
int ps_op_dice_from_sums(ps_context* ctx, int32_t kind, const float* logits, const int32_t* labels, const float* class_weights, const double* sums,
                         float grad_scale, int64_t R, int64_t C, float* loss, float* dlogits);

/* counts f64 [2] = n_valid, n_correct of the accuracy rule above, for a loss that does not come through ps_op_dice_sums.  1 <= C <= 64. */
int ps_op_top1_counts(ps_context* ctx, const float* logits, const int32_t* labels, int64_t R, int64_t C, double* counts);

/* ps_randla_backward / ps_randla_train_step (pointseg_train_ops.h) under the objective loss_kind; those two are the PS_LOSS_CE,
 * accuracy = NULL calls of these.  class_weights f32 [num_classes] is required (PS_LOSS_DICE does not read it).  accuracy f32 [1], may be
 * NULL (then nothing is launched for it): THIS rank's, over the rows of this call.  logits may be NULL.
 *
 * Data-parallel (ps_trainer_set_collective).  With an active collective and the sync_bn bit set, the Dice kinds all-reduce the first 3 C
 * doubles of the sums through the callback (dtype 1: one more call per step than PS_LOSS_CE, 8 * 3 C more bytes) and take grad_scale =
 * world_size, so that the step's mean over the ranks is the gradient of the ONE Dice over all ranks' rows -- "W ranks x one cloud" is the
 * step of "one rank x W clouds", as for the cross-entropy with shared statistics -- and every rank returns that one loss.  Otherwise each
 * rank takes the Dice of its own rows (grad_scale = 1, no extra call): the step then minimises the MEAN of the ranks' own Dice losses, which
 * is not the Dice of the union. */
int ps_randla_backward_loss(ps_trainer* t, const ps_pyramid* pyr, const float* features, const int32_t* labels, const float* class_weights,
                            int32_t loss_kind, float* loss, float* accuracy, float* logits);
int ps_randla_train_step_loss(ps_trainer* t, const ps_pyramid* pyr, const float* features, const int32_t* labels, const float* class_weights,
                              int32_t loss_kind, float* loss, float* accuracy, float* logits);

#ifdef __cplusplus
}
#endif

#endif /* POINTSEG_TRAIN_LOSS_H */
