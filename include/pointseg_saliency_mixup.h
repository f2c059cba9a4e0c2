/* include/pointseg_saliency_mixup.h -- config.MIXUP of the saliency attention network's trainer: training batches whose neighbouring samples
 * are mixed on the device (csrc/saliency_data.hip), softmax + weighted Dice on the soft labels that mixing makes (csrc/saliency_train.hip),
 * and the whole-graph gradient and the training step on them (csrc/saliency_step.hip).  Same conventions as pointseg_saliency_data.h,
 * pointseg_saliency_attention.h and pointseg_saliency_step.h, whose hard-label entry points these stand next to.  All citations are relative
 * to the reference repository root.
 *
 * What each entry point replaces
 * ------------------------------
 *   ps_patch_sample_mixup              the one-hot labels of SaliencyAttention/data_sampler.py:329-337, BatchData.get_data with B + 1 accepted
 *                                      samples whose neighbour pairs are mixed (data_sampler.py:90-96; its reject loop :77-96), and mixup,
 *                                      SaliencyAttention/utils.py:511-527
 *   ps_softmax_dice_soft_loss          dice_mixup and the Loss branch that calls it, SaliencyAttention/model.py:550-590, 602-612
 *   ps_softmax_dice_soft_loss_bwd      what tf.gradients makes of it
 *   ps_saliency_backward_soft          ps_saliency_backward with that loss
 *   ps_saliency_train_step_soft        ps_saliency_train_step with that loss
 */
#ifndef POINTSEG_SALIENCY_MIXUP_H
#define POINTSEG_SALIENCY_MIXUP_H

#include "pointseg_saliency_data.h"
#include "pointseg_saliency_step.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the mixed gather --------------------------------------------------------------------------------------------------------------------------
 * The bank, P, T, seed and mode are ps_patch_sample's.  A batch of B mixed slots is made of B + 1 DRAWN samples i = 0 .. B: cand is
 * HOST i32 [B + 1, T], and everything ps_patch_sample's rule keys by the slot -- s(i, t) = hash32(seed + 0x9E3779B9 * (i * T + t + 1)),
 * the centres, the windows, the uniform fill keyed by s(i, t) -- is keyed by the sample index i.
 *
 *   choice of try (the reject loop runs on a holder that grows to B + 1 samples; pos(i, t) as in ps_patch_sample):
 *       PS_PATCH_RANDOM        every sample takes t = 0
 *       PS_PATCH_ALL_POSITIVE  sample i takes the first t with pos(i, t) > 0
 *       PS_PATCH_ONE_POSITIVE  the check fires when the holder has B - 1 samples: samples 0 .. B-2 and sample B take t = 0; sample B-1 takes
 *                              t = 0 if some sample i < B-1 has pos(i, 0) > 0, otherwise the first t with pos(B-1, t) > 0 (for B = 1 there
 *                              is no earlier sample: sample 0 must be positive).  This is NOT ps_patch_sample's rule at B + 1 slots, which
 *                              forces the last slot.
 *       no try qualifies: the sample takes t = T - 1 and its ok flag is 0.
 *
 *   mixing, slot b = mix(sample b, sample b + 1, gamma[b]); sample b + 1 is the same drawn patch (try, centre, fill) in slots b and b + 1.
 *   With g = float32(gamma[b]) and h = float32(1.0 - gamma[b]) (the subtraction in float64):
 *       image   fl32(fl32(g * a) + fl32(h * b))       two products and one sum, each rounded: no fused multiply-add
 *       soft    the same rule on the samples' one-hot rows of num_classes values: 0, g, h or fl32(g + h) (which is not always 1).  Outside a
 *               sample's copied box its label is 0 (its row is class 0); a label >= num_classes gives an all-zero row for its sample
 *       weight  (w1 != 0) | (w2 != 0) as 1.0f / 0.0f; outside a sample's copied box its weight is 0
 *   float32(gamma) may be exactly 1 while h is a tiny non-zero number: nothing is special-cased.
 *
 * Outputs, DEVICE: out_images f32 [B, P0, P1, P2, C], out_weights f32 [B, P0, P1, P2], out_soft f32 [B, P0, P1, P2, num_classes] (what
 * ps_softmax_dice_soft_loss takes), out_info i32 [B + 1, 8], one row per DRAWN sample, the columns of ps_patch_sample.
 * Limits: B in [1, PS_PATCH_MAX_B - 1], num_classes in [2, 16], B * P0 * P1 * P2 * num_classes < 2^31; ps_patch_sample's other limits.
 * gamma: HOST double [B], each finite and in [0, 1] (the reference draws np.random.beta(0.4, 0.4)).
 * Two launches (ps_patch_sample's count over the (B + 1) * T candidates; one gather that reads both source windows of an output piece,
 * mixes and stores -- no buffer of B + 1 patches), asynchronous on the context's stream, no host read; integer sums only in the count: two
 * runs give the same bytes.  Every argument error returns PS_EINVAL before anything is enqueued, the outputs untouched. */
int ps_patch_sample_mixup(ps_context* ctx, const float* const* images, const uint8_t* const* labels, const uint8_t* const* weights,
                          const int64_t* dims, int64_t n, int32_t C, const int32_t* cand, int32_t B, int32_t T, const int64_t* P, uint32_t seed,
                          int32_t mode, int32_t num_classes, const double* gamma, float* out_images, float* out_weights, float* out_soft,
                          int32_t* out_info);

/* ---- softmax + weighted Dice on soft labels ----------------------------------------------------------------------------------------------------
 * logits f32 [B, V, C], soft f32 [B, V, C], weight f32 [B, V] or NULL (ones).  With p = softmax(logits), g_vc the soft label, w the weight:
 *   S0_c = sum_v w g_vc p_vc    S1_c = sum_v w p_vc^2    S2_c = sum_v w g_vc
 *   num_c = 2 S0_c    D_c = S1_c + S2_c + 1e-5    loss_b = 1 - mean_c num_c / D_c    loss = mean_b loss_b
 *   G_vc = -(dloss / (B C)) (2 w g_vc / D_c - 2 num_c w p_vc / D_c^2)        dlogits_vc = p_vc (G_vc - sum_k p_vk G_vk)
 * ps_softmax_dice_loss's algebra with [g = c] replaced by g_vc, by the same kernels (one body, the label source a template parameter), the
 * same float64 partials per slab of 4096 voxels in the same order: soft = one_hot(labels) gives loss, sums and dlogits byte-equal to the
 * hard-label ops.  The soft labels receive no gradient.  Every contract of ps_softmax_dice_loss / _bwd holds: C in [2, 16], sums f64
 * [B, C, 3], the two-call scratch protocol, argument errors before anything is enqueued (the context looked at last), dlogits may be logits,
 * dloss == NULL means 1, and where p is exactly 0 or 1 the gradient is exactly 0.  The soft rows are read 16 bytes at a time where
 * C % 4 == 0 and they are 16-byte aligned, 8 bytes where C == 2 and they are 8-byte aligned. */
int ps_softmax_dice_soft_loss(ps_context* ctx, const void* logits, const void* soft, const void* weight, int64_t B, int64_t V, int64_t C, void* loss,
                              void* sums, void* scratch, int64_t* scratch_bytes);
int ps_softmax_dice_soft_loss_bwd(ps_context* ctx, const void* logits, const void* soft, const void* weight, const void* sums, const void* dloss,
                                  int64_t B, int64_t V, int64_t C, void* dlogits);

/* ---- the whole graph on soft labels -------------------------------------------------------------------------------------------------------------
 * ps_saliency_backward and ps_saliency_train_step with soft f32 [B, D, H, W, num_classes] in place of labels: the same graph walker, its
 * one loss node taking the label kind.  Everything else -- arguments, limits, scratch size, the order of every sum -- is theirs. */
int ps_saliency_backward_soft(ps_context* ctx, const void* x, const void* soft, const void* weight, int64_t B, int64_t D, int64_t H, int64_t W,
                              int64_t C_in, int64_t num_classes, const void* weights, int64_t weight_count, void* grads, void* loss, void* logits,
                              void* scratch, int64_t* scratch_bytes);
int ps_saliency_train_step_soft(ps_context* ctx, const void* x, const void* soft, const void* weight, int64_t B, int64_t D, int64_t H, int64_t W,
                                int64_t C_in, int64_t num_classes, void* params, int64_t weight_count, void* grads, void* accum, float learning_rate,
                                const ps_saliency_step_options* options, void* loss, void* logits, void* scratch, int64_t* scratch_bytes);

#ifdef __cplusplus
}
#endif

#endif /* POINTSEG_SALIENCY_MIXUP_H */
