/* include/pointseg_saliency_map.h -- the saliency attention map of a WHOLE volume behind one call: the sliding-window average of
 * pointseg_saliency.h around the network's forward, in one to three anatomical views, with the left-right test flip, fused
 * (csrc/saliency_map.hip; the window table and the scratch plan: csrc/saliency_map_plan.h).  Same conventions as
 * pointseg_saliency_precision.h, whose ps_saliency_forward_prec it runs per batch of windows: status codes, ps_last_error, caller-owned
 * device buffers, the context's stream, the two-call scratch protocol.  It is what a deployment hands to the threshold of
 * ps_volume_sample (probs) -- `segment_one_image` and the `eval_*` path of the reference.  All citations are relative to the reference
 * repository root.
 *
 * What it replaces
 * ----------------
 *   overlapping_inference       SaliencyAttention/eval.py:103-193   the window loop, the sum and the count, the division
 *   segment_one_image           SaliencyAttention/eval.py:355-411   one volume through the loop
 *   transpose_volumes           SaliencyAttention/utils.py:80-104   config.DIRECTION: the network looks at sagittal or coronal slices
 *   flip_lr, TEST_FLIP          SaliencyAttention/utils.py:15-28, eval.py:461-463   (probs + probs_flip) / 2.0
 *   MULTI_VIEW                  SaliencyAttention/eval.py:254       (ax + transpose(sa) + transpose(co)) / 3.0
 *
 * The rule: out is a pure function of the arguments
 * -------------------------------------------------
 * Views.  The network of views[i] sees the volume with its axes permuted; vol is [D, H, W] per channel:
 *   PS_VIEW_AXIAL     view = vol
 *   PS_VIEW_SAGITTAL  view[i, j, k] = vol[j, k, i], extents (W, D, H): np.transpose(x, (2, 0, 1)); its map comes back by (1, 2, 0)
 *   PS_VIEW_CORONAL   view[i, j, k] = vol[j, i, k], extents (H, D, W): np.transpose(x, (1, 0, 2)); its map comes back by the same
 * Flip pass.  It runs on vol'[d, h, w] = vol[d, h, W - 1 - w] -- the mirror comes BEFORE the view transform, as flip_lr does -- and its map
 * is mirrored back along W.
 * One pass (one view, flipped or not), on the view's extents (n0, n1, n2):
 *   the window origins per view axis a are window_origins(n_a, patch[a], step[a]) = 0, step, 2 step, ... below max(1, n_a - patch[a] + step[a])
 *   (eval.py:142-144; with step > patch the last origin can lie behind the volume: that window adds nothing, as numpy's empty slice);
 *   the windows are visited with axis 0 outermost and axis 2 innermost; what a window overhangs the volume by is 0;
 *   the window's softmax probabilities come from ps_saliency_forward_prec at `precision`; the part inside the volume is added to a float32
 *   sum, in window order, and 1 to an int32 count (eval.py:168-174); m = sum / count, ps_saliency_finish's division (eval.py:176-177); a
 *   voxel no window covers gives 0.
 * Fusion.  For f in {unflipped, flipped}: fused_f = m_v0 when n_views == 1, otherwise
 *   fused_f = fl32(fl32(... fl32(m_v0 + m_v1) ...) / float(n_views)), the views in the order of `views` -- a correctly rounded float32
 *   division, not a multiplication by a rounded reciprocal.  out = fused_0 when flip == 0, otherwise out = fl32(fl32(fused_0 + fused_1) * 0.5f).
 * The sums are float32 where the reference's are float64, as the window average's have been since pointseg_saliency.h.
 *
 * Guarantees.  The bytes of out do not depend on `batch`: the samples of a forward batch do not see each other (pointseg_saliency.h), and
 * the windows of a batch are added in window order.  Nothing uses a float atomic: two runs give the same bytes.  With n_views = 1, the
 * axial view, flip = 0 and batch = 1 the bytes are those of the ps_saliency_forward_prec / ps_saliency_accumulate / ps_saliency_finish loop.
 *
 * Memory.  No permuted or mirrored copy of the volume is made and no map is held in view orientation: the views and the mirror are index
 * arithmetic inside the window gather and the window add.  Beside out the scratch holds the current pass's sum and (more than one view)
 * the running fusion, each a [D, H, W, num_classes] float map, one int32 count [D, H, W], `batch` input windows, `batch` probability
 * windows, and ps_saliency_forward's scratch at B = batch.  The sizing call returns that number from the shapes alone.
 */
#ifndef POINTSEG_SALIENCY_MAP_H
#define POINTSEG_SALIENCY_MAP_H

#include "pointseg_saliency_precision.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { PS_VIEW_AXIAL = 0, PS_VIEW_SAGITTAL = 1, PS_VIEW_CORONAL = 2 };
enum { PS_VOLUME_CDHW = 0, PS_VOLUME_DHWC = 1 }; /* the reference's [mod, d, h, w] / PatchBank's channels-last image */

/*   volume        float32, [C_in, D, H, W] (PS_VOLUME_CDHW) or [D, H, W, C_in] (PS_VOLUME_DHWC), resident on the device
 *   views         n_views in [1, 3] distinct PS_VIEW_* values (host memory)
 *   weights       n_views device weight buffers (a host array of device pointers): weights[i] is the network trained for views[i], in
 *                 ps_saliency_forward's layout, weight_count = ps_saliency_weight_count(C_in, num_classes) values each
 *   patch, step   three values each (host memory), in VIEW axes; patch: multiples of 16, step: at least 1
 *   flip          0 or 1;  batch: in [1, 8], the windows per forward call;  precision: a PS_PREC_* value
 *   out           float32 [D, H, W, num_classes], in the volume's orientation; must not overlap the volume or the scratch
 * Limits: 1 <= C_in <= 16, 2 <= num_classes <= 16, P0 * P1 * P2 * 128 < 2^31 (ps_saliency_forward's),
 * D * H * W * max(C_in, num_classes) < 2^31 (ps_saliency_accumulate's), and every window's end, origin + patch, below 2^31.
 * Every argument error returns PS_EINVAL before anything is enqueued, with out untouched, also in the call that sizes the scratch: a NULL
 * pointer (in the sizing call the context, volume, weights and out are not looked at and may be NULL), a view or layout out of range, a
 * repeated view, n_views, batch, flip or precision out of range, a patch extent that is no multiple of 16, a step below 1, C_in,
 * num_classes or weight_count that are not the network's, a breach of the 2^31 limits.
 * Asynchronous on the context's stream, no synchronisation, no host read, no allocation. */
int ps_saliency_map(ps_context* ctx, const void* volume, int32_t layout, int64_t C_in, int64_t D, int64_t H, int64_t W, int64_t num_classes,
                    int32_t n_views, const int32_t* views, const void* const* weights, int64_t weight_count, const int64_t* patch,
                    const int64_t* step, int32_t flip, int32_t batch, int32_t precision, void* out, void* scratch, int64_t* scratch_bytes);

#ifdef __cplusplus
}
#endif

#endif /* POINTSEG_SALIENCY_MAP_H */
