/* include/pointseg_saliency_view.h -- config.DIRECTION and the left-right flip on the TRAINING side of the saliency attention network: the
 * patch sampler of pointseg_saliency_data.h and the mixed sampler of pointseg_saliency_mixup.h seen through an anatomical view, with a
 * per-sample mirror of the view's last axis (csrc/saliency_data.hip; the candidate table: csrc/saliency_sampler_plan.h).
 * With it the three networks that ps_saliency_map (pointseg_saliency_map.h) fuses can be trained from ONE resident bank.  Same conventions
 * as the two headers it extends.  All citations are relative to the reference repository root.
 *
 * What each entry point replaces
 * ------------------------------
 *   ps_patch_sample_view          sampler3d, SaliencyAttention/data_sampler.py:169-214, with config.DIRECTION: transpose_volumes
 *                                 (SaliencyAttention/utils.py:80-104) of every modality, the label and the weight BEFORE the centre is drawn
 *                                 and the windows are cut, and its np.flip(..., -1) augmentation (data_sampler.py:190-207)
 *   ps_patch_sample_mixup_view    the same under config.MIXUP (pointseg_saliency_mixup.h)
 *
 * The rule: a pure function of the arguments
 * ------------------------------------------
 * View extents.  The bank and dims stay in VOLUME axes [d, h, w], channels last.  The sampler sees each candidate volume through
 * pointseg_saliency_map.h's permutation:
 *   PS_VIEW_AXIAL     view = vol
 *   PS_VIEW_SAGITTAL  view[i, j, k] = vol[j, k, i], extents (W, D, H): np.transpose(x, (2, 0, 1))
 *   PS_VIEW_CORONAL   view[i, j, k] = vol[j, i, k], extents (H, D, W): np.transpose(x, (1, 0, 2))
 * P, the centres, the windows and info's c0, c1, c2 are in VIEW axes.
 * What is unchanged.  Everything ps_patch_sample derives per axis a is derived on the view's extent a with the same hashes: x0, x1, the
 * centre draw h_a, r0, r1, the copied box.  The fill is keyed by the linear index j within the slot's VIEW patch [P0, P1, P2, C], before
 * the flip.  pos(b, t) -- a box is the same set of voxels in any view --, the choice of try in all three modes and the mixed holder's rule
 * are unchanged.
 * Flip.  It comes last, per DRAWN sample, and for mixed batches before mixing: out[i, j, k, c] = unflipped[i, j, P2 - 1 - k, c].  It applies
 * to image (its fill mirrored with it), weight and label alike: np.flip(sub, -1).
 * info[7] is the sample's flip bit.  It stays 0 through ps_patch_sample and ps_patch_sample_mixup.
 *
 * The defining identity.  The outputs are byte-equal to ps_patch_sample / ps_patch_sample_mixup run on a bank of permuted CONTIGUOUS
 * COPIES (np.transpose(x, (2, 0, 1)) / (1, 0, 2) of image, label and weight, with the copies' dims), followed by the flip of the flagged
 * samples (for a mixed batch: of the drawn samples, before they are mixed).  tests/saliency_view_ref.py restates it in numpy.
 *
 * The old entries.  ps_patch_sample and ps_patch_sample_mixup ARE the PS_VIEW_AXIAL, flip = NULL calls of these two: one body each, the same
 * kernels, the same bytes.
 *
 * Arguments: those of the entry extended, then
 *   view   a PS_VIEW_* value
 *   flip   HOST i32, one 0 / 1 per drawn sample -- [B], or [B + 1] for a mixed batch -- or NULL: none
 * Argument errors: a view out of range or a flip value other than 0 / 1 returns PS_EINVAL before anything is enqueued, the outputs
 * untouched.  Every limit and error of the old entries holds on the view's extents.  The sagittal view's gather runs on a three-dimensional
 * grid and takes B * P1 < 2^24, P0 <= 65535 * min(32, 128 / C) and P2 <= 65535 * 32 on top.
 *
 * Launches and memory.  Still two launches, asynchronous on the context's stream, no host read, no float atomic: two runs give the same
 * bytes.  No permuted or mirrored copy of a volume exists at any time: the view and the mirror are index arithmetic inside the gather (the
 * sagittal view, whose rows run along the volume's H, goes through an LDS tile).  Scratch remains the candidate table plus the counts from
 * the context's arena, its size independent of the volumes' sizes.
 */
#ifndef POINTSEG_SALIENCY_VIEW_H
#define POINTSEG_SALIENCY_VIEW_H

#include "pointseg_saliency_map.h"
#include "pointseg_saliency_mixup.h"

#ifdef __cplusplus
extern "C" {
#endif

int ps_patch_sample_view(ps_context* ctx, const float* const* images, const uint8_t* const* labels, const uint8_t* const* weights, const int64_t* dims,
                         int64_t n, int32_t C, const int32_t* cand, int32_t B, int32_t T, const int64_t* P, uint32_t seed, int32_t mode, int32_t view,
                         const int32_t* flip, float* out_images, float* out_weights, int32_t* out_labels, int32_t* out_info);

int ps_patch_sample_mixup_view(ps_context* ctx, const float* const* images, const uint8_t* const* labels, const uint8_t* const* weights,
                               const int64_t* dims, int64_t n, int32_t C, const int32_t* cand, int32_t B, int32_t T, const int64_t* P, uint32_t seed,
                               int32_t mode, int32_t num_classes, const double* gamma, int32_t view, const int32_t* flip, float* out_images,
                               float* out_weights, float* out_soft, int32_t* out_info);

#ifdef __cplusplus
}
#endif

#endif /* POINTSEG_SALIENCY_VIEW_H */
