/* include/pointseg_saliency_data.h -- the data side of the saliency attention network (include/pointseg_saliency.h and its two training
 * headers): volumes prepared on the device and kept there, and training batches of patches drawn from them with no host read.  Same
 * conventions as pointseg.h (status codes, ps_last_error, caller-owned buffers, the context's stream).  All citations are relative to
 * the reference repository root.
 *
 * What each entry point replaces
 * ------------------------------
 *   ps_saliency_brats_measure          crop_brain_region, SaliencyAttention/utils.py:30-60, as far as it looks: get_none_zero_region
 *   ps_saliency_brats_apply            (utils.py:313-331) of the first modality, crop_ND_volume_with_bounding_box (:362-388),
 *                                      weight = crop > 0, itensity_normalize_one_volume (:333-349) per cropped modality, the label remap
 *   ps_saliency_pancreas_prepare       load_pancreas_img, utils.py:62-78: itensity_rescaling_one_volume (:351-360), weight = 1
 *   ps_patch_sample                    sampler3d (SaliencyAttention/data_sampler.py:169-214) -- get_random_roi_sampling_center
 *                                      (utils.py:390-421), extract_roi_from_volume (:423-452) of the modalities, the label and the weight
 *                                      -- and BatchData.get_data's reject loop (data_sampler.py:77-88, config.DATA_SAMPLING)
 *
 * A prepared volume is channels-last, so that a patch row is one contiguous run: image f32 [d, h, w, C], label u8 [d, h, w], weight u8
 * [d, h, w] (0 / 1).  Mixed batches (config.MIXUP) are pointseg_saliency_mixup.h's; a DIRECTION other than axial and the left-right
 * flip are pointseg_saliency_view.h's, whose PS_VIEW_AXIAL, flip = NULL call ps_patch_sample is.
 */
#ifndef POINTSEG_SALIENCY_DATA_H
#define POINTSEG_SALIENCY_DATA_H

#include "pointseg.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PS_PATCH_MAX_B 64
#define PS_PATCH_MAX_T 16
#define PS_PATCH_MAX_C 16

#define PS_PATCH_RANDOM 0       /* config.DATA_SAMPLING: anything else */
#define PS_PATCH_ALL_POSITIVE 1 /* 'all_positive' */
#define PS_PATCH_ONE_POSITIVE 2 /* 'one_positive', the reference's setting */

/* ---- BraTS form (csrc/saliency_data.hip) ----------------------------------------------------------------------------------------------------
 * raw: DEVICE f32 [C, D, H, W], C in [1, 16], D * H * W < 2^31.  Two calls, because the crop's shape is only known after the first:
 *
 * ps_saliency_brats_measure
 *     box[a], box[3 + a]   (HOST int64[6], min and max INCLUSIVE) the bounding box of raw[0] != 0, grown by `margin` (>= 0; 5 in the
 *                          reference) and clamped to the volume
 *     stats[2 c], [2 c + 1] (HOST double[2 C]) the mean and the population standard deviation of the voxels > 0 of modality c INSIDE the box
 *     The statistics are float64 sums in a fixed order (per slab of 4096 crop voxels, then over the slabs: two runs give the same bits);
 *     the deviation is two-pass, as NumPy's.  Scratch comes from the context's grow-only arena.  This call synchronises the stream ONCE
 *     (the box and the sums come back in one copy): once per volume, at load time.
 *     Errors (PS_EINVAL, nothing written): raw[0] all zero (the reference raises on .min() of an empty array); a modality with no voxel > 0
 *     inside the box, or with a deviation of 0 (the reference would write a volume of NaN or inf).
 *
 * ps_saliency_brats_apply   box and stats as measured (HOST).  Asynchronous on the context's stream, no synchronisation.  DEVICE outputs,
 *     with d = box[3] - box[0] + 1 etc.:
 *     image  f32 [d, h, w, C]   v == 0 ? 0 : float32((double(v) - mean_c) / std_c) -- negative voxels are normalised like the rest, only
 *                               the statistics leave them out
 *     weight u8 [d, h, w]       raw[0] > 0
 *     label  u8 [d, h, w]       seg (DEVICE int32 [D, H, W]) cropped and remapped: 4 -> 3 when num_class == 4, else 4 -> 1 and 2 -> 1;
 *                               zeros when seg is NULL
 */
int ps_saliency_brats_measure(ps_context* ctx, const float* raw, int32_t C, int64_t D, int64_t H, int64_t W, int32_t margin, int64_t* box,
                              double* stats);
int ps_saliency_brats_apply(ps_context* ctx, const float* raw, const int32_t* seg, int32_t C, int64_t D, int64_t H, int64_t W, int32_t num_class,
                            const int64_t* box, const double* stats, float* image, uint8_t* label, uint8_t* weight);

/* ---- Pancreas form ---------------------------------------------------------------------------------------------------------------------------
 * ct: DEVICE, n voxels of `dtype` (PS_VOLUME_I16 | PS_VOLUME_F32).  image f32 [n] = float32((double(v) + 100) / 340), weight u8 [n] = 1,
 * out_label u8 [n] = label (DEVICE u8 [n]) unchanged, zeros when label is NULL.  No crop.  Asynchronous, no synchronisation. */
int ps_saliency_pancreas_prepare(ps_context* ctx, const void* ct, int32_t dtype, int64_t n, const uint8_t* label, float* image, uint8_t* out_label,
                                 uint8_t* weight);

/* ---- the patch sampler -----------------------------------------------------------------------------------------------------------------------
 * The bank: HOST tables over n prepared volumes -- images[v], labels[v], weights[v] DEVICE pointers, dims int64 [n, 3] -- and one C.
 * The batch: B slots, a patch P[3] (HOST, any extents >= 1), T >= 1 tries per slot and cand (HOST i32 [B, T]): cand[b, t] is the volume of
 * candidate t of slot b -- the reference's "skip this datapoint, take the next of the shuffled list".  A volume may appear many times.
 *
 * The rule, a pure function of (bank, cand, P, seed, mode) (restated in numpy by tests/saliency_data_ref.py).  All arithmetic is mod 2^32,
 * hash32 = lowbias32 (x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16),
 * point_hash(j, s) = hash32(j * 2654435761 ^ s).
 *
 *   centre of (slot b, try t, axis a), with in = dims[cand[b, t]][a], out = P[a]:
 *       x0 = out / 2, x1 = in - x0                                  (integer division)
 *       x1 <= x0:  centre = (x0 + x1) / 2, nothing is drawn
 *       else:      s(b, t) = hash32(seed + 0x9E3779B9 * (b * T + t + 1)), h_a = hash32(s(b, t) + 0x85EBCA6B * (a + 1)),
 *                  centre = x0 + ((uint64) h_a * (x1 - x0 + 1) >> 32)  -- uniform on [x0, x1], both ends included; the multiply-shift's
 *                  bias is at most span / 2^32
 *     This is what the reference DOES: sampler3d passes the string "full", get_random_roi_sampling_center tests sample_mode[i] == 'full'
 *     on its characters, never true, so its 'valid' branch runs: x0 = int(out / 2), x1 = in - x0, random.randint(x0, x1).  An odd extent
 *     at its highest centre leaves one row of fill at the far end.
 *   window (extract_roi_from_volume), per axis: r0 = min(out / 2, centre), r1 = min(out - out / 2, in - centre); patch rows
 *       [out / 2 - r0, out / 2 + r1) come from volume rows [centre - r0, centre + r1).
 *   outside that box: label and weight are 0; image element j -- the linear index within the slot's [P0, P1, P2, C] patch -- is
 *       (point_hash(j, s_fill) >> 8) * 2^-24 with s_fill = hash32(s(b, t) + 0x85EBCA6B * 4): uniform on [0, 1), the reference's
 *       np.random.random_sample fill.
 *   choice of try, with pos(b, t) = the number of labels > 0 inside the copied box:
 *       PS_PATCH_RANDOM        every slot takes t = 0
 *       PS_PATCH_ALL_POSITIVE  slot b takes the first t with pos(b, t) > 0
 *       PS_PATCH_ONE_POSITIVE  slots 0 .. B-2 take t = 0; slot B-1 takes t = 0 if any earlier slot has pos(b, 0) > 0, otherwise the
 *                              first t with pos(B-1, t) > 0
 *       no try qualifies: the slot takes t = T - 1 and its ok flag is 0.  The reference would go on skipping datapoints; here the flag,
 *       not an endless loop, reports it.
 *
 * Outputs, DEVICE: images f32 [B, P0, P1, P2, C], weights f32 [B, P0, P1, P2], labels i32 [B, P0, P1, P2] (what ps_softmax_dice_loss
 * takes), info i32 [B, 8] = {try, volume, c0, c1, c2, pos, ok, 0}.
 * Limits: B in [1, 64], T in [1, 16], C in [1, 16], every dim >= 1 with d * h * w * C < 2^31, every P[a] >= 1 with P0 * P1 * P2 * C < 2^31.
 * Two launches (a count of the candidate windows that can matter; a gather whose workgroups each derive the tries from the counts),
 * asynchronous on the context's stream, no host read; integer sums only, so two runs give the same bytes.  Scratch (the candidate table
 * and the counts) comes from the context's arena.  Every argument error -- a NULL pointer, a volume id outside the bank, a dim < 1, P, B, T,
 * C or mode out of range -- returns PS_EINVAL before anything is enqueued, the outputs untouched. */
int ps_patch_sample(ps_context* ctx, const float* const* images, const uint8_t* const* labels, const uint8_t* const* weights, const int64_t* dims,
                    int64_t n, int32_t C, const int32_t* cand, int32_t B, int32_t T, const int64_t* P, uint32_t seed, int32_t mode, float* out_images,
                    float* out_weights, int32_t* out_labels, int32_t* out_info);

#ifdef __cplusplus
}
#endif

#endif /* POINTSEG_SALIENCY_DATA_H */
