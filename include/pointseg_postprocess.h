/* include/pointseg_postprocess.h -- the clean-up of a predicted label volume between ps_probs_to_labels and ps_seg_metrics: connected
 * components, binary morphology, component selection, hole filling and the BraTS chain built from them (csrc/postprocess.hip).  Same
 * conventions as pointseg.h and pointseg_prepare.h (status codes, ps_last_error, caller-owned device buffers, the context's stream); kept
 * out of pointseg.h because a host that only drives the network never needs it.  All citations are relative to the reference repository
 * root.
 *
 * What each entry point replaces
 * ------------------------------
 *   ps_label_components    scipy.ndimage.label(x, generate_binary_structure(3, c)) and the ndimage.sum(...) of the component sizes,
 *                          SaliencyAttention/utils.py:112-114, 136-138 (again in PointSegment/utils/process_tf.py:112-114, 136-138)
 *   ps_binary_morph        ndimage.morphology.binary_closing(x, structure=generate_binary_structure(3, 2)), SaliencyAttention/eval.py:35, 41
 *   ps_keep_components     get_largest_two_component and remove_external_core, SaliencyAttention/utils.py:106-164
 *                          (PointSegment/utils/process_tf.py:106-164)
 *   ps_fill_holes          scipy.ndimage.morphology.binary_fill_holes(x), SaliencyAttention/eval.py:402
 *   ps_brats_postprocess   post_processing, SaliencyAttention/eval.py:20-55
 *
 * Common to all five.  A volume is device memory, [d0, d1, d2] row-major (d2 fastest), every dimension >= 1 and V = d0 * d1 * d2 < 2^31.
 * A mask is a uint8 volume: non-zero = set; mask outputs hold 0 / 1.  connectivity c in {1, 2, 3}: two voxels are neighbours when their
 * coordinates differ by at most 1 on every axis and on at most c axes -- the 6-, 18- and 26-neighbourhood of generate_binary_structure(3, c).
 * Input and output arrays must not overlap.
 * Scratch: the two-call protocol of ps_volume_zoom -- scratch == NULL only fills *scratch_bytes, from the shape (and the rule) alone: the
 * volume pointers and the context are not looked at and may be NULL, every other argument is checked as in the second call.  The second
 * call takes device memory of at least that size, 256-byte aligned, valid until the stream has passed the call.
 * Asynchronous on the context's stream, no synchronisation, no host read of any count.  Every argument error returns PS_EINVAL before
 * anything is enqueued.  Every result is an integer computed with integer atomics: two runs give the same bytes.
 */
#ifndef POINTSEG_POSTPROCESS_H
#define POINTSEG_POSTPROCESS_H

#include "pointseg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ps_binary_morph op */
#define PS_MORPH_DILATE 1
#define PS_MORPH_ERODE 2
#define PS_MORPH_CLOSE 3 /* dilate, then erode */
#define PS_MORPH_OPEN 4  /* erode, then dilate */

/* ps_keep_components rule */
#define PS_KEEP_ABOVE 1
#define PS_KEEP_LARGEST_TWO 2
#define PS_KEEP_OVERLAP 3

/* ---- connected components ----------------------------------------------------------------------------------------------------------------
 * Replaces `labeled_array, numpatches = ndimage.label(img, s)` and `sizes = ndimage.sum(img, labeled_array, range(1, numpatches + 1))`
 * (SaliencyAttention/utils.py:112-114, 136-138).  The labelled set is the non-zero voxels of `volume` (background == 0) or its zero
 * voxels (background == 1).
 *   labels   int32[V]: 0 outside the labelled set, otherwise 1 .. n
 *   n        one int32: the number of components
 *   sizes    int32, room for (V + 1) / 2 entries (the most components a volume can have); entries [0, n) are written: voxels of component k + 1
 *   touches  uint8, room for (V + 1) / 2 entries; entries [0, n) are written: 1 when component k + 1 has a voxel on a face of the array
 *            (a coordinate equal to 0 or to d - 1), else 0
 * sizes and touches may each be NULL.
 * Numbering: component k is the one whose smallest linear index is the k-th smallest among all components -- the order in which a raster
 * scan meets them, which is scipy's (tests/test_postprocess_rule.py pins it).
 * Scratch: three int32 volumes, the workspace of one prefix sum over V words and 256 bytes of counters. */
int ps_label_components(ps_context* ctx, const void* volume, int64_t d0, int64_t d1, int64_t d2, int32_t connectivity, int32_t background,
                        void* labels, void* n, void* sizes, void* touches, void* scratch, int64_t* scratch_bytes);

/* ---- binary dilation, erosion, closing, opening --------------------------------------------------------------------------------------------
 * Replaces ndimage.binary_dilation / binary_erosion / binary_closing / binary_opening (x, structure=generate_binary_structure(3, c),
 * iterations) with their defaults (SaliencyAttention/eval.py:35, 41 call the closing with c = 2).  in, out: masks.
 * The rule: one dilation sets a voxel that is set or has a set neighbour; one erosion keeps a voxel that is set and whose neighbours are
 * all set.  Everything outside the array counts as 0 for BOTH (scipy's border_value = 0), so an erosion clears every voxel on a face that
 * has a neighbour outside -- a closing erodes what touches a face: a full 3 x 3 x 3 cube closes to its centre voxel.  REPRODUCED, on purpose.
 * iterations >= 1: CLOSE is `iterations` dilations, then `iterations` erosions; OPEN the other way round.
 * Scratch: one byte volume. */
int ps_binary_morph(ps_context* ctx, const void* in, int64_t d0, int64_t d1, int64_t d2, int32_t op, int32_t connectivity, int32_t iterations,
                    void* out, void* scratch, int64_t* scratch_bytes);

/* ---- component selection --------------------------------------------------------------------------------------------------------------------
 * Replaces get_largest_two_component(img, False, threshold) and remove_external_core(lab_main, lab_ext) (SaliencyAttention/utils.py:106-164,
 * which label with generate_binary_structure(3, 2): pass connectivity = 2 for theirs).  mask, out: masks; n = the number of components of
 * `mask`, size = a component's voxel count.  The decision is taken on the device from the counts.
 *   PS_KEEP_ABOVE        n == 1: the mask as it is (the threshold is NOT applied to a lone component -- the reference's rule, kept);
 *                        n == 0: empty; otherwise every component with size > threshold (strict).  threshold >= 0.
 *   PS_KEEP_LARGEST_TWO  n <= 1: the mask as it is; otherwise the largest component, and the second largest when 10 * size2 > size1.
 *                        Components of equal size rank by their label, the lower one first (the reference raises on such a tie).
 *   PS_KEEP_OVERLAP      every component of which at least half the voxels are non-zero in `main` (a mask of the same shape):
 *                        2 * overlap >= size, in integers.  The reference's fixed ratio 0.5.
 * threshold is read by PS_KEEP_ABOVE alone, main by PS_KEEP_OVERLAP alone (NULL otherwise).
 * Scratch: two int32 volumes (three for PS_KEEP_OVERLAP) and 256 bytes of counters. */
int ps_keep_components(ps_context* ctx, const void* mask, int64_t d0, int64_t d1, int64_t d2, int32_t connectivity, int32_t rule,
                       int64_t threshold, const void* main, void* out, void* scratch, int64_t* scratch_bytes);

/* ---- hole filling ---------------------------------------------------------------------------------------------------------------------------
 * Replaces ndimage.morphology.binary_fill_holes(x) with its default structure (SaliencyAttention/eval.py:402).  The rule: a hole is a
 * 6-connected component of the zero voxels that has no voxel on a face of the array; out = mask | holes.  The zero voxels
 * connect through faces alone, so a shell that hangs together by diagonals only (the six face neighbours of one voxel) still closes its
 * cavity, and a tunnel with a diagonal step does not open one.
 * Scratch: two int32 volumes and 256 bytes of counters. */
int ps_fill_holes(ps_context* ctx, const void* mask, int64_t d0, int64_t d1, int64_t d2, void* out, void* scratch, int64_t* scratch_bytes);

/* ---- the BraTS clean-up in one call -------------------------------------------------------------------------------------------------------
 * Replaces post_processing(pred1, temp_weight) (SaliencyAttention/eval.py:20-55).  pred: uint8 labels in {0, 1, 2, 4}; weight: a mask
 * (non-zero = brain) or NULL for none; out: uint8 labels.  The rule, in order:
 *   whole = pred > 0, core = pred > 0 and pred != 2, enh = pred == 4, each only where weight is set
 *   whole = PS_KEEP_ABOVE(close(whole), wt_threshold)                  close: PS_MORPH_CLOSE, connectivity 2, 1 iteration;
 *   core  = PS_KEEP_ABOVE(close(core & whole), wt_threshold)           components of connectivity 2
 *   enh   = enh & core; when count(whole) > 100 and 0 < count(enh) < 100, enh is cleared
 *   out   = 2 where whole, then 1 where core, then 4 where enh         (the closing may put core voxels outside whole: they are 1)
 * wt_threshold >= 0; the reference's value is 2000.
 * Scratch: one byte volume, two int32 volumes and 256 bytes of counters. */
int ps_brats_postprocess(ps_context* ctx, const void* pred, const void* weight, int64_t d0, int64_t d1, int64_t d2, int64_t wt_threshold,
                         void* out, void* scratch, int64_t* scratch_bytes);

#ifdef __cplusplus
}
#endif

#endif /* POINTSEG_POSTPROCESS_H */
