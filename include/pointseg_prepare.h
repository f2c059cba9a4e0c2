/* include/pointseg_prepare.h -- dataset preparation in front of the entry points of pointseg.h that needs kernels of its own.  Same
 * conventions as pointseg.h (status codes, ps_last_error, caller-owned buffers, the context's stream); kept out of that header because
 * a host that only drives the network never needs it.  All citations are relative to the reference repository root.
 *
 * What each entry point replaces
 * ------------------------------
 *   ps_volume_zoom                     the resampling of a raw NIH Pancreas-CT volume, PointSegment/utils/cvt_CT_down.py:79-104 and
 *                                      cvt_CT.py:79-105: scipy.ndimage.zoom(ct, (spacing_z / 1, 1, 1), order=3) and zoom(ct, 0.5, order=3)
 *                                      on the int16 CT, the same two with order=0 on the uint8 label, np.flip(ct, 1) and the HU clip
 */
#ifndef POINTSEG_PREPARE_H
#define POINTSEG_PREPARE_H

#include "pointseg.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PS_VOLUME_U8 3 /* next to PS_VOLUME_I16 / PS_VOLUME_F32 */

/* ---- spline zoom of a volume (csrc/resample.hip) -------------------------------------------------------------------------------------------
 * Replaces scipy.ndimage.zoom(x, zoom, order) with its defaults (mode='constant', cval=0, prefilter=True, grid_mode=False) as
 * PointSegment/utils/cvt_CT_down.py:80, 82, 97, 99 and cvt_CT.py:80, 82, 98, 100 call it, with np.flip(ct_array, 1) (cvt_CT.py:85) and the
 * clip to [lower, upper] (cvt_CT_down.py:103-104, cvt_CT.py:104-105) fused in.  in / out: device memory, [n0, n1, n2] / [m0, m1, m2]
 * row-major, both of `dtype` (PS_VOLUME_I16 | PS_VOLUME_F32 | PS_VOLUME_U8); order 0 or 3.
 *
 * The rule (restated in tests/zoom_ref.py), per axis with n input and m output samples.  The caller passes the output shape -- scipy's is
 * m = int(round(n * zoom)) with Python's round -- and everything else follows from the two shapes:
 *     cc      = j * ((n - 1) / (m - 1)) in double, two operations (scale = 0 when m == 1)
 *     cc > n - 1 happens through rounding alone (30 -> 15: j = 14 gives 29.000000000000004); scipy then takes the voxel as outside
 *     the array and writes cval = 0 -- a whole plane of zeros at the far end of such an axis.  REPRODUCED here, on purpose.
 *     order 0 the sample at floor(cc + 0.5)
 *     order 3 float64 throughout: the cubic B-spline prefilter along every axis of length >= 2 (pole z = sqrt(3) - 2, gain 6, causal start
 *             c[0] = (c[0] + z^(n-1) c[n-1] + sum_{i=1..n-2} (z^i + z^(2n-2-i)) c[i]) / (1 - z^(2n-2)), anticausal start
 *             c[n-1] = z / (z^2 - 1) (z c[n-2] + c[n-1])), then the taps floor(cc) - 1 .. + 2 with weights (1-t)^3 / 6,
 *             (3t^3 - 6t^2 + 4) / 6, (-3t^3 + 3t^2 + 3t + 1) / 6, t^3 / 6 (t = cc - floor(cc)), tap indices mirrored about the end
 *             samples (-1 -> 1, n -> n - 2, period 2n - 2; a length-1 axis maps to 0), tensor product over the axes
 *     output  integers: t > 0 ? t + 0.5 : t - 0.5, clamp to the type's range, truncate; float32: (float) of the double
 * The order of the float64 sums is not scipy's: axes are filtered and interpolated one after the other (4 + 4 + 4 taps on shrinking
 * volumes), the start sum stops after 64 terms (|z|^64 < 1e-36), and for the integer dtypes an axis with m == n passes straight through
 * (its exact result is the input sample).  An int16 result can therefore differ from scipy's only where the float64 value sits on a
 * rounding tie to within the summation error; float32 results agree to ~1e-12 of the input's magnitude.
 *
 * flip_axes: bit a set = the input is read with axis a reversed (np.flip(in, a) in front of the zoom; exact, an index map).
 * clamp != 0: the output is limited to [clamp_lo, clamp_hi] after the rounding (np.clip behind the zoom; exact).  For the integer
 * dtypes both bounds must be integers inside the type's range.
 * Limits: every dimension in [1, 2^30], n0 * n1 * n2 < 2^31 and m0 * m1 * m2 < 2^31.
 * Scratch: two-call protocol as ps_volume_sample -- scratch == NULL only fills *scratch_bytes (order 3: two float64 volumes of at most
 * max(n0 n1 n2, m0 m1 m2) elements each, plus 48 bytes per output index of each axis; order 0: the latter alone).  That call works from
 * the shapes, dtype and order alone: in and out are not looked at and may be NULL, every other argument is checked as in the second
 * call.  The second call takes device memory of at least that size, 256-byte aligned, valid until the stream has passed the call.
 * Asynchronous on the context's stream, no synchronisation.  Every argument error returns PS_EINVAL before anything is enqueued. */
int ps_volume_zoom(ps_context* ctx, const void* in, int32_t dtype, int64_t n0, int64_t n1, int64_t n2,
                   int32_t order, int64_t m0, int64_t m1, int64_t m2, uint32_t flip_axes,
                   int32_t clamp, double clamp_lo, double clamp_hi,
                   void* out, void* scratch, int64_t* scratch_bytes);

#ifdef __cplusplus
}
#endif

#endif /* POINTSEG_PREPARE_H */
