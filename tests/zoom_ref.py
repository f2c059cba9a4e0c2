"""numpy restatement of the rule ps_volume_zoom follows (include/pointseg_prepare.h): scipy.ndimage.zoom(x, zoom, order) with its defaults
(mode='constant', cval=0, prefilter=True, grid_mode=False) for 3-D int16 / uint8 / float32 input and order 0 or 3.  No scipy in here:
test_zoom_rule.py holds this file against scipy and against recorded scipy results, test_gpu_volume_zoom.py holds the kernels against it.

    shape    m = int(round(n * zoom)) per axis, Python's round (half to even) of the double product; the zoom is used for nothing else
    coord    cc = j * ((n - 1) / (m - 1)) in double (scale 0 when m == 1); cc > n - 1 (by rounding alone, e.g. 30 -> 15: j = 14 gives
             29.000000000000004) makes the output voxel 0
    order 3  float64 throughout: cubic B-spline prefilter along every axis of length >= 2 (pole sqrt(3) - 2, gain 6, mirror start),
             then the four taps floor(cc) - 1 .. + 2, indices mirrored about the end samples, tensor product over the axes
    order 0  the sample at floor(cc + 0.5)
    output   integers: +-0.5, clamp to the type's range, truncate (half away from zero, saturating); float32: one cast
"""
import numpy as np

POLE = np.sqrt(3.0) - 2.0
TIE_WINDOW = 1e-6  # |distance to a rounding tie| below which summation order decides an integer output


def out_shape(shape, zoom):
    z = (zoom,) * 3 if np.isscalar(zoom) else tuple(zoom)
    return tuple(int(round(n * f)) for n, f in zip(shape, z))


def coords(n, m):
    """cc[j] in double and the mask of the output indices scipy zeroes."""
    scale = (n - 1) / (m - 1) if m > 1 else 0.0
    cc = np.arange(m, dtype=np.float64) * scale
    return cc, cc > n - 1


def prefilter_axis(c, axis):
    """In place along `axis` of the float64 array c (length >= 2)."""
    c = np.moveaxis(c, axis, 0)
    n = c.shape[0]
    z = POLE
    c *= (1.0 - z) * (1.0 - 1.0 / z)
    acc = c[0] + z ** (n - 1) * c[n - 1]
    for i in range(1, n - 1):
        acc = acc + (z ** i + z ** (2 * n - 2 - i)) * c[i]
    c[0] = acc / (1.0 - z ** (2 * n - 2))
    for i in range(1, n):
        c[i] += z * c[i - 1]
    c[n - 1] = z / (z * z - 1.0) * (z * c[n - 2] + c[n - 1])
    for i in range(n - 2, -1, -1):
        c[i] = z * (c[i + 1] - c[i])


def mirror(i, n):
    """Index i (any integer array) mirrored about the end samples of a length-n axis: -1 -> 1, n -> n - 2, period 2 n - 2."""
    if n == 1:
        return np.zeros_like(i)
    p = 2 * n - 2
    i = np.mod(i, p)
    return np.where(i >= n, p - i, i)


def taps(n, m):
    """Per output index of one axis: weights f64 [m, 4], mirrored indices [m, 4], zeroed mask [m]."""
    cc, zero = coords(n, m)
    f = np.floor(cc)
    t = cc - f
    w = np.stack([(1 - t) ** 3 / 6, (3 * t ** 3 - 6 * t ** 2 + 4) / 6, (-3 * t ** 3 + 3 * t ** 2 + 3 * t + 1) / 6, t ** 3 / 6], -1)
    idx = mirror(f.astype(np.int64)[:, None] + np.arange(-1, 3)[None, :], n)
    return w, idx, zero


def to_dtype(v, dtype):
    """The float64 result -> the output dtype."""
    dtype = np.dtype(dtype)
    if dtype.kind == "f":
        return v.astype(dtype)
    info = np.iinfo(dtype)
    return np.trunc(np.clip(np.where(v > 0, v + 0.5, v - 0.5), info.min, info.max)).astype(dtype)


def zoom_f64(x, shape):
    """Order 3, before the output conversion: float64 [shape]."""
    c = np.array(x, dtype=np.float64)
    for a in range(3):
        if c.shape[a] >= 2:
            prefilter_axis(c, a)
    tp = [taps(n, m) for n, m in zip(x.shape, shape)]
    out = np.zeros(shape, np.float64)
    (w0, i0, z0), (w1, i1, z1), (w2, i2, z2) = tp
    for a in range(4):
        for b in range(4):
            for d in range(4):
                out += (w0[:, a, None, None] * w1[None, :, b, None] * w2[None, None, :, d]) * c[i0[:, a, None, None], i1[None, :, b, None], i2[None, None, :, d]]
    out[z0[:, None, None] | z1[None, :, None] | z2[None, None, :]] = 0.0
    return out


def zoom(x, zoom, order=3):
    """scipy.ndimage.zoom(x, zoom, order=order) for a 3-D array."""
    x = np.asarray(x)
    shape = out_shape(x.shape, zoom)
    if order == 3:
        return to_dtype(zoom_f64(x, shape), x.dtype)
    if order != 0:
        raise ValueError("order must be 0 or 3")
    sel, zero = [], []
    for n, m in zip(x.shape, shape):
        cc, z = coords(n, m)
        sel.append(np.minimum(np.floor(cc + 0.5).astype(np.int64), n - 1))
        zero.append(z)
    out = x[sel[0][:, None, None], sel[1][None, :, None], sel[2][None, None, :]].copy()
    out[zero[0][:, None, None] | zero[1][None, :, None] | zero[2][None, None, :]] = 0
    return out


def ties(x, shape):
    """Mask of the voxels whose float64 value, after the +-0.5 shift, lies within TIE_WINDOW of an integer: there the order of the sums
    decides which integer comes out, and a comparison leaves them out."""
    v = zoom_f64(x, shape)
    s = np.where(v > 0, v + 0.5, v - 0.5)
    return np.abs(s - np.round(s)) < TIE_WINDOW


# ---- the inputs of the test cases (the golden file holds scipy's outputs for cases 0 - 8) -------------------------------------------------

CASES = [
    ((23, 40, 37), 0.5),
    ((9, 16, 16), (2.5, 1, 1)),
    ((31, 30, 29), 0.5),
    ((2, 5, 4), 0.5),
    ((7, 11, 13), (0.75, 1, 1)),
    ((1, 6, 5), (1, 0.5, 0.5)),
    ((3, 3, 3), 2.0),
    ((40, 24, 24), (0.7, 1, 1)),
    ((24, 33, 65), (1, 0.5, 0.5)),
    ((70, 130, 67), 0.5),  # restatement only, not in the golden file
]
GOLDEN_CASES = 9


def case_inputs(k):
    """int16 CT, its float32 form (x 0.37) and a 0 / 1 / 2 label of case k."""
    shape = CASES[k][0]
    ct = np.random.default_rng(k).integers(-1024, 3072, shape).astype(np.int16)
    f32 = (ct * 0.37).astype(np.float32)
    seg = np.random.default_rng(1000 + k).integers(0, 3, shape).astype(np.uint8)
    return ct, f32, seg


# ---- the comparisons both test files make -----------------------------------------------------------------------------------------------
# order 0: equality.  int16 order 3: equality except on rounding ties, which may be at most 1 % of a case with a resampled axis shorter
# than 16 (a 7-long line makes the spline values rationals with a small denominator) and none otherwise.  float32 order 3: within
# 1e-9 * max|input| in float64 (a few hundred times the float64 summation-order differences, 1e5 below fp32 arithmetic) or one float32 ulp.

def check_i16(got, want, x, k):
    """int16 order 3 of the input x (case k, or any label) against scipy's / the restatement's `want`."""
    assert got.shape == want.shape and got.dtype == want.dtype
    tie = ties(x, want.shape)
    short = any(m != n and n < 16 for n, m in zip(x.shape, want.shape))
    print("case %s: %d ties of %d voxels, %d voxels differ, %d of them outside the ties" % (k, tie.sum(), tie.size, (got != want).sum(),
                                                                                            ((got != want) & ~tie).sum()))
    assert tie.sum() <= (0.01 * tie.size if short else 0)
    assert np.array_equal(got[~tie], want[~tie])


def check_f32(got, want, x, k):
    assert got.shape == want.shape and got.dtype == np.float32
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    ulp = np.spacing(np.abs(want))
    print("case %s: max |diff| = %.3e, bound %.3e" % (k, err.max(), 1e-9 * np.abs(x).max()))
    assert ((err <= 1e-9 * np.abs(x).astype(np.float64).max()) | (err <= ulp)).all()


# ---- the Pancreas chain (PointSegment/utils/cvt_CT_down.py:79-104, cvt_CT.py:79-105) on the restatement -----------------------------------

def crop_box(shape, crop):
    """cvt_CT.py:88-90: inclusive (start, end) per axis, clamped to the volume."""
    return tuple(slice(max(0, int(s)), min(n - 1, int(e)) + 1) for n, (s, e) in zip(shape, crop))


def resample_chain(ct, seg, spacing_z, slice_thickness=1, down_scale=0.5, lower=-100, upper=240, flip_y=False, crop=None):
    if spacing_z != slice_thickness:
        ct = zoom(ct, (spacing_z / slice_thickness, 1, 1), order=3)
        seg = zoom(seg, (spacing_z / slice_thickness, 1, 1), order=0)
    if flip_y:
        ct = np.flip(ct, 1)
    if crop is not None:
        box = crop_box(seg.shape, crop)
        ct, seg = ct[box], seg[box]
    if down_scale != 1:
        ct = zoom(ct, (down_scale,) * 3, order=3)
        seg = zoom(seg, (down_scale,) * 3, order=0)
    return np.clip(ct, lower, upper), seg
