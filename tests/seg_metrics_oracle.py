"""Test-side restatement of the evaluation metrics of the reference (utils/evaluationBraTS.py:13-64, evaluationPancreas.py:14-37) and of
medpy's hd95(result, reference, voxelspacing, connectivity=1), which those scripts import:

    border(M)   = M ^ binary_erosion(M, generate_binary_structure(3, 1), iterations=1)   (border_value 0: array faces are border)
    d_AB        = distance_transform_edt(~border(B), sampling=spacing)[border(A)]
    hd95        = np.percentile(np.hstack((d_PT, d_TP)), 95)

in two forms: with scipy (what medpy runs) and as an O(|A| |B|) brute force in numpy (no scipy).  medpy raises on an empty mask; the
rules of point_unet_amd.metrics are restated here: both empty -> 0, exactly one empty -> +inf.

Also the integer-formula volumes of the tests and of tests/golden/make_seg_metrics_golden.py: no RNG, no scipy, the same on every
machine.
"""
import numpy as np

BRATS_REGIONS = {"WT": (1, 2, 4), "TC": (1, 4), "ET": (4,)}
BRATS_SHAPE = (155, 240, 240)


# ---- metrics ------------------------------------------------------------------------------------------------------------------------
def dice(p, t):
    """evaluationBraTS.py:22-25"""
    sp, st = int(p.sum()), int(t.sum())
    if sp + st == 0:
        return 1.0
    return 2 * int(np.logical_and(p, t).sum()) / (sp + st)


def border_scipy(m):
    from scipy.ndimage import binary_erosion, generate_binary_structure
    m = np.asarray(m, bool)
    return m ^ binary_erosion(m, structure=generate_binary_structure(m.ndim, 1), iterations=1)


def border_numpy(m):
    """The same 6-neighbourhood border with array shifts: a voxel of M with a neighbour outside M or outside the array."""
    m = np.asarray(m, bool)
    pad = np.pad(m, 1, constant_values=False)
    inner = np.ones_like(m)
    for a in range(3):
        for s in (-1, 1):
            inner &= np.roll(pad, s, axis=a)[1:-1, 1:-1, 1:-1]
    return m & ~inner


def _percentile95(d):
    return float(np.percentile(d, 95))


def hd95_scipy(p, t, spacing=(1.0, 1.0, 1.0)):
    from scipy.ndimage import distance_transform_edt
    p, t = np.asarray(p, bool), np.asarray(t, bool)
    if not p.any() and not t.any():
        return 0.0
    if not p.any() or not t.any():
        return float("inf")
    bp, bt = border_scipy(p), border_scipy(t)
    d_pt = distance_transform_edt(~bt, sampling=spacing)[bp]
    d_tp = distance_transform_edt(~bp, sampling=spacing)[bt]
    return _percentile95(np.hstack((d_pt, d_tp)))


def _nearest(a, b, spacing, chunk=2048):
    """for every row of a (integer index triples): the distance to the nearest row of b, float64"""
    sp = np.asarray(spacing, np.float64)
    A, B = a.astype(np.float64) * sp, b.astype(np.float64) * sp
    out = np.empty(len(A))
    for i in range(0, len(A), chunk):
        d2 = ((A[i:i + chunk, None, :] - B[None, :, :]) ** 2).sum(-1)
        out[i:i + chunk] = np.sqrt(d2.min(1))
    return out


def hd95_brute(p, t, spacing=(1.0, 1.0, 1.0)):
    p, t = np.asarray(p, bool), np.asarray(t, bool)
    if not p.any() and not t.any():
        return 0.0
    if not p.any() or not t.any():
        return float("inf")
    bp, bt = np.argwhere(border_numpy(p)), np.argwhere(border_numpy(t))
    return _percentile95(np.hstack((_nearest(bp, bt, spacing), _nearest(bt, bp, spacing))))


def region_metrics(pred, truth, regions=BRATS_REGIONS, spacing=(1.0, 1.0, 1.0), brute=False):
    """{name: {"dice", "hd95", "n_pred", "n_truth", "n_both"}} -- what point_unet_amd.metrics.segmentation_metrics returns"""
    out = {}
    for name, labels in regions.items():
        p, t = np.isin(pred, labels), np.isin(truth, labels)
        hd = (hd95_brute if brute else hd95_scipy)(p, t, spacing)
        out[name] = {"dice": dice(p, t), "hd95": hd, "n_pred": int(p.sum()), "n_truth": int(t.sum()),
                     "n_both": int(np.logical_and(p, t).sum())}
    return out


# ---- volumes from integer formulas --------------------------------------------------------------------------------------------------
def _grid(shape):
    return np.meshgrid(*[np.arange(n, dtype=np.int64) for n in shape], indexing="ij")


def hash3(x, y, z):
    h = (x * 73856093) ^ (y * 19349663) ^ (z * 83492791)
    h = (h ^ (h >> 13)) * 1274126177
    return (h ^ (h >> 16)) & 0x7FFFFFFF


def _ellipsoid(g, c, r):
    """integer test: sum ((i - c) * R / r)^2 <= R^2 with R = prod r (no floating point)"""
    R = int(np.prod(r))
    acc = 0
    for gi, ci, ri in zip(g, c, r):
        acc = acc + ((gi - ci) * (R // ri)) ** 2
    return acc <= R * R


def label_pair(shape, variant=0):
    """A (pred, truth) pair of uint8 BraTS-style label volumes {0, 1, 2, 4}: nested ellipsoids (WT 2 > TC 1 > ET 4), a box that touches
    two array faces, a one-voxel-thin sheet, a single voxel, a second component and hash speckle; `variant` shifts pred against truth."""
    g = _grid(shape)
    x, y, z = g
    n = np.array(shape, np.int64)
    c = n // 2
    truth = np.zeros(shape, np.uint8)
    r = np.maximum(n * 3 // 10, 2)
    truth[_ellipsoid(g, c, r)] = 2
    truth[_ellipsoid(g, c + [1, -2, 1], np.maximum(r * 3 // 5, 1))] = 1
    truth[_ellipsoid(g, c + [2, 0, -1], np.maximum(r * 3 // 10, 1))] = 4
    truth[(x < n[0] // 5) & (y < n[1] // 6) & (z >= n[2] - n[2] // 4)] = 4           # box on two faces
    truth[(x == n[0] - 2) & (y >= 1) & (y < n[1] - 1)] = 1                            # thin sheet
    truth[(hash3(x, y, z) % 211 == 0)] = 2                                          # speckle
    pred = np.zeros(shape, np.uint8)
    s = np.array([1 + variant, -1 - 2 * variant, 2], np.int64)
    pred[_ellipsoid(g, c + s, r + [1, -1, 0])] = 2
    pred[_ellipsoid(g, c + s + [0, -1, 2], np.maximum(r * 3 // 5 - 1, 1))] = 1
    pred[_ellipsoid(g, c + s + [3, 1, -1], np.maximum(r * 3 // 10, 1))] = 4
    pred[(x < n[0] // 4) & (y < n[1] // 6 + 1) & (z >= n[2] - n[2] // 4 - 1)] = 4
    pred[_ellipsoid(g, [n[0] - n[0] // 6, n[1] // 5, n[2] // 5], np.maximum(n // 12, 1))] = 1  # a second component
    pred[(y == n[1] - 3) & (x >= 2) & (x < n[0] - 2)] = 2                             # thin sheet on another axis
    pred[(hash3(z, x, y) % 173 == 0)] = 4                                           # speckle
    pred[n[0] - 1, n[1] - 1, 0] = 4                                                 # single corner voxel
    return pred, truth


CLASS_OF_LABEL = {0: 0, 1: 1, 2: 2, 4: 3}  # inverse of genSegmentationBraTS.py:76's class 3 -> label 4


def chain_points(pred, n=180000):
    """The sampled voxels of the full-chain case: the n non-zero voxels of pred with the smallest hash (ties by index), as (i0, i1, i2)
    rows, and the label volume that results when only they carry their label (every other voxel is unsampled: label 0)."""
    idx = np.flatnonzero(pred)
    ijk = np.stack(np.unravel_index(idx, pred.shape), 1).astype(np.int64)
    h = hash3(ijk[:, 0], ijk[:, 1], ijk[:, 2])
    sel = ijk[np.lexsort((idx, h))[:n]]
    out = np.zeros_like(pred)
    out[sel[:, 0], sel[:, 1], sel[:, 2]] = pred[sel[:, 0], sel[:, 1], sel[:, 2]]
    return sel, out
