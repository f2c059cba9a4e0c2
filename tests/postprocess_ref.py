"""numpy restatement of the rules of include/pointseg_postprocess.h: connected components with raster-order numbering, binary
morphology with a zero border for dilation AND erosion, the three component-selection rules, hole filling and the BraTS chain.  No scipy
here; test_postprocess_rule.py ties this file to scipy's and the reference's recorded results (golden/postprocess.npz), and
test_gpu_postprocess.py ties the kernels to this file.

The inputs are integer formulas of the voxel coordinates (no RNG), so they are the same arrays on every machine."""
import numpy as np

KEEP_ABOVE, KEEP_LARGEST_TWO, KEEP_OVERLAP = 1, 2, 3


def offsets(connectivity):
    """The neighbourhood of generate_binary_structure(3, c) without its centre: at most c coordinates differ, each by 1."""
    return [(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1) if 0 < abs(a) + abs(b) + abs(c) <= connectivity]


def _shift(x, off):
    """y[p] = x[p + off], zero where p + off is outside the array."""
    y = np.zeros_like(x)
    src, dst = [], []
    for n, o in zip(x.shape, off):
        if abs(o) >= n:
            return y
        src.append(slice(max(o, 0), n + min(o, 0)))
        dst.append(slice(max(-o, 0), n + min(-o, 0)))
    y[tuple(dst)] = x[tuple(src)]
    return y


# ---- connected components ---------------------------------------------------------------------------------------------------------------

def label(volume, connectivity=1, background=False):
    """(labels int32, n, sizes int32[n], touches uint8[n]).  Union-find with root = smallest linear index; component k is the one whose
    smallest linear index is the k-th smallest."""
    fg = (np.asarray(volume) == 0) if background else (np.asarray(volume) != 0)
    shape, V = fg.shape, fg.size
    idx = np.arange(V, dtype=np.int64).reshape(shape)
    us, vs = [], []
    for off in offsets(connectivity):
        if off > (0, 0, 0):
            continue  # each pair once
        both = fg & _shift(fg, off)
        us.append(idx[both])
        vs.append(_shift(idx, off)[both])
    u, v = np.concatenate(us), np.concatenate(vs)
    par = np.arange(V, dtype=np.int64)
    while True:
        pu, pv = par[u], par[v]
        hi, lo = np.maximum(pu, pv), np.minimum(pu, pv)
        m = hi != lo
        if not m.any():
            break
        np.minimum.at(par, hi[m], lo[m])  # a parent only decreases
        while True:
            pp = par[par]
            if np.array_equal(pp, par):
                break
            par = pp
    flat = fg.reshape(-1)
    roots = np.flatnonzero(flat & (par == np.arange(V)))  # ascending: the numbering
    rank = np.zeros(V, np.int64)
    rank[roots] = np.arange(1, len(roots) + 1)
    labels = np.where(flat, rank[par], 0).astype(np.int32).reshape(shape)
    n = len(roots)
    sizes = np.bincount(labels.reshape(-1), minlength=n + 1)[1:].astype(np.int32)
    face = np.zeros(shape, bool)
    for a in range(3):
        sl = [slice(None)] * 3
        for e in (0, -1):
            sl[a] = e
            face[tuple(sl)] = True
    touches = np.zeros(n + 1, np.uint8)
    touches[np.unique(labels[face])] = 1
    return labels, n, sizes, touches[1:]


# ---- morphology -------------------------------------------------------------------------------------------------------------------------

def dilate(mask, connectivity, iterations=1):
    m = np.asarray(mask) != 0
    for _ in range(iterations):
        out = m.copy()
        for off in offsets(connectivity):
            out |= _shift(m, off)
        m = out
    return m.astype(np.uint8)


def erode(mask, connectivity, iterations=1):
    """Outside the array counts as 0 here too: a voxel with a neighbour outside goes."""
    m = np.asarray(mask) != 0
    for _ in range(iterations):
        out = m.copy()
        for off in offsets(connectivity):
            out &= _shift(m, off)
        m = out
    return m.astype(np.uint8)


def closing(mask, connectivity, iterations=1):
    return erode(dilate(mask, connectivity, iterations), connectivity, iterations)


def opening(mask, connectivity, iterations=1):
    return dilate(erode(mask, connectivity, iterations), connectivity, iterations)


MORPH = {1: dilate, 2: erode, 3: closing, 4: opening}  # PS_MORPH_*


# ---- selection --------------------------------------------------------------------------------------------------------------------------

def keep_components(mask, rule, connectivity=2, threshold=0, main=None):
    m = (np.asarray(mask) != 0).astype(np.uint8)
    labels, n, sizes, _ = label(m, connectivity)
    sizes = sizes.astype(np.int64)
    if rule == KEEP_ABOVE:
        if n == 1:
            return m  # the threshold is not applied to a lone component
        keep = sizes > threshold
    elif rule == KEEP_LARGEST_TWO:
        if n <= 1:
            return m
        order = sorted(range(n), key=lambda k: (-sizes[k], k))  # ties: the lower label first
        keep = np.zeros(n, bool)
        keep[order[0]] = True
        if 10 * sizes[order[1]] > sizes[order[0]]:
            keep[order[1]] = True
    elif rule == KEEP_OVERLAP:
        overlap = np.bincount(labels[np.asarray(main) != 0].reshape(-1), minlength=n + 1)[1:]
        keep = 2 * overlap >= sizes
    else:
        raise ValueError(rule)
    return np.concatenate([[False], keep])[labels].astype(np.uint8)


def fill_holes(mask):
    m = np.asarray(mask) != 0
    labels, n, _, touches = label(m, 1, background=True)
    hole = np.concatenate([[False], touches == 0])[labels]
    return (m | hole).astype(np.uint8)


def brats_post_processing(pred, weight=None, wt_threshold=2000):
    p = np.asarray(pred).astype(np.int64)
    if weight is not None:
        p = np.where(np.asarray(weight) != 0, p, 0)
    whole, core, enh = p > 0, (p > 0) & (p != 2), p == 4
    whole = keep_components(closing(whole, 2), KEEP_ABOVE, 2, wt_threshold) != 0
    core = keep_components(closing(core & whole, 2), KEEP_ABOVE, 2, wt_threshold) != 0
    enh = enh & core
    if whole.sum() > 100 and 0 < enh.sum() < 100:
        enh[...] = False
    out = 2 * whole.astype(np.uint8)
    out[core] = 1
    out[enh] = 4
    return out


# ---- inputs: integer formulas of the coordinates ------------------------------------------------------------------------------------------

def _grid(shape):
    return np.meshgrid(*[np.arange(n, dtype=np.int64) for n in shape], indexing="ij")


def _ball(shape, centre, radii):
    """Integer ellipsoid test: sum ((x - c) * (R / r))^2 <= R^2 with R = 840, a multiple of every radius used."""
    x = _grid(shape)
    return sum(((x[a] - centre[a]) * (840 // radii[a])) ** 2 for a in range(3)) <= 840 * 840


def _hash(shape, salt):
    x, y, z = _grid(shape)
    h = (x * 73856093 + y * 19349663 + z * 83492791 + salt * 2654435761) & 0xFFFFFFFF
    h = ((h ^ (h >> 15)) * 2246822519) & 0xFFFFFFFF
    return h ^ (h >> 13)


def specks(shape, one_in, salt=0):
    return (_hash(shape, salt) % one_in == 0).astype(np.uint8)


def checkerboard(shape):
    x, y, z = _grid(shape)
    return ((x + y + z) % 2 == 0).astype(np.uint8)


def serpentine(shape, step=2):
    """A one-voxel-wide path: every `step`-th row along the last axis, joined at alternating ends, the planes of every `step`-th first
    index joined the same way.  One component at every connectivity."""
    d0, d1, d2 = shape
    m = np.zeros(shape, np.uint8)
    rows = list(range(0, d1, step))
    end = 0  # the end of the last axis at which the path currently stands
    planes = list(range(0, d0, step))
    for pi, i in enumerate(planes):
        order = rows if pi % 2 == 0 else rows[::-1]
        for ri, j in enumerate(order):
            m[i, j, :] = 1
            end = d2 - 1 - end
            if ri + 1 < len(order):
                a, b = sorted((j, order[ri + 1]))
                m[i, a:b + 1, end] = 1
        if pi + 1 < len(planes):
            m[i:planes[pi + 1] + 1, order[-1], end] = 1
    return m


def blobs_and_specks(shape, salt=0):
    """Three ellipsoids of distinct sizes scaled to the shape, plus isolated noise."""
    d = np.array(shape)
    m = np.zeros(shape, bool)
    for c, r in (((0.3, 0.3, 0.3), (0.22, 0.2, 0.2)), ((0.7, 0.7, 0.65), (0.15, 0.14, 0.16)), ((0.25, 0.8, 0.8), (0.08, 0.09, 0.1))):
        radii = [_radius(max(1, int(r[a] * d[a]))) for a in range(3)]
        m |= _ball(shape, [int(c[a] * d[a]) for a in range(3)], radii)
    return (m | (specks(shape, 37, salt) != 0)).astype(np.uint8)


def _radius(r):
    """The nearest radius not above r that divides 840."""
    while 840 % r:
        r -= 1
    return r


GOLDEN_SHAPE = (32, 40, 48)


def brats_pred(variant):
    """A prediction at GOLDEN_SHAPE: a large tumour (whole > core > enhancing), a second whole-tumour blob of a few hundred voxels with a
    core of its own, and label noise.  variant 0: an enhancing region of several hundred voxels (kept); variant 1: one below 100 voxels
    (cleared by the small-enhancing-region rule)."""
    s = GOLDEN_SHAPE
    p = np.zeros(s, np.uint8)
    p[_ball(s, (16, 20, 24), (12, 15, 20))] = 2
    p[_ball(s, (16, 20, 24), (8, 10, 14))] = 1
    p[_ball(s, (16, 20, 24), (5, 6, 7) if variant == 0 else (1, 2, 2))] = 4
    p[_ball(s, (5, 6, 6), (4, 4, 5))] = 2
    p[_ball(s, (5, 6, 6), (2, 2, 2))] = 1
    h = _hash(s, 11 + variant)
    noise = h % 41 == 0
    p[noise] = np.array([1, 2, 4, 0], np.uint8)[(h[noise] >> 8) % 4]
    return p


def brats_weight():
    """The brain: an ellipsoid that cuts the large tumour's rim and most of the second blob."""
    return _ball(GOLDEN_SHAPE, (17, 21, 25), (14, 15, 21)).astype(np.uint8)


def two_blob_mask(ratio_kept):
    """KEEP_LARGEST_TWO input at GOLDEN_SHAPE: the second largest is above (True) or below (False) a tenth of the largest; specks."""
    s = GOLDEN_SHAPE
    m = _ball(s, (14, 18, 20), (10, 12, 14)) | _ball(s, (25, 32, 39), (6, 7, 8) if ratio_kept else (2, 3, 3)) | _ball(s, (4, 34, 8), (2, 2, 3))
    far = ~dilate(m, 3, 2).astype(bool)
    return (m | ((specks(s, 53, 5) != 0) & far)).astype(np.uint8)


def overlap_masks():
    """KEEP_OVERLAP input at GOLDEN_SHAPE: (main, ext).  ext holds boxes of distinct sizes: inside main, mostly inside, exactly half
    inside (kept: 2 * overlap >= size), mostly outside, and outside."""
    s = GOLDEN_SHAPE
    main, ext = np.zeros(s, np.uint8), np.zeros(s, np.uint8)
    main[4:20, 4:30, 4:30] = 1
    ext[6:10, 6:10, 6:10] = 1        # 64, inside
    ext[17:22, 8:12, 8:12] = 1       # 80, 48 inside
    ext[18:22, 20:24, 20:23] = 1     # 48, 24 inside: exactly half
    ext[18:25, 14:17, 14:17] = 1     # 63, 18 inside
    ext[26:30, 32:38, 40:45] = 1     # 120, outside
    return main, ext


def hole_cases(shape=GOLDEN_SHAPE):
    """Five objects: (1) a box shell around a cavity: filled; (2) the same against the first face with one wall voxel out, a tunnel to the
    face: not filled; (3) the six face neighbours of one voxel, a shell that hangs together by diagonals alone: its centre is filled;
    (4) a shell whose two-voxel wall is pierced by a tunnel with a corner-diagonal step: the zero voxels connect through faces only, so
    the cavity and the inner tunnel voxel are filled, the outer tunnel voxel is not; (5) a shell in the cavity of a shell: all filled."""
    m = np.zeros(shape, np.uint8)
    m[10:17, 2:9, 2:9] = 1
    m[11:16, 3:8, 3:8] = 0
    m[0:7, 12:19, 2:9] = 1
    m[1:6, 13:18, 3:8] = 0
    m[0, 15, 5] = 0
    for a in range(3):
        for e in (-1, 1):
            q = [20, 5, 20]
            q[a] += e
            m[tuple(q)] = 1
    m[0:8, 22:29, 2:9] = 1
    m[2:7, 23:28, 3:8] = 0
    m[1, 25, 5] = 0
    m[0, 26, 6] = 0
    m[12:23, 12:23, 20:31] = 1
    m[13:22, 13:22, 21:30] = 0
    m[15:20, 15:20, 23:28] = 1
    m[16:19, 16:19, 24:27] = 0
    return m
