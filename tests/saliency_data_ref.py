"""numpy restatement of include/pointseg_saliency_data.h (csrc/saliency_data.hip): the preparation of a volume for the saliency network
(crop_brain_region / load_pancreas_img, SaliencyAttention/utils.py:30-78) and the patch sampler's rule (sampler3d and BatchData's reject
loop, SaliencyAttention/data_sampler.py:77-88, 169-214) as a pure function of (bank, cand, P, seed, mode).  uint32 arithmetic wraps mod 2^32.

    s(b, t)  = hash32(seed + 0x9E3779B9 * (b * T + t + 1))
    h_a      = hash32(s(b, t) + 0x85EBCA6B * (a + 1))                    a = 0, 1, 2
    centre_a = x0 + (h_a * (x1 - x0 + 1) >> 32)  with x0 = out // 2, x1 = in - x0   ((x0 + x1) // 2 when x1 <= x0)
    s_fill   = hash32(s(b, t) + 0x85EBCA6B * 4);  fill of element j = (hash32(j * 2654435761 ^ s_fill) >> 8) * 2^-24

test_saliency_data_rule.py holds it against the reference's own functions (tests/golden/saliency_data.npz); test_gpu_saliency_data.py
holds the kernels against it."""
import numpy as np

from dropout_ref import hash32, uniform

SEED_MUL = 0x9E3779B9
AXIS_MUL = 0x85EBCA6B
M32 = 0xFFFFFFFF
MODES = ("random", "all_positive", "one_positive")


# ---- preparation ---------------------------------------------------------------------------------------------------------------------------

def none_zero_box(vol, margin):
    """(bbmin, bbmax), inclusive: the box of vol != 0 grown by margin and clamped.  ValueError when vol is all zero."""
    nz = np.nonzero(vol)
    if nz[0].size == 0:
        raise ValueError("the volume is all zero")
    lo = [max(int(i.min()) - margin, 0) for i in nz]
    hi = [min(int(i.max()) + margin, n - 1) for i, n in zip(nz, vol.shape)]
    return lo, hi


def remap_labels(seg, num_class):
    seg = np.asarray(seg).copy()
    if num_class == 4:
        seg[seg == 4] = 3
    else:
        seg[seg == 4] = 1
        seg[seg == 2] = 1
    return seg


def brats_prepare(raw, seg=None, num_class=2, margin=5):
    """raw f32 [C, D, H, W], seg integer [D, H, W] or None -> {"box": (bbmin, bbmax), "image" f32 [d, h, w, C], "label" u8, "weight" u8}."""
    raw = np.asarray(raw, np.float32)
    lo, hi = none_zero_box(raw[0], margin)
    sl = tuple(slice(a, b + 1) for a, b in zip(lo, hi))
    crop = raw[(slice(None),) + sl]
    image = np.empty(crop.shape[1:] + (crop.shape[0],), np.float32)
    for c in range(crop.shape[0]):
        v = crop[c].astype(np.float64)
        pix = v[v > 0]
        if pix.size == 0:
            raise ValueError("modality %d has no voxel above zero" % c)
        mean, std = pix.mean(), pix.std()
        if not std > 0:
            raise ValueError("modality %d has std 0" % c)
        image[..., c] = np.where(v == 0, 0.0, (v - mean) / std).astype(np.float32)
    label = np.zeros(crop.shape[1:], np.uint8) if seg is None else remap_labels(seg, num_class)[sl].astype(np.uint8)
    return {"box": (lo, hi), "image": image, "label": label, "weight": (crop[0] > 0).astype(np.uint8)}


def pancreas_prepare(ct, label=None):
    """ct [D, H, W] -> {"image" f32 [D, H, W, 1] = float32((double(v) + 100) / 340), "label" u8 (zeros without one), "weight" u8 ones}."""
    ct = np.asarray(ct)
    image = ((ct.astype(np.float64) + 100.0) / 340.0).astype(np.float32)[..., None]
    lab = np.zeros(ct.shape, np.uint8) if label is None else np.asarray(label).astype(np.uint8)
    return {"image": image, "label": lab, "weight": np.ones(ct.shape, np.uint8)}


# ---- the sampler's rule --------------------------------------------------------------------------------------------------------------------

def try_seed(seed, b, t, T):
    return int(hash32((seed + SEED_MUL * (b * T + t + 1)) & M32))


def centre_range(n_in, n_out):
    """(x0, x1): the centre is drawn from [x0, x1], both included -- or is (x0 + x1) // 2 when x1 <= x0."""
    x0 = n_out // 2
    return x0, n_in - x0


def centre_from_hash(n_in, n_out, h):
    x0, x1 = centre_range(n_in, n_out)
    if x1 <= x0:
        return (x0 + x1) // 2
    return x0 + ((int(h) * (x1 - x0 + 1)) >> 32)


def centres(dims, P, s):
    """The centre of a try with seed s = s(b, t) in a volume of extents dims."""
    return [centre_from_hash(dims[a], P[a], hash32((s + AXIS_MUL * (a + 1)) & M32)) for a in range(3)]


def window(dims, P, centre):
    """Per axis (patch slice, volume slice) of extract_roi_from_volume."""
    out = []
    for a in range(3):
        half = P[a] // 2
        r0, r1 = min(half, centre[a]), min(P[a] - half, dims[a] - centre[a])
        out.append((slice(half - r0, half + r1), slice(centre[a] - r0, centre[a] + r1)))
    return out


def fill_seed(s):
    return int(hash32((s + AXIS_MUL * 4) & M32))


def extract(vol, P, centre, s_fill):
    """One slot from vol = {"image" [d, h, w, C], "label", "weight"}: (image f32 [P0, P1, P2, C], weight f32, label i32, pos)."""
    C = vol["image"].shape[3]
    P = tuple(P)
    image = uniform(P[0] * P[1] * P[2] * C, s_fill).reshape(P + (C,))
    weight = np.zeros(P, np.float32)
    label = np.zeros(P, np.int32)
    w = window(vol["label"].shape, P, centre)
    dst, src = tuple(x[0] for x in w), tuple(x[1] for x in w)
    image[dst] = vol["image"][src]
    weight[dst] = vol["weight"][src]
    label[dst] = vol["label"][src]
    return image, weight, label, int((vol["label"][src] > 0).sum())


def choose(pos, mode):
    """pos [B][T] -> [(try, ok)] per slot."""
    B, T = len(pos), len(pos[0])

    def first(b):
        for t in range(T):
            if pos[b][t] > 0:
                return t, 1
        return T - 1, 0

    if mode == "random":
        return [(0, 1)] * B
    if mode == "all_positive":
        return [first(b) for b in range(B)]
    if mode != "one_positive":
        raise ValueError(mode)
    out = [(0, 1)] * (B - 1)
    out.append((0, 1) if any(pos[b][0] > 0 for b in range(B - 1)) else first(B - 1))
    return out


def sample(bank, cand, P, seed, mode):
    """bank: a list of prepared volumes; cand int [B, T].  Returns (images, weights, labels, info) as ps_patch_sample writes them."""
    cand = np.asarray(cand)
    B, T = cand.shape
    C = bank[0]["image"].shape[3]
    P = tuple(int(p) for p in P)
    tries = [[None] * T for _ in range(B)]
    for b in range(B):
        for t in range(T):
            vol = bank[cand[b, t]]
            s = try_seed(seed, b, t, T)
            c = centres(vol["label"].shape, P, s)
            tries[b][t] = (c,) + extract(vol, P, c, fill_seed(s))
    picks = choose([[tries[b][t][4] for t in range(T)] for b in range(B)], mode)
    images = np.empty((B,) + P + (C,), np.float32)
    weights = np.empty((B,) + P, np.float32)
    labels = np.empty((B,) + P, np.int32)
    info = np.zeros((B, 8), np.int32)
    for b, (t, ok) in enumerate(picks):
        c, images[b], weights[b], labels[b], pos = tries[b][t]
        info[b] = [t, cand[b, t], c[0], c[1], c[2], pos, ok, 0]
    return images, weights, labels, info
