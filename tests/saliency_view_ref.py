"""numpy restatement of include/pointseg_saliency_view.h: the patch sampler and the mixed sampler through an anatomical view, with the
per-sample flip.  It IS the header's defining identity: saliency_data_ref.sample / saliency_mixup_ref.sample_mixup run on np.transpose'd
copies of every volume (transpose_volumes, SaliencyAttention/utils.py:80-104), followed by np.flip(..., -1) of the flagged drawn samples
(sampler3d, SaliencyAttention/data_sampler.py:190-207) -- for a mixed batch before the pairs are mixed.

test_saliency_view_rule.py holds it against the reference's own sampler3d (tests/golden/saliency_view.npz); test_gpu_saliency_view.py holds
the kernels against it."""
import numpy as np

import saliency_data_ref as ref
import saliency_mixup_ref as mref

VIEWS = ("axial", "sagittal", "coronal")
VIEW_ID = {"axial": 0, "sagittal": 1, "coronal": 2}
AXES = {"axial": (0, 1, 2), "sagittal": (2, 0, 1), "coronal": (1, 0, 2)}  # view axis a runs along volume axis AXES[view][a]


def to_view(vol, view):
    """A prepared volume {"image" [d, h, w, C], "label", "weight"} as the view's network sees it: contiguous permuted copies."""
    ax = AXES[view]
    return {"image": np.ascontiguousarray(np.transpose(vol["image"], ax + (3,))), "label": np.ascontiguousarray(np.transpose(vol["label"], ax)),
            "weight": np.ascontiguousarray(np.transpose(vol["weight"], ax))}


def view_bank(bank, view):
    return [to_view(v, view) for v in bank]


def box(dims, P, view, h):
    """saliency_sampler_plan.h's sampler_box: (ext, c, lo, n, vsrc, vn) of a candidate with centre hashes h[3] (view axes)."""
    ax = AXES[view]
    ext = [int(dims[ax[a]]) for a in range(3)]
    c = [ref.centre_from_hash(ext[a], P[a], h[a]) for a in range(3)]
    w = ref.window(ext, P, c)
    lo, n = [w[a][0].start for a in range(3)], [w[a][0].stop - w[a][0].start for a in range(3)]
    vsrc, vn = [0] * 3, [0] * 3
    for a in range(3):
        vsrc[ax[a]], vn[ax[a]] = w[a][1].start, n[a]
    return ext, c, lo, n, vsrc, vn


def _flip_bits(flip, drawn):
    bits = np.zeros(drawn, np.int32) if flip is None else np.asarray(flip, np.int32)
    assert bits.shape == (drawn,) and np.isin(bits, (0, 1)).all()
    return bits


def sample_view(bank, cand, P, seed, mode, view="axial", flip=None, permuted=None):
    """(images, weights, labels, info) as ps_patch_sample_view writes them.  bank: the volumes in VOLUME axes; permuted: view_bank(bank, view)
    when the caller keeps it."""
    cand = np.asarray(cand)
    bits = _flip_bits(flip, cand.shape[0])
    images, weights, labels, info = ref.sample(view_bank(bank, view) if permuted is None else permuted, cand, P, seed, mode)
    for b in np.nonzero(bits)[0]:
        images[b], weights[b], labels[b] = np.flip(images[b], 2), np.flip(weights[b], 2), np.flip(labels[b], 2)
    info[:, 7] = bits
    return images, weights, labels, info


def sample_mixup_view(bank, cand, P, seed, mode, K, gamma, view="axial", flip=None, permuted=None):
    """(images, weights, soft, info) as ps_patch_sample_mixup_view writes them: the drawn samples are flipped BEFORE they are mixed, so a flip
    on drawn sample b + 1 shows in slots b and b + 1.  Built from the B + 1 drawn samples themselves (the plain sampler's tries under the mixed
    choice), then saliency_mixup_ref's mix."""
    cand = np.asarray(cand)
    n, T = cand.shape
    B = n - 1
    P = tuple(int(p) for p in P)
    bits = _flip_bits(flip, n)
    vols = view_bank(bank, view) if permuted is None else permuted
    tries = [[None] * T for _ in range(n)]
    for i in range(n):
        for t in range(T):
            vol = vols[cand[i, t]]
            s = ref.try_seed(seed, i, t, T)
            c = ref.centres(vol["label"].shape, P, s)
            tries[i][t] = (c,) + ref.extract(vol, P, c, ref.fill_seed(s))
    picks = mref.choose_mixup([[tries[i][t][4] for t in range(T)] for i in range(n)], mode)
    info = np.zeros((n, 8), np.int32)
    drawn = []
    for i, (t, ok) in enumerate(picks):
        c, image, weight, label, pos = tries[i][t]
        if bits[i]:
            image, weight, label = np.flip(image, 2), np.flip(weight, 2), np.flip(label, 2)
        info[i] = [t, cand[i, t], c[0], c[1], c[2], pos, ok, bits[i]]
        drawn.append((image, weight, mref.one_hot(label, K)))
    images = np.stack([mref.mix(drawn[b][0], drawn[b + 1][0], gamma[b]) for b in range(B)])
    weights = np.stack([mref.mix_weights(drawn[b][1], drawn[b + 1][1]) for b in range(B)])
    soft = np.stack([mref.mix(drawn[b][2], drawn[b + 1][2], gamma[b]) for b in range(B)])
    return images, weights, soft, info
