"""numpy / torch restatement of include/pointseg_saliency_mixup.h: the mixed batch (the one-hot labels of SaliencyAttention/data_sampler.py:
329-337, BatchData.get_data's holder of B + 1 samples, data_sampler.py:77-96, and mixup, SaliencyAttention/utils.py:511-527) on top of
saliency_data_ref.py's seeds, centres, windows and extraction, and dice_mixup (SaliencyAttention/model.py:550-590, 602-612) in torch.

    g = float32(gamma), h = float32(1.0 - gamma)        (the subtraction in float64)
    mixed = fl32(fl32(g * a) + fl32(h * b))             images and one-hot rows alike; weight = (w1 != 0) | (w2 != 0)

test_saliency_mixup_rule.py holds `mix` against the reference's own mixup (tests/golden/saliency_mixup.npz); test_gpu_saliency_mixup.py holds
the kernels against this file."""
import numpy as np
import torch

import saliency_data_ref as ref


def mix(a, b, gamma):
    """fl32(fl32(g * a) + fl32(h * b)) of two float32 arrays: every product and the sum rounded to float32 on its own."""
    g, h = np.float32(gamma), np.float32(1.0 - float(gamma))
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return ((g * a).astype(np.float32) + (h * b).astype(np.float32)).astype(np.float32)


def mix_weights(w1, w2):
    return np.logical_or(np.asarray(w1) != 0, np.asarray(w2) != 0).astype(np.float32)


def one_hot(label, K):
    """float32 [..., K]; a label >= K gives an all-zero row."""
    return (np.asarray(label)[..., None] == np.arange(K)).astype(np.float32)


def choose_mixup(pos, mode):
    """pos [B + 1][T], one row per DRAWN sample -> [(try, ok)] per sample.  one_positive: the reject loop's check fires when the holder has
    B - 1 samples, so sample B - 1 is the forced one and sample B is free."""
    n, T = len(pos), len(pos[0])
    B = n - 1
    if B < 1:
        raise ValueError("a mixed batch needs at least two samples")

    def first(i):
        for t in range(T):
            if pos[i][t] > 0:
                return t, 1
        return T - 1, 0

    if mode == "random":
        return [(0, 1)] * n
    if mode == "all_positive":
        return [first(i) for i in range(n)]
    if mode != "one_positive":
        raise ValueError(mode)
    out = [(0, 1)] * n
    if not any(pos[i][0] > 0 for i in range(B - 1)):
        out[B - 1] = first(B - 1)
    return out


def sample_mixup(bank, cand, P, seed, mode, K, gamma, cache=None):
    """bank: a list of prepared volumes; cand int [B + 1, T]; gamma float64 [B].  Returns (images [B, P, C], weights [B, P], soft [B, P, K],
    info [B + 1, 8]) as ps_patch_sample_mixup writes them.  cache: a dict that keeps the extracted tries between calls on ONE bank (a try is
    a function of its volume, P, seed, i, t and T)."""
    cand = np.asarray(cand)
    n, T = cand.shape
    B = n - 1
    P = tuple(int(p) for p in P)
    tries = [[None] * T for _ in range(n)]
    for i in range(n):
        for t in range(T):
            key = (int(cand[i, t]), P, int(seed), i, t, T)
            hit = None if cache is None else cache.get(key)
            if hit is None:
                vol = bank[cand[i, t]]
                s = ref.try_seed(seed, i, t, T)
                c = ref.centres(vol["label"].shape, P, s)
                hit = (c,) + ref.extract(vol, P, c, ref.fill_seed(s))
                if cache is not None:
                    cache[key] = hit
            tries[i][t] = hit
    picks = choose_mixup([[tries[i][t][4] for t in range(T)] for i in range(n)], mode)
    info = np.zeros((n, 8), np.int32)
    drawn = []
    for i, (t, ok) in enumerate(picks):
        c, image, weight, label, pos = tries[i][t]
        info[i] = [t, cand[i, t], c[0], c[1], c[2], pos, ok, 0]
        drawn.append((image, weight, one_hot(label, K)))
    images = np.stack([mix(drawn[b][0], drawn[b + 1][0], gamma[b]) for b in range(B)])
    weights = np.stack([mix_weights(drawn[b][1], drawn[b + 1][1]) for b in range(B)])
    soft = np.stack([mix(drawn[b][2], drawn[b + 1][2], gamma[b]) for b in range(B)])
    return images, weights, soft, info


def soft_dice_loss(logits, soft, weight=None):
    """dice_mixup: logits [B, ..., C], soft [B, ..., C], weight [B, ...] or None (ones) -> the 0-dim loss, in the logits' dtype.
    saliency_train_ref.softmax_dice_loss with [g = c] replaced by g_vc."""
    B, C = logits.shape[0], logits.shape[-1]
    p = torch.softmax(logits.reshape(B, -1, C), -1)
    g = soft.reshape(B, -1, C).to(p.dtype)
    w = torch.ones(g.shape[:2], dtype=p.dtype, device=p.device) if weight is None else weight.reshape(B, -1).to(p.dtype)
    w = w[..., None]
    num = 2.0 * (w * g * p).sum(1)
    den = (w * p * p).sum(1) + (w * g).sum(1) + 1e-5
    return (1.0 - (num / den).mean(1)).mean()
