"""numpy restatement of the training-batch sampler of csrc/cloud_sample.hip (ps_cloud_sample, include/pointseg.h): the rule of the
reference's BraTS generator (PointSegment/runBraTS.py:91-130) -- every positive point, a uniform subset of the background up to N points,
a uniform permutation -- as a pure function of (cloud, labels, N, seed, slot).  uint32 arithmetic wraps mod 2^32; keys are uint64.

    s_sel(b)    = hash32(seed + 0x9E3779B9 * (2b + 1))
    s_perm(b)   = hash32(seed + 0x9E3779B9 * (2b + 2))
    key_sel(i)  = hash32(i * 2654435761 ^ s_sel(b))  << 32 | i
    key_perm(i) = hash32(i * 2654435761 ^ s_perm(b)) << 32 | i
    S           = {label > 0} + the N - |positives| background points with the smallest key_sel
    row t       = the element of S with the t-th smallest key_perm

test_cloud_sample_rule.py checks its statistics on the CPU; test_gpu_cloud_sample.py checks the kernels against it bit for bit."""
import numpy as np

from dropout_ref import INDEX_MUL, hash32

SEED_MUL = 0x9E3779B9
M32 = 0xFFFFFFFF


def slot_seeds(seed, b):
    """(s_sel, s_perm) of slot b."""
    s_sel = hash32((seed + SEED_MUL * (2 * b + 1)) & M32)
    s_perm = hash32((seed + SEED_MUL * (2 * b + 2)) & M32)
    return np.uint32(s_sel), np.uint32(s_perm)


def hashes(n, s):
    """hash32(i * 2654435761 ^ s) for i < n, uint32."""
    i = np.arange(n, dtype=np.uint32)
    with np.errstate(over="ignore"):
        return hash32((i * np.uint32(INDEX_MUL)) ^ np.uint32(s))


def keys(n, s):
    """hash << 32 | i for i < n, uint64 (unique: the index breaks every tie of the hash)."""
    return (hashes(n, s).astype(np.uint64) << np.uint64(32)) | np.arange(n, dtype=np.uint64)


def sample_indices(labels, n, N, seed, b):
    """The cloud-local indices of slot b: int64 [N].  labels: integer [n] or None (all background)."""
    pos = np.zeros(n, bool) if labels is None else np.asarray(labels).reshape(-1)[:n] > 0
    P = int(pos.sum())
    if not P <= N <= n:
        raise ValueError("need positives <= N <= n, got %d, %d, %d" % (P, N, n))
    s_sel, s_perm = slot_seeds(seed, b)
    bg = np.flatnonzero(~pos)
    need = N - P
    S = np.flatnonzero(pos)
    if need:
        ks = keys(n, s_sel)[bg]
        S = np.concatenate([S, bg[np.argpartition(ks, need - 1)[:need]]])
    kp = keys(n, s_perm)[S]
    return S[np.argsort(kp, kind="stable")]


def sample(xyz, modalities, labels, offsets, positives, cloud_ids, N, seed):
    """The batch ps_cloud_sample writes: xyz f32 [B,N,3], features f32 [B,N,3+C] = [xyz | modalities], labels i32 [B,N] (zeros without
    labels), idx i32 [B,N] (cloud-local).  xyz [total,3], modalities [total,C], labels [total] or None, offsets [n_clouds+1]."""
    del positives  # (the device recounts them; the rule does not need them)
    B = len(cloud_ids)
    C = modalities.shape[1]
    out_xyz = np.empty((B, N, 3), np.float32)
    out_f = np.empty((B, N, 3 + C), np.float32)
    out_l = np.zeros((B, N), np.int32)
    out_i = np.empty((B, N), np.int32)
    for b, c in enumerate(cloud_ids):
        r0, r1 = int(offsets[c]), int(offsets[c + 1])
        lab = None if labels is None else labels[r0:r1]
        idx = sample_indices(lab, r1 - r0, N, seed, b)
        rows = r0 + idx
        out_i[b] = idx
        out_xyz[b] = xyz[rows]
        out_f[b, :, :3] = xyz[rows]
        out_f[b, :, 3:] = modalities[rows]
        if labels is not None:
            out_l[b] = labels[rows]
    return out_xyz, out_f, out_l, out_i


def batch_seed(seed, epoch, batch, rank=0):
    """CloudBank.epoch_batches' seed of batch `batch` of epoch `epoch` on rank `rank` (point-unet_amd/dataset.py)."""
    x = int(hash32((seed + 0x9E3779B9 * (epoch + 1)) & M32))
    x = int(hash32((x + 0x85EBCA6B * (batch + 1)) & M32))
    return int(hash32((x + 0xC2B2AE35 * (rank + 1)) & M32))
