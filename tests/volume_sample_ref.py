"""numpy restatement of ps_volume_sample (csrc/volume_sample.hip, include/pointseg.h): the Pancreas preparation of the reference
(PointSegment/utils/dataPreparePancreas.py:34-46, 132-169; utils/genBinaryMap.py:67-80; PointSegment/utils/over_sampling.py:58-65) as a pure
function of (volume, positive set, N, seed, loop).  v = (x * Y + y) * Z + z; uint32 arithmetic wraps mod 2^32; keys are uint64.

    M           = mask != 0, or probs[..., channel] >= float32(threshold); `dilate` rounds of the 6-neighbourhood dilation; OR truth != 0
    s_sel(l)    = hash32(seed + 0x9E3779B9 * (2l + 1))                       (cloud_sample_ref.slot_seeds, the loop as the slot)
    key_sel(v)  = hash32(v * 2654435761 ^ s_sel(l)) << 32 | v
    row t < P   of every loop: the t-th voxel of M in ascending v
    row P + t   of loop l: the voxel outside M with the t-th smallest key_sel

test_volume_sample_rule.py checks its statistics on the CPU; test_gpu_volume_sample.py checks the kernels against it bit for bit."""
import math

import numpy as np

from cloud_sample_ref import keys, slot_seeds


def threshold_mask(probs, channel=1, threshold=0.9):
    """probs [..., C] -> bool [...]: compared in float32, as `seg >= threshold` on the float32 array point2prod saved."""
    return np.asarray(probs, np.float32)[..., channel] >= np.float32(threshold)


def dilate(m, rounds=1):
    """scipy.ndimage.binary_dilation(m, iterations=rounds) with its default structure (6-neighbourhood, outside the array = 0), as shifted ORs."""
    m = np.asarray(m) != 0
    for _ in range(rounds):
        out = m.copy()
        for ax in range(m.ndim):
            lo = [slice(None)] * m.ndim
            hi = [slice(None)] * m.ndim
            lo[ax], hi[ax] = slice(0, -1), slice(1, None)
            out[tuple(hi)] |= m[tuple(lo)]
            out[tuple(lo)] |= m[tuple(hi)]
        m = out
    return m


def positive_mask(mask=None, probs=None, channel=1, threshold=0.9, dilate_rounds=0, truth=None):
    """M as uint8 0 / 1 of the volume's shape."""
    m = (np.asarray(mask) != 0) if mask is not None else threshold_mask(probs, channel, threshold)
    m = dilate(m, dilate_rounds)
    if truth is not None:
        m = m | (np.asarray(truth) != 0)
    return m.astype(np.uint8)


def sample_indices(mask, N, seed, loop):
    """The flat voxel indices of loop `loop`: int64 [N].  mask: anything whose != 0 is M (any shape; flattened in C order)."""
    pos_mask = np.asarray(mask).reshape(-1) != 0
    n = pos_mask.size
    pos = np.flatnonzero(pos_mask)
    P = len(pos)
    if not P <= N <= n:
        raise ValueError("need positives <= N <= n, got %d, %d, %d" % (P, N, n))
    need = N - P
    if need == 0:
        return pos
    bg = np.flatnonzero(~pos_mask)
    ks = keys(n, slot_seeds(seed, loop)[0])[bg]
    if need < len(bg):
        part = np.argpartition(ks, need - 1)[:need]
    else:
        part = np.arange(len(bg))
    part = part[np.argsort(ks[part])]
    return np.concatenate([pos, bg[part]])


def statistics(volume):
    """(mean, std) of all voxels in float64.  Integer volumes: exact integer sums, n * sum(x^2) - sum(x)^2 rounded once."""
    v = np.asarray(volume)
    if v.dtype.kind in "iu":
        x = v.reshape(-1).astype(np.int64)
        n, s, q = int(x.size), int(x.sum()), int((x * x).sum())
        return s / n, math.sqrt(float(n * q - s * s)) / n
    d = v.astype(np.float64)
    return float(d.mean()), float(d.std())


def values(volume, idx, mean, std):
    """(float32)(((double)raw - mean) / std) of the voxels idx."""
    raw = np.asarray(volume).reshape(-1)[idx].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return ((raw - mean) / std).astype(np.float32)


def rows(shape, idx):
    """origin int32 [..., 3] = (x, y, z) and xyz float32 [..., 3] = origin / shape (one float32 division) of flat indices idx."""
    X, Y, Z = shape
    idx = np.asarray(idx, np.int64)
    origin = np.stack([idx // (Y * Z), (idx // Z) % Y, idx % Z], -1).astype(np.int32)
    xyz = origin.astype(np.float32) / np.array([X, Y, Z], np.float32)
    return origin, xyz


def sample(volume, mask, N, loops, seed, label_src=None):
    """What ps_volume_sample writes for a FINAL mask M: dict of idx i32 [L,N], origin i32 [L,N,3], xyz f32 [L,N,3], features f32 [L,N,4],
    labels i32 [L,N], stats (mean, std), positives."""
    volume = np.asarray(volume)
    m = (np.asarray(mask) != 0).reshape(-1)
    idx = np.stack([sample_indices(m, N, seed, l) for l in range(loops)]) if N else np.zeros((loops, 0), np.int64)
    origin, xyz = rows(volume.shape, idx)
    mean, std = statistics(volume)
    val = values(volume, idx, mean, std)
    lab = (np.asarray(label_src).reshape(-1)[idx] if label_src is not None else m[idx]).astype(np.int32)
    return dict(idx=idx.astype(np.int32), origin=origin, xyz=xyz, features=np.concatenate([xyz, val[..., None]], -1).astype(np.float32), labels=lab,
                stats=(mean, std), positives=int(m.sum()))
