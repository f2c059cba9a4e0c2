"""Clouds and oracle results shared by the per-K tests of the K-NN search (tests/test_host_logic.py on the CPU door,
tests/test_gpu_knn_sizes.py on the kernels).  Every cloud is built once per session and handed out read-only; the oracle's answer for a
(cloud, K) pair is computed once and shared the same way."""
import functools

import numpy as np

from conftest import brats_cloud, uniform_cloud

SELF_KINDS = ("uniform", "lattice", "duplicates")


def _frozen(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def cloud(kind):
    """uniform: 2 000 tie-free points.  lattice: 4 000 voxels of a 32 x 32 x 24 grid, equal distances everywhere (the ellipsoid of
    brats_cloud holds ~0.38 of the grid: 9 300 voxels, enough for 4 000).  duplicates: 300 points, each 8 times, shuffled.
    line: the geometric progression 0.97^i on the x axis, 1 100 points, shuffled -- a 50-deep tree (tests/test_gpu_knn.py::
    test_unbalanced_cloud_is_finished_by_the_straggler_kernel, small variant)."""
    rng = np.random.default_rng(23)
    if kind == "uniform":
        return _frozen(uniform_cloud(2000, 21))
    if kind == "lattice":
        return _frozen(brats_cloud(4000, 22, grid=(32, 32, 24)))
    if kind == "duplicates":
        d = np.repeat(rng.random((300, 3), dtype=np.float32), 8, axis=0)
        rng.shuffle(d)
        return _frozen(d)
    if kind == "line":
        n = 1100
        p = np.stack([0.97 ** np.arange(n), np.zeros(n), np.zeros(n)], 1).astype(np.float32)
        return _frozen(p[rng.permutation(n)])
    raise KeyError(kind)


@functools.lru_cache(maxsize=None)
def foreign():
    """Queries that are not the support: B = 2, 2 000 support points, 1 500 queries over 1.4 times the support's box."""
    rng = np.random.default_rng(24)
    s = rng.random((2, 2000, 3), dtype=np.float32)
    q = rng.random((2, 1500, 3), dtype=np.float32) * np.float32(1.4) - np.float32(0.2)
    return _frozen(s), _frozen(q)


_oracle_cache = {}


def oracle_self(oracle, kind, K):
    """oracle.knn_batch of cloud(kind) against itself, int64 [1, n, K]."""
    key = (kind, K)
    if key not in _oracle_cache:
        p = cloud(kind)
        _oracle_cache[key] = _frozen(oracle.knn_batch(p[None], p[None], K))
    return _oracle_cache[key]


def tiny(n, seed=0):
    return np.random.default_rng(1000 * seed + n).random((n, 3), dtype=np.float32)
