"""The K-NN search and the index pyramid at EVERY compiled list size K (PS_KNN_KS of csrc/kdtree.h: knn_kernel<K> behind ps_knn_batch /
ps_knn_batch_i64, knn_pair_kernel<K> behind ps_pyramid_build), index for index against the oracle.  Much of the per-query code is
written per K -- the seeded start of the self queries (2K-1 window for K <= 32, single window below 2K-1 queries and for K = 48, 64,
no seed below K queries), the result store (int4 rows for K % 4 == 0, a scalar loop otherwise, to `out` and to the pooling table),
the wave-uniform insertion TopkInsertFrom<K, J>, the zero padding of lists that never fill -- so each size runs each of them here.
tests/test_knn_size_coverage.py holds COMPILED_KS to the header: a size compiled later does not ship untested."""
import ctypes

import numpy as np
import pytest

import knn_cases

pytestmark = pytest.mark.gpu

# every K the kernels are compiled for: PS_KNN_KS of csrc/kdtree.h
COMPILED_KS = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 20, 24, 32, 48, 64]
STORE_PATH_KS = [7, 12]     # one K of the scalar store, one of the int4 store
DEEP_STACK_KS = [13, 48, 64]
REFUSED_KS = [0, 17, 33, 65]
SENTINEL = -7


def _knn_gpu(s, q, K):
    from point_unet_amd.utils.nearest_neighbors.lib.python import nearest_neighbors as nn
    return nn.knn_batch(s, q, K, omp=True)


def _cfg(K):
    from point_unet_amd.helper_tool import ConfigBraTS

    class Cfg(ConfigBraTS):
        num_layers = 2
        sub_sampling_ratio = [2, 2]
        k_n = K

    return Cfg


def _build(xyz, K):
    """-> ([xyz], [neigh_idx], [sub_idx], [interp_idx], [order]) of the two levels as numpy arrays."""
    import torch
    from point_unet_amd.pyramid import build_pyramid
    pyr = build_pyramid(torch.tensor(xyz, device="cuda"), _cfg(K))
    torch.cuda.synchronize()
    return tuple([t.cpu().numpy() for t in tables] for tables in (pyr.xyz, pyr.neigh_idx, pyr.sub_idx, pyr.interp_idx, pyr.order))


def _check_pyramid(oracle, xyz, K, what):
    from oracle import randla_oracle as ro
    got_xyz, got_nbr, got_pool, got_up, got_order = _build(xyz, K)
    pts, nbr, pool, up = ro.build_pyramid(lambda s, q, k: oracle.knn_batch(s, q, k), xyz, K, [2, 2])
    for i in range(2):
        assert got_nbr[i].shape == nbr[i].shape and got_pool[i].shape == pool[i].shape and got_up[i].shape == up[i].shape, (what, i)
        assert np.array_equal(got_xyz[i], pts[i]), ("xyz", what, i)
        assert np.array_equal(got_nbr[i], nbr[i]), ("neigh_idx", what, i)
        assert np.array_equal(got_pool[i], pool[i]), ("sub_idx", what, i)
        assert np.array_equal(got_up[i], up[i]), ("interp_idx", what, i)
        for b in range(xyz.shape[0]):
            assert np.array_equal(np.sort(got_order[i][b]), np.arange(pts[i].shape[1])), ("order", what, i, b)


def _threshold_cloud(rng, n0, variant, B=1):
    """The three clouds of test_gpu_knn.py::test_seeded_searches_at_their_size_thresholds."""
    if variant == 0:    # coarse lattice: many exactly equal distances
        return rng.integers(0, 5, (B, n0, 3)).astype(np.float32) / 4
    if variant == 1:    # a third of the points duplicated
        xyz = rng.random((B, n0, 3)).astype(np.float32)
        for b in range(B):
            dup = rng.integers(0, n0, n0 // 3)
            xyz[b, rng.permutation(n0)[:n0 // 3]] = xyz[b, dup]
        return xyz
    xyz = np.zeros((B, n0, 3), np.float32)  # a thin line: leaf order is spatial order, the window bound is as tight as it gets
    for b in range(B):
        xyz[b, :, 0] = rng.permutation(n0).astype(np.float32) / n0
    return xyz


def pyramid_sizes(K):
    """Cloud sizes n0 for ratios [2, 2].  The self queries of a level of nq points start seeded from the 2K-1 window (K <= 32,
    nq >= 2K-1), from the single K window (K <= nq, and nq < 2K-1 or K > 32), or unseeded (nq < K): n0 = K, K+1, 2K-2, 2K-1, 2K put
    level 0 on each side of both thresholds, n0 = 2K .. 4K+1 do the same for level 1 (n0 // 2 = K, K+1, 2K-2, 2K-1, 2K) while
    level 0 is past them, n0 = 2K-2 leaves level 1 below K; 8K+3 and 2 500 are odd sizes of several workgroups.  The last level must
    keep one point (n0 >= 4)."""
    sizes = {K, K + 1, 2 * K - 2, 2 * K - 1, 2 * K, 2 * K + 1, 2 * K + 2, 2 * K + 3, 4 * K - 4, 4 * K - 3, 4 * K - 2, 4 * K - 1, 4 * K,
             4 * K + 1, 8 * K + 3, 2500}
    return sorted(n for n in sizes if n >= 4)


def seed_form(K, nq):
    """How knn_body<K> starts the self queries of a level of nq points (csrc/knn.hip)."""
    if K == 1 or nq < K:
        return "unseeded"
    return "window_2k-1" if K <= 32 and nq >= 2 * K - 1 else "single_window"


# ---- knn_kernel<K> through nearest_neighbors.knn_batch ---------------------------------------------------------------------------
@pytest.mark.parametrize("K", COMPILED_KS)
def test_plain_kernel_self_queries(oracle, K):
    for kind in knn_cases.SELF_KINDS:
        p = knn_cases.cloud(kind)
        got = _knn_gpu(p[None], p[None], K)
        assert got.dtype == np.int64 and np.array_equal(got, knn_cases.oracle_self(oracle, kind, K)), kind


@pytest.mark.parametrize("K", COMPILED_KS)
def test_plain_kernel_queries_outside_the_support(oracle, K):
    s, q = knn_cases.foreign()
    assert np.array_equal(_knn_gpu(s, q, K), oracle.knn_batch(s, q, K))


@pytest.mark.parametrize("K", COMPILED_KS)
def test_plain_kernel_tiny_clouds(oracle, K):
    for n in sorted({1, K - 1, K, K + 1, 2 * K - 2, 2 * K - 1, 2 * K} - {0}):
        p = knn_cases.tiny(n, 1)
        got = _knn_gpu(p[None], p[None], K)
        assert np.array_equal(got, oracle.knn_batch(p[None], p[None], K)), n
        assert not got[:, :, n:].any(), n  # the slots a list of n < K points never fills read 0


@pytest.mark.parametrize("K", STORE_PATH_KS)
def test_device_pointer_forms_agree(oracle, lib, K):
    import torch
    from point_unet_amd import _lib, runtime
    s, q = knn_cases.foreign()
    want = oracle.knn_batch(s, q, K)
    ds, dq = torch.tensor(s, device="cuda"), torch.tensor(q, device="cuda")
    o32 = torch.full(want.shape, SENTINEL, dtype=torch.int32, device="cuda")
    o64 = torch.full(want.shape, SENTINEL, dtype=torch.int64, device="cuda")
    ctx = runtime.default_context(0)
    torch.cuda.synchronize()
    B, n1, n2 = s.shape[0], s.shape[1], q.shape[1]
    _lib.check(lib.ps_knn_batch(ctx.handle, runtime.ptr(ds), runtime.ptr(dq), B, n1, n2, 3, K, runtime.ptr(o32), 1))
    _lib.check(lib.ps_knn_batch_i64(ctx.handle, runtime.ptr(ds), runtime.ptr(dq), B, n1, n2, 3, K, runtime.ptr(o64), 1))
    torch.cuda.synchronize()
    h32 = np.full(want.shape, SENTINEL, np.int32)
    _lib.check(lib.ps_knn_batch(ctx.handle, runtime.ptr(s), runtime.ptr(q), B, n1, n2, 3, K, runtime.ptr(h32), 0))
    assert np.array_equal(o32.cpu().numpy(), want.astype(np.int32))
    assert np.array_equal(o64.cpu().numpy(), want)
    assert np.array_equal(o32.cpu().numpy().astype(np.int64), o64.cpu().numpy())
    assert np.array_equal(h32, o32.cpu().numpy())


# ---- knn_pair_kernel<K> through pyramid.build_pyramid -----------------------------------------------------------------------------
@pytest.mark.parametrize("K", COMPILED_KS)
def test_pyramid_at_the_seed_thresholds(oracle, K):
    rng = np.random.default_rng(100 + K)
    for n0 in pyramid_sizes(K):
        for variant in range(3):
            _check_pyramid(oracle, _threshold_cloud(rng, n0, variant), K, (n0, variant))


@pytest.mark.parametrize("K", COMPILED_KS)
def test_pyramid_of_two_clouds(oracle, K):
    rng = np.random.default_rng(200 + K)
    for n0, variant in ((8 * K + 3, 0), (1201, 1)):
        _check_pyramid(oracle, _threshold_cloud(rng, n0, variant, B=2), K, (n0, variant))


# ---- deep stacks with long lists ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", DEEP_STACK_KS)
def test_deep_tree_with_long_lists(oracle, K):
    """The geometric line: a 50-deep tree, so a query defers far more children than the 8-entry LDS window of the kernels' stack holds
    and the spill path runs -- with 2K list registers beside it at K = 48 and 64."""
    p = knn_cases.cloud("line")
    assert np.array_equal(_knn_gpu(p[None], p[None], K), knn_cases.oracle_self(oracle, "line", K))
    _check_pyramid(oracle, p[None], K, "line")


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def _listed_sizes(msg):
    return [int(t) for t in msg.split("compiled sizes:")[1].rstrip(")").split()]


@pytest.mark.parametrize("K", REFUSED_KS)
def test_knn_batch_refuses_an_uncompiled_k(lib, K):
    import torch
    from point_unet_amd import runtime
    p = knn_cases.tiny(100, 2)
    ctx = runtime.default_context(0)
    out = np.full((1, 100, max(K, 1)), SENTINEL, np.int32)
    assert lib.ps_knn_batch(ctx.handle, runtime.ptr(p), runtime.ptr(p), 1, 100, 100, 3, K, runtime.ptr(out), 0) == 1  # PS_EINVAL
    msg = lib.ps_last_error().decode()
    assert "K=%d" % K in msg and _listed_sizes(msg) == COMPILED_KS, msg
    assert (out == SENTINEL).all()
    dp = torch.from_numpy(p).cuda()
    dout = torch.full((1, 100, max(K, 1)), SENTINEL, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    assert lib.ps_knn_batch_i64(ctx.handle, runtime.ptr(dp), runtime.ptr(dp), 1, 100, 100, 3, K, runtime.ptr(dout), 1) == 1
    assert _listed_sizes(lib.ps_last_error().decode()) == COMPILED_KS
    torch.cuda.synchronize()
    assert (dout.cpu().numpy() == SENTINEL).all()


@pytest.mark.parametrize("K", REFUSED_KS)
def test_pyramid_build_refuses_an_uncompiled_k_before_any_work(lib, K):
    """The refusal leaves the pyramid as the caller handed it over: not stamped as built, and no table -- xyz included, which the tree
    builders write -- touched."""
    import torch
    from point_unet_amd import runtime
    from point_unet_amd.pyramid import alloc_pyramid
    xyz = torch.from_numpy(knn_cases.tiny(300, 3)[None]).cuda()
    pyr = alloc_pyramid(1, 300, [2, 2], 66, xyz.device)   # (buffers wide enough for any of the refused K)
    tables = pyr.xyz + pyr.neigh_idx + pyr.sub_idx + pyr.interp_idx + pyr.order
    for t in tables:
        t.fill_(SENTINEL)
    pyr.struct.built = 12345
    ctx = runtime.default_context(0)
    torch.cuda.synchronize()
    rc = lib.ps_pyramid_build(ctx.handle, runtime.ptr(xyz), 1, 300, 2, (ctypes.c_int32 * 2)(2, 2), K, ctypes.byref(pyr.struct))
    assert rc == 1  # PS_EINVAL
    msg = lib.ps_last_error().decode()
    assert "K=%d" % K in msg and _listed_sizes(msg) == COMPILED_KS, msg
    assert pyr.struct.built == 0
    torch.cuda.synchronize()
    for t in tables:
        assert (t.cpu().numpy() == SENTINEL).all()
    # the context is as usable as before
    from point_unet_amd.pyramid import build_pyramid
    ok = build_pyramid(xyz, _cfg(4))
    torch.cuda.synchronize()
    assert ok.struct.built != 0 and int(ok.neigh_idx[0].min()) >= 0 and int(ok.neigh_idx[0].max()) < 300


# ---- determinism ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", STORE_PATH_KS)
def test_two_runs_are_equal_byte_for_byte(K):
    p = knn_cases.cloud("lattice")
    assert _knn_gpu(p[None], p[None], K).tobytes() == _knn_gpu(p[None], p[None], K).tobytes()
    first, second = _build(p[None], K), _build(p[None], K)
    for a, b in zip(first, second):
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes()
