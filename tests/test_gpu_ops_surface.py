"""The op-by-op inference surface of csrc/ops.hip on every kernel path and edge: ps_op_gather_neighbour[_ex], ps_op_relative_pos_encoding,
ps_op_random_sample[_ties], ps_op_nearest_interpolation, ps_op_conv1x1[_ex], ps_op_att_pool, ps_op_half_to_float, ps_op_probs_to_volume.

The C entries are called through ctypes so that pointers, strides and alignment are the test's to choose; the package wrappers are called
next to them where one exists.  Every reference is NumPy (float64 where arithmetic is involved), every output buffer starts as a NaN
sentinel that is wider (row stride > payload) and longer (two rows past the end) than what the op may write, and every element is
compared.  Each case names, in a comment, the kernel the dispatch condition of ops.hip / rowgemm.hip / randla.hip selects for it.

An unaligned base is a view one element into a larger torch buffer (torch's allocator hands out 512-byte aligned blocks)."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24          # unit roundoff of float32
PS_EINVAL = 1             # include/pointseg.h
NAN_BITS = 0x7FC00000     # what torch.full(..., nan) stores
f32, i32, f64 = np.float32, np.int32, np.float64


@pytest.fixture(scope="module")
def env(lib):
    from point_unet_amd import runtime
    return lib, runtime.default_context(0).handle


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _to_dev(a, off=0):
    """Flat device copy of `a` starting `off` elements into a fresh buffer (off = 1: a base that is not 16-byte aligned)."""
    a = np.ascontiguousarray(a)
    buf = torch.zeros(a.size + off + 4, dtype=torch.from_numpy(a[:0].reshape(-1)).dtype, device="cuda")
    v = buf[off:off + a.size]
    v.copy_(torch.from_numpy(a.reshape(-1)))
    assert v.data_ptr() % 16 == (off * a.itemsize) % 16
    return v


def _sentinel(rows, ld, off=0):
    """[rows + 2, ld] of NaN, `off` floats into its buffer"""
    n = (rows + 2) * ld
    buf = torch.full((n + off + 4,), float("nan"), device="cuda")
    return buf[off:off + n].view(rows + 2, ld)


def _intact(t):
    return bool((t.cpu().numpy().view(np.uint32) == NAN_BITS).all())


def _payload(out, rows, width):
    """The [rows, width] the op owns; the padding columns and the rows past the end must still hold the sentinel."""
    assert _intact(out[:rows, width:]), "padding columns were written"
    assert _intact(out[rows:]), "rows past the end were written"
    return out[:rows, :width].cpu().numpy()


def _ratio(err, bound):
    assert (err[bound == 0] == 0).all()
    return float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0


# =====================================================================================================================================
# 1. gathers: ps_op_gather_neighbour, _ex, ps_op_nearest_interpolation  (launch_gather_rows: the float4 kernel needs d % 4 == 0,
#    ldo % 4 == 0 and both bases 16-byte aligned; everything else is gather_rows_kernel)
# =====================================================================================================================================
GATHER_CASES = [  # d, ldo - d, pc offset, out offset
    (1, 0, 0, 0),      # gather_rows_kernel (d % 4 != 0)
    (3, 0, 0, 0),      # gather_rows_kernel
    (7, 0, 0, 0),      # gather_rows_kernel
    (130, 0, 0, 0),    # gather_rows_kernel
    (4, 0, 0, 0),      # gather_rows4_kernel
    (24, 0, 0, 0),     # gather_rows4_kernel
    (132, 0, 0, 0),    # gather_rows4_kernel
    (8, 0, 1, 0),      # gather_rows_kernel (pc not 16-byte aligned)
    (8, 0, 0, 1),      # gather_rows_kernel (out not 16-byte aligned)
    (8, 1, 0, 0),      # gather_rows_kernel (_ex, ldo = d + 1)
    (8, 4, 0, 0),      # gather_rows4_kernel (_ex, ldo = d + 4)
    (3, 2, 0, 0),      # gather_rows_kernel (_ex, d and ldo both odd sizes)
]


def _gather_ref(pc, idx):
    B, M, K = idx.shape
    return np.take_along_axis(pc, idx.reshape(B, M * K, 1).astype(np.int64), axis=1).reshape(B * M * K, pc.shape[2])


def _indices(rng, B, N, M, K):
    idx = rng.integers(0, N, (B, M, K)).astype(i32)
    idx[:, 0, 0] = 0
    idx[:, -1, -1] = N - 1
    return idx


@pytest.mark.parametrize("d,pad,pc_off,out_off", GATHER_CASES)
def test_gather_neighbour_and_nearest_interpolation(env, d, pad, pc_off, out_off):
    lib, h = env
    B, N, M = 3, 37, 11
    ldo = d + pad
    for K in (1, 5, 16):
        rng = np.random.default_rng(1000 * d + K)
        pc = rng.standard_normal((B, N, d)).astype(f32)
        idx = _indices(rng, B, N, M, K)
        rows = B * M * K
        assert (rows * d) % 256 and (d % 4 or (rows * d // 4) % 256)  # the last block is partial
        want = _gather_ref(pc, idx)
        dpc, didx = _to_dev(pc, pc_off), _to_dev(idx)
        out = _sentinel(rows, ldo, out_off)
        assert lib.ps_op_gather_neighbour_ex(h, _p(dpc), _p(didx), B, N, M, K, d, _p(out), ldo) == 0
        assert _payload(out, rows, d).tobytes() == want.tobytes(), (d, K, "ex")
        if not pad:
            out = _sentinel(rows, d, out_off)
            assert lib.ps_op_gather_neighbour(h, _p(dpc), _p(didx), B, N, M, K, d, _p(out)) == 0
            assert _payload(out, rows, d).tobytes() == want.tobytes(), (d, K)
    if not pad:  # nearest_interpolation: the same two kernels with one index per row, M (up-sampled) > N
        rng = np.random.default_rng(d)
        M2 = 53
        feat = rng.standard_normal((B, N, d)).astype(f32)
        idx = _indices(rng, B, N, M2, 1)
        assert (B * M2 * d) % 256
        out = _sentinel(B * M2, d, out_off)
        assert lib.ps_op_nearest_interpolation(h, _p(_to_dev(feat, pc_off)), _p(_to_dev(idx)), B, N, M2, d, _p(out)) == 0
        assert _payload(out, B * M2, d).tobytes() == _gather_ref(feat, idx).tobytes()


def test_gather_wrappers_and_empty_calls(env):
    lib, h = env
    from point_unet_amd.RandLANet import Network
    rng = np.random.default_rng(5)
    B, N, M, K = 3, 37, 11, 5
    for d in (3, 24):  # gather_rows_kernel, gather_rows4_kernel
        pc = rng.standard_normal((B, N, d)).astype(f32)
        idx = _indices(rng, B, N, M, K)
        got = Network.gather_neighbour(torch.from_numpy(pc).cuda(), torch.from_numpy(idx).cuda()).cpu().numpy()
        assert got.shape == (B, M, K, d) and got.tobytes() == _gather_ref(pc, idx).tobytes()
        up = _indices(rng, B, N, 53, 1)
        got = Network.nearest_interpolation(torch.from_numpy(pc[:, :, None]).cuda(), torch.from_numpy(up).cuda()).cpu().numpy()
        assert got.shape == (B, 53, 1, d) and got.tobytes() == _gather_ref(pc, up).tobytes()
    # B = 0 and M = 0: OK, nothing written
    dpc, didx = _to_dev(np.zeros((4, 8), f32)), _to_dev(np.zeros(16, i32))
    for Bz, Mz in ((0, 2), (1, 0)):
        out = _sentinel(4, 8)
        assert lib.ps_op_gather_neighbour(h, _p(dpc), _p(didx), Bz, 4, Mz, 2, 8, _p(out)) == 0
        assert lib.ps_op_gather_neighbour_ex(h, _p(dpc), _p(didx), Bz, 4, Mz, 2, 8, _p(out), 8) == 0
        assert lib.ps_op_nearest_interpolation(h, _p(dpc), _p(didx), Bz, 4, Mz, 8, _p(out)) == 0
        assert _intact(out)


# =====================================================================================================================================
# 2. ps_op_relative_pos_encoding (relpos_kernel)
# =====================================================================================================================================
@pytest.mark.parametrize("K", [1, 5, 16, 32])
def test_relative_pos_encoding(env, K):
    """Coordinates of about +-300: columns 1..9 (differences and copies) bit for bit; the distance against the float64 root of the float64
    sum of squares of the float32 differences within 3 * 2^-24 * dis: the two roundings of the sum (with or without contraction) are
    halved by the root, plus the rounding of the root itself.  Rows that are their own neighbour have distance exactly 0."""
    lib, h = env
    from point_unet_amd.RandLANet import Network
    B, N = 3, 257
    rng = np.random.default_rng(K)
    xyz = ((rng.random((B, N, 3)) - 0.5) * 600.0).astype(f32)
    idx = _indices(rng, B, N, N, K)
    idx[:, 1::2, 0] = np.arange(N, dtype=i32)[1::2]  # every other point is its own first neighbour
    nbr = np.stack([xyz[b][idx[b]] for b in range(B)], 0)
    centre = np.broadcast_to(xyz[:, :, None, :], nbr.shape)
    rel = centre - nbr  # float32
    dis = np.sqrt((rel.astype(f64) ** 2).sum(-1))
    total = B * N * K
    out = _sentinel(total, 10)
    assert lib.ps_op_relative_pos_encoding(h, _p(_to_dev(xyz)), _p(_to_dev(idx)), B, N, K, _p(out)) == 0
    got = _payload(out, total, 10).reshape(B, N, K, 10)
    assert got[..., 1:].tobytes() == np.concatenate([rel, centre, nbr], -1).astype(f32).tobytes()
    err, bound = np.abs(got[..., 0].astype(f64) - dis), 3 * EPS * dis
    assert (dis == 0).sum() >= B * (N // 2) and dis.max() > 300
    print("relative_pos_encoding K=%d: distance err/bound %.3f" % (K, _ratio(err, bound)))
    assert (err <= bound).all()
    wrapped = Network.relative_pos_encoding(torch.from_numpy(xyz).cuda(), torch.from_numpy(idx).cuda()).cpu().numpy()
    assert wrapped.tobytes() == got.tobytes()


# =====================================================================================================================================
# 3. ps_op_random_sample[_ties]  (ops.hip: d % 4 == 0 and aligned feature / out -> pool_max() of randla.hip, which picks
#    pool_max_kernel<16> / <32> for K = 16 / 32 on a 16-byte aligned index table and <0> otherwise; else pool_max_scalar_kernel)
# =====================================================================================================================================
POOL_PATHS = [  # K, d, index offset, feature offset, out offset
    (16, 8, 0, 0, 0),    # pool_max_kernel<16>
    (32, 8, 0, 0, 0),    # pool_max_kernel<32>
    (1, 8, 0, 0, 0),     # pool_max_kernel<0>
    (5, 8, 0, 0, 0),     # pool_max_kernel<0>
    (40, 8, 0, 0, 0),    # pool_max_kernel<0>
    (16, 8, 1, 0, 0),    # pool_max_kernel<0> (index table not 16-byte aligned)
    (16, 1, 0, 0, 0),    # pool_max_scalar_kernel (d % 4 != 0)
    (16, 6, 0, 0, 0),    # pool_max_scalar_kernel
    (16, 8, 0, 1, 0),    # pool_max_scalar_kernel (feature not 16-byte aligned)
    (5, 8, 0, 0, 1),     # pool_max_scalar_kernel (out not 16-byte aligned)
]
POOL_SHAPES = [(1, 1), (3, 1), (1, 7), (3, 3), (3, 13)]  # B, M: B*M = 1, 3, 7, 9 leave XCD slices empty; 3 x 13 is no multiple of 8


def _pool_ref(feat, idx):
    g = np.stack([feat[b][idx[b]] for b in range(feat.shape[0])], 0)  # [B, M, K, d]
    m = np.max(g, axis=2)
    return m, (g == m[:, :, None, :]).sum(2)


def _negative_features(rng, shape):
    """all below zero (a maximum seeded with 0 shows), a few -inf"""
    f = (-0.5 - rng.random(shape)).astype(f32)
    f[rng.random(shape) < 0.03] = -np.inf
    return f


@pytest.mark.parametrize("K,d,idx_off,feat_off,out_off", POOL_PATHS)
def test_random_sample_paths(env, K, d, idx_off, feat_off, out_off):
    lib, h = env
    N = 29
    for B, M in POOL_SHAPES:
        rng = np.random.default_rng(K * 1000 + d * 10 + B * M)
        feat = _negative_features(rng, (B, N, d))
        idx = _indices(rng, B, N, M, K) if M > 1 else rng.integers(0, N, (B, M, K)).astype(i32)
        want, _ = _pool_ref(feat, idx)
        out = _sentinel(B * M, d, out_off)
        assert lib.ps_op_random_sample(h, _p(_to_dev(feat, feat_off)), _p(_to_dev(idx, idx_off)), B, N, M, K, d, _p(out)) == 0
        got = _payload(out, B * M, d)
        assert got.max() < 0 and got.tobytes() == want.reshape(B * M, d).tobytes(), (B, M)


@pytest.mark.parametrize("K,d,idx_off,feat_off", [(16, 8, 0, 0), (32, 8, 0, 0), (5, 8, 0, 0), (16, 8, 1, 0), (16, 6, 0, 0), (16, 8, 0, 1)])
def test_random_sample_infinities_and_signed_zeros(env, K, d, idx_off, feat_off):
    """-inf, +inf, -0.0 and +0.0 among the gathered rows: equal to np.max as values (fmaxf may return either zero)."""
    lib, h = env
    B, N, M = 3, 29, 13
    rng = np.random.default_rng(K + d + idx_off + feat_off)
    feat = rng.choice(np.array([-np.inf, -2.0, -0.0, 0.0, np.inf], f32), size=(B, N, d), p=[0.45, 0.35, 0.1, 0.08, 0.02]).astype(f32)
    idx = _indices(rng, B, N, M, K)
    want, _ = _pool_ref(feat, idx)
    assert len(np.unique(want)) >= 2 and (want == 0).any() and np.isinf(want).any()
    out = _sentinel(B * M, d)
    assert lib.ps_op_random_sample(h, _p(_to_dev(feat, feat_off)), _p(_to_dev(idx, idx_off)), B, N, M, K, d, _p(out)) == 0
    assert np.array_equal(_payload(out, B * M, d), want.reshape(B * M, d))


def test_random_sample_grid_stride_and_wrapper(env):
    """B*M*d/4 > 2^20 float4s: the 4096 workgroups of pool_max_kernel<16> walk their XCD slice twice."""
    lib, h = env
    from point_unet_amd.RandLANet import Network
    B, N, M, K, d = 1, 300, 20000, 16, 256
    assert B * M * d // 4 > 2 ** 20
    rng = np.random.default_rng(11)
    feat = _negative_features(rng, (B, N, d))
    idx = _indices(rng, B, N, M, K)
    want = feat[0][idx[0, :, 0]]
    for k in range(1, K):
        want = np.maximum(want, feat[0][idx[0, :, k]])
    out = _sentinel(B * M, d)
    assert lib.ps_op_random_sample(h, _p(_to_dev(feat)), _p(_to_dev(idx)), B, N, M, K, d, _p(out)) == 0
    assert _payload(out, B * M, d).tobytes() == want.tobytes()
    # the package wrapper, on a small case (pool_max_kernel<16>)
    f, ix = feat[:, :, :8].copy(), idx[:, :13].copy()
    got = Network.random_sample(torch.from_numpy(f[:, :, None]).cuda(), torch.from_numpy(ix).cuda()).cpu().numpy()
    assert got.shape == (1, 13, 1, 8) and got[:, :, 0].tobytes() == _pool_ref(f, ix)[0].tobytes()


@pytest.mark.parametrize("K,idx_off", [(16, 0), (32, 0), (40, 0), (16, 1)])  # pool_max_kernel<16>, <32>, <0>, <0>
def test_random_sample_ties(env, K, idx_off):
    """Features from four values: between 2 and K gathered rows attain the maximum; the counts are exact."""
    lib, h = env
    B, N, M, d = 3, 29, 13, 8
    rng = np.random.default_rng(K)
    feat = rng.choice(np.array([-4.0, -2.0, -1.0, -0.5], f32), size=(B, N, d)).astype(f32)
    idx = _indices(rng, B, N, M, K)
    want, ties = _pool_ref(feat, idx)
    assert ties.min() >= 1 and ties.max() >= 6 and (ties >= 2).mean() > 0.5
    out = _sentinel(B * M, d)
    dt = torch.full((B * M + 2, d), 0xEE, dtype=torch.uint8, device="cuda")
    assert lib.ps_op_random_sample_ties(h, _p(_to_dev(feat)), _p(_to_dev(idx, idx_off)), B, N, M, K, d, _p(out), _p(dt)) == 0
    assert _payload(out, B * M, d).tobytes() == want.reshape(B * M, d).tobytes()
    got = dt.cpu().numpy()
    assert np.array_equal(got[:B * M], ties.reshape(B * M, d)) and (got[B * M:] == 0xEE).all()


# =====================================================================================================================================
# 4. ps_op_att_pool (att_pool_op_kernel<16> for K <= 16, <32> above; K * d * 4 bytes of dynamic LDS)
# =====================================================================================================================================
def _att_ref(f, w):
    """float64 value and the elementwise bar: with e = 2^-24, delta = (d + 1) e max_k sum_j |f[k,j]| |w[j,col]| bounds the error of a
    score, so a softmax weight is off by at most 2 delta + 3 e relative (exponent argument, subtraction, expf) -- twice that for the
    quotient of two such sums -- and the two K-term sums and the division add 2 (K + 2) e."""
    f, w = f.astype(f64), w.astype(f64)
    K, d = f.shape[1:]
    s = f @ w
    a = np.exp(s - s.max(1, keepdims=True))
    want = (f * a).sum(1) / a.sum(1)
    delta = (d + 1) * EPS * (np.abs(f) @ np.abs(w)).max(1)
    bound = np.abs(f).max(1) * (2 * (2 * delta + 3 * EPS) + 2 * (K + 2) * EPS)
    return want, bound, s


def _att_check(env, fset, wfc, tag):
    lib, h = env
    R, K, d = fset.shape
    want, bound, _ = _att_ref(fset, wfc)
    out = _sentinel(R, d)
    assert lib.ps_op_att_pool(h, _p(_to_dev(fset)), _p(_to_dev(wfc)), R, K, d, _p(out)) == 0, lib.ps_last_error()
    err = np.abs(_payload(out, R, d).astype(f64) - want)
    print("att_pool %s R=%d K=%d d=%d: err/bound %.4f" % (tag, R, K, d, _ratio(err, bound)))
    assert (err <= bound).all(), (tag, float((err / bound).max()))


ATT_CASES = [  # K, d, the row counts
    (1, 7, (3,)),           # att_pool_op_kernel<16>, one neighbour (softmax = 1), 15 predicated lanes
    (3, 5, (3,)),           # att_pool_op_kernel<16>, K < KMAX
    (16, 32, (40,)),        # att_pool_op_kernel<16>, K = KMAX
    (17, 257, (40,)),       # att_pool_op_kernel<32>, K < KMAX, a second column for thread 0 only
    (32, 64, (40,)),        # att_pool_op_kernel<32>, K = KMAX
    (32, 512, (1, 40)),     # att_pool_op_kernel<32>, 64 KB of LDS: the hipFuncSetAttribute branch (the network's own largest)
    (24, 1024, (1, 40)),    # att_pool_op_kernel<32>, 96 KB, four columns per thread
    (32, 1280, (1, 40)),    # att_pool_op_kernel<32>, exactly the 160 KB limit
]


@pytest.mark.parametrize("K,d,Rs", ATT_CASES)
def test_att_pool_against_float64(env, K, d, Rs):
    for R in Rs:
        rng = np.random.default_rng(K * 10000 + d + R)
        fset = rng.standard_normal((R, K, d)).astype(f32)
        wfc = (rng.standard_normal((d, d)) / np.sqrt(d)).astype(f32)
        _att_check(env, fset, wfc, "plain")


@pytest.mark.parametrize("K,d", [(16, 32), (5, 12)])  # att_pool_op_kernel<16>
def test_att_pool_more_rows_than_workgroups(env, K, d):
    """R = 2050 > 2048 workgroups: two workgroups take a second row, through the leading __syncthreads of the row loop."""
    rng = np.random.default_rng(K)
    fset = rng.standard_normal((2050, K, d)).astype(f32)
    wfc = (rng.standard_normal((d, d)) * 0.3).astype(f32)
    _att_check(env, fset, wfc, "grid-stride")


def test_att_pool_scores_that_need_the_max_subtraction(env):
    """att_pool_op_kernel<16> at (16, 32) with fset scaled until the largest score is 92: expf of it overflows float32."""
    rng = np.random.default_rng(3)
    fset = rng.standard_normal((40, 16, 32)).astype(f32)
    wfc = (rng.standard_normal((32, 32)) * 0.3).astype(f32)
    fset = (fset * (92.0 / (fset.astype(f64) @ wfc.astype(f64)).max())).astype(f32)
    s = _att_ref(fset, wfc)[2]
    assert 89.0 < s.max() < 95.0 and s.min() < -40.0
    _att_check(env, fset, wfc, "large scores")


@pytest.mark.parametrize("K,d", [(0, 8), (33, 8), (32, 1281), (8, 0)])
def test_att_pool_refusals(env, K, d):
    lib, h = env
    fset, wfc = _to_dev(np.zeros(max(K * d, 1) * 2, f32)), _to_dev(np.zeros(max(d * d, 1), f32))
    out = _sentinel(2, max(d, 1))
    assert lib.ps_op_att_pool(h, _p(fset), _p(wfc), 2, K, d, _p(out)) == PS_EINVAL
    assert b"ps_op_att_pool" in lib.ps_last_error() and _intact(out)


# =====================================================================================================================================
# 5. ps_op_conv1x1[_ex] through rowgemm() (rowgemm.hip) and tinyconv_kernel (ops.hip)
#    ntb = 1 / 2 / 4 for cout < 32 / < 64 / >= 64, cblocks = ceil(cout / 16 ntb), tiles16 = ceil(R / 16).
#    direct: cin % 16 == 0, ldx % 4 == 0, x 16-byte aligned;  split-K: cin >= 256 and tiles16 * cblocks < 2048;
#    RT = 2: tiles16 * cblocks >= 8192;  streaming (not tested here): >= 32768 with cin <= 128.
# =====================================================================================================================================
def _bf16_rne(a):
    u = np.ascontiguousarray(a, f32).view(np.uint32)
    return ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)).view(f32)


def _products(x, W, bf16):
    xr, Wr = (_bf16_rne(x), _bf16_rne(W)) if bf16 else (x, W)
    return xr.astype(f64) @ Wr.astype(f64), np.abs(xr).astype(f64) @ np.abs(Wr).astype(f64)


def _conv_check(env, dx, ldx, dW, xw, axw, b, leaky, accum, ldy, seed, tag):
    """|got - want| <= (cin + 3) 2^-24 (|x| |w| + |b|), elementwise: the worst-case fp32 dot product in any order (cin products,
    cin additions with the bias, the LeakyReLU product); the accumulate epilogue adds one rounding of the sum."""
    lib, h = env
    R, cout = xw.shape
    cin = dW.numel() // cout
    bb = np.zeros(cout, f32) if b is None else b
    lin, mag = xw + bb.astype(f64), axw + np.abs(bb).astype(f64)
    want = np.where(lin >= 0, lin, lin * f64(f32(0.2))) if leaky else lin
    bound = (cin + 3) * EPS * mag
    y = _sentinel(R, ldy)
    if accum:
        old = np.random.default_rng(seed).standard_normal((R, cout)).astype(f32)
        y[:R, :cout] = torch.from_numpy(old).cuda()
        want = want + old.astype(f64)
        bound = bound + EPS * np.abs(want)
    db = None if b is None else _to_dev(b)
    assert lib.ps_op_conv1x1_ex(h, _p(dx), ldx, _p(dW), _p(db), R, cin, cout, leaky, accum, _p(y), ldy) == 0, lib.ps_last_error()
    err = np.abs(_payload(y, R, cout).astype(f64) - want)
    r = _ratio(err, bound)
    print("conv1x1 %s R=%d cin=%d cout=%d leaky=%d accum=%d bias=%d: err/bound %.4f" % (tag, R, cin, cout, leaky, accum, b is not None, r))
    assert (err <= bound).all(), (tag, r, np.argwhere(err > bound)[:8].tolist())


def _conv_case(env, R, cin, cout, ldx=None, x_off=0, bias=True, leaky=0, accum=0, bf16=False, tag=""):
    ldx = ldx or cin
    rng = np.random.default_rng(R * 7 + cin * 3 + cout + accum)
    x = rng.standard_normal((R, cin)).astype(f32)
    wide = np.full((R, ldx), 7.0e3, f32)  # the columns past cin belong to somebody else
    wide[:, :cin] = x
    W = (rng.standard_normal((cin, cout)) / np.sqrt(cin)).astype(f32)
    b = rng.standard_normal(cout).astype(f32) if bias else None
    xw, axw = _products(x, W, bf16)
    _conv_check(env, _to_dev(wide, x_off), ldx, _to_dev(W), xw, axw, b, leaky, accum, cout + 3, R, tag)


GENERIC = [  # R, cin, cout, ldx, x offset, bias, leaky, accum
    (1, 1, 1, None, 0, True, 0, 0),          # rowgemm_kernel<1>
    (65, 7, 8, 8, 0, False, 1, 0),           # rowgemm_kernel<1>, a second row block of one row
    (63, 3, 33, None, 0, True, 1, 1),        # rowgemm_kernel<2>, column 32 alone in the last tile
    (129, 70, 100, 71, 0, False, 0, 0),      # rowgemm_kernel<4>
    (100, 32, 40, 33, 0, True, 1, 0),        # rowgemm_kernel<2> (ldx % 4 != 0 keeps cin = 32 off the direct kernel)
    (100, 32, 40, None, 1, False, 0, 1),     # rowgemm_kernel<2> (x not 16-byte aligned)
    (129, 70, 100, None, 0, True, 1, 1),     # rowgemm_kernel<4>, accumulate
    (65, 7, 8, None, 0, True, 0, 1),         # rowgemm_kernel<1>, accumulate
]
DIRECT_RT1 = [
    (17, 16, 8, None, 0, True, 0, 0),        # rowgemm_direct_kernel<1,1,false>
    (100, 48, 40, 52, 0, False, 1, 0),       # rowgemm_direct_kernel<2,1,false>
    (1000, 80, 72, None, 0, True, 1, 1),     # rowgemm_direct_kernel<4,1,false>: the second column block holds 8 columns
]
SPLIT_K = [
    (5, 256, 16, None, 0, True, 1, 0),       # rowgemm_direct_kernel<1,1,true>
    (33, 272, 48, 276, 0, False, 0, 1),      # rowgemm_direct_kernel<2,1,true>: five chunks, the last holds 16 channels
    (351, 1536, 64, None, 0, True, 0, 0),    # rowgemm_direct_kernel<4,1,true>
    (16 * 2047, 256, 16, None, 0, False, 0, 0),      # rowgemm_direct_kernel<1,1,true>: tiles16 * cblocks = 2047
    (16 * 2047 + 1, 256, 16, None, 0, True, 1, 0),   # rowgemm_direct_kernel<1,1,false>: 2048
]
DIRECT_RT2 = [
    (131056, 16, 8, None, 0, True, 0, 0),    # rowgemm_direct_kernel<1,1,false>: tiles16 * cblocks = 8191
    (131057, 16, 8, 20, 0, False, 1, 0),     # rowgemm_direct_kernel<1,2,false>: 8192, R = 17 mod 32
    (65537, 32, 40, None, 0, True, 0, 1),    # rowgemm_direct_kernel<2,2,false>: R = 1 mod 32, the last wave's second row tile is past the end
    (40000, 64, 200, 72, 0, True, 1, 0),     # rowgemm_direct_kernel<4,2,false>
]


@pytest.mark.parametrize("R,cin,cout,ldx,x_off,bias,leaky,accum", GENERIC + DIRECT_RT1 + SPLIT_K + DIRECT_RT2)
def test_conv1x1_fp32_kernels(env, R, cin, cout, ldx, x_off, bias, leaky, accum):
    _conv_case(env, R, cin, cout, ldx, x_off, bias, leaky, accum, tag="fp32")


# the direct cases with cin % 16 == 0 again: rowgemm_direct_bf16_kernel<1|2|4, 1> and <1|2|4, 2> (the bf16 flavour has no split-K form:
# the cin >= 256 cases run RT = 1)
@pytest.mark.parametrize("R,cin,cout,ldx,x_off,bias,leaky,accum", DIRECT_RT1 + SPLIT_K[:3] + DIRECT_RT2)
def test_conv1x1_bf16_mode(env, R, cin, cout, ldx, x_off, bias, leaky, accum):
    lib, h = env
    try:
        assert lib.ps_set_train_gemm_bf16(h, 1) == 0
        _conv_case(env, R, cin, cout, ldx, x_off, bias, leaky, accum, bf16=True, tag="bf16")
    finally:
        assert lib.ps_set_train_gemm_bf16(h, 0) == 0


def test_conv1x1_wrapper(env):
    from point_unet_amd.RandLANet import Network
    rng = np.random.default_rng(2)
    x = rng.standard_normal((5, 20, 48)).astype(f32)
    W, b = (rng.standard_normal((48, 40)) / 7).astype(f32), rng.standard_normal(40).astype(f32)
    for leaky in (False, True):  # rowgemm_direct_kernel<2,1,false>
        got = Network.conv2d(torch.from_numpy(x).cuda(), torch.from_numpy(W).cuda(), torch.from_numpy(b).cuda(), leaky=leaky).cpu().numpy()
        xw, axw = _products(x.reshape(100, 48), W, False)
        lin = xw + b
        want = np.where(lin >= 0, lin, lin * f64(f32(0.2))) if leaky else lin
        assert got.shape == (5, 20, 40)
        assert (np.abs(got.reshape(100, 40) - want) <= 51 * EPS * (axw + np.abs(b))).all()


@pytest.fixture(scope="module")
def tiny():
    """The rows of the tinyconv_kernel<16,16> cases (R >= 2^20, 16 -> 16, ldx and ldy multiples of 4, aligned bases) with their float64
    products, computed once."""
    R = 2 ** 20 + 3
    rng = np.random.default_rng(16)
    x = rng.standard_normal((R, 16)).astype(f32)
    W = (rng.standard_normal((16, 16)) / 4).astype(f32)
    return {"dx": _to_dev(x), "dW": _to_dev(W), "b": rng.standard_normal(16).astype(f32), False: _products(x, W, False), True: _products(x, W, True)}


# tinyconv_kernel<16,16>.  ldy = cout + 4, not cout + 3: tinyconv_fits() wants ldy % 4 == 0, and an odd stride sends the shape to the
# streaming kernel, which has its own test.
@pytest.mark.parametrize("bias,leaky,accum,bf16", [(True, 0, 0, False), (True, 1, 1, False), (False, 0, 0, False), (False, 1, 1, False),
                                                   (True, 1, 1, True)])
def test_conv1x1_tinyconv_16_16(env, tiny, bias, leaky, accum, bf16):
    lib, h = env
    xw, axw = tiny[bf16]
    try:
        assert lib.ps_set_train_gemm_bf16(h, 1 if bf16 else 0) == 0
        _conv_check(env, tiny["dx"], 16, tiny["dW"], xw, axw, tiny["b"] if bias else None, leaky, accum, 20, 1, "tinyconv bf16=%d" % bf16)
    finally:
        assert lib.ps_set_train_gemm_bf16(h, 0) == 0


# =====================================================================================================================================
# 6. ps_op_half_to_float (half_to_float_kernel: min(ceil(n / 256), 4096) workgroups, grid-stride)
# =====================================================================================================================================
def _half_check(env, bits):
    lib, h = env
    n = len(bits)
    want = bits.view(np.float16).astype(f32)
    out = _sentinel(n, 1)
    src = _to_dev(bits.view(np.int16))
    assert lib.ps_op_half_to_float(h, _p(src), n, _p(out)) == 0
    got = _payload(out, n, 1).reshape(-1)
    nan = np.isnan(want)
    assert np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])
    assert np.isnan(got[nan]).all() and np.array_equal(np.signbit(got[nan]), np.signbit(want[nan]))
    return int(nan.sum())


def test_half_to_float_every_pattern_and_sizes(env):
    """All 65 536 binary16 patterns (subnormals, +-0, +-inf, the 2046 NaNs) in one call; n = 2^20 + 257 (each thread of the 4096
    workgroups takes a second element, 257 a third); n = 1; n = 0."""
    lib, h = env
    every = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    assert _half_check(env, every) == 2046
    rng = np.random.default_rng(0)
    _half_check(env, rng.integers(0, 65536, 2 ** 20 + 257).astype(np.uint16))
    for one in (0x0001, 0x8000, 0x7C00, 0xFE00, 0x3C00):  # smallest subnormal, -0, +inf, a negative NaN, 1.0
        _half_check(env, np.array([one], np.uint16))
    out = _sentinel(4, 1)
    assert lib.ps_op_half_to_float(h, _p(_to_dev(every[:4].view(np.int16))), 0, _p(out)) == 0 and _intact(out)


# =====================================================================================================================================
# 7. ps_op_probs_to_volume (winner_rows_kernel, winner_vox_kernel, fill_volume_kernel)
# =====================================================================================================================================
def _volume_ref(logits, p_idx, xyz, total, Z, X, Y):
    """the reference's loop (testBraTS.py:83-101, 226-231); rows and points that fall outside are skipped"""
    n, C = logits.shape
    z64 = logits.astype(f64)
    e = np.exp(z64 - z64.max(1, keepdims=True)) if n else z64
    probs = e / e.sum(1, keepdims=True) if n else z64
    test_probs = np.zeros((total, C))
    hit = np.zeros(total, bool)  # the points some row was sampled for
    for j in range(n):
        i = j if p_idx is None else int(p_idx[j])
        if 0 <= i < total:
            test_probs[i] = probs[j]
            hit[i] = True
    volume = np.zeros((Z, X, Y, C))
    sampled = np.zeros((Z, X, Y), bool)
    for i in range(total):
        x, y, z = (int(v) for v in xyz[i])
        if 0 <= x < X and 0 <= y < Y and 0 <= z < Z:
            volume[z][x][y] = test_probs[i]
            sampled[z][x][y] = hit[i]
    return np.moveaxis(volume, 1, 2), np.moveaxis(sampled, 1, 2)


@pytest.mark.parametrize("C", [1, 2, 4, 13])
@pytest.mark.parametrize("mode", ["identity", "table", "table with skipped rows", "no rows", "large logits"])
def test_probs_to_volume(env, C, mode):
    lib, h = env
    from point_unet_amd.postprocess import point2prod
    Z, X, Y = 5, 9, 7  # 315 voxels: a second, partial block
    total = 700
    rng = np.random.default_rng(C * 10 + len(mode))
    xyz = np.stack([rng.integers(0, X, total), rng.integers(0, Y, total), rng.integers(0, Z, total)], 1).astype(i32)  # duplicates are the rule
    for axis, dim in enumerate((X, Y, Z)):  # one component just outside, either side: such points are skipped
        xyz[10 + axis, axis] = -1
        xyz[20 + axis, axis] = dim
    xyz[-1] = xyz[0]  # the last point sits on the first one's voxel and wins it
    if mode == "identity":
        n, p_idx = 600, None  # points 600.. were not sampled
    elif mode == "no rows":
        n, p_idx = 0, None
    else:
        n = 500
        p_idx = rng.integers(0, total, n).astype(i32)
        p_idx[-1] = p_idx[0]
        if mode == "table with skipped rows":
            p_idx[5], p_idx[6], p_idx[7] = -1, total, total + 9
    logits = rng.standard_normal((max(n, 1), C)).astype(f32)
    if mode == "large logits":
        logits = np.where(rng.random(logits.shape) < 0.5, f32(90.0), f32(-90.0)).astype(f32) + logits
    want, sampled = _volume_ref(logits[:n], p_idx, xyz, total, Z, X, Y)
    nvox = Z * X * Y
    assert nvox % 256 and (n == 0 or 0 < sampled.sum() < nvox)
    vol = _sentinel(nvox, C)
    scratch = torch.empty(total + nvox, dtype=torch.int32, device="cuda")
    dl, dp, dxyz = _to_dev(logits), (None if p_idx is None else _to_dev(p_idx)), _to_dev(xyz)
    assert lib.ps_op_probs_to_volume(h, _p(dl), n, C, _p(dp), _p(dxyz), total, Z, X, Y, _p(vol), _p(scratch)) == 0
    got = _payload(vol, nvox, C).reshape(Z, Y, X, C)
    assert (got[~sampled] == 0).all() and not np.signbit(got[~sampled]).any()
    assert np.abs(got - want).max() <= 1e-6  # values <= 1, C <= 13: (C + 4) 2^-24 plus the error of expf
    if n == 0:
        assert not got.any()
    else:
        pi = None if p_idx is None else torch.from_numpy(p_idx).cuda()
        wrapped = point2prod(torch.from_numpy(logits[:n]).cuda(), pi, torch.from_numpy(xyz).cuda(), (Z, X, Y)).cpu().numpy()
        assert wrapped.shape == (Z, Y, X, C) and wrapped.tobytes() == got.tobytes()


# =====================================================================================================================================
# 9. argument checks: PS_EINVAL before anything is enqueued
# =====================================================================================================================================
REFUSED = [dict(B=-1), dict(M=-1), dict(N=0), dict(K=0), dict(d=0), dict(N=-5), dict(K=-1), dict(d=-4), dict(N=2 ** 31), dict(M=2 ** 31),
           dict(K=2 ** 31), dict(d=2 ** 31), dict(B=-1, M=-1)]


@pytest.mark.parametrize("entry", ["ps_op_random_sample", "ps_op_random_sample_ties", "ps_op_relative_pos_encoding",
                                   "ps_op_nearest_interpolation", "ps_op_gather_neighbour", "ps_op_gather_neighbour_ex"])
def test_shape_refusals(env, entry):
    lib, h = env
    src, idx = _to_dev(np.zeros(256, f32)), _to_dev(np.zeros(256, i32))
    fn = getattr(lib, entry)
    takes = {"ps_op_relative_pos_encoding": "BNK", "ps_op_nearest_interpolation": "BNMd"}.get(entry, "BNMKd")
    seen = 0
    for bad in REFUSED:
        if not set(bad) <= set(takes):
            continue
        s = dict(B=1, N=4, M=2, K=2, d=4)
        s.update(bad)
        out = _sentinel(8, 16)
        ties = torch.full((64,), 0xEE, dtype=torch.uint8, device="cuda")
        args = [h, _p(src), _p(idx)] + [s[k] for k in takes] + [_p(out)]
        if entry == "ps_op_random_sample_ties":
            args.append(_p(ties))
        if entry == "ps_op_gather_neighbour_ex":
            args.append(max(s["d"], 4))
        assert fn(*args) == PS_EINVAL, (entry, bad)
        assert entry.replace("_ex", "").encode() in lib.ps_last_error(), lib.ps_last_error()
        assert _intact(out) and bool((ties == 0xEE).all()), (entry, bad)
        seen += 1
    assert seen >= 7
    if entry == "ps_op_gather_neighbour_ex":  # rows per cloud M * K is an `int` in the kernels
        out = _sentinel(8, 16)
        assert fn(h, _p(src), _p(idx), 1, 4, 2 ** 30, 2, 4, _p(out), 4) == PS_EINVAL and _intact(out)
