"""Op-level checks of the training ops of include/pointseg_train_ops.h that the whole-step tests cannot see: Adam beyond its first step
(moments carried, beta powers, the host-side lr_t, the trainer's step counter), dropout against an independent restatement
(dropout_ref.py), BatchNorm split at its reduction (the SyncBN protocol) and its row-strided forms, the BatchNorm statistics of channels
whose mean is large against their spread, the leaky-ReLU slope at exactly 0, the conv+BN backward entries, the weighted cross-entropy
at its edges and the elementwise helpers.  Every op is called directly on the default context (the slice kernel on a tuned context) and
compared with float64.  Sizes are odd, and some exceed the grid of the grid-stride loops (8192 x 256 elements; 1024 x 256 rows for the
cross-entropy)."""
import ctypes

import numpy as np
import pytest

import dropout_ref as dr
import netcase

pytestmark = pytest.mark.gpu

LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-8
BN_EPS = 1e-6


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _env():
    from point_unet_amd import _lib, runtime
    return _lib, _lib.lib(), runtime.default_context(0).handle


def _dev(a):
    """A device copy of `a`.  Bind it to a name for as long as a kernel may read it: a pointer to a temporary is freed at once, and the
    caching allocator hands its block to the next allocation."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _f32(x):
    """The float64 value of x rounded to float32 (what a float parameter of the C ABI carries)."""
    return float(np.float32(x))


def _ulp32(a):
    a = np.abs(np.asarray(a, dtype=np.float64)).astype(np.float32)
    return np.spacing(np.maximum(a, np.float32(np.finfo(np.float32).tiny))).astype(np.float64)


# ---- Adam -------------------------------------------------------------------------------------------------------------------------------
def _lr_t(t, lr=LR):
    b1, b2 = _f32(B1), _f32(B2)
    return _f32(lr) * np.sqrt(1.0 - b2 ** float(t)) / (1.0 - b1 ** float(t))


def _adam64(p, m, v, g, t, lr=LR):
    """tf.train.AdamOptimizer in float64 on the float32 hyper-parameters the kernel receives."""
    b1, b2, eps = _f32(B1), _f32(B2), _f32(EPS)
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    return p - _lr_t(t, lr) * m / (np.sqrt(v) + eps), m, v


def _adam_grads(rng, kind, base, t):
    """Five kinds of gradient: 0 magnitudes from 1e-6 to 1e2 (fresh every step), 1 exact zeros, 2 below eps, 3 sign flips every step,
    4 constant sign."""
    n = kind.size
    g = np.where(rng.random(n) < 0.5, -1.0, 1.0) * 10.0 ** rng.uniform(-6.0, 2.0, n)
    g = np.where(kind == 1, 0.0, g)
    g = np.where(kind == 2, base * 1e-9 * np.where(rng.random(n) < 0.5, -1.0, 1.0), g)
    g = np.where(kind == 3, base * (-1.0) ** t, g)
    g = np.where(kind == 4, base * (1.0 + 0.5 * rng.random(n)), g)
    return g.astype(np.float32)


def test_adam_tracks_float64_adam_over_200_steps():
    """200 consecutive ps_op_adam calls against a float64 Adam fed the same fp32 gradients: m and v at relative 1e-5 (m relative to the
    gradient scale sqrt(v), since a mean of signed gradients may cancel), p within 1e-3 lr t.  A wrong beta power or a moment dropped
    between steps moves p by O(lr); zero gradients leave p, m and v exactly as they were."""
    import torch
    _lib, L, h = _env()
    n = 1_000_003
    rng = np.random.default_rng(11)
    kind = rng.integers(0, 5, n)
    base = 10.0 ** rng.uniform(-3.0, 1.0, n)
    p0 = rng.standard_normal(n).astype(np.float32)
    P, M, V = _dev(p0), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    p64, m64, v64 = p0.astype(np.float64), np.zeros(n), np.zeros(n)
    checked = 0
    for t in range(1, 201):
        g = _adam_grads(rng, kind, base, t)
        G = _dev(g)
        _lib.check(L.ps_op_adam(h, _p(P), _p(G), _p(M), _p(V), n, LR, B1, B2, EPS, t))
        p64, m64, v64 = _adam64(p64, m64, v64, g.astype(np.float64), t)
        if t in (1, 2, 3, 10, 50, 200):
            p, m, v = _host(P).astype(np.float64), _host(M).astype(np.float64), _host(V).astype(np.float64)
            assert np.all(np.abs(v - v64) <= 1e-5 * v64), (t, np.abs(v - v64).max())
            assert np.all(np.abs(m - m64) <= 1e-5 * np.maximum(np.abs(m64), np.sqrt(v64))), (t, np.abs(m - m64).max())
            err = np.abs(p - p64)
            assert err.max() <= 1e-3 * LR * t, (t, err.max(), int(err.argmax()), int(kind[err.argmax()]))
            zero = kind == 1
            assert np.array_equal(p[zero], p0[zero].astype(np.float64)) and not m[zero].any() and not v[zero].any()
            checked += 1
    assert checked == 6
    # the constant-sign and flipping entries moved: a test that never moved p would pass the bars above
    assert np.abs(p64 - p0)[kind == 4].min() > 0.1 * LR


@pytest.mark.parametrize("t", [1, 2, 10, 1000, 10 ** 6, 2 ** 31 + 5])
def test_adam_one_step_from_zero_moments_at_any_step(t):
    """From m = v = 0 one step is p -= lr_t (1-b1) g / (sqrt((1-b2) g^2) + eps) with lr_t = lr sqrt(1-b2^t)/(1-b1^t) formed on the host in
    double from the int64 step (2^31 + 5 does not fit an int).  n wraps the grid-stride loop."""
    import torch
    _lib, L, h = _env()
    n = 2 ** 21 + 4099
    rng = np.random.default_rng(t % 1000)
    g = (np.where(rng.random(n) < 0.5, -1.0, 1.0) * 10.0 ** rng.uniform(-10.0, 2.0, n)).astype(np.float32)
    g[::7] = 0.0
    P, M, V = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    G = _dev(g)
    _lib.check(L.ps_op_adam(h, _p(P), _p(G), _p(M), _p(V), n, LR, B1, B2, EPS, t))
    want, _, _ = _adam64(np.zeros(n), np.zeros(n), np.zeros(n), g.astype(np.float64), t)
    got = _host(P).astype(np.float64)
    assert np.all(np.abs(got - want) <= 1e-6 * np.abs(want)), (t, np.abs(got - want).max())
    assert np.abs(got[np.abs(g) > 1e-3]).min() > 0.99 * _lr_t(t) * 0.1 / np.sqrt(1.0 - _f32(B2))


def _trainer(engine):
    import torch
    from point_unet_amd import weights
    from point_unet_amd.pyramid import build_pyramid
    from point_unet_amd.train import Trainer
    cfg, xyz, feats = netcase.small_deep(1500, seed=2, B=2)
    cfg.d_out = [16, 32, 64, 32, 16]
    params = weights.init_params(cfg, seed=3, randomize_bn=True)
    labels = np.random.default_rng(3).integers(0, cfg.num_classes, xyz.shape[:2]).astype(np.int32)
    cw = np.linspace(1.0, 2.0, cfg.num_classes).astype(np.float32)
    tr = Trainer(cfg, params=params, learning_rate=LR, class_weights=cw, keep_prob=0.5, engine=engine)
    pyr = build_pyramid(torch.from_numpy(xyz).cuda(), cfg)
    return tr, (pyr, torch.from_numpy(feats).cuda(), torch.from_numpy(labels).cuda())


def _check_adam_step(before, g, t, after):
    """One Adam step of the trainer against float64 from the fp32 state the kernel itself started from.  before / after = (p, m, v) as
    float64 copies of the stored fp32 buffers, g = the trainer's own gradient (tr.grad).  The fp32 evaluation errs by a few ulps of the
    terms before they cancel: m = b1 m' + (1-b1) g cancels when the gradient changes sign between steps, so its bar is relative to
    b1 |m'| + (1-b1) |g| (not to |m|), and the update's bar carries that error through lr_t / (sqrt(v) + eps).  v has no cancellation
    (a floor of a few fp32 denormal spacings for tiny gradients); p rounds once more on the subtraction."""
    p0, m0, v0 = before
    p1, m1, v1 = after
    want_p, want_m, want_v = _adam64(p0, m0, v0, g, t)
    b1, b2, eps = _f32(B1), _f32(B2), _f32(EPS)
    sm = b1 * np.abs(m0) + (1.0 - b1) * np.abs(g)
    sv = b2 * v0 + (1.0 - b2) * g * g
    assert np.all(np.abs(v1 - want_v) <= 1e-6 * sv + 1e-44), ("v", np.abs(v1 - want_v).max())
    bar_m = 4e-7 * sm + 1e-44
    assert np.all(np.abs(m1 - want_m) <= bar_m), ("m", np.abs(m1 - want_m).max())
    update = np.abs(want_p - p0)
    bar_p = 2.5e-7 * np.abs(want_p) + 1e-6 * update + _lr_t(t) * bar_m / (np.sqrt(want_v) + eps) + 1e-30
    err = np.abs(p1 - want_p)
    assert np.all(err <= bar_p), ("p", t, err.max(), int(np.argmax(err / bar_p)), float((err / bar_p).max()))
    # every entry whose update exceeds two fp32 spacings of p moved (a skipped or zeroed update passes nothing above either)
    moves = update > 2 * _ulp32(p0)
    assert np.all(p1[moves] != p0[moves])
    if not m0.any():  # from zero moments nothing cancels: the update is about lr_t / sqrt(1 - b2) wherever |g| >> eps
        assert moves.sum() > 1000


def _state(tr):
    return tuple(_host(b).astype(np.float64) for b in (tr.flat, tr.m, tr.v))


@pytest.mark.parametrize("engine", ["native", "python"])
def test_trainer_adam_step_counter_and_moments(engine):
    """The trainer's Adam: (1) a fresh trainer set to step k takes the step t = k + 1 (ps_trainer_set_step, then get_step), its update the
    closed form at t = k + 1 from zero moments; (2) two consecutive steps from step 0 equal a float64 Adam fed the trainer's own gradients
    (tr.grad), with m and v carried -- which separates Adam from the noise of the gradients.  Each step is checked from the fp32 state the
    kernel started from (_check_adam_step): the Python tape's gradients carry float-atomic noise from run to run, and a float64 chain of
    its own would compare the second step's cancellations against a different starting m."""
    from point_unet_amd import _lib
    for k in (9, 999):
        tr, batch = _trainer(engine)
        tr.step = k  # train_step hands it to ps_trainer_set_step (native) / the tape's ps_op_adam (python)
        before = _state(tr)
        assert not before[1].any() and not before[2].any()
        tr.train_step(*batch)
        assert tr.step == k + 1
        if engine == "native":
            assert _lib.lib().ps_trainer_get_step(tr._h) == k + 1
        g = _host(tr.grad).astype(np.float64)
        assert np.abs(g).max() > 0
        _check_adam_step(before, g, k + 1, _state(tr))
        del tr, batch
    tr, batch = _trainer(engine)
    state = _state(tr)
    for t in (1, 2):
        tr.train_step(*batch)
        assert tr.step == t
        g = _host(tr.grad).astype(np.float64)
        after = _state(tr)
        _check_adam_step(state, g, t, after)
        state = after


# ---- dropout and the elementwise helpers ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("keep", [0.1, 0.5, 0.9, 1.0])
def test_dropout_mask_is_the_restatement_bit_for_bit(keep):
    """mask == dropout_ref.dropout_mask, y == x * mask and ps_op_mul(dy, mask) == dy * mask, all bit for bit; the mask holds only 0 and
    float32(1 / keep).  n = 2^22 + 3 wraps the grid-stride loop twice."""
    import torch
    _lib, L, h = _env()
    n = 2 ** 22 + 3
    rng = np.random.default_rng(int(keep * 10))
    x = rng.standard_normal(n).astype(np.float32)
    seed = dr.step_seed(41, 3)
    X = _dev(x)
    Y, Mk = torch.empty(n, device="cuda"), torch.empty(n, device="cuda")
    _lib.check(L.ps_op_dropout(h, _p(X), n, seed, keep, _p(Y), _p(Mk)))
    mask, want = _host(Mk), dr.dropout_mask(n, seed, keep)
    assert np.array_equal(mask.view(np.uint32), want.view(np.uint32)), int(np.count_nonzero(mask != want))
    assert set(np.unique(mask).tolist()) <= {0.0, float(np.float32(1.0) / np.float32(keep))}
    assert np.array_equal(_host(Y).view(np.uint32), (x * want).view(np.uint32))
    dy = rng.standard_normal(n).astype(np.float32)
    DX = torch.empty(n, device="cuda")
    DY = _dev(dy)
    _lib.check(L.ps_op_mul(h, _p(DY), _p(Mk), n, _p(DX)))
    assert np.array_equal(_host(DX).view(np.uint32), (dy * want).view(np.uint32))
    if keep < 1.0:
        kept = np.count_nonzero(mask) / n
        assert abs(kept - keep) <= 6.0 * np.sqrt(keep * (1.0 - keep) / n)


def test_axpy_mul_and_add_lrelu_bwd_against_float64():
    """1 fp32 ulp of the float64 result (axpy: plus half an ulp of alpha x, the product the unfused form rounds); n wraps the grid."""
    _lib, L, h = _env()
    n = 2 ** 21 + 2 ** 20 + 13
    rng = np.random.default_rng(5)
    x = (rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 3, n)).astype(np.float32)
    y = (rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 3, n)).astype(np.float32)
    alpha = np.float32(-0.3711)
    Y = _dev(y)
    X, Yb = _dev(x), _dev(y)
    _lib.check(L.ps_op_axpy(h, float(alpha), _p(X), n, _p(Y)))
    ax = float(alpha) * x.astype(np.float64)
    want = y.astype(np.float64) + ax
    assert np.all(np.abs(_host(Y) - want) <= _ulp32(want) + 0.5 * _ulp32(ax))
    import torch
    out = torch.empty(n, device="cuda")
    _lib.check(L.ps_op_mul(h, _p(X), _p(Yb), n, _p(out)))
    want = x.astype(np.float64) * y.astype(np.float64)
    assert np.all(np.abs(_host(out) - want) <= 0.5 * _ulp32(want))
    # add_lrelu_bwd: ds = dy where y > 0, 0.2 dy elsewhere -- y = +0.0 and -0.0 included (tf's LeakyReluGrad: slope 1 only where > 0)
    yy = rng.standard_normal(n).astype(np.float32)
    yy[::5] = 0.0
    yy[2::10] = -0.0
    dy = rng.standard_normal(n).astype(np.float32)
    DY, YY = _dev(dy), _dev(yy)
    _lib.check(L.ps_op_add_lrelu_bwd(h, _p(DY), _p(YY), n, _p(out)))
    want = np.where(yy > 0, dy.astype(np.float64), _f32(0.2) * dy.astype(np.float64))
    got = _host(out)
    assert np.all(np.abs(got - want) <= 0.5 * _ulp32(want))
    zero = yy == 0
    assert zero.sum() >= n // 5 and np.array_equal(got[zero], (np.float32(0.2) * dy)[zero])


# ---- weighted cross-entropy -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 2, 13, 64])
def test_weighted_ce_edges_against_float64(C):
    """Logits of +-80, labels -1 and C (ignored: zero gradient rows, not in the mean), R above 1024 x 256 rows; all rows ignored: NaN loss
    and an all-zero gradient."""
    import torch
    _lib, L, h = _env()
    R = 1024 * 256 + 777
    g = torch.Generator().manual_seed(C)
    z = torch.randn(R, C, generator=g) * 3
    z[::97] = 80.0 * torch.sign(torch.randn(z[::97].shape, generator=g))
    z[5::101, 0] = -80.0
    y = torch.randint(0, C, (R,), generator=g).int()
    y[::13] = -1
    y[7::17] = C
    w = torch.rand(C, generator=g) + 0.5
    Z, Y, W = z.cuda(), y.cuda(), w.cuda()
    loss, dz = torch.zeros(1, device="cuda"), torch.full((R, C), 7.0, device="cuda")
    _lib.check(L.ps_op_weighted_ce(h, _p(Z), _p(Y), _p(W), R, C, _p(loss), _p(dz)))
    keep = (y >= 0) & (y < C)
    zd = z.double().requires_grad_(True)
    ref = (torch.nn.functional.cross_entropy(zd[keep], y[keep].long(), reduction="none") * w.double()[y[keep].long()]).mean()
    ref.backward()
    assert abs(float(loss) - float(ref)) <= 1e-5 * max(1.0, abs(float(ref))), (float(loss), float(ref))
    got = dz.cpu().double()
    assert float((got - zd.grad).abs().max()) <= 1e-5 * max(float(zd.grad.abs().max()), 1e-30)
    assert float(got[~keep].abs().max()) == 0.0
    none = torch.full((R,), -1, dtype=torch.int32)
    none[1::2] = C
    NONE = none.cuda()
    _lib.check(L.ps_op_weighted_ce(h, _p(Z), _p(NONE), _p(W), R, C, _p(loss), _p(dz)))
    assert np.isnan(float(loss)) and float(dz.abs().max()) == 0.0


# ---- BatchNorm ---------------------------------------------------------------------------------------------------------------------------------
def _bn64(x, gamma, beta, leaky, dy=None):
    """float64 BatchNorm with batch statistics (population variance) [+ LeakyReLU 0.2] and, with dy, its autograd gradients."""
    import torch
    xd = torch.from_numpy(x.astype(np.float64)).requires_grad_(True)
    gd = torch.from_numpy(gamma.astype(np.float64)).requires_grad_(True)
    bd = torch.from_numpy(beta.astype(np.float64)).requires_grad_(True)
    mean, var = xd.mean(0), xd.var(0, unbiased=False)
    z = (xd - mean) / torch.sqrt(var + _f32(BN_EPS)) * gd + bd
    y = torch.nn.functional.leaky_relu(z, 0.2) if leaky else z
    out = {"y": y.detach().numpy(), "z": z.detach().numpy(), "mean": mean.detach().numpy(), "var": var.detach().numpy(),
           "invstd": 1.0 / np.sqrt(var.detach().numpy() + _f32(BN_EPS))}
    if dy is not None:
        y.backward(torch.from_numpy(dy.astype(np.float64)))
        out.update(dx=xd.grad.numpy(), dgamma=gd.grad.numpy(), dbeta=bd.grad.numpy())
    return out


def _away_from_kink(dy, z, leaky):
    """dy with the rows zeroed where z is within rounding of the kink (0 < |z| < 1e-4): there fp32 and float64 may pick different slopes."""
    if not leaky:
        return dy
    return np.where((np.abs(z) < 1e-4) & (z != 0), 0.0, dy).astype(np.float32)


def _bn_case(R, C, seed, r=3.0):
    rng = np.random.default_rng(seed)
    sigma = 10.0 ** rng.uniform(-1, 1, C)
    x = (r * sigma + sigma * rng.standard_normal((R, C))).astype(np.float32)
    gamma = (rng.random(C) + 0.5).astype(np.float32)
    beta = rng.standard_normal(C).astype(np.float32)
    return rng, x, gamma, beta


def _rel_close(got, want, bar, scale=None):
    scale = np.abs(want) if scale is None else scale
    err = np.abs(np.asarray(got, np.float64) - want)
    return bool(np.all(err <= bar * scale)), float((err / np.maximum(scale, 1e-300)).max())


@pytest.mark.parametrize("leaky", [0, 1])
@pytest.mark.parametrize("C", [1, 3, 8, 32, 64, 128])
def test_split_batchnorm_equals_the_whole_batch(C, leaky):
    """The SyncBN protocol on one GPU: sums of each part, added on the host, apply with R_total; bwd_sums of each part, added, bwd_apply.
    Against float64 BatchNorm and autograd over the whole tensor (channel means at most 3 standard deviations: the float sums that cross
    the ranks bound the variance to ~1e-7 r^2 of itself, pointseg_train_ops.h)."""
    import torch
    _lib, L, h = _env()
    for parts in ((1, 4098), (1031, 2606), (2606, 1)):
        R = sum(parts)
        rng, x, gamma, beta = _bn_case(R, C, 100 * C + R + leaky)
        ref = _bn64(x, gamma, beta, leaky)
        dy = _away_from_kink(rng.standard_normal((R, C)).astype(np.float32), ref["z"], leaky)
        ref = _bn64(x, gamma, beta, leaky, dy)
        X, G, Bt, DY = _dev(x), _dev(gamma), _dev(beta), _dev(dy)
        sums = torch.zeros(2 * C, device="cuda")
        offs = np.cumsum((0,) + parts)
        for a, b in zip(offs[:-1], offs[1:]):
            part = torch.empty(2 * C, device="cuda")
            _lib.check(L.ps_op_bn_train_sums(h, _p(X[a:b]), b - a, C, _p(part)))
            sums += part  # (the all-reduce)
        Y = torch.empty(R, C, device="cuda")
        st = torch.empty(3, C, device="cuda")
        for a, b in zip(offs[:-1], offs[1:]):
            _lib.check(L.ps_op_bn_train_apply(h, _p(X[a:b]), _p(G), _p(Bt), _p(sums), b - a, R, C, BN_EPS, leaky, _p(Y[a:b]), _p(st[0]), _p(st[1]),
                                              _p(st[2])))
        mean, invstd, var = _host(st)
        assert _rel_close(var, ref["var"], 1e-5)[0] and _rel_close(invstd, ref["invstd"], 1e-5)[0], (parts, var, ref["var"])
        assert np.all(np.abs(mean - ref["mean"]) <= 1e-6 * np.sqrt(ref["var"]) + 1e-6 * np.abs(ref["mean"]))
        assert _rel_close(_host(Y), ref["y"], 2e-5, np.abs(gamma) * 6 + np.abs(beta))[0], parts
        dg, dbt = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
        for a, b in zip(offs[:-1], offs[1:]):
            pg, pb = torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
            _lib.check(L.ps_op_bn_train_bwd_sums(h, _p(DY[a:b]), _p(X[a:b]), _p(G), _p(Bt), _p(st[0]), _p(st[1]), b - a, C, leaky, _p(pg), _p(pb)))
            dg += pg
            dbt += pb
        gscale = np.abs(dy).sum(0) * 6
        assert _rel_close(_host(dbt), ref["dbeta"], 1e-5, gscale)[0] and _rel_close(_host(dg), ref["dgamma"], 1e-5, gscale)[0]
        DX = torch.empty(R, C, device="cuda")
        for a, b in zip(offs[:-1], offs[1:]):
            _lib.check(L.ps_op_bn_train_bwd_apply(h, _p(DY[a:b]), _p(X[a:b]), _p(G), _p(Bt), _p(st[0]), _p(st[1]), _p(dbt), _p(dg), b - a, R, C, leaky,
                                                  _p(DX[a:b])))
        ok, worst = _rel_close(_host(DX), ref["dx"], 2e-5, np.abs(ref["dx"]).max(0))
        assert ok, (parts, worst)


@pytest.mark.parametrize("C", [3, 8, 32, 64])
def test_row_strided_batchnorm_writes_only_its_columns(C):
    """The _ex forms with ldy = C + 5 and with a column block of a wider tensor: the results equal the dense forms, the columns outside the
    block keep a sentinel bit for bit; dy read from a column block gives the dense gradients."""
    import torch
    _lib, L, h = _env()
    R = 2999
    rng, x, gamma, beta = _bn_case(R, C, C)
    X, G, Bt = _dev(x), _dev(gamma), _dev(beta)
    dense = torch.empty(R, C, device="cuda")
    st0 = torch.empty(5, C, device="cuda")
    _lib.check(L.ps_op_bn_train_fwd(h, _p(X), _p(G), _p(Bt), R, C, BN_EPS, 1, _p(dense), _p(st0[0]), _p(st0[1]), _p(st0[2]), _p(st0[3])))
    sums = st0[3:5].reshape(-1).clone()
    _lib.check(L.ps_op_bn_train_sums(h, _p(X), R, C, _p(sums)))
    dy = rng.standard_normal((R, C)).astype(np.float32)
    DY = _dev(dy)
    dx0, dg0, db0 = torch.empty(R, C, device="cuda"), torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
    _lib.check(L.ps_op_bn_train_bwd(h, _p(DY), _p(X), _p(G), _p(Bt), _p(st0[0]), _p(st0[1]), R, C, 1, _p(dx0), _p(dg0), _p(db0)))
    gscale = np.abs(dy).sum(0) * 6

    def _same(a, b, scale=None):
        b = _host(b).astype(np.float64)
        return _rel_close(_host(a), b, 1e-5, np.abs(b).max(0) if scale is None else scale)[0]

    sentinel = np.float32(-1234.5)
    for ld, off in ((C + 5, 0), (2 * C + 8, C + 4), (C + 7, 3)):
        for op in ("fwd_ex", "fwd_mov", "apply_ex"):
            wide = torch.full((R, ld), float(sentinel), device="cuda")
            st = torch.empty(5, C, device="cuda")
            Y = wide.view(-1)[off:]
            if op == "fwd_ex":
                _lib.check(L.ps_op_bn_train_fwd_ex(h, _p(X), _p(G), _p(Bt), R, C, BN_EPS, 1, _p(Y), ld, _p(st[0]), _p(st[1]), _p(st[2]), _p(st[3])))
            elif op == "fwd_mov":
                mm, mv = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")
                _lib.check(L.ps_op_bn_train_fwd_mov(h, _p(X), _p(G), _p(Bt), R, C, BN_EPS, 1, _p(Y), ld, _p(st[0]), _p(st[1]), _p(st[2]), _p(st[3]),
                                                    _p(mm), _p(mv), 0.99))
            else:
                _lib.check(L.ps_op_bn_train_apply_ex(h, _p(X), _p(G), _p(Bt), _p(sums), R, R, C, BN_EPS, 1, _p(Y), ld, _p(st[0]), _p(st[1]), _p(st[2])))
            w = _host(wide)
            inside = np.zeros((R, ld), bool)
            inside[:, off:off + C] = True
            assert np.array_equal(w[~inside].view(np.uint32), np.full((~inside).sum(), sentinel).view(np.uint32)), (op, ld, off)
            ok, worst = _rel_close(w[:, off:off + C], _host(dense).astype(np.float64), 1e-5, np.abs(_host(dense)).max(0) + 1)
            assert ok, (op, ld, off, worst)
        wide = torch.full((R, ld), float(sentinel), device="cuda")
        wide[:, off:off + C] = DY
        DYb = wide.view(-1)[off:]
        # (a strided dy may take the scalar path where the dense one took float4 loads: another summation order, hence a tolerance)
        dx, dg, db = torch.empty(R, C, device="cuda"), torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
        _lib.check(L.ps_op_bn_train_bwd_ex(h, _p(DYb), ld, _p(X), _p(G), _p(Bt), _p(st0[0]), _p(st0[1]), R, C, 1, _p(dx), _p(dg), _p(db)))
        assert _same(dx, dx0) and _same(dg, dg0, gscale) and _same(db, db0, gscale), (ld, off)
        _lib.check(L.ps_op_bn_train_bwd_sums_ex(h, _p(DYb), ld, _p(X), _p(G), _p(Bt), _p(st0[0]), _p(st0[1]), R, C, 1, _p(dg), _p(db)))
        assert _same(dg, dg0, gscale) and _same(db, db0, gscale), (ld, off)
        _lib.check(L.ps_op_bn_train_bwd_apply_ex(h, _p(DYb), ld, _p(X), _p(G), _p(Bt), _p(st0[0]), _p(st0[1]), _p(db0), _p(dg0), R, R, C, 1, _p(dx)))
        assert _same(dx, dx0), (ld, off)
        assert np.array_equal(_host(wide)[:, off + C:].view(np.uint32), np.full((R, ld - off - C), sentinel).view(np.uint32))


def _contexts():
    import contextlib
    import tuning
    from point_unet_amd import runtime

    @contextlib.contextmanager
    def default():
        yield runtime.default_context(0)
    return {"generic": default, "slice": lambda: tuning.tuned_context(bn_slice=1)}


@pytest.mark.parametrize("path", ["generic", "slice"])
def test_moving_statistics_after_three_calls(path):
    """ps_op_bn_train_fwd_mov three times: moving = 0.99 moving + 0.01 batch, against a float64 EMA (R <= 4096, C % 32 == 0: the one-launch
    kernel on the slice path)."""
    import torch
    _lib = _env()[0]
    L = _lib.lib()
    R, C = 3001, 64
    mom = _f32(0.99)
    with _contexts()[path]() as ctx:
        h = ctx.handle
        mm, mv = torch.full((C,), 0.5, device="cuda"), torch.full((C,), 2.0, device="cuda")
        m64, v64 = np.full(C, 0.5), np.full(C, 2.0)
        for call in range(3):
            rng, x, gamma, beta = _bn_case(R, C, 7 + call, r=2.0 + call)
            Y, st = torch.empty(R, C, device="cuda"), torch.empty(5, C, device="cuda")
            X, G, Bt = _dev(x), _dev(gamma), _dev(beta)
            _lib.check(L.ps_op_bn_train_fwd_mov(h, _p(X), _p(G), _p(Bt), R, C, BN_EPS, 1, _p(Y), C, _p(st[0]), _p(st[1]),
                                                _p(st[2]), _p(st[3]), _p(mm), _p(mv), 0.99))
            ref = _bn64(x, gamma, beta, 1)
            m64 = mom * m64 + (1.0 - mom) * ref["mean"]
            v64 = mom * v64 + (1.0 - mom) * ref["var"]
            assert _rel_close(_host(st[2]), ref["var"], 1e-5)[0]
        assert _rel_close(_host(mm), m64, 1e-5)[0] and _rel_close(_host(mv), v64, 1e-5)[0], (_host(mv), v64)


@pytest.mark.parametrize("path,form,C,shift", [("generic", "float4", 32, 0), ("generic", "fixed-channel", 32, 1), ("generic", "per-channel", 13, 0),
                                               ("slice", "one-launch", 32, 0)])
def test_batchnorm_statistics_of_offset_channels(path, form, C, shift):
    """Channels r sigma + N(0, sigma^2), r in {0, 3, 10, 30, 100}, one near-constant and one constant channel (value 100: var 0, invstd
    rsqrt(eps)): var and invstd at relative 1e-5 of float64 through fwd, fwd_mov and bwd; y and dx at the same relative error.  fp32 one-pass
    sums E[x^2] - mean^2 lose ~1e-7 r^2 of the variance.  Every branch of the statistics: colreduce2's float4 path (C = 32, aligned rows),
    its fixed-channel path (256 % C == 0, x one float off 16-byte alignment), its per-channel path (C = 13) and the one-launch slice
    kernel."""
    import torch
    _lib = _env()[0]
    L = _lib.lib()
    R = 180_000 if path == "generic" else 4000
    nr = C - 2
    rng = np.random.default_rng(31)
    rs = np.resize(np.array([0.0, 3.0, 10.0, 30.0, 100.0]), nr)
    sigma = 10.0 ** rng.uniform(-2, 2, nr)
    x = np.empty((R, C), np.float32)
    x[:, :nr] = rs * sigma + sigma * rng.standard_normal((R, nr))
    x[:, nr] = 100.0 + 1e-2 * rng.standard_normal(R)
    x[:, nr + 1] = 100.0
    gamma = (rng.random(C) + 0.5).astype(np.float32)
    beta = rng.standard_normal(C).astype(np.float32)
    dy = rng.standard_normal((R, C)).astype(np.float32)
    ref = _bn64(x, gamma, beta, 0, dy)
    assert ref["var"][nr + 1] == 0.0
    xbuf = torch.empty(R * C + shift, device="cuda")
    xbuf[shift:] = torch.from_numpy(x.reshape(-1)).cuda()
    X = xbuf[shift:]  # (shift = 1: the rows start 4 bytes past a 16-byte boundary)
    assert (X.data_ptr() % 16 == 0) == (shift == 0)
    G, Bt, DY = _dev(gamma), _dev(beta), _dev(dy)
    # beyond the bar: the stored fp32 mean is off by up to half an ulp, an error of delta in every xhat (r = 1e4 in the near-constant channel)
    delta = 0.5 * _ulp32(ref["mean"]) * ref["invstd"]
    ybar = 1e-5 * np.abs(ref["y"]).max(0) + np.abs(gamma) * delta
    dxbar = 1e-5 * np.abs(ref["dx"]).max(0) + np.abs(gamma) * ref["invstd"] * np.abs(ref["dgamma"]) / R * delta
    with _contexts()[path]() as ctx:
        h = ctx.handle
        for op in ("fwd", "fwd_mov"):
            Y, st = torch.empty(R, C, device="cuda"), torch.empty(5, C, device="cuda")
            if op == "fwd":
                _lib.check(L.ps_op_bn_train_fwd(h, _p(X), _p(G), _p(Bt), R, C, BN_EPS, 0, _p(Y), _p(st[0]), _p(st[1]), _p(st[2]), _p(st[3])))
            else:
                mm, mv = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
                _lib.check(L.ps_op_bn_train_fwd_mov(h, _p(X), _p(G), _p(Bt), R, C, BN_EPS, 0, _p(Y), C, _p(st[0]), _p(st[1]), _p(st[2]), _p(st[3]),
                                                    _p(mm), _p(mv), 0.99))
                mv64 = (1.0 - _f32(0.99)) * ref["var"]
                assert _rel_close(_host(mv), mv64, 1e-5)[0], (op, path, _host(mv), mv64)
            mean, invstd, var = _host(st[:3])
            ok_v, worst_v = _rel_close(var, ref["var"], 1e-5)
            ok_i, worst_i = _rel_close(invstd, ref["invstd"], 1e-5)
            per_r = " ".join("r=%g: %.2e" % (r, np.max(np.abs(var[:nr][rs == r] / ref["var"][:nr][rs == r] - 1))) for r in (0, 3, 10, 30, 100))
            report = "%s %s %s C=%d: relative var error %s; near-constant %.2e; constant channel var %.3e invstd %.4g (want %.4g); worst invstd %.2e" % (
                op, path, form, C, per_r, abs(var[nr] / ref["var"][nr] - 1), var[nr + 1], invstd[nr + 1], ref["invstd"][nr + 1], worst_i)
            print(report)
            assert ok_v and ok_i, report
            assert abs(invstd[nr + 1] * np.sqrt(_f32(BN_EPS)) - 1) <= 1e-6
            ok_y, worst_y = _rel_close(_host(Y), ref["y"], 1.0, ybar)
            assert ok_y, (op, path, form, worst_y)
        DX, dg, db = torch.empty(R, C, device="cuda"), torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
        _lib.check(L.ps_op_bn_train_bwd(h, _p(DY), _p(X), _p(G), _p(Bt), _p(st[0]), _p(st[1]), R, C, 0, _p(DX), _p(dg), _p(db)))
        ok, worst = _rel_close(_host(DX), ref["dx"], 1.0, dxbar)
        assert ok, (path, form, worst)


# ---- the leaky-ReLU slope at exactly 0 ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["generic", "slice"])
def test_batchnorm_backward_uses_slope_02_at_zero(path):
    """A constant channel with beta = 0 sits exactly on the kink (xhat = 0, z = 0): the reference's LeakyReluGrad passes 0.2 of the gradient
    there (slope 1 only where z > 0), so dbeta = 0.2 sum dy -- through bn_train_bwd, bwd_ex, bwd_sums and bwd_apply."""
    import torch
    _lib = _env()[0]
    L = _lib.lib()
    R, C = 3001, 32
    rng, x, gamma, beta = _bn_case(R, C, 77)
    x[:, 5] = 7.0
    beta[5] = 0.0
    ref = _bn64(x, gamma, beta, 1)
    assert ref["z"][:, 5].max() == 0.0 and ref["z"][:, 5].min() == 0.0
    dy = _away_from_kink(rng.standard_normal((R, C)).astype(np.float32), ref["z"], 1)
    ref = _bn64(x, gamma, beta, 1, dy)
    assert abs(ref["dbeta"][5] - 0.2 * dy[:, 5].astype(np.float64).sum()) <= 1e-9 * np.abs(dy[:, 5]).sum()
    X, G, Bt, DY = _dev(x), _dev(gamma), _dev(beta), _dev(dy)
    with _contexts()[path]() as ctx:
        h = ctx.handle
        Y, st = torch.empty(R, C, device="cuda"), torch.empty(5, C, device="cuda")
        _lib.check(L.ps_op_bn_train_fwd(h, _p(X), _p(G), _p(Bt), R, C, BN_EPS, 1, _p(Y), _p(st[0]), _p(st[1]), _p(st[2]), _p(st[3])))
        assert _host(st[0])[5] == 7.0 and _host(st[2])[5] == 0.0 and not _host(Y)[:, 5].any()
        gscale = np.abs(dy).sum(0) * 6
        for form in ("bwd", "bwd_ex", "split"):
            DX, dg, db = torch.empty(R, C, device="cuda"), torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
            if form == "bwd":
                _lib.check(L.ps_op_bn_train_bwd(h, _p(DY), _p(X), _p(G), _p(Bt), _p(st[0]), _p(st[1]), R, C, 1, _p(DX), _p(dg), _p(db)))
            elif form == "bwd_ex":
                _lib.check(L.ps_op_bn_train_bwd_ex(h, _p(DY), C, _p(X), _p(G), _p(Bt), _p(st[0]), _p(st[1]), R, C, 1, _p(DX), _p(dg), _p(db)))
            else:
                _lib.check(L.ps_op_bn_train_bwd_sums(h, _p(DY), _p(X), _p(G), _p(Bt), _p(st[0]), _p(st[1]), R, C, 1, _p(dg), _p(db)))
                _lib.check(L.ps_op_bn_train_bwd_apply(h, _p(DY), _p(X), _p(G), _p(Bt), _p(st[0]), _p(st[1]), _p(db), _p(dg), R, R, C, 1, _p(DX)))
            got_db = _host(db)
            assert abs(got_db[5] - ref["dbeta"][5]) <= 1e-5 * gscale[5], (form, path, got_db[5], ref["dbeta"][5], dy[:, 5].sum())
            assert _rel_close(got_db, ref["dbeta"], 1e-5, gscale)[0] and _rel_close(_host(dg), ref["dgamma"], 1e-5, gscale)[0], form
            assert _rel_close(_host(DX), ref["dx"], 2e-5, np.abs(ref["dx"]).max(0))[0], form


def _conv_bn64(x, w, b, gamma, beta, leaky, dz):
    import torch
    xd, wd, bd = (torch.from_numpy(a.astype(np.float64)).requires_grad_(True) for a in (x, w, b))
    gd, btd = (torch.from_numpy(a.astype(np.float64)).requires_grad_(True) for a in (gamma, beta))
    y = xd @ wd + bd
    mean, var = y.mean(0), y.var(0, unbiased=False)
    z = (y - mean) / torch.sqrt(var + _f32(BN_EPS)) * gd + btd
    out = torch.nn.functional.leaky_relu(z, 0.2) if leaky else z
    res = {"z": z.detach().numpy(), "out": out.detach().numpy(), "mean": mean.detach().numpy(), "var": var.detach().numpy(), "ysum": y.detach().numpy().sum(0)}
    if dz is not None:
        out.backward(torch.from_numpy(dz.astype(np.float64)))
        res.update(dx=xd.grad.numpy(), dw=wd.grad.numpy(), db=bd.grad.numpy(), dgamma=gd.grad.numpy(), dbeta=btd.grad.numpy())
    return res


@pytest.mark.parametrize("C", [8, 16, 32, 64])
def test_conv_bn_train_backward_against_float64_autograd(C):
    """conv(C -> C) + BatchNorm + LeakyReLU through ps_op_conv_bn_train_sums / _apply / _bwd_sums / _bwd_apply (and _bwd_sums2 / _apply_w)
    against float64 autograd.  Output channel 0 is constant (its weight column 0, beta 0): the slope there is 0.2."""
    import torch
    _lib, L, h = _env()
    R = 3001
    CP = max(C, 16)
    rng = np.random.default_rng(C)
    x = rng.standard_normal((R, C)).astype(np.float32)
    w = (rng.standard_normal((C, C)) / np.sqrt(C)).astype(np.float32)
    w[:, 0] = 0.0
    b = rng.standard_normal(C).astype(np.float32)
    gamma = (rng.random(C) + 0.5).astype(np.float32)
    beta = rng.standard_normal(C).astype(np.float32)
    beta[0] = 0.0
    pre = _conv_bn64(x, w, b, gamma, beta, 1, None)
    dz = _away_from_kink(rng.standard_normal((R, C)).astype(np.float32), pre["z"], 1)
    ref = _conv_bn64(x, w, b, gamma, beta, 1, dz)
    assert ref["var"][0] == 0.0 and not ref["z"][:, 0].any()
    X, W, Bb, G, Bt, DZ = (_dev(a) for a in (x, w, b, gamma, beta, dz))
    sums = torch.empty(3 * CP, dtype=torch.float64, device="cuda")
    _lib.check(L.ps_op_conv_bn_train_sums(h, _p(X), C, _p(W), _p(Bb), R, C, _p(sums)))
    s = _host(sums)
    mean = s[:C] / R
    var = np.maximum(s[CP:CP + C] / R - mean * mean, 0.0)
    assert _rel_close(mean, ref["mean"], 1e-5, np.sqrt(ref["var"]) + np.abs(ref["mean"]))[0]
    assert _rel_close(var, ref["var"], 1e-4, ref["var"] + 1e-7 * np.abs(ref["mean"]) ** 2)[0]
    assert _rel_close(s[2 * CP:2 * CP + C], x.astype(np.float64).sum(0), 1e-6, np.abs(x).sum(0))[0]
    invstd = (1.0 / np.sqrt(ref["var"] + _f32(BN_EPS))).astype(np.float32)
    mean32 = ref["mean"].astype(np.float32)
    scale = (gamma * invstd).astype(np.float32)
    Mn, Is, Sc = _dev(mean32), _dev(invstd), _dev(scale)
    out = torch.empty(R, C, device="cuda")
    _lib.check(L.ps_op_conv_bn_train_apply(h, _p(X), C, _p(W), _p(Bb), R, C, _p(Mn), _p(Sc), _p(Bt), _p(out), C))
    assert _rel_close(_host(out), ref["out"], 1e-4, np.abs(ref["out"]).max(0) + 1e-6)[0]
    bs = torch.empty(3 * CP + 2 * CP * CP, device="cuda")
    _lib.check(L.ps_op_conv_bn_train_bwd_sums(h, _p(X), C, _p(W), _p(Bb), R, C, _p(Mn), _p(Is), _p(Sc), _p(Bt), _p(DZ), C, _p(bs)))
    bsh = _host(bs).astype(np.float64)
    S1, S2 = bsh[:C], bsh[CP:CP + C]
    A = bsh[3 * CP:3 * CP + CP * CP].reshape(CP, CP)[:C, :C]
    Gm = bsh[3 * CP + CP * CP:].reshape(CP, CP)[:C, :C]
    gscale = np.abs(dz).sum(0) * 6
    assert _rel_close(S1, ref["dbeta"], 1e-5, gscale)[0], (S1[0], ref["dbeta"][0])
    assert _rel_close(S2, ref["dgamma"], 1e-5, gscale)[0]
    dw = gamma * invstd * (A - np.outer(s[2 * CP:2 * CP + C], S1) / R - Gm * S2 / R)
    assert _rel_close(dw, ref["dw"], 1e-4, np.abs(ref["dw"]).max() + 0 * dw)[0]
    m1 = np.zeros(CP, np.float32)
    m2 = np.zeros(CP, np.float32)
    m1[:C], m2[:C] = S1 / R, S2 / R
    dx = torch.full((R, C), 5.0, device="cuda")
    M1, M2 = _dev(m1), _dev(m2)
    _lib.check(L.ps_op_conv_bn_train_bwd_apply(h, _p(X), C, _p(W), _p(Bb), R, C, _p(Mn), _p(Is), _p(Sc), _p(Bt), _p(M1), _p(M2), _p(DZ), C, 0,
                                               _p(dx), C))
    assert _rel_close(_host(dx), ref["dx"], 1e-4, np.abs(ref["dx"]).max() + 0 * ref["dx"])[0]
    # the weight gradient out of the apply pass (the form the C++ step uses; C = 8 runs on csrc/convbn_rows.hip)
    s12 = torch.empty(3 * C, device="cuda")
    _lib.check(L.ps_op_conv_bn_train_bwd_sums2(h, _p(X), C, _p(W), _p(Bb), R, C, _p(Mn), _p(Is), _p(Sc), _p(Bt), _p(DZ), C, _p(s12)))
    s12h = _host(s12).astype(np.float64)
    assert _rel_close(s12h[:C], ref["dbeta"], 1e-5, gscale)[0] and _rel_close(s12h[C:2 * C], ref["dgamma"], 1e-5, gscale)[0], (s12h[0], ref["dbeta"][0])
    dw2, db2 = torch.empty(C, C, device="cuda"), torch.empty(C, device="cuda")
    _lib.check(L.ps_op_conv_bn_train_bwd_apply_w(h, _p(X), C, _p(W), _p(Bb), R, C, _p(Mn), _p(Is), _p(Sc), _p(Bt), _p(s12), 1.0 / R, _p(DZ), C, 0, _p(dx),
                                                 C, _p(dw2), _p(db2)))
    assert _rel_close(_host(dx), ref["dx"], 1e-4, np.abs(ref["dx"]).max() + 0 * ref["dx"])[0]
    assert _rel_close(_host(dw2), ref["dw"], 1e-4, np.abs(ref["dw"]).max() + 0 * ref["dw"])[0]


def _off_grid(a, how, fill):
    """A device copy of the [R, C] array `a` (or, a = None, `fill` everywhere) as a view the 16-byte paths cannot take: rows of pitch C + 1
    ("pitch") or a base one float past an aligned address ("offset").  Returns (view, pitch, the elements around it that nothing may write)."""
    import torch
    R, C = fill.shape if a is None else a.shape
    if how == "pitch":
        buf = torch.full((R, C + 1), 7.75, device="cuda")
        view, ld, guard = buf[:, :C], C + 1, buf[:, C]
    else:
        buf = torch.full((1 + R * C,), 7.75, device="cuda")
        view, ld, guard = buf[1:].view(R, C), C, buf[:1]
    view.copy_(_dev(fill if a is None else a))
    assert view.data_ptr() % 16 != 0 or ld % 4 != 0
    return view, ld, guard


@pytest.mark.parametrize("C", [16, 64])
def test_conv_bn_train_rows_off_the_16_byte_grid_against_float64_autograd(C):
    """The second data path of the square kernels (csrc/smallconv_train.hip, a.vec == 0): dz or out / dx rows that are not 16-byte aligned or
    whose pitch is no multiple of 4 travel as 4-byte accesses in the accumulator layout -- loads of dz, direct stores of z and dx, `*dst + acc`
    for accumulate.  _apply, _bwd_sums, _bwd_sums2, _bwd_apply (fresh and accumulated) and _bwd_apply_w against float64 autograd with the bars
    of test_conv_bn_train_backward_against_float64_autograd; R = 37 is three tiles, the last one ragged, and fewer tiles than waves.  The
    floats between and in front of the rows keep their value."""
    import torch
    _lib, L, h = _env()
    R = 37
    CP = max(C, 16)
    rng = np.random.default_rng(100 + C)
    x = rng.standard_normal((R, C)).astype(np.float32)
    w = (rng.standard_normal((C, C)) / np.sqrt(C)).astype(np.float32)
    b = rng.standard_normal(C).astype(np.float32)
    gamma = (rng.random(C) + 0.5).astype(np.float32)
    beta = rng.standard_normal(C).astype(np.float32)
    pre = _conv_bn64(x, w, b, gamma, beta, 1, None)
    dz = _away_from_kink(rng.standard_normal((R, C)).astype(np.float32), pre["z"], 1)
    ref = _conv_bn64(x, w, b, gamma, beta, 1, dz)
    old = rng.standard_normal((R, C)).astype(np.float32)
    invstd = (1.0 / np.sqrt(ref["var"] + _f32(BN_EPS))).astype(np.float32)
    scale = (gamma * invstd).astype(np.float32)
    X, W, Bb, Bt, Mn, Is, Sc = (_dev(a) for a in (x, w, b, beta, ref["mean"].astype(np.float32), invstd, scale))
    gscale = np.abs(dz).sum(0) * 6
    dx_bar = np.abs(ref["dx"]).max() + 0 * ref["dx"]
    dw_bar = np.abs(ref["dw"]).max() + 0 * ref["dw"]
    for how in ("pitch", "offset"):
        DZ, lddz, dz_guard = _off_grid(dz, how, None)
        out, ldo, out_guard = _off_grid(None, how, np.full((R, C), 5.0, np.float32))
        _lib.check(L.ps_op_conv_bn_train_apply(h, _p(X), C, _p(W), _p(Bb), R, C, _p(Mn), _p(Sc), _p(Bt), _p(out), ldo))
        assert _rel_close(_host(out), ref["out"], 1e-4, np.abs(ref["out"]).max(0) + 1e-6)[0], how
        bs = torch.empty(3 * CP + 2 * CP * CP, device="cuda")
        _lib.check(L.ps_op_conv_bn_train_bwd_sums(h, _p(X), C, _p(W), _p(Bb), R, C, _p(Mn), _p(Is), _p(Sc), _p(Bt), _p(DZ), lddz, _p(bs)))
        bsh = _host(bs).astype(np.float64)
        S1, S2 = bsh[:C], bsh[CP:CP + C]
        A = bsh[3 * CP:3 * CP + CP * CP].reshape(CP, CP)[:C, :C]
        Gm = bsh[3 * CP + CP * CP:].reshape(CP, CP)[:C, :C]
        assert _rel_close(S1, ref["dbeta"], 1e-5, gscale)[0] and _rel_close(S2, ref["dgamma"], 1e-5, gscale)[0], how
        dw = gamma * invstd * (A - np.outer(x.astype(np.float64).sum(0), S1) / R - Gm * S2 / R)
        assert _rel_close(dw, ref["dw"], 1e-4, dw_bar)[0], how
        s12 = torch.empty(3 * C, device="cuda")
        _lib.check(L.ps_op_conv_bn_train_bwd_sums2(h, _p(X), C, _p(W), _p(Bb), R, C, _p(Mn), _p(Is), _p(Sc), _p(Bt), _p(DZ), lddz, _p(s12)))
        s12h = _host(s12).astype(np.float64)
        assert _rel_close(s12h[:C], ref["dbeta"], 1e-5, gscale)[0] and _rel_close(s12h[C:2 * C], ref["dgamma"], 1e-5, gscale)[0], how
        m1 = np.zeros(CP, np.float32)
        m2 = np.zeros(CP, np.float32)
        m1[:C], m2[:C] = S1 / R, S2 / R
        M1, M2 = _dev(m1), _dev(m2)
        dw2, db2 = torch.empty(C, C, device="cuda"), torch.empty(C, device="cuda")
        for accumulate in (0, 1):
            want = ref["dx"] + (old.astype(np.float64) if accumulate else 0.0)
            dx, lddx, dx_guard = _off_grid(old, how, None)
            _lib.check(L.ps_op_conv_bn_train_bwd_apply(h, _p(X), C, _p(W), _p(Bb), R, C, _p(Mn), _p(Is), _p(Sc), _p(Bt), _p(M1), _p(M2), _p(DZ), lddz,
                                                       accumulate, _p(dx), lddx))
            assert _rel_close(_host(dx), want, 1e-4, dx_bar)[0], (how, accumulate)
            dxw, lddxw, dxw_guard = _off_grid(old, how, None)
            _lib.check(L.ps_op_conv_bn_train_bwd_apply_w(h, _p(X), C, _p(W), _p(Bb), R, C, _p(Mn), _p(Is), _p(Sc), _p(Bt), _p(s12), 1.0 / R, _p(DZ), lddz,
                                                         accumulate, _p(dxw), lddxw, _p(dw2), _p(db2)))
            assert _rel_close(_host(dxw), want, 1e-4, dx_bar)[0], (how, accumulate)
            assert _rel_close(_host(dw2), ref["dw"], 1e-4, dw_bar)[0], (how, accumulate)
            for guard in (dz_guard, out_guard, dx_guard, dxw_guard):
                assert float(np.abs(_host(guard) - 7.75).max()) == 0.0, (how, accumulate)


def test_conv_bn_train_refuses_what_it_is_not_compiled_for():
    """_supported(C) is false outside {8, 16, 32, 64}; for such a C, and for rows that are not 16-byte aligned, every entry returns an
    error with ps_last_error set and writes nothing."""
    import torch
    _lib, L, h = _env()
    assert [C for C in range(0, 257) if L.ps_op_conv_bn_train_supported(C)] == [8, 16, 32, 64]
    R = 101
    buf = torch.zeros(R * 132 + 64, device="cuda")
    par = torch.ones(128 * 128, device="cuda")
    sentinel = torch.full((3 * 64 + 2 * 64 * 64,), 3.25, device="cuda")
    dsent = torch.full((3 * 64,), 3.25, dtype=torch.float64, device="cuda")
    cases = [(12, buf, 12), (128, buf, 128), (16, buf[1:], 16), (16, buf, 18), (32, buf[2:], 32)]
    for C, xb, ld in cases:
        msgs = []
        for name, call in [
            ("sums", lambda: L.ps_op_conv_bn_train_sums(h, _p(xb), ld, _p(par), _p(par), R, C, _p(dsent))),
            ("apply", lambda: L.ps_op_conv_bn_train_apply(h, _p(xb), ld, _p(par), _p(par), R, C, _p(par), _p(par), _p(par), _p(sentinel), C)),
            ("bwd_sums", lambda: L.ps_op_conv_bn_train_bwd_sums(h, _p(xb), ld, _p(par), _p(par), R, C, _p(par), _p(par), _p(par), _p(par), _p(buf), C,
                                                                _p(sentinel))),
            ("bwd_apply", lambda: L.ps_op_conv_bn_train_bwd_apply(h, _p(xb), ld, _p(par), _p(par), R, C, _p(par), _p(par), _p(par), _p(par), _p(par),
                                                                  _p(par), _p(buf), C, 0, _p(sentinel), C)),
        ]:
            rc = call()
            assert rc != 0, (name, C, ld)
            msgs.append(L.ps_last_error().decode())
            assert "ps_op_conv_bn_train_" + name in msgs[-1], msgs[-1]
        torch.cuda.synchronize()
        assert float((sentinel - 3.25).abs().max()) == 0.0 and float((dsent - 3.25).abs().max()) == 0.0, (C, ld)


def test_fused_batchnorm_backwards_use_slope_02_at_zero():
    """The recompute forms of the other BatchNorm layers (csrc/rectconv_train.hip, locse_train.hip): an output channel with a zero weight
    column and beta = 0 is constant at the kink; its dbeta (S1) is 0.2 of the sum of dz."""
    import torch
    _lib, L, h = _env()
    rng = np.random.default_rng(9)
    # rectangular conv + BN, (cin, cout) = (16, 32)
    R, ci, co = 3001, 16, 32
    x = rng.standard_normal((R, ci)).astype(np.float32)
    w = (rng.standard_normal((ci, co)) / 4).astype(np.float32)
    w[:, 3] = 0.0
    b = rng.standard_normal(co).astype(np.float32)
    gamma = (rng.random(co) + 0.5).astype(np.float32)
    beta = rng.standard_normal(co).astype(np.float32)
    beta[3] = 0.0
    pre = _conv_bn64(x, w, b, gamma, beta, 1, None)
    dz = _away_from_kink(rng.standard_normal((R, co)).astype(np.float32), pre["z"], 1)
    ref = _conv_bn64(x, w, b, gamma, beta, 1, dz)
    invstd = (1.0 / np.sqrt(ref["var"] + _f32(BN_EPS))).astype(np.float32)
    s12 = torch.empty(2 * co, device="cuda")
    dev = [_dev(a) for a in (x, w, b, ref["mean"].astype(np.float32), invstd, gamma * invstd, beta, dz)]
    X, W, Bb, Mn, Is, Sc, Bt, DZ = (_p(t) for t in dev)
    _lib.check(L.ps_op_convbn_train_bwd_sums(h, X, ci, W, Bb, R, ci, co, Mn, Is, Sc, Bt, 1, DZ, co, _p(s12)))
    got = _host(s12).astype(np.float64)
    gscale = np.abs(dz).sum(0) * 6
    assert _rel_close(got[:co], ref["dbeta"], 1e-5, gscale)[0], (got[3], ref["dbeta"][3])
    assert _rel_close(got[co:], ref["dgamma"], 1e-5, gscale)[0]
    # LocSE: y = enc10(xyz, idx) . w + b, h = 8; channel 2 constant
    B, N, K, hh = 1, 1500, 16, 8
    xyz = rng.random((B * N, 3)).astype(np.float32)
    idx = rng.integers(0, N, (B, N, K)).astype(np.int32)
    w = rng.standard_normal((10, hh)).astype(np.float32) / 3
    w[:, 2] = 0.0
    b = rng.standard_normal(hh).astype(np.float32)
    gamma = (rng.random(hh) + 0.5).astype(np.float32)
    beta = rng.standard_normal(hh).astype(np.float32)
    beta[2] = 0.0
    sums = torch.empty(2 * hh, dtype=torch.float64, device="cuda")
    XYZ, IDX, W, Bb = _dev(xyz), _dev(idx), _dev(w), _dev(b)
    _lib.check(L.ps_op_locse_train_sums(h, _p(XYZ), _p(IDX), B, N, K, _p(W), _p(Bb), hh, _p(sums)))
    s = _host(sums)
    M = B * N * K
    mean = s[:hh] / M
    var = np.maximum(s[hh:] / M - mean * mean, 0.0)
    assert mean[2] == b[2] and var[2] == 0.0
    inv = (1.0 / np.sqrt(var + _f32(BN_EPS))).astype(np.float32)
    dz = rng.standard_normal((M, hh)).astype(np.float32)
    out = torch.empty(23 * hh + 16, device="cuda")
    dev = [_dev(a) for a in (gamma * inv, beta, mean.astype(np.float32), inv, dz)]
    Sc, Bt, Mn, Is, DZ = (_p(t) for t in dev)
    _lib.check(L.ps_op_locse_train_bwd(h, _p(XYZ), _p(IDX), B, N, K, _p(W), _p(Bb), hh, Sc, Bt, Mn, Is, DZ, hh, _p(out)))
    S1 = _host(out)[:hh]
    want = 0.2 * dz[:, 2].astype(np.float64).sum()
    assert abs(S1[2] - want) <= 1e-5 * np.abs(dz[:, 2]).sum(), (S1[2], want, dz[:, 2].sum())
