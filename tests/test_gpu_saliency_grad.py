"""The kernels of include/pointseg_saliency_train.h -- the convolution's data, weight and bias gradient and the gradients of instance
norm + ReLU -- against float64 torch.autograd on the CPU through saliency_ref's conv3d_same, upsample, torch.cat and instance_norm_relu,
each fed a random dy from a fixed seed.

The bar is test_gpu_saliency.py's rule, per gradient tensor: the test also measures what the same autograd makes of the case in
torch-CPU float32 against float64; the kernel may be 4 x that far off (another summation order of the same fp32 roundings) plus
1e-6 * max|expected|.  Both numbers are printed (DESIGN.md 4.10 records them)."""
import ctypes
import functools

import numpy as np
import pytest

import saliency_ref as ref
from test_gpu_saliency import _bar

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

K333 = (3, 3, 3)


def _sal():
    from point_unet_amd import saliency
    return saliency


def _cuda(a):
    return None if a is None else torch.from_numpy(a).cuda()


def _out_shape(shape, up, stride):
    return tuple(-(-n * up // stride) for n in shape)


# ---- the convolution ---------------------------------------------------------------------------------------------------------------------------

def _conv_inputs(shape, k, c1, cout, stride=1, dilation=1, B=2, bias=True, seed=0, c2=0, up=1):
    rng = np.random.default_rng(seed)
    cin = c1 + c2
    x = rng.standard_normal((B,) + shape + (c1,)).astype(np.float32)
    x2 = rng.standard_normal((B,) + shape + (c2,)).astype(np.float32) if c2 else None
    w = (rng.standard_normal(k + (cin, cout)) * np.sqrt(2.0 / (k[0] * k[1] * k[2] * cin))).astype(np.float32)
    b = (rng.standard_normal(cout) * 0.1).astype(np.float32) if bias else None
    dy = rng.standard_normal((B,) + _out_shape(shape, up, stride) + (cout,)).astype(np.float32)
    return x, x2, w, b, dy


def _conv_autograd(x, x2, w, b, dy, stride, dilation, up, dt):
    leaf = lambda a: None if a is None else torch.from_numpy(a).to(dt).requires_grad_()
    leaves = {"x": leaf(x), "x2": leaf(x2), "w": leaf(w), "bias": leaf(b)}
    inp = leaves["x"] if x2 is None else torch.cat([leaves["x"], leaves["x2"]], -1)
    y = ref.conv3d_same(ref.upsample(inp, up) if up > 1 else inp, leaves["w"], leaves["bias"], stride, dilation)
    names = [n for n in leaves if leaves[n] is not None]
    grads = torch.autograd.grad(y, [leaves[n] for n in names], torch.from_numpy(dy).to(dt))
    return {n: g.numpy() for n, g in zip(names, grads)}


def _conv_case(shape, k, c1, cout, stride=1, dilation=1, B=2, bias=True, seed=0, c2=0, up=1):
    """Runs the case on the device and checks every gradient; returns (inputs, device gradients as numpy)."""
    x, x2, w, b, dy = inputs = _conv_inputs(shape, k, c1, cout, stride, dilation, B, bias, seed, c2, up)
    want64, want32 = (_conv_autograd(x, x2, w, b, dy, stride, dilation, up, dt) for dt in (torch.float64, torch.float32))
    got = _sal().conv3d_backward(_cuda(dy), _cuda(x), _cuda(w), stride, dilation, _cuda(x2), up, need=tuple(want64))
    assert set(got) == set(want64)
    got = {n: g.cpu().numpy() for n, g in got.items()}
    what = "conv3d gradient %s k=%s %d+%d->%d stride %d dilation %d up %d" % (shape, k, c1, c2, cout, stride, dilation, up)
    for n in want64:
        _bar(got[n], want64[n], want32[n], "%s: d%s" % (what, n))
    return inputs, got


@pytest.mark.parametrize("k", [(3, 3, 3), (1, 1, 1), (1, 9, 9), (9, 1, 1), (9, 1, 9), (1, 9, 1), (9, 9, 1), (1, 1, 9)])
def test_conv3d_gradient_kernel_extents(k):
    _conv_case((5, 7, 9), k, 6, 10)


@pytest.mark.parametrize("shape", [(5, 7, 9), (6, 8, 10)])
def test_conv3d_gradient_stride_2_both_padding_parities(shape):
    _conv_case(shape, K333, 6, 10, stride=2)


@pytest.mark.parametrize("dilation", [3, 5, 7])
def test_conv3d_gradient_dilation(dilation):
    _, got = _conv_case((5, 7, 9), K333, 6, 10, dilation=dilation)
    if dilation == 7:  # the outer taps of the D (5) and H (7) axes never reach the input: their dw is exactly 0 (W = 9 is reached: 0 + 7 < 9)
        dw = got["w"]
        assert not dw[[0, 2]].any() and not dw[:, [0, 2]].any() and dw[1, 1].any()


@pytest.mark.parametrize("cin, cout", [(1, 16), (4, 16), (16, 64), (32, 1), (128, 2), (384, 64), (256, 32), (17, 5), (33, 65)])
def test_conv3d_gradient_channel_tails(cin, cout):
    _conv_case((4, 6, 8), K333, cin, cout, bias=cout != 5)


@pytest.mark.parametrize("shape, cin, cout", [((9, 15, 17), 4, 16), ((9, 15, 17), 3, 33), ((9, 15, 17), 5, 70), ((3, 5, 9), 8, 256)])
def test_conv3d_gradient_reduction_tails(shape, cin, cout):
    """2295 voxels: no multiple of the 128-row tile of the data gradient nor of the 32-voxel chunk of the weight gradient; 135: one ragged
    64-row tile; one, three and five column tiles."""
    _conv_case(shape, K333, cin, cout, B=1)


def test_conv3d_gradient_three_slabs_ragged():
    """The weight gradient sums slabs of 4096 output voxels per sample: 21 x 20 x 20 = 8400 voxels are two full slabs and one of 208
    voxels, which is six chunks of 32 and a ragged one of 16."""
    _conv_case((21, 20, 20), K333, 3, 5, B=1)


def test_conv3d_gradient_114_partials():
    """29 x 90 x 89 = 232 290 output voxels are 57 slabs, the last of 2914 voxels; two samples make 114 partials per weight, which
    reduce_partials2_kernel<float, double> adds with its unrolled loop run once by some groups and twice by others (three slabs: never)."""
    _conv_case((29, 90, 89), K333, 3, 5)


def test_conv3d_gradient_113_slabs_of_one_sample():
    """77 x 77 x 78 = 462 462 voxels: 113 slabs of one sample, the last of 3710 voxels; the smallest kernel."""
    _conv_case((77, 77, 78), (1, 1, 1), 3, 5, B=1)


@pytest.mark.parametrize("up, c1, c2, stride", [(1, 16, 48, 1), (2, 40, 0, 1), (4, 7, 0, 1), (2, 5, 30, 1), (3, 6, 0, 2)])
def test_conv3d_gradient_fused_concat_and_upsampling(up, c1, c2, stride):
    (x, x2, w, b, dy), got = _conv_case((3, 4, 5), K333, c1, 24, stride=stride, seed=up * 100 + c1, c2=c2, up=up)
    assert got["x"].shape == x.shape and (c2 == 0 or got["x2"].shape == x2.shape)
    # the weight and bias gradient of the same call on the materialised input: the same products in the same order
    xd = _cuda(x) if x2 is None else torch.cat([_cuda(x), _cuda(x2)], -1)
    full = ref.upsample(xd, up).contiguous()  # (copies, no arithmetic)
    plain = _sal().conv3d_backward(_cuda(dy), full, _cuda(w), stride, 1, need=("w", "bias"))
    assert np.array_equal(plain["w"].cpu().numpy(), got["w"]) and np.array_equal(plain["bias"].cpu().numpy(), got["bias"])


def test_conv3d_gradient_optional_outputs():
    """Each legal combination of NULL results gives the remaining ones byte-equal to the all-results call."""
    sal = _sal()
    x, x2, w, b, dy = (_cuda(a) for a in _conv_inputs((4, 6, 8), K333, 17, 33, c2=20, seed=3))
    every = sal.conv3d_backward(dy, x, w, x2=x2)
    assert set(every) == {"x", "x2", "w", "bias"}
    for need in (("x",), ("x2",), ("x", "x2"), ("w",), ("bias",), ("w", "bias"), ("x2", "bias")):
        part = sal.conv3d_backward(dy, x, w, x2=x2, need=need)
        assert set(part) == set(need)
        for n in need:
            assert torch.equal(part[n], every[n]), (need, n)
    # up-sampled: the data gradient goes through scratch
    x, x2, w, b, dy = (_cuda(a) for a in _conv_inputs((3, 4, 5), K333, 5, 24, c2=30, up=2, seed=4))
    every = sal.conv3d_backward(dy, x, w, x2=x2, up=2, need=("x", "x2"))
    for need in (("x",), ("x2",)):
        assert torch.equal(sal.conv3d_backward(dy, x, w, x2=x2, up=2, need=need)[need[0]], every[need[0]]), need


# ---- instance norm + ReLU ------------------------------------------------------------------------------------------------------------------------

def _c_norm_bwd(x, y, dy, gamma, want=(True, True, True), in_place=False, banded=False):
    """ps_instance_norm_relu_bwd called directly, on scratch of exactly the reported size: (dx, dgamma, dbeta), None where not wanted.
    in_place: dx is (a copy of) dy.  banded: every result and the scratch are followed by a 4096-byte band that must stay untouched."""
    from point_unet_amd import _lib, runtime
    B, V, C = x.shape
    bands = []
    dx = (dy.clone() if in_place else _result(x.shape, bands, banded)) if want[0] else None
    dgamma = _result((C,), bands, banded) if want[1] else None
    dbeta = _result((C,), bands, banded) if want[2] else None
    ctx = runtime.default_context(0)
    ctx.use_torch_stream()
    fn = _lib.lib().ps_instance_norm_relu_bwd
    need = ctypes.c_int64(0)
    _lib.check(fn(None, None, None, None, B, V, C, None, ref.EPS, None, None, None, None, ctypes.byref(need)))
    scratch = _result((need.value,), bands, banded, torch.uint8)
    _lib.check(fn(ctx.handle, runtime.ptr(x), runtime.ptr(y), runtime.ptr(dx if in_place else dy), B, V, C, runtime.ptr(gamma), ref.EPS, runtime.ptr(dx),
                  runtime.ptr(dgamma), runtime.ptr(dbeta), runtime.ptr(scratch), ctypes.byref(need)))
    _check_bands(bands)
    return dx, dgamma, dbeta


BAND = 4096


def _result(shape, bands, banded, dtype=torch.float32):
    """An uninitialised device tensor; banded: followed by BAND bytes of 0xA5 in the same allocation."""
    n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    buf = torch.full((n + (BAND if banded else 0),), 0xA5, dtype=torch.uint8, device="cuda")
    if banded:
        bands.append(buf[n:])
    return buf[:n].view(dtype).reshape(shape)


def _check_bands(bands):
    for i, band in enumerate(bands):
        assert band.numel() == BAND and bool((band == 0xA5).all()), "the band behind result %d was written" % i


def _norm_case(x, gamma, beta, what, seed=0):
    """dy from a fixed seed; y handed to the kernel is the float64 reference's forward cast to float32, so the mask equals autograd's."""
    dy = np.random.default_rng(1000 + seed).standard_normal(x.shape).astype(np.float32)
    want = []
    for dt in (torch.float64, torch.float32):
        leaves = [torch.from_numpy(a).to(dt).requires_grad_() for a in (x, gamma, beta)]
        y = ref.instance_norm_relu(*leaves)
        want.append([g.numpy() for g in torch.autograd.grad(y, leaves, torch.from_numpy(dy).to(dt))])
        if dt == torch.float64:
            y32 = y.detach().to(torch.float32).cuda()
    xd, dyd, gd = _cuda(x), _cuda(dy), _cuda(gamma)
    got = _sal().instance_norm_relu_backward(dyd, xd, y32, gd)
    for i, n in enumerate(("dx", "dgamma", "dbeta")):
        _bar(got[i].cpu().numpy(), want[0][i], want[1][i], "%s: %s" % (what, n))
    # in place (dx is dy) gives the same bytes
    same = _c_norm_bwd(xd, y32, dyd, gd, in_place=True)
    assert all(torch.equal(a, b) for a, b in zip(same, got))
    return got


# (the last four: 49 and 113 slabs per sample, the reducer's unrolled loop once and twice; C = 5 on the float path, C = 8 on the 16-byte one)
@pytest.mark.parametrize("V, C", [(1, 5), (2, 3), (400, 3), (400, 64), (5000, 1), (9001, 70), (4097, 130), (196609, 5), (196609, 8), (458753, 5), (458753, 8)])
def test_instance_norm_relu_gradient_values(V, C):
    rng = np.random.default_rng(V + C)
    x = (rng.standard_normal((2, V, C)) * rng.uniform(0.5, 3.0, C) + rng.standard_normal(C)).astype(np.float32)
    gamma, beta = rng.uniform(0.5, 1.5, C).astype(np.float32), (rng.standard_normal(C) * 0.2).astype(np.float32)
    dx, _, _ = _norm_case(x, gamma, beta, "instance_norm_relu gradient V=%d C=%d" % (V, C), seed=V + C)
    if V == 1:  # variance 0, x - mean 0: exactly 0
        assert not dx.any()


def test_instance_norm_relu_gradient_constant_channel():
    rng = np.random.default_rng(5)
    x = rng.standard_normal((2, 400, 4)).astype(np.float32)
    x[:, :, 2] = 3.7
    x[1, :, 0] = -1e3
    gamma, beta = np.array([1.0, 0.5, 2.0, 1.5], np.float32), np.array([0.1, -0.2, 0.3, 0.0], np.float32)
    dx, dgamma, dbeta = _norm_case(x, gamma, beta, "instance_norm_relu gradient constant channel", seed=5)
    assert bool(torch.isfinite(dx).all()) and bool(torch.isfinite(dgamma).all()) and bool(torch.isfinite(dbeta).all())


def test_instance_norm_relu_gradient_cancellation():
    """Mean 50, deviation 1 over 131 072 voxels: the float64 sums keep the variance."""
    rng = np.random.default_rng(6)
    x = (50.0 + rng.standard_normal((1, 131072, 3))).astype(np.float32)
    _norm_case(x, np.ones(3, np.float32), np.full(3, 1.5, np.float32), "instance_norm_relu gradient cancellation", seed=6)


def test_instance_norm_relu_gradient_optional_outputs():
    rng = np.random.default_rng(8)
    x = _cuda(rng.standard_normal((2, 4500, 7)).astype(np.float32))
    dy = _cuda(rng.standard_normal((2, 4500, 7)).astype(np.float32))
    gamma = _cuda(rng.uniform(0.5, 1.5, 7).astype(np.float32))
    y = _sal().instance_norm_relu(x, gamma, torch.zeros(7, device="cuda"))
    every = _c_norm_bwd(x, y, dy, gamma)
    for want in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1)):
        part = _c_norm_bwd(x, y, dy, gamma, want=want)
        for w, a, b in zip(want, part, every):
            assert (a is None) if not w else torch.equal(a, b), want


# ---- determinism -----------------------------------------------------------------------------------------------------------------------------

def test_gradients_are_deterministic():
    sal = _sal()
    x, _, w, b, dy = (_cuda(a) for a in _conv_inputs((9, 15, 17), K333, 5, 70, seed=9))
    one, two = sal.conv3d_backward(dy, x, w), sal.conv3d_backward(dy, x, w)
    assert set(one) == {"x", "w", "bias"} and all(torch.equal(one[n], two[n]) for n in one)
    gamma, beta = torch.rand(70, device="cuda") + 0.5, torch.zeros(70, device="cuda")
    y = sal.instance_norm_relu(dy, gamma, beta)
    g = torch.randn(dy.shape, generator=torch.Generator().manual_seed(9)).cuda()
    one, two = sal.instance_norm_relu_backward(g, dy, y, gamma), sal.instance_norm_relu_backward(g, dy, y, gamma)
    assert all(torch.equal(a, b) for a, b in zip(one, two))


# ---- scratch and bounds ----------------------------------------------------------------------------------------------------------------------

def _c_conv_bwd(which, x, x2, w, dy, stride, dilation, up):
    """ps_conv3d_bwd_data / ps_conv3d_bwd_weight called directly: scratch of exactly the reported size, a band behind every result."""
    from point_unet_amd import _lib, runtime
    B, Ds, Hs, Ws, C1 = x.shape
    C2 = 0 if x2 is None else x2.shape[4]
    geometry = (B, Ds, Hs, Ws, C1, C2, up, w.shape[0], w.shape[1], w.shape[2], w.shape[4], stride, dilation)
    bands = []
    ctx = runtime.default_context(0)
    ctx.use_torch_stream()
    need = ctypes.c_int64(0)
    if which == "data":
        fn = _lib.lib().ps_conv3d_bwd_data
        outs = [_result(x.shape, bands, True), None if x2 is None else _result(x2.shape, bands, True)]
        head = lambda real: (runtime.ptr(dy), runtime.ptr(w)) if real else (None, None)
    else:
        fn = _lib.lib().ps_conv3d_bwd_weight
        outs = [_result(w.shape, bands, True), _result((w.shape[4],), bands, True)]
        head = lambda real: (runtime.ptr(x), runtime.ptr(x2), runtime.ptr(dy)) if real else (None, None, None)
    _lib.check(fn(None, *head(False), *geometry, None, None, None, ctypes.byref(need)))
    scratch = _result((need.value,), bands, True, torch.uint8)
    _lib.check(fn(ctx.handle, *head(True), *geometry, runtime.ptr(outs[0]), runtime.ptr(outs[1]), runtime.ptr(scratch), ctypes.byref(need)))
    _check_bands(bands)
    return outs


@pytest.mark.parametrize("up, c2, stride", [(1, 0, 1), (2, 9, 1), (1, 9, 2)])
def test_conv3d_gradient_scratch_and_bounds(up, c2, stride):
    sal = _sal()
    x, x2, w, b, dy = (_cuda(a) for a in _conv_inputs((5, 7, 9), K333, 6, 33, stride=stride, c2=c2, up=up, seed=10))
    want = sal.conv3d_backward(dy, x, w, stride, 1, x2, up)
    dx, dx2 = _c_conv_bwd("data", x, x2, w, dy, stride, 1, up)
    dw, db = _c_conv_bwd("weight", x, x2, w, dy, stride, 1, up)
    assert torch.equal(dx, want["x"]) and torch.equal(dw, want["w"]) and torch.equal(db, want["bias"])
    assert dx2 is None or torch.equal(dx2, want["x2"])


def test_instance_norm_relu_gradient_scratch_and_bounds():
    rng = np.random.default_rng(11)
    x = _cuda(rng.standard_normal((2, 4097, 5)).astype(np.float32))
    dy = _cuda(rng.standard_normal((2, 4097, 5)).astype(np.float32))
    gamma = _cuda(rng.uniform(0.5, 1.5, 5).astype(np.float32))
    y = _sal().instance_norm_relu(x, gamma, torch.zeros(5, device="cuda"))
    got = _c_norm_bwd(x, y, dy, gamma, banded=True)
    assert all(torch.equal(a, b) for a, b in zip(got, _sal().instance_norm_relu_backward(dy, x, y, gamma)))


# ---- the two autograd Functions in a chain ---------------------------------------------------------------------------------------------------

CHAIN = (("a", 3, 8, True), ("b", 8, 8, True), ("s", 8, 16, True), ("u", 16, 8, True), ("f", 16, 2, False))  # name, cin, cout, has norm


@functools.lru_cache(maxsize=None)
def _chain_params():
    rng = np.random.default_rng(20)
    p = {}
    for name, cin, cout, norm in CHAIN:
        p[name + "/kernel"] = (rng.standard_normal((3, 3, 3, cin, cout)) * np.sqrt(2.0 / (27 * cin))).astype(np.float32)
        p[name + "/bias"] = (rng.standard_normal(cout) * 0.1).astype(np.float32)
        if norm:
            p[name + "/gamma"] = rng.uniform(0.5, 1.5, cout).astype(np.float32)
            p[name + "/beta"] = (rng.standard_normal(cout) * 0.2).astype(np.float32)
    x = rng.standard_normal((2, 4, 6, 8, 3)).astype(np.float32)
    r = rng.standard_normal((2, 4, 6, 8, 2)).astype(np.float32)
    return p, x, r


def _chain(P, x, conv, norm):
    """One residual block, a stride-2 level, up-sampling back, a concat: conv(x, name, stride, x2, up) and norm(t, name) are the two layers."""
    a = norm(conv(x, "a"), "a")
    block = norm(conv(a, "b"), "b") + a
    s = norm(conv(block, "s", stride=2), "s")
    u = norm(conv(s, "u", up=2), "u")
    return conv(block, "f", x2=u)


def _device_chain():
    sal = _sal()
    p, x, r = _chain_params()
    P = {k: _cuda(v).requires_grad_() for k, v in p.items()}
    xd = _cuda(x).requires_grad_()
    masks = {}

    def conv(t, name, stride=1, x2=None, up=1):
        return sal.differentiable_conv3d(t, P[name + "/kernel"], P[name + "/bias"], stride=stride, x2=x2, up=up)

    def norm(t, name):
        y = sal.differentiable_instance_norm_relu(t, P[name + "/gamma"], P[name + "/beta"])
        masks[name] = (y.detach() > 0).cpu()
        return y

    loss = (_chain(P, xd, conv, norm) * _cuda(r)).sum()
    loss.backward()
    grads = {k: v.grad for k, v in P.items()}
    grads["x"] = xd.grad
    assert all(g is not None for g in grads.values())
    return grads, masks


def _reference_chain(masks, dt):
    """The same chain in saliency_ref terms, every ReLU replaced by the device forward's mask: both sides differentiate the same
    piecewise-linear function, so no element has to be left out."""
    p, x, r = _chain_params()
    P = {k: torch.from_numpy(v).to(dt).requires_grad_() for k, v in p.items()}
    xt = torch.from_numpy(x).to(dt).requires_grad_()

    def conv(t, name, stride=1, x2=None, up=1):
        inp = t if x2 is None else torch.cat([t, x2], -1)
        return ref.conv3d_same(ref.upsample(inp, up) if up > 1 else inp, P[name + "/kernel"], P[name + "/bias"], stride)

    def norm(t, name):
        mean = t.mean((1, 2, 3), keepdim=True)
        var = ((t - mean) ** 2).mean((1, 2, 3), keepdim=True)
        return ((t - mean) * torch.rsqrt(var + ref.EPS) * P[name + "/gamma"] + P[name + "/beta"]) * masks[name].to(dt)

    loss = (_chain(P, xt, conv, norm) * torch.from_numpy(r).to(dt)).sum()
    names = list(P) + ["x"]
    grads = torch.autograd.grad(loss, [P[k] for k in P] + [xt])
    return {k: g.numpy() for k, g in zip(names, grads)}


def test_autograd_chain():
    got, masks = _device_chain()
    want64, want32 = _reference_chain(masks, torch.float64), _reference_chain(masks, torch.float32)
    assert set(got) == set(want64) and len(got) == 5 * 2 + 4 * 2 + 1
    for name in want64:
        _bar(got[name].cpu().numpy(), want64[name], want32[name], "autograd chain: d %s" % name)
    again, masks2 = _device_chain()
    assert all(torch.equal(masks[k], masks2[k]) for k in masks)
    assert all(torch.equal(got[k], again[k]) for k in got)
