"""The kernels of include/pointseg_saliency_attention.h -- the channel attention, the spatial gate and softmax + weighted Dice, forward and
backward -- and the graph that point_unet_amd.saliency.TrainableSaliencyNet composes from them, against float64 torch.autograd on the CPU
through saliency_train_ref.

The bar is test_gpu_saliency.py's rule (`_bar`), per result tensor: the test also measures what the same computation makes of the case in
torch-CPU float32 against float64; the kernel may be 4 x that far off plus 1e-6 * max|expected|.  Both numbers are printed (DESIGN.md 4.11
records them).  Every ReLU of a reference is replaced by the mask of the device's own forward, so both sides differentiate the same
piecewise-linear function and nothing is left out.

Every direct call below gives each result between two guard bands of 4096 sentinel floats and scratch of exactly the reported size between
two more; the bands are checked after the call."""
import ctypes
import functools
import time

import numpy as np
import pytest

import saliency_ref as ref
import saliency_train_ref as tref
from test_gpu_saliency import _bar

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

BAND = 4096 * 4  # bytes: 4096 sentinel floats
F64, F32 = torch.float64, torch.float32


def _sal():
    from point_unet_amd import saliency
    return saliency


def _cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.detach().cpu().numpy()


# ---- banded results and the direct calls -------------------------------------------------------------------------------------------------------

def _banded(shape, bands, dtype=torch.float32):
    """An uninitialised device tensor between two bands of 0xA5 bytes in one allocation."""
    n = int(np.prod(shape, dtype=np.int64)) * torch.empty((), dtype=dtype).element_size()
    buf = torch.full((BAND + n + BAND,), 0xA5, dtype=torch.uint8, device="cuda")
    bands += [buf[:BAND], buf[BAND + n:]]
    return buf[BAND:BAND + n].view(dtype).reshape(shape)


def _check_bands(bands):
    for i, band in enumerate(bands):
        assert band.numel() == BAND and bool((band == 0xA5).all()), "guard band %d was written" % i


def _ctx():
    from point_unet_amd import runtime
    ctx = runtime.default_context(0)
    ctx.use_torch_stream()
    return ctx


def _two_call(bands, call):
    """call(ctx, scratch, byref(need)): the sizing call with a NULL context, then the run on banded scratch of exactly that size."""
    from point_unet_amd import _lib, runtime
    need = ctypes.c_int64(0)
    _lib.check(call(None, None, ctypes.byref(need)))
    scratch = _banded((need.value,), bands, torch.uint8)
    _lib.check(call(_ctx().handle, runtime.ptr(scratch), ctypes.byref(need)))


def _c_ca(x, w1, b1, w2, b2, want_y=True, in_place=False):
    """ps_channel_attention called directly: (y, mean, hidden, scale).  in_place: y is (a copy of) x."""
    from point_unet_amd import _lib, runtime
    p = runtime.ptr
    B, V, C = x.shape
    Ch = w1.shape[1]
    bands = []
    mean, hidden, scale = _banded((B, C), bands), _banded((B, Ch), bands), _banded((B, C), bands)
    if in_place:
        x = y = _banded(x.shape, bands).copy_(x)
    else:
        y = _banded(x.shape, bands) if want_y else None
    fn = _lib.lib().ps_channel_attention
    _two_call(bands, lambda ctx, s, n: fn(ctx, p(x), B, V, C, Ch, p(w1), p(b1), p(w2), p(b2), p(mean), p(hidden), p(scale), p(y), s, n))
    _check_bands(bands)
    return y, mean, hidden, scale


CA_RESULTS = ("dx", "dw1", "db1", "dw2", "db2")


def _c_ca_bwd(x, dy, mean, hidden, scale, w1, w2, want=CA_RESULTS, in_place=False):
    """ps_channel_attention_bwd called directly: a dict of the wanted results.  in_place: dx is (a copy of) dy."""
    from point_unet_amd import _lib, runtime
    p = runtime.ptr
    B, V, C = x.shape
    Ch = w1.shape[1]
    bands = []
    shapes = {"dx": x.shape, "dw1": (C, Ch), "db1": (Ch,), "dw2": (Ch, C), "db2": (C,)}
    out = {k: _banded(shapes[k], bands) if k in want else None for k in CA_RESULTS}
    if in_place:
        dy = out["dx"].copy_(dy)
    fn = _lib.lib().ps_channel_attention_bwd
    _two_call(bands, lambda ctx, s, n: fn(ctx, p(x), p(dy), p(mean), p(hidden), p(scale), p(w1), p(w2), B, V, C, Ch,
                                              *(p(out[k]) for k in CA_RESULTS), s, n))
    _check_bands(bands)
    return {k: v for k, v in out.items() if v is not None}


def _c_gate(a1, a2, a3, f, in_place=False):
    from point_unet_amd import _lib, runtime
    p = runtime.ptr
    B, V, C = f.shape
    bands = []
    sa = _banded((B, V), bands)
    y = _banded(f.shape, bands)
    if in_place:
        f = y.copy_(f)
    _lib.check(_lib.lib().ps_spatial_gate(_ctx().handle, p(a1), p(a2), p(a3), p(f), B, V, C, p(sa), p(y)))
    _check_bands(bands)
    return y, sa


def _c_gate_bwd(dy, f, sa, want=("df", "da"), in_place=False):
    from point_unet_amd import _lib, runtime
    p = runtime.ptr
    B, V, C = f.shape
    bands = []
    df = _banded(f.shape, bands) if "df" in want else None
    da = _banded((B, V), bands) if "da" in want else None
    if in_place:
        dy = df.copy_(dy)
    _lib.check(_lib.lib().ps_spatial_gate_bwd(_ctx().handle, p(dy), p(f), p(sa), B, V, C, p(df), p(da)))
    _check_bands(bands)
    return {k: v for k, v in (("df", df), ("da", da)) if v is not None}


def _c_loss(logits, labels, weight):
    from point_unet_amd import _lib, runtime
    p = runtime.ptr
    B, V, C = logits.shape
    bands = []
    loss, sums = _banded((), bands), _banded((B, C, 3), bands, torch.float64)
    fn = _lib.lib().ps_softmax_dice_loss
    _two_call(bands, lambda ctx, s, n: fn(ctx, p(logits), p(labels), p(weight), B, V, C, p(loss), p(sums), s, n))
    _check_bands(bands)
    return loss, sums


def _c_loss_bwd(logits, labels, weight, sums, dloss=None, in_place=False):
    from point_unet_amd import _lib, runtime
    p = runtime.ptr
    B, V, C = logits.shape
    bands = []
    dlogits = _banded(logits.shape, bands)
    if in_place:
        logits = dlogits.copy_(logits)
    _lib.check(_lib.lib().ps_softmax_dice_loss_bwd(_ctx().handle, p(logits), p(labels), p(weight), p(sums), p(dloss), B, V, C, p(dlogits)))
    _check_bands(bands)
    return dlogits


# ---- channel attention -------------------------------------------------------------------------------------------------------------------------

def ca_inputs(V, C, Ch, B=2):
    """(The seeds: with this offset every case of CA_CASES has hidden units on both sides of the ReLU and no pre-activation of the float64
    reference within 1e-2 of 0; the tests assert the 1e-4 the kernel's float32 hidden needs.)"""
    rng = np.random.default_rng(100000 + 1000 * V + 10 * C + Ch + B)
    x = (rng.standard_normal((B, V, C)) * rng.uniform(0.5, 2.0, C) + rng.standard_normal(C)).astype(np.float32)
    dy = rng.standard_normal((B, V, C)).astype(np.float32)
    w1 = (rng.standard_normal((C, Ch)) * np.sqrt(2.0 / C)).astype(np.float32)
    w2 = (rng.standard_normal((Ch, C)) * np.sqrt(2.0 / Ch)).astype(np.float32)
    b1, b2 = (rng.standard_normal(Ch) * 0.1).astype(np.float32), (rng.standard_normal(C) * 0.1).astype(np.float32)
    return x, dy, w1, b1, w2, b2


def ca_reference(inputs, mask, dt):
    """The forward's four results and the five gradients in `dt`; mask [B, Ch] stands in for the hidden ReLU (None: free).  Also the
    smallest |pre-activation| of the hidden layer."""
    x, dy, w1, b1, w2, b2 = (torch.from_numpy(a).to(dt).requires_grad_() for a in inputs)
    pre = []
    y = tref.channel_attention(x, w1, b1, w2, b2, None if mask is None else torch.from_numpy(mask), pre)
    g = torch.autograd.grad(y, (x, w1, b1, w2, b2), dy.detach())
    mean = x.detach().mean(1)
    hidden = pre[0] * torch.from_numpy(mask).to(dt) if mask is not None else torch.relu(pre[0])
    scale = torch.sigmoid(hidden @ w2.detach() + b2.detach())
    out = dict(y=y, mean=mean, hidden=hidden, scale=scale, dx=g[0], dw1=g[1], db1=g[2], dw2=g[3], db2=g[4])
    return {k: _np(v) for k, v in out.items()}, float(pre[0].abs().min())


# (the last four: 49 and 113 slabs per sample, where reduce_partials.h runs its unrolled loop once and twice)
CA_CASES = [(1, 4, 1, 2), (7, 5, 3, 2), (7, 5, 3, 1), (4097, 8, 2, 2), (9001, 384, 96, 2), (196609, 5, 3, 2), (196609, 8, 2, 2), (458753, 5, 3, 2), (458753, 8, 2, 2)]


@pytest.mark.parametrize("V, C, Ch, B", CA_CASES)
def test_channel_attention_values(V, C, Ch, B):
    inputs = ca_inputs(V, C, Ch, B)
    x, dy, w1, b1, w2, b2 = (_cuda(a) for a in inputs)
    y, mean, hidden, scale = _c_ca(x, w1, b1, w2, b2)
    got = dict(y=y, mean=mean, hidden=hidden, scale=scale, **_c_ca_bwd(x, dy, mean, hidden, scale, w1, w2))
    mask = _np(hidden > 0)  # the knife edge: the mask is the device's, and the seed keeps every pre-activation away from 0
    want64, edge = ca_reference(inputs, mask, F64)
    want32, _ = ca_reference(inputs, mask, F32)
    assert edge >= 1e-4, "a hidden pre-activation of the float64 reference lies within 1e-4 of 0 (%g): choose another seed" % edge
    assert np.array_equal(mask, ca_reference(inputs, None, F64)[0]["hidden"] > 0) and mask.any() and not mask.all()
    for k in want64:
        _bar(_np(got[k]), want64[k], want32[k], "channel attention V=%d C=%d Ch=%d B=%d: %s" % (V, C, Ch, B, k))
    # the Python wrappers give the same bytes
    py = _sal().channel_attention(x, w1, b1, w2, b2)
    assert all(torch.equal(a, b) for a, b in zip(py, (y, mean, hidden, scale)))
    pyb = _sal().channel_attention_backward(dy, x, mean, hidden, scale, w1, w2)
    assert all(torch.equal(pyb[k[1:]], got[k]) for k in CA_RESULTS)


def test_channel_attention_optional_results_in_place_and_determinism():
    from point_unet_amd import _lib
    x, dy, w1, b1, w2, b2 = (_cuda(a) for a in ca_inputs(4500, 12, 3))
    y, mean, hidden, scale = _c_ca(x, w1, b1, w2, b2)
    only = _c_ca(x, w1, b1, w2, b2, want_y=False)  # y NULL: the scale alone
    assert only[0] is None and all(torch.equal(a, b) for a, b in zip(only[1:], (mean, hidden, scale)))
    same = _c_ca(x, w1, b1, w2, b2, in_place=True)  # y is x
    assert all(torch.equal(a, b) for a, b in zip(same, (y, mean, hidden, scale)))
    every = _c_ca_bwd(x, dy, mean, hidden, scale, w1, w2)
    for k in CA_RESULTS:  # each result alone
        alone = _c_ca_bwd(x, dy, mean, hidden, scale, w1, w2, want=(k,))
        assert set(alone) == {k} and torch.equal(alone[k], every[k]), k
    with pytest.raises(_lib.PointSegError, match="every result is NULL"):
        _c_ca_bwd(x, dy, mean, hidden, scale, w1, w2, want=())
    again = _c_ca_bwd(x, dy, mean, hidden, scale, w1, w2, in_place=True)  # dx is dy; and a second run
    assert all(torch.equal(again[k], every[k]) for k in CA_RESULTS)


# ---- spatial gate ------------------------------------------------------------------------------------------------------------------------------

def gate_inputs(V, C, B=2):
    rng = np.random.default_rng(100 * V + C)
    a = [rng.standard_normal((B, V)).astype(np.float32) for _ in range(3)]
    f, dy = (rng.standard_normal((B, V, C)).astype(np.float32) for _ in range(2))
    return a[0], a[1], a[2], f, dy


def gate_reference(inputs, dt):
    a1, a2, a3, f, dy = (torch.from_numpy(a).to(dt).requires_grad_() for a in inputs)
    y = tref.spatial_gate(a1, a2, a3, f)
    g = torch.autograd.grad(y, (a1, a2, a3, f), dy.detach())
    assert torch.equal(g[0], g[1]) and torch.equal(g[0], g[2])
    return {k: _np(v) for k, v in dict(y=y, sa=torch.sigmoid((a1 + a2) + a3), da=g[0], df=g[3]).items()}


@pytest.mark.parametrize("V, C", [(1, 1), (5, 3), (300, 64), (4099, 64), (257, 130)])
def test_spatial_gate_values(V, C):
    inputs = gate_inputs(V, C)
    a1, a2, a3, f, dy = (_cuda(a) for a in inputs)
    y, sa = _c_gate(a1, a2, a3, f)
    got = dict(y=y, sa=sa, **_c_gate_bwd(dy, f, sa))
    want64, want32 = gate_reference(inputs, F64), gate_reference(inputs, F32)
    for k in want64:
        _bar(_np(got[k]), want64[k], want32[k], "spatial gate V=%d C=%d: %s" % (V, C, k))
    py = _sal().spatial_gate(a1, a2, a3, f)
    assert torch.equal(py[0], y) and torch.equal(py[1], sa)
    pyb = _sal().spatial_gate_backward(dy, f, sa)
    assert torch.equal(pyb["f"], got["df"]) and torch.equal(pyb["a"], got["da"])


@pytest.mark.parametrize("V, C", [(4099, 64), (257, 130)])
def test_spatial_gate_optional_results_in_place_and_determinism(V, C):
    from point_unet_amd import _lib
    a1, a2, a3, f, dy = (_cuda(a) for a in gate_inputs(V, C))
    y, sa = _c_gate(a1, a2, a3, f)
    same = _c_gate(a1, a2, a3, f, in_place=True)  # y is f
    assert torch.equal(same[0], y) and torch.equal(same[1], sa)
    every = _c_gate_bwd(dy, f, sa)
    for k in ("df", "da"):
        alone = _c_gate_bwd(dy, f, sa, want=(k,))
        assert set(alone) == {k} and torch.equal(alone[k], every[k]), k
    with pytest.raises(_lib.PointSegError, match="every result is NULL"):
        _c_gate_bwd(dy, f, sa, want=())
    again = _c_gate_bwd(dy, f, sa, in_place=True)  # df is dy; and a second run
    assert torch.equal(again["df"], every["df"]) and torch.equal(again["da"], every["da"])


# ---- softmax + weighted Dice -------------------------------------------------------------------------------------------------------------------

def loss_inputs(V, C, B=2, kind="plain"):
    rng = np.random.default_rng(100 * V + C)
    logits = (rng.standard_normal((B, V, C)) * 2.0).astype(np.float32)
    labels = rng.integers(0, C, (B, V)).astype(np.int32)
    weight = rng.uniform(0.2, 3.0, (B, V)).astype(np.float32)
    if kind == "no weight":
        weight = None
    elif kind == "absent class":
        labels[labels == C - 1] = 0
    elif kind == "out of range":
        labels[0, V // 2] = C
        labels[B - 1, 0] = -1
    elif kind == "zero weights":
        weight[:] = 0
    elif kind == "saturated":  # the first half of every sample at +-80: p is exactly 0 or 1 there
        half = V // 2
        logits[:, :half] = np.where(rng.integers(0, C, (B, half, 1)) == np.arange(C)[None, None, :], 80.0, -80.0).astype(np.float32)
    return logits, labels, weight


def loss_reference(inputs, dloss, dt):
    logits, labels, weight = inputs
    z = torch.from_numpy(logits).to(dt).requires_grad_()
    loss = tref.softmax_dice_loss(z, torch.from_numpy(labels), None if weight is None else torch.from_numpy(weight).to(dt))
    (g,) = torch.autograd.grad(loss, z, torch.tensor(dloss, dtype=dt))
    return dict(loss=_np(loss), dlogits=_np(g))


def _loss_case(V, C, kind="plain", dloss=0.75):
    inputs = loss_inputs(V, C, kind=kind)
    logits, labels, weight = (_cuda(a) for a in inputs)
    loss, sums = _c_loss(logits, labels, weight)
    dl = torch.tensor(dloss, dtype=torch.float32, device="cuda")
    got = dict(loss=loss, dlogits=_c_loss_bwd(logits, labels, weight, sums, dl))
    want64, want32 = loss_reference(inputs, dloss, F64), loss_reference(inputs, dloss, F32)
    for k in want64:
        _bar(_np(got[k]), want64[k], want32[k], "softmax dice V=%d C=%d %s: %s" % (V, C, kind, k))
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(got["dlogits"]).all()) and bool(torch.isfinite(sums).all())
    # dlogits is logits (in place); dloss NULL is 1; the Python wrappers; a second run
    assert torch.equal(_c_loss_bwd(logits, labels, weight, sums, dl, in_place=True), got["dlogits"])
    one = torch.ones((), device="cuda")
    assert torch.equal(_c_loss_bwd(logits, labels, weight, sums, None), _c_loss_bwd(logits, labels, weight, sums, one))
    py = _sal().softmax_dice_loss(logits, labels, weight)
    assert py[0].dim() == 0 and py[0].is_cuda and torch.equal(py[0], loss) and torch.equal(py[1], sums)
    assert torch.equal(_sal().softmax_dice_loss_backward(logits, labels, weight, sums, dl), got["dlogits"])
    return inputs, got


# (the last four: 49 and 113 slabs per sample)
@pytest.mark.parametrize("V, C", [(1, 2), (5, 2), (4097, 2), (9001, 4), (300, 16), (196609, 2), (196609, 4), (458753, 2), (458753, 4)])
def test_softmax_dice_loss_values(V, C):
    _loss_case(V, C)


@pytest.mark.parametrize("kind", ["no weight", "absent class", "out of range"])
def test_softmax_dice_loss_cases(kind):
    _loss_case(4500, 3, kind)
    _loss_case(301, 2, kind)


def test_softmax_dice_loss_all_weights_zero():
    for V, C in ((4500, 3), (301, 2)):
        _, got = _loss_case(V, C, "zero weights")
        assert float(got["loss"]) == 1.0 and not bool(got["dlogits"].any())


def test_softmax_dice_loss_saturated_logits():
    for V, C in ((4500, 3), (301, 2), (64, 4)):
        _, got = _loss_case(V, C, "saturated")
        assert not bool(got["dlogits"][:, :V // 2].any())  # p exactly 0 or 1: exactly no gradient
        assert bool(got["dlogits"][:, V // 2:].any())


# ---- the autograd Functions ----------------------------------------------------------------------------------------------------------------------

def test_autograd_functions_hand_the_kernels_gradients_on():
    sal = _sal()
    x, dy, w1, b1, w2, b2 = (_cuda(a) for a in ca_inputs(300, 8, 2))
    leaves = [t.clone().requires_grad_() for t in (x, w1, b1, w2, b2)]
    y = sal.differentiable_channel_attention(*leaves)
    y.backward(dy)
    _, mean, hidden, scale = sal.channel_attention(x, w1, b1, w2, b2)
    want = sal.channel_attention_backward(dy, x, mean, hidden, scale, w1, w2)
    assert all(torch.equal(t.grad, want[k]) for t, k in zip(leaves, ("x", "w1", "b1", "w2", "b2")))
    a1, a2, a3, f, dy = (_cuda(a) for a in gate_inputs(300, 8))
    leaves = [t.clone().requires_grad_() for t in (a1[..., None], a2, a3, f)]  # ([B, V, 1] and [B, V]: the gradient takes the input's shape)
    sal.differentiable_spatial_gate(*leaves).backward(dy)
    want = sal.spatial_gate_backward(dy, f, sal.spatial_gate(a1, a2, a3, f)[1])
    assert leaves[0].grad.shape == (2, 300, 1) and all(torch.equal(t.grad.reshape(2, 300), want["a"]) for t in leaves[:3])
    assert torch.equal(leaves[3].grad, want["f"])
    logits, labels, weight = (_cuda(a) for a in loss_inputs(300, 2))
    z = logits.clone().requires_grad_()
    loss = sal.differentiable_softmax_dice_loss(z, labels, weight)
    assert loss.dim() == 0 and loss.is_cuda
    (loss * 0.75).backward()  # the upstream gradient reaches the kernel as a device pointer
    _, sums = sal.softmax_dice_loss(logits, labels, weight)
    assert torch.equal(z.grad, sal.softmax_dice_loss_backward(logits, labels, weight, sums, torch.tensor(0.75, device="cuda")))


# ---- the whole graph ---------------------------------------------------------------------------------------------------------------------------

def graph_inputs(shape, seed=0):
    """(params, x, labels, weight) for a patch [B, D, H, W, 1] and two classes: init_params (gammas from [0.5, 1.5]), random labels, random
    positive weights."""
    rng = np.random.default_rng(seed)
    params = _sal().init_params(1, 2, seed=seed)
    x = rng.standard_normal(shape + (1,)).astype(np.float32)
    labels = rng.integers(0, 2, shape).astype(np.int32)
    weight = rng.uniform(0.2, 3.0, shape).astype(np.float32)
    return params, x, labels, weight


def reference_graph(inputs, masks, dt):
    """(loss, logits, gradients by name) of saliency_train_ref in `dt`, on the CPU."""
    params, x, labels, weight = inputs
    P = tref.leaves(params, dt)
    logits = tref.graph(P, torch.from_numpy(x).to(dt), masks)
    loss = tref.softmax_dice_loss(logits, torch.from_numpy(labels), torch.from_numpy(weight).to(dt))
    grads = torch.autograd.grad(loss, list(P.values()))
    return float(loss.detach()), _np(logits), {k: _np(g) for k, g in zip(P, grads)}


def _device_graph(inputs):
    params, x, labels, weight = inputs
    net = _sal().TrainableSaliencyNet(params, 1, 2)
    masks = {}
    logits = net.logits(_cuda(x), masks)
    loss = _sal().differentiable_softmax_dice_loss(logits, _cuda(labels), _cuda(weight))
    loss.backward()
    return net, loss.detach(), logits.detach(), {n: p.grad for n, p in net.named_parameters()}, masks


@functools.lru_cache(maxsize=None)
def _graph_case():
    """The device run at [2, 32, 16, 16, 1] (two slabs at full resolution, V = 2 at the bottom level) and its two CPU references, once per
    session."""
    inputs = graph_inputs((2, 32, 16, 16))
    dev = _device_graph(inputs)
    t0 = time.time()
    want64, want32 = reference_graph(inputs, dev[4], F64), reference_graph(inputs, dev[4], F32)
    print("whole graph: the two CPU references took %.1f s" % (time.time() - t0))
    return inputs, dev, want64, want32


def test_graph_gradients_of_every_parameter():
    inputs, (net, loss, logits, grads, masks), want64, want32 = _graph_case()
    names = list(_sal().param_shapes(1, 2))
    assert list(grads) == names and all(g is not None for g in grads.values())  # none missing
    assert len(masks) == sum(1 for _, _, _, norm in _sal().layer_table(1, 2) if norm) + 1
    _bar(_np(loss), np.asarray(want64[0]), np.asarray(want32[0], np.float32), "whole graph: loss")
    for n in names:
        assert tuple(grads[n].shape) == tuple(want64[2][n].shape), n
        _bar(_np(grads[n]), want64[2][n], want32[2][n], "whole graph: d %s" % n)


def test_graph_forward_and_export():
    inputs, (net, loss, logits, grads, masks), want64, want32 = _graph_case()
    _bar(_np(logits), want64[1], want32[1], "whole graph: logits")
    inference = _sal().SaliencyNet(net.export(), 1, 2).forward(_cuda(inputs[1]))
    _bar(_np(inference), want64[1], want32[1], "whole graph: SaliencyNet(export()) logits")


def test_graph_is_deterministic():
    inputs, (net, loss, logits, grads, masks), _, _ = _graph_case()
    _, loss2, logits2, grads2, masks2 = _device_graph(inputs)
    assert torch.equal(loss, loss2) and torch.equal(logits, logits2)
    assert all(torch.equal(masks[k], masks2[k]) for k in masks)
    assert all(torch.equal(grads[k], grads2[k]) for k in grads)


def test_graph_one_voxel_at_the_bottom():
    """[1, 16, 16, 16, 1]: the bottom level is one voxel, its instance norm has variance 0 and sends no gradient back -- every gradient is
    finite and those of down4_conv_*'s kernels are exactly 0."""
    _, _, _, grads, _ = _device_graph(graph_inputs((1, 16, 16, 16), seed=1))
    assert all(bool(torch.isfinite(g).all()) for g in grads.values())
    for i in (0, 1):
        assert not bool(grads[ref.SCOPE + "down4_conv_%d/kernel" % i].any())
    assert bool(grads[ref.SCOPE + "down3_conv_1/kernel"].any()) and bool(grads[ref.SCOPE + "final/kernel"].any())


# ---- learning ------------------------------------------------------------------------------------------------------------------------------------

LEARN_SEED = 2


def reference_losses(inputs, steps=3, lr=0.01):
    """The losses before each of `steps` reference_optimizer steps and after the last, on the CPU in float64 with free ReLUs."""
    params, x, labels, weight = inputs
    net = torch.nn.Module()
    for k, v in params.items():
        net.register_parameter(k, torch.nn.Parameter(torch.from_numpy(v).to(F64)))
    opt = _sal().reference_optimizer(net, lr)
    xt, lt, wt = torch.from_numpy(x).to(F64), torch.from_numpy(labels), torch.from_numpy(weight).to(F64)
    out = []
    for step in range(steps + 1):
        loss = tref.softmax_dice_loss(tref.graph(dict(net.named_parameters()), xt), lt, wt)
        out.append(float(loss.detach()))
        if step < steps:
            opt.zero_grad()
            loss.backward()
            opt.step()
    return out


def _learn(inputs, steps=3):
    params, x, labels, weight = inputs
    net = _sal().TrainableSaliencyNet(params, 1, 2)
    opt = _sal().reference_optimizer(net, lr=0.01)
    xd, ld, wd = _cuda(x), _cuda(labels), _cuda(weight)
    losses = []
    for _ in range(steps):
        opt.zero_grad()
        loss = net.loss(xd, ld, wd)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    with torch.no_grad():
        losses.append(float(net.loss(xd, ld, wd)))
    return losses, {n: p.detach().clone() for n, p in net.named_parameters()}


def test_three_optimizer_steps_learn():
    """One fixed [1, 16, 16, 16, 1] patch, three reference_optimizer steps at lr = 0.01.  LEARN_SEED is a seed for which the float64 CPU
    reference (free ReLUs) lowers the loss over the three steps; that is confirmed first, then asked of the device."""
    inputs = graph_inputs((1, 16, 16, 16), seed=LEARN_SEED)
    t0 = time.time()
    cpu = reference_losses(inputs)
    print("learning: CPU float64 losses %s (%.1f s)" % (cpu, time.time() - t0))
    assert cpu[3] < cpu[0], "the reference does not learn on this seed: choose another"
    losses, params = _learn(inputs)
    print("learning: device losses %s" % (losses,))
    assert losses[3] < losses[0]
    losses2, params2 = _learn(inputs)
    assert losses2 == losses and all(torch.equal(params[n], params2[n]) for n in params)
