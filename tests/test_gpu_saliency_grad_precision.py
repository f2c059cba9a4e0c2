"""The two reduced modes of include/pointseg_saliency_train_precision.h on the GPU -- the convolution's data gradient on csrc/conv3d_bf16.hip's
kernel with its gather policy, its weight and bias gradient on csrc/conv3d_train_bf16.hip -- on the smallest shapes that cross every tile,
chunk, slab and fetch-form boundary, up to TrainableSaliencyNet(precision=).

Bars.  Every bar is the project's op bar, 4 x |torch-CPU float32 - float64 on the SAME operands| + 1e-6 * max|expected| (_bar).  "bf16x3" is
held to it against the float64 autograd gradient of the EXACT operands: the dropped piece products are below 2^-25 of a product.  "bf16" is
held to it against the float64 gradient of the ROUNDED operands (saliency_grad_precision_ref.py): products of bfloat16 values are exact in
fp32, so only the accumulation order separates the kernel from that oracle.  The 3 x 3 x 3 6 -> 10 case also has to lie MORE than 100 bars
from the exact-operand gradient in "bf16" (dx, dw and dbias): a mode that silently ran fp32 would pass everything else
(test_saliency_grad_precision_rule.py shows the reference alone keeps that distance).  All numbers are printed (DESIGN.md 4.16 records them).

Under "bf16x3" the library runs the split kernels where they were measured faster and the fp32 kernels elsewhere (the weight
gradient from 64 input and 32 output channels on, the data gradient where C_out is a multiple of 4); the bars are the same either way, and
the cases marked "split" below are there so that every test also runs the split kernels."""
import ctypes
import functools

import numpy as np
import pytest

import saliency_grad_precision_ref as gref
import saliency_ref as ref
from test_gpu_saliency_precision import _bar

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

K333 = (3, 3, 3)
MODES = ["bf16x3", "bf16"]
F64, F32 = torch.float64, torch.float32


def _sal():
    from point_unet_amd import saliency
    return saliency


def _cuda(t):
    return None if t is None else t.cuda()


# ---- the op cases ---------------------------------------------------------------------------------------------------------------------------------

def _case(shape, k, c1, cout, stride=1, dilation=1, B=2, seed=0, c2=0, up=1):
    return _case_once(shape, k, c1, cout, stride, dilation, B, seed, c2, up)


@functools.lru_cache(maxsize=None)
def _case_once(shape, k, c1, cout, stride, dilation, B, seed, c2, up):
    """The operands (CPU float32 tensors x, x2, w, dy: test_gpu_saliency_grad.py's recipe) and the CPU gradients {exact or rounded:
    {float64 or float32: {name: numpy}}}, computed once per case and left unchanged."""
    rng = np.random.default_rng(seed)
    cin = c1 + c2
    x = torch.from_numpy(rng.standard_normal((B,) + shape + (c1,)).astype(np.float32))
    x2 = torch.from_numpy(rng.standard_normal((B,) + shape + (c2,)).astype(np.float32)) if c2 else None
    w = torch.from_numpy((rng.standard_normal(k + (cin, cout)) * np.sqrt(2.0 / (k[0] * k[1] * k[2] * cin))).astype(np.float32))
    dy = torch.from_numpy(rng.standard_normal((B,) + tuple(-(-n * up // stride) for n in shape) + (cout,)).astype(np.float32))
    refs = {}
    for rounded in (False, True):
        for dt in (F64, F32):
            dx, dx2 = gref.data_grad_rounded(dy, w, (B,) + shape, stride, dilation, up, c1, dt, rounded)
            g = {"x": dx, "w": gref.weight_grad_rounded(x, x2, up, dy, k, stride, dilation, dt, rounded), "bias": gref.bias_grad_rounded(dy, dt, rounded)}
            if c2:
                g["x2"] = dx2
            refs[rounded, dt] = {n: t.numpy() for n, t in g.items()}
    return (x, x2, w, dy), refs


def _check(mode, shape, k, c1, cout, stride=1, dilation=1, B=2, seed=0, c2=0, up=1):
    """Runs the case on the device in `mode` and holds every gradient to its bar; returns (operands, device gradients, bars by name)."""
    (x, x2, w, dy), refs = _case(shape, k, c1, cout, stride, dilation, B, seed, c2, up)
    got = _sal().conv3d_backward(_cuda(dy), _cuda(x), _cuda(w), stride, dilation, _cuda(x2), up, precision=mode)
    want64, want32 = refs[mode == "bf16", F64], refs[mode == "bf16", F32]
    assert set(got) == set(want64)
    what = "%s conv3d gradient %s k=%s %d+%d->%d stride %d dilation %d up %d" % (mode, shape, k, c1, c2, cout, stride, dilation, up)
    bars = {n: _bar(got[n].cpu().numpy(), want64[n], want32[n], "%s: d%s" % (what, n))[1] for n in want64}
    return (x, x2, w, dy), got, bars


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k", [(1, 1, 1), (3, 3, 3), (1, 9, 9), (9, 1, 9), (9, 9, 1)])
def test_kernel_extents(k, mode):
    """315 voxels = 9 chunks of 32 and 27, and 27 = 3 groups of 8 and 3: the chunk's tail and the tail of a thread's 8 voxels."""
    _, got, bars = _check(mode, (5, 7, 9), k, 6, 10)
    if mode == "bf16" and k == K333:
        exact = _case((5, 7, 9), k, 6, 10)[1][False, F64]
        for n in ("x", "w", "bias"):
            off = float(np.abs(got[n].cpu().numpy() - exact[n]).max())
            print("bf16 d%s: %.3e from the exact-operand float64 gradient (%.0f bars)" % (n, off, off / bars[n]))
            assert off > 100.0 * bars[n], n


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", [(5, 7, 9), (6, 8, 10)])
def test_stride_2_both_padding_parities(shape, mode):
    _check(mode, shape, K333, 6, 10, stride=2)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dilation", [3, 5, 7])
def test_dilation(dilation, mode):
    _, got, _ = _check(mode, (5, 7, 9), K333, 6, 10, dilation=dilation)
    if dilation == 7:  # the outer taps of the D (5) and H (7) axes never reach the input: their dw is exactly 0 in every mode
        dw = got["w"].cpu().numpy()
        assert not dw[[0, 2]].any() and not dw[:, [0, 2]].any() and dw[1, 1].any()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("cin, cout", [(1, 16), (4, 16), (17, 5), (33, 65), (128, 2), (8, 256), (64, 32), (65, 36), (96, 68)])
def test_channel_tails(cin, cout, mode):
    """(4, 16) and (8, 256) take the 16-byte fetch of dy, the others of the first six the 4-byte one; C_out around the 32 / 64 column tiles,
    rows (27 cin + 1) around the 64 / 128 row tiles.  The last three are split in both gradients: one column tile, two, and three."""
    _check(mode, (4, 6, 8), K333, cin, cout)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape, cin, cout", [((16, 16, 16), 4, 4), ((21, 20, 20), 3, 5)])
def test_slabs(shape, cin, cout, mode):
    """4096 voxels: exactly one full slab.  8400: three slabs, the last of 208 voxels = six chunks of 32 and a ragged one of 16."""
    _check(mode, shape, K333, cin, cout, B=1)


@pytest.mark.parametrize("mode, k, cin, cout", [("bf16", K333, 3, 5), ("bf16x3", (1, 1, 1), 64, 32)])
def test_114_partials(mode, k, cin, cout):
    """29 x 90 x 89 = 232 290 output voxels are 57 slabs per sample, the last of 2914 voxels: two samples make 114 partials per weight, where the
    reducer runs its unrolled loop once in some groups and twice in others.  64 -> 32 is the smallest channel pair whose "bf16x3" weight
    gradient runs the split kernel."""
    try:
        _check(mode, (29, 90, 89), k, cin, cout)
    finally:
        _case_once.cache_clear()  # (hundreds of megabytes of operands and references that no other test shares)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("up, c1, c2, stride, cout", [(1, 16, 48, 1, 24), (2, 5, 30, 1, 24), (4, 7, 0, 1, 24), (3, 6, 0, 2, 24), (2, 40, 24, 1, 40)])
def test_fused_concat_and_upsampling(up, c1, c2, stride, cout, mode):
    """(the last case: split in both gradients)"""
    (x, x2, w, dy), got, _ = _check(mode, (3, 4, 5), K333, c1, cout, stride=stride, seed=up * 100 + c1, c2=c2, up=up)
    assert got["x"].shape == x.shape and (c2 == 0 or got["x2"].shape == x2.shape)
    # the weight and bias gradient of the same call on the materialised input: the same operand values in the same order
    full = ref.upsample(x if x2 is None else torch.cat([x, x2], -1), up).contiguous()  # (copies, no arithmetic: rounding commutes with them)
    plain = _sal().conv3d_backward(_cuda(dy), _cuda(full), _cuda(w), stride, 1, need=("w", "bias"), precision=mode)
    assert torch.equal(plain["w"], got["w"]) and torch.equal(plain["bias"], got["bias"])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("c1, c2, cout", [(17, 20, 33), (40, 24, 36)])
def test_optional_results(c1, c2, cout, mode):
    """dx only, dx2 only, dw only, dbias only: each gives the bytes of the full call (a NULL result narrows the column or row range).
    (40 + 24 -> 36: split in both gradients)"""
    sal = _sal()
    x, x2, w, dy = (_cuda(t) for t in _case((4, 6, 8), K333, c1, cout, seed=3, c2=c2)[0])
    every = sal.conv3d_backward(dy, x, w, x2=x2, precision=mode)
    assert set(every) == {"x", "x2", "w", "bias"}
    for need in (("x",), ("x2",), ("w",), ("bias",)):
        part = sal.conv3d_backward(dy, x, w, x2=x2, need=need, precision=mode)
        assert set(part) == set(need) and torch.equal(part[need[0]], every[need[0]]), need
    # up-sampled: the data gradient goes through scratch
    x, x2, w, dy = (_cuda(t) for t in _case((3, 4, 5), K333, c1, cout, seed=4, c2=c2, up=2)[0])
    every = sal.conv3d_backward(dy, x, w, x2=x2, up=2, need=("x", "x2"), precision=mode)
    for need in (("x",), ("x2",)):
        assert torch.equal(sal.conv3d_backward(dy, x, w, x2=x2, up=2, need=need, precision=mode)[need[0]], every[need[0]]), need


# ---- the entries themselves ------------------------------------------------------------------------------------------------------------------------

BAND = 4096


def _result(shape, bands, dtype=torch.float32):
    """An uninitialised device tensor followed by BAND bytes of 0xA5 in the same allocation."""
    n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    buf = torch.full((n + BAND,), 0xA5, dtype=torch.uint8, device="cuda")
    bands.append(buf[n:])
    return buf[:n].view(dtype).reshape(shape)


def _check_bands(bands):
    for i, band in enumerate(bands):
        assert band.numel() == BAND and bool((band == 0xA5).all()), "the band behind result %d was written" % i


def _entry(which, x, x2, w, dy, stride, dilation, up, prec, old=False):
    """ps_conv3d_bwd_data_prec / ps_conv3d_bwd_weight_prec (old: the entries without `precision`) called directly: scratch of exactly the
    reported size, a band behind every result and behind the scratch.  Returns (the two results, the scratch size)."""
    from point_unet_amd import _lib, runtime
    B, Ds, Hs, Ws, C1 = x.shape
    C2 = 0 if x2 is None else x2.shape[4]
    geometry = (B, Ds, Hs, Ws, C1, C2, up, w.shape[0], w.shape[1], w.shape[2], w.shape[4], stride, dilation)
    tail = () if old else (prec,)
    bands = []
    ctx = runtime.default_context(0)
    ctx.use_torch_stream()
    need = ctypes.c_int64(0)
    if which == "data":
        fn = _lib.lib().ps_conv3d_bwd_data if old else _lib.lib().ps_conv3d_bwd_data_prec
        outs = [_result(x.shape, bands), None if x2 is None else _result(x2.shape, bands)]
        head = lambda real: (runtime.ptr(dy), runtime.ptr(w)) if real else (None, None)  # noqa: E731
    else:
        fn = _lib.lib().ps_conv3d_bwd_weight if old else _lib.lib().ps_conv3d_bwd_weight_prec
        outs = [_result(w.shape, bands), _result((w.shape[4],), bands)]
        head = lambda real: (runtime.ptr(x), runtime.ptr(x2), runtime.ptr(dy)) if real else (None, None, None)  # noqa: E731
    _lib.check(fn(None, *head(False), *geometry, None, None, None, ctypes.byref(need), *tail))
    scratch = _result((need.value,), bands, torch.uint8)
    _lib.check(fn(ctx.handle, *head(True), *geometry, runtime.ptr(outs[0]), runtime.ptr(outs[1]), runtime.ptr(scratch), ctypes.byref(need), *tail))
    _check_bands(bands)
    return outs, need.value


# a concat behind up = 2: both scratch parts, ragged tiles everywhere; 6 + 9 -> 33, and 40 + 24 -> 36 (split in both gradients)
FUSED_CASE = ((5, 7, 9), K333, 6, 33, 1, 1, 2, 10, 9, 2)
FUSED_CASES = [FUSED_CASE, ((5, 7, 9), K333, 40, 36, 1, 1, 2, 10, 24, 2)]


def test_fp32_passes_through_the_new_entries():
    from point_unet_amd import _lib
    x, x2, w, dy = (_cuda(t) for t in _case(*FUSED_CASE)[0])
    for which in ("data", "weight"):
        new, n_new = _entry(which, x, x2, w, dy, 1, 1, 2, _lib.PS_PREC_FP32)
        old, n_old = _entry(which, x, x2, w, dy, 1, 1, 2, None, old=True)
        assert n_new == n_old and all(torch.equal(a, b) for a, b in zip(new, old)), which
    want = _sal().conv3d_backward(dy, x, w, x2=x2, up=2)
    again = _sal().conv3d_backward(dy, x, w, x2=x2, up=2, precision="fp32")
    assert all(torch.equal(want[n], again[n]) for n in want)


def test_bad_precision_and_scratch_size():
    from point_unet_amd import _lib
    lib = _lib.lib()
    geometry = (2, 5, 7, 9, 6, 9, 2, 3, 3, 3, 33, 1, 1)
    for fn, head in ((lib.ps_conv3d_bwd_data_prec, (None,) * 3), (lib.ps_conv3d_bwd_weight_prec, (None,) * 4)):
        sizes = []
        for prec in (_lib.PS_PREC_FP32, _lib.PS_PREC_BF16X3, _lib.PS_PREC_BF16):
            need = ctypes.c_int64(-1)
            assert fn(*head, *geometry, None, None, None, ctypes.byref(need), prec) == 0
            sizes.append(need.value)
        assert sizes[0] == sizes[1] == sizes[2] > 0
        for prec in (3, -1):
            need = ctypes.c_int64(-7)
            assert fn(*head, *geometry, None, None, None, ctypes.byref(need), prec) == 1 and need.value == -7  # PS_EINVAL with scratch == NULL
            assert fn(*head, *geometry, None, None, ctypes.c_void_p(4096), ctypes.byref(need), prec) == 1 and b"precision" in lib.ps_last_error()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", FUSED_CASES, ids=["6+9to33", "40+24to36"])
def test_scratch_and_bounds(case, mode):
    from point_unet_amd import _lib
    x, x2, w, dy = (_cuda(t) for t in _case(*case)[0])
    prec = _lib.SALIENCY_PRECISIONS[mode]
    want = _sal().conv3d_backward(dy, x, w, x2=x2, up=2, precision=mode)
    (dx, dx2), _ = _entry("data", x, x2, w, dy, 1, 1, 2, prec)
    (dw, db), _ = _entry("weight", x, x2, w, dy, 1, 1, 2, prec)
    assert torch.equal(dx, want["x"]) and torch.equal(dx2, want["x2"]) and torch.equal(dw, want["w"]) and torch.equal(db, want["bias"])


# ---- determinism ---------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape, cin, cout", [((21, 20, 20), 3, 5), ((9, 15, 17), 64, 36)])
def test_two_runs_give_the_same_bytes(shape, cin, cout, mode):
    """(64 -> 36: split in both gradients)"""
    sal = _sal()
    x, x2, w, dy = (_cuda(t) for t in _case(shape, K333, cin, cout, B=1)[0])
    one, two = sal.conv3d_backward(dy, x, w, precision=mode), sal.conv3d_backward(dy, x, w, precision=mode)
    assert set(one) == {"x", "w", "bias"} and all(torch.equal(one[n], two[n]) for n in one)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("up, c2, stride, cout", [(1, 0, 2, 33), (2, 9, 1, 33), (1, 0, 2, 36), (2, 9, 1, 36)])
def test_data_gradient_of_a_batch_equals_the_single_runs(up, c2, stride, cout, mode):
    """(C_out = 36: the split data gradient)"""
    sal = _sal()
    x, x2, w, dy = (_cuda(t) for t in _case((5, 7, 9), K333, 6, cout, stride, 1, 2, 10, c2, up)[0])
    both = sal.conv3d_backward(dy, x, w, stride, 1, x2, up, need=("x", "x2"), precision=mode)
    for b in (0, 1):
        one = sal.conv3d_backward(dy[b:b + 1], x[b:b + 1], w, stride, 1, None if x2 is None else x2[b:b + 1], up, need=("x", "x2"), precision=mode)
        assert all(torch.equal(both[n][b:b + 1], one[n]) for n in both), b


# ---- autograd ------------------------------------------------------------------------------------------------------------------------------------------

def _device_chain(mode):
    """test_gpu_saliency_grad.py's chain ([2, 4, 6, 8, 3]: a residual block, a stride-2 level, an up-sampled convolution, a concat) with every
    convolution, forward and backward, at `mode`."""
    from test_gpu_saliency_grad import _chain, _chain_params
    sal = _sal()
    p, x, r = _chain_params()
    P = {k: torch.from_numpy(v).cuda().requires_grad_() for k, v in p.items()}
    xd = torch.from_numpy(x).cuda().requires_grad_()
    masks = {}

    def conv(t, name, stride=1, x2=None, up=1):
        return sal.differentiable_conv3d(t, P[name + "/kernel"], P[name + "/bias"], stride=stride, x2=x2, up=up, precision=mode)

    def norm(t, name):
        y = sal.differentiable_instance_norm_relu(t, P[name + "/gamma"], P[name + "/beta"])
        masks[name] = (y.detach() > 0).cpu()
        return y

    loss = (_chain(P, xd, conv, norm) * torch.from_numpy(r).cuda()).sum()
    loss.backward()
    grads = {k: v.grad for k, v in P.items()}
    grads["x"] = xd.grad
    assert all(g is not None for g in grads.values())
    return grads, masks


@pytest.mark.parametrize("mode", MODES)
def test_autograd_chain(mode):
    from test_gpu_saliency_grad import _reference_chain
    got, masks = _device_chain(mode)
    again, masks2 = _device_chain(mode)
    assert all(torch.equal(masks[k], masks2[k]) for k in masks)
    assert all(torch.equal(got[k], again[k]) for k in got)  # two backward() runs: the same bytes
    if mode == "bf16x3":  # the bars of test_gpu_saliency_grad.py's test_autograd_chain
        want64, want32 = _reference_chain(masks, F64), _reference_chain(masks, F32)
        assert set(got) == set(want64) and len(got) == 5 * 2 + 4 * 2 + 1
        for name in want64:
            _bar(got[name].cpu().numpy(), want64[name], want32[name], "bf16x3 autograd chain: d %s" % name)
    else:
        assert all(bool(torch.isfinite(g).all()) for g in got.values())


NET_SHAPE = (1, 32, 16, 16)  # the bottom level holds two voxels
# Which patch.  With two voxels at the bottom level an instance norm there is close to a sign function of the two values' difference, and
# the whole gradient is ill-conditioned in the forward's roundings: with the ReLUs fixed, torch-CPU float32 stands 0.2 % to 9 % (relative
# L2 over all parameters, seeds 0 to 3 of test_gpu_saliency_train.py's graph_inputs) from float64, so the bar -- four times ONE such draw --
# is held by another fp32-level computation only with some luck.  At seed 0 the draw is the small one and the fp32 kernels themselves, the
# code these modes promise the accuracy class of, stand at 2.2 bars (median) and 6.1 (worst); "bf16x3" at 0.76 and 2.3, and one bias
# gradient that is 0 but for rounding has a bar of 1e-19.  What "bf16x3" promises is the class of the fp32 entries, so the
# patch is the first seed at which the fp32 graph -- code this file does not test -- keeps the bars; the test confirms that first, from the
# fp32 run and its own references, and then asks "bf16x3".
NET_SEED = 1


@functools.lru_cache(maxsize=None)
def _net_inputs():
    from test_gpu_saliency_train import graph_inputs
    return graph_inputs(NET_SHAPE, seed=NET_SEED)


def _device_graph(**kw):
    """(loss, gradients by name, masks) of TrainableSaliencyNet(params, 1, 2, **kw) on the fixed patch."""
    params, x, labels, weight = _net_inputs()
    net = _sal().TrainableSaliencyNet(params, 1, 2, **kw)
    masks = {}
    loss = net.loss(torch.from_numpy(x).cuda(), torch.from_numpy(labels).cuda(), torch.from_numpy(weight).cuda(), masks)
    loss.backward()
    return loss.detach(), {n: p.grad for n, p in net.named_parameters()}, masks


def _graph_against_its_references(precision):
    """[(what, device value, float64, float32)] for the loss and every parameter's gradient: saliency_train_ref's graph with its ReLUs
    replaced by this device forward's masks."""
    from test_gpu_saliency_train import reference_graph
    loss, grads, masks = _device_graph(precision=precision)
    want64, want32 = reference_graph(_net_inputs(), masks, F64), reference_graph(_net_inputs(), masks, F32)
    names = list(_sal().param_shapes(1, 2))
    assert list(grads) == names and all(g is not None for g in grads.values())
    rows = [("loss", loss.cpu().numpy(), np.asarray(want64[0]), np.asarray(want32[0], np.float32))]
    return rows + [("d " + n, grads[n].cpu().numpy(), want64[2][n], want32[2][n]) for n in names]


def test_trainable_net_bf16x3_meets_the_fp32_bars():
    worst = 0.0
    for what, got, want64, want32 in _graph_against_its_references("fp32"):
        bar = 4.0 * float(np.abs(want32.astype(np.float64) - want64).max()) + 1e-6 * float(np.abs(want64).max())
        worst = max(worst, float(np.abs(got.astype(np.float64) - want64).max()) / bar)
    print("fp32 whole graph %s seed %d: the worst tensor stands at %.2f of its bar" % (NET_SHAPE, NET_SEED, worst))
    assert worst <= 1.0, "the patch does not qualify: the fp32 graph itself misses the bar here"
    for what, got, want64, want32 in _graph_against_its_references("bf16x3"):
        _bar(got, want64, want32, "bf16x3 whole graph: " + what)


def test_trainable_net_fp32_is_the_default_and_bf16_is_its_own():
    loss0, base, _ = _device_graph()
    loss1, fp32, _ = _device_graph(precision="fp32")
    assert torch.equal(loss0, loss1) and all(torch.equal(base[n], fp32[n]) for n in base)
    loss2, one, _ = _device_graph(precision="bf16")
    loss3, two, _ = _device_graph(precision="bf16")
    assert torch.equal(loss2, loss3) and all(torch.equal(one[n], two[n]) for n in one)  # two runs: the same bytes
    assert all(bool(torch.isfinite(g).all()) for g in one.values()) and bool(torch.isfinite(loss2))
    assert not all(torch.equal(one[n], base[n]) for n in one)
    flat = lambda g: torch.cat([g[n].double().reshape(-1) for n in g])  # noqa: E731
    d = float((flat(one) - flat(base)).norm() / flat(base).norm())
    print("bf16 whole graph %s: loss %.6f (fp32 %.6f); relative L2 distance of the gradient from the fp32 gradient %.3e" % (NET_SHAPE, float(loss2), float(loss0), d))
