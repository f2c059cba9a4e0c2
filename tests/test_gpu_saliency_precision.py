"""The two reduced modes of include/pointseg_saliency_precision.h on the GPU (csrc/conv3d_bf16.hip), on the shapes of test_gpu_saliency.py
-- the smallest that cross every tile, chunk and fetch-form boundary.

Bars.  An op: the project's op bar, 4 x (torch-CPU float32 vs float64 on the SAME operands) + 1e-6 * max|expected|.  "bf16" is held to it
against the float64 convolution of the ROUNDED operands (saliency_precision_ref.conv3d_rounded): the products of bfloat16 values are exact
in fp32, so only the accumulation order separates the kernel from that oracle.  "bf16x3" is held to it against the float64 convolution of
the EXACT operands: the dropped piece products are below 2^-25 of a product, less than one fp32 add's rounding.  The 3x3x3 6 -> 10 case also
has to be MORE than 100 bars away from the exact result in "bf16": a mode that silently ran fp32 would pass everything else.
The network: "bf16x3" the fp32 network's bars (logits 1e-4, probabilities 5e-5, taps 1e-4 * max|tap|); "bf16" within 2 E + 1e-4 of the exact
float64 logits, E = max|forward_rounded - forward| -- a 1e-6 difference in an activation can flip a bfloat16 rounding downstream, so the kernel
may be as far from its rounded model as that model is from exact -- and more than 1e-4 away from the fp32 mode."""
import ctypes
import functools

import numpy as np
import pytest

import saliency_precision_ref as pref
import saliency_ref as ref

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

K3 = (3, 3, 3)


def _sal():
    from point_unet_amd import saliency
    return saliency


# ---- the op cases ---------------------------------------------------------------------------------------------------------------------------------
# (shape, kernel, cin, cout, stride, dilation, B, bias)
CASES = [((5, 7, 9), k, 6, 10, 1, 1, 2, True) for k in (K3, (1, 1, 1), (1, 9, 9), (9, 1, 1), (9, 1, 9), (1, 9, 1), (9, 9, 1), (1, 1, 9))]
CASES += [(shape, K3, 6, 10, 2, 1, 2, True) for shape in ((5, 7, 9), (6, 8, 10))]
CASES += [((5, 7, 9), K3, 6, 10, 1, d, 2, True) for d in (3, 5, 7)]
# 17, 33, 1 (and the 6 above) take the scalar fetch, the multiples of 4 the 16-byte one; C_out around the 32 / 64 column tiles
CASES += [((4, 6, 8), K3, cin, cout, 1, 1, 2, cout != 5) for cin, cout in ((1, 16), (4, 16), (16, 64), (32, 1), (128, 2), (384, 64), (256, 32), (17, 5), (33, 65))]
# 2295 output voxels run the 128-row form (no multiple of 128), 135 the 64-row one
CASES += [(shape, K3, cin, cout, 1, 1, 1, True) for shape, cin, cout in (((9, 15, 17), 4, 16), ((9, 15, 17), 3, 33), ((9, 15, 17), 5, 70), ((3, 5, 9), 8, 256))]
CASES += [((5, 7, 9), K3, 6, 10, 1, 1, 2, False)]
MODE_ON_CASE = ((5, 7, 9), K3, 6, 10, 1, 1, 2, True)
# (up, C1, C2, stride): the last one is a concat on the 16-byte fetch
FUSED = [(1, 16, 48, 1), (2, 40, 0, 1), (4, 7, 0, 1), (2, 5, 30, 1), (3, 6, 0, 2), (2, 8, 24, 1)]


def _case_id(c):
    return "%s-k%s-%dto%d-s%d-d%d-B%d%s" % ("x".join(map(str, c[0])), "".join(map(str, c[1])), c[2], c[3], c[4], c[5], c[6], "" if c[7] else "-nobias")


def _four_refs(x, w, b, stride, dilation):
    """(exact float64, exact float32, rounded float64, rounded float32) as numpy, from CPU float32 tensors."""
    out = [ref.conv3d_same(x.to(dt), w.to(dt), None if b is None else b.to(dt), stride, dilation).numpy() for dt in (torch.float64, torch.float32)]
    out += [pref.conv3d_rounded(x, w, b, stride, dilation, dt).numpy() for dt in (torch.float64, torch.float32)]
    return out


@functools.lru_cache(maxsize=None)
def _op_case(case):
    """The operands and the four CPU results, computed once per case and left unchanged."""
    shape, k, cin, cout, stride, dilation, B, bias = case
    rng = np.random.default_rng(0)
    x = torch.from_numpy(rng.standard_normal((B,) + shape + (cin,)).astype(np.float32))
    w = torch.from_numpy((rng.standard_normal(k + (cin, cout)) * np.sqrt(2.0 / (k[0] * k[1] * k[2] * cin))).astype(np.float32))
    b = torch.from_numpy((rng.standard_normal(cout) * 0.1).astype(np.float32)) if bias else None
    return (x, w, b) + tuple(_four_refs(x, w, b, stride, dilation))


@functools.lru_cache(maxsize=None)
def _fused_case(case):
    up, c1, c2, stride = case
    g = torch.Generator().manual_seed(up * 100 + c1)
    x = torch.randn((2, 3, 4, 5, c1), generator=g)
    x2 = torch.randn((2, 3, 4, 5, c2), generator=g) if c2 else None
    w = torch.randn((3, 3, 3, c1 + c2, 24), generator=g) * 0.1
    b = torch.randn(24, generator=g)
    full = ref.upsample(torch.cat([x, x2], -1) if c2 else x, up).contiguous()  # (copies, no arithmetic: rounding commutes with them)
    return (x, x2, w, b, full) + tuple(_four_refs(full, w, b, stride, 1))


def _bar(got, want64, want32, what):
    """The op bar of test_gpu_saliency.py; returns (error, bar)."""
    err = float(np.abs(got.astype(np.float64) - want64).max())
    cpu = float(np.abs(want32.astype(np.float64) - want64).max())
    bar = 4.0 * cpu + 1e-6 * float(np.abs(want64).max())
    print("%s: kernel %.3e, torch-CPU float32 %.3e, bar %.3e (max |expected| %.2f)" % (what, err, cpu, bar, np.abs(want64).max()))
    assert got.shape == want64.shape
    assert err <= bar, what
    return err, bar


def _run(case, precision):
    x, w, b = _op_case(case)[:3]
    _, _, _, _, stride, dilation, _, _ = case
    return _sal().conv3d(x.cuda(), w.cuda(), None if b is None else b.cuda(), stride, dilation, precision=precision).cpu().numpy()


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_conv3d_bf16_against_the_rounded_operands(case):
    _, _, _, exact64, _, round64, round32 = _op_case(case)
    got = _run(case, "bf16")
    _, bar = _bar(got, round64, round32, "bf16 conv3d " + _case_id(case))
    if case == MODE_ON_CASE:
        off = float(np.abs(got - exact64).max())
        print("bf16 conv3d %s: %.3e from the exact-operand float64 result (%.0f bars)" % (_case_id(case), off, off / bar))
        assert off > 100.0 * bar


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_conv3d_bf16x3_against_the_exact_operands(case):
    _, _, _, exact64, exact32, _, _ = _op_case(case)
    _bar(_run(case, "bf16x3"), exact64, exact32, "bf16x3 conv3d " + _case_id(case))


@pytest.mark.parametrize("precision", ["bf16", "bf16x3"])
@pytest.mark.parametrize("case", FUSED, ids=lambda c: "up%d-%d+%d-s%d" % c)
def test_conv3d_fused_concat_and_upsampling(case, precision):
    sal = _sal()
    up, c1, c2, stride = case
    x, x2, w, b, full, exact64, exact32, round64, round32 = _fused_case(case)
    xd, x2d, wd, bd = x.cuda(), (x2.cuda() if c2 else None), w.cuda(), b.cuda()
    fused = sal.conv3d(xd, wd, bd, stride=stride, x2=x2d, up=up, precision=precision)
    plain = sal.conv3d(full.cuda(), wd, bd, stride=stride, precision=precision)
    assert fused.shape == plain.shape == (2, -(-3 * up // stride), -(-4 * up // stride), -(-5 * up // stride), 24)
    assert torch.equal(fused, plain)  # the same operand values in the same order, whichever fetch form each takes
    want = (round64, round32) if precision == "bf16" else (exact64, exact32)
    _bar(fused.cpu().numpy(), want[0], want[1], "%s conv3d fused up %d, %d + %d channels, stride %d" % ((precision,) + case))


# ---- fp32 is the old entry, byte for byte ------------------------------------------------------------------------------------------------------------

def _ctx():
    from point_unet_amd import runtime
    ctx = runtime.default_context(0)
    ctx.use_torch_stream()
    return ctx


def test_fp32_passes_through_conv3d():
    from point_unet_amd import _lib, runtime
    case = ((4, 6, 8), K3, 16, 64, 1, 1, 2, True)
    x, w, b = (t.cuda() for t in _op_case(case)[:3])
    old = _sal().conv3d(x, w, b)
    new = torch.empty_like(old)
    _lib.check(_lib.lib().ps_conv3d_prec(_ctx().handle, runtime.ptr(x), None, 2, 4, 6, 8, 16, 0, 1, runtime.ptr(w), runtime.ptr(b), 3, 3, 3, 64, 1, 1,
                                         runtime.ptr(new), _lib.PS_PREC_FP32))
    assert torch.equal(new, old)
    assert torch.equal(_sal().conv3d(x, w, b, precision="fp32"), old)


# ---- the network --------------------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _net_case(shape, cin):
    """(params, patch, exact float64 logits, exact float64 taps, rounded-operand float64 logits), computed once per shape and left unchanged."""
    params = _sal().init_params(cin, 2, seed=11)
    x = np.random.default_rng(12).standard_normal((1,) + shape + (cin,)).astype(np.float32)
    taps = {}
    l64 = ref.forward(params, x, torch.float64, taps)
    return params, x, l64, taps, pref.forward_rounded(params, x)


@functools.lru_cache(maxsize=None)
def _net(shape, cin, precision):
    return _sal().SaliencyNet(_net_case(shape, cin)[0], cin, 2, precision=precision)


NET_SHAPES = [((16, 32, 32), 1), ((16, 32, 48), 4)]


def test_fp32_passes_through_the_network():
    from point_unet_amd import _lib, runtime
    params, x, _, _, _ = _net_case((16, 32, 32), 1)
    net = _net((16, 32, 32), 1, "fp32")
    xd = torch.from_numpy(x).cuda()
    old = net.forward_taps(xd)
    logits, probs = torch.empty_like(old["logits"]), torch.empty_like(old["probs"])
    fn = _lib.lib().ps_saliency_forward_prec
    ctx = _ctx()
    need = ctypes.c_int64(0)
    call = lambda scratch: fn(ctx.handle, runtime.ptr(xd), 1, 16, 32, 32, 1, 2, runtime.ptr(net.weights), net.weights.numel(), runtime.ptr(logits),  # noqa: E731
                              runtime.ptr(probs), None, scratch, ctypes.byref(need), _lib.PS_PREC_FP32)
    _lib.check(call(None))
    assert need.value == net.scratch_bytes
    buf = torch.empty(need.value, dtype=torch.uint8, device="cuda")
    _lib.check(call(runtime.ptr(buf)))
    assert torch.equal(logits, old["logits"]) and torch.equal(probs, old["probs"])


@pytest.mark.parametrize("shape, cin", NET_SHAPES)
def test_network_bf16x3_meets_the_fp32_bars(shape, cin):
    params, x, l64, taps, _ = _net_case(shape, cin)
    net = _net(shape, cin, "bf16x3")
    xd = torch.from_numpy(x).cuda()
    out = net.forward_taps(xd)
    logits, probs = out["logits"].cpu().numpy(), out["probs"].cpu().numpy()
    report = []
    for name in ("down4", "c345", "sa", "c12"):
        got, want = out[name].cpu().numpy(), taps[name]
        assert got.shape == want.shape, name
        report.append((name, float(np.abs(got - want).max()), float(np.abs(want).max())))
    lerr = float(np.abs(logits - l64).max())
    perr = float(np.abs(probs - ref.softmax(l64)).max())
    print("bf16x3 network %s x %d: logits %.3e (max |logit| %.2f), probabilities %.3e; taps %s"
          % (shape, cin, lerr, np.abs(l64).max(), perr, ", ".join("%s %.3e of %.2f" % r for r in report)))
    for name, err, mag in report:
        assert err <= 1e-4 * mag, name
    assert lerr <= 1e-4
    assert perr <= 5e-5
    assert np.abs(probs.sum(-1) - 1.0).max() <= 1e-6
    assert torch.equal(net.forward(xd), out["logits"]) and torch.equal(net.probs(xd), out["probs"])  # a second run: the same bytes


@pytest.mark.parametrize("shape, cin", NET_SHAPES)
def test_network_bf16_is_as_close_as_its_rounded_model(shape, cin):
    params, x, l64, _, lround = _net_case(shape, cin)
    net = _net(shape, cin, "bf16")
    xd = torch.from_numpy(x).cuda()
    out = net.forward_taps(xd)
    logits, probs = out["logits"].cpu().numpy(), out["probs"].cpu().numpy()
    fp32 = _net(shape, cin, "fp32").forward(xd).cpu().numpy()
    E = float(np.abs(lround - l64).max())
    err = float(np.abs(logits - l64).max())
    to_model = float(np.abs(logits - lround).max())
    to_fp32 = float(np.abs(logits - fp32).max())
    print("bf16 network %s x %d: E = |forward_rounded - forward| %.3e; kernel - exact float64 %.3e (bar %.3e); kernel - forward_rounded %.3e; "
          "kernel(bf16) - kernel(fp32) %.3e; max |logit| %.2f" % (shape, cin, E, err, 2 * E + 1e-4, to_model, to_fp32, np.abs(l64).max()))
    assert np.isfinite(logits).all() and np.isfinite(probs).all() and all(bool(torch.isfinite(out[k]).all()) for k in ("down4", "c345", "sa", "c12"))
    assert err <= 2.0 * E + 1e-4
    assert to_fp32 > 1e-4
    assert np.abs(probs.sum(-1) - 1.0).max() <= 1e-6
    assert torch.equal(net.forward(xd), out["logits"]) and torch.equal(net.probs(xd), out["probs"])  # a second run: the same bytes


@pytest.mark.parametrize("precision", ["bf16x3", "bf16"])
def test_network_batch_of_two_equals_two_single_runs(precision):
    _, x, _, _, _ = _net_case((16, 32, 32), 1)
    net = _net((16, 32, 32), 1, precision)
    a = torch.from_numpy(x).cuda()
    b = torch.from_numpy(np.random.default_rng(13).standard_normal(x.shape).astype(np.float32) * 2.0 + 0.5).cuda()
    both = net.forward(torch.cat([a, b], 0))
    la, lb = net.forward(a), net.forward(b)
    assert not torch.equal(la, lb)
    assert torch.equal(both[0:1], la) and torch.equal(both[1:2], lb)


def test_trainable_net_exports_at_a_precision():
    sal = _sal()
    params = _net_case((16, 32, 32), 1)[0]
    tnet = sal.TrainableSaliencyNet(params, 1, 2)
    net = tnet.export(precision="bf16")
    assert isinstance(net, sal.SaliencyNet) and net.precision == "bf16" and torch.equal(net.weights, _net((16, 32, 32), 1, "bf16").weights)
    assert set(tnet.export()) == set(params)


# ---- the window average inherits the net's precision ------------------------------------------------------------------------------------------------

def test_saliency_map_with_a_bf16_net():
    sal = _sal()
    patch, steps = (16, 32, 32), (12, 24, 24)
    params = sal.init_params(1, 2, seed=21)
    vol = np.random.default_rng(22).standard_normal((23, 40, 50)).astype(np.float32)
    net = sal.SaliencyNet(params, 1, 2, precision="bf16")
    got = sal.saliency_map(torch.from_numpy(vol).cuda(), net, patch, steps).cpu().numpy()
    assert got.shape == (23, 40, 50, 2) and got.dtype == np.float32
    own, count = ref.overlapping_inference(vol[None], lambda w: net.probs(torch.from_numpy(w).cuda()).cpu().numpy(), patch, steps, 2)
    fp32_net = sal.SaliencyNet(params, 1, 2)
    window = np.zeros((1,) + patch + (1,), np.float32)
    window[0, :, :, :, 0] = vol[:16, :32, :32]
    wd = torch.from_numpy(window).cuda()
    assert not torch.equal(net.probs(wd), fp32_net.probs(wd))  # the map below is the bf16 net's
    e_own = float(np.abs(got - own).max())
    print("saliency_map, bf16 net: %.3e from the restatement on the device's own window probabilities" % e_own)
    assert count.min() == 1 and count.max() == 8
    assert e_own <= 1e-6
    assert np.abs(got.sum(-1) - 1.0).max() <= 1e-6
