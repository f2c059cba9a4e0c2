"""The kernels of include/pointseg_saliency.h against the float64 restatement (saliency_ref.py): the convolution's geometry and channel
tails, the fused concat / up-sampling, instance norm + ReLU, the whole network with four tapped activations, and the window average.

The op bar: the test also measures what torch-CPU float32 makes of the same case against float64; the kernel may be 4 x that far off
(another summation order of the same fp32 roundings) plus 1e-6 * max|expected|.  A single-plane bf16 product sits two orders of magnitude
above it.  Both numbers are printed (DESIGN.md 4.9 records them).  The network bars are the issue's: logits 1e-4, probabilities 5e-5,
taps 1e-4 * max|tap|."""
import functools

import numpy as np
import pytest

import saliency_ref as ref

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def _sal():
    from point_unet_amd import saliency
    return saliency


def _bar(got, want64, want32, what):
    err = float(np.abs(got.astype(np.float64) - want64).max())
    cpu = float(np.abs(want32.astype(np.float64) - want64).max())
    bar = 4.0 * cpu + 1e-6 * float(np.abs(want64).max())
    print("%s: kernel %.3e, torch-CPU float32 %.3e, bar %.3e (max |expected| %.2f)" % (what, err, cpu, bar, np.abs(want64).max()))
    assert got.shape == want64.shape
    assert err <= bar, what


def _conv_case(shape, k, cin, cout, stride=1, dilation=1, B=2, bias=True, seed=0):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B,) + shape + (cin,)).astype(np.float32)
    w = (rng.standard_normal(k + (cin, cout)) * np.sqrt(2.0 / (k[0] * k[1] * k[2] * cin))).astype(np.float32)
    b = (rng.standard_normal(cout) * 0.1).astype(np.float32) if bias else None
    want = [ref.conv3d_same(torch.from_numpy(x).to(dt), torch.from_numpy(w).to(dt), torch.from_numpy(b).to(dt) if bias else None, stride, dilation).numpy()
            for dt in (torch.float64, torch.float32)]
    got = _sal().conv3d(torch.from_numpy(x).cuda(), torch.from_numpy(w).cuda(), torch.from_numpy(b).cuda() if bias else None, stride, dilation)
    _bar(got.cpu().numpy(), want[0], want[1], "conv3d %s k=%s %d->%d stride %d dilation %d" % (shape, k, cin, cout, stride, dilation))


# ---- 1. geometry ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [(3, 3, 3), (1, 1, 1), (1, 9, 9), (9, 1, 1), (9, 1, 9), (1, 9, 1), (9, 9, 1), (1, 1, 9)])
def test_conv3d_kernel_extents(k):
    _conv_case((5, 7, 9), k, 6, 10)


@pytest.mark.parametrize("shape", [(5, 7, 9), (6, 8, 10)])
def test_conv3d_stride_2_both_padding_parities(shape):
    _conv_case(shape, (3, 3, 3), 6, 10, stride=2)


@pytest.mark.parametrize("dilation", [3, 5, 7])
def test_conv3d_dilation(dilation):
    _conv_case((5, 7, 9), (3, 3, 3), 6, 10, dilation=dilation)


# ---- 2. channel tails: C_in around the K chunk of 32, C_out around the 16 / 32 / 64 column tiles ----------------------------------------------------

@pytest.mark.parametrize("cin, cout", [(1, 16), (4, 16), (16, 64), (32, 1), (128, 2), (384, 64), (256, 32), (17, 5), (33, 65)])
def test_conv3d_channel_tails(cin, cout):
    _conv_case((4, 6, 8), (3, 3, 3), cin, cout, bias=cout != 5)


@pytest.mark.parametrize("shape, cin, cout", [((9, 15, 17), 4, 16), ((9, 15, 17), 3, 33), ((9, 15, 17), 5, 70), ((3, 5, 9), 8, 256)])
def test_conv3d_row_tile_tails(shape, cin, cout):
    """2295 output voxels run the 128-row form (no multiple of 128), 135 the 64-row one; one, two and five column tiles."""
    _conv_case(shape, (3, 3, 3), cin, cout, B=1)


# ---- 3. the fused concat and up-sampling equal the same convolution on the materialised input ------------------------------------------------------

@pytest.mark.parametrize("up, c1, c2, stride", [(1, 16, 48, 1), (2, 40, 0, 1), (4, 7, 0, 1), (2, 5, 30, 1), (3, 6, 0, 2)])
def test_conv3d_fused_concat_and_upsampling(up, c1, c2, stride):
    sal = _sal()
    g = torch.Generator().manual_seed(up * 100 + c1)
    x = torch.randn((2, 3, 4, 5, c1), generator=g).cuda()
    x2 = torch.randn((2, 3, 4, 5, c2), generator=g).cuda() if c2 else None
    w = (torch.randn((3, 3, 3, c1 + c2, 24), generator=g) * 0.1).cuda()
    b = torch.randn(24, generator=g).cuda()
    full = ref.upsample(torch.cat([x, x2], -1) if c2 else x, up).contiguous()  # (copies, no arithmetic)
    fused = sal.conv3d(x, w, b, stride=stride, x2=x2, up=up)
    plain = sal.conv3d(full, w, b, stride=stride)
    assert fused.shape == plain.shape == (2, -(-3 * up // stride), -(-4 * up // stride), -(-5 * up // stride), 24)
    assert torch.equal(fused, plain)  # the same products in the same order


# ---- 4.-6. instance norm + ReLU ------------------------------------------------------------------------------------------------------------------

def _norm_case(x, gamma, beta):
    want = [ref.instance_norm_relu(torch.from_numpy(x).to(dt), torch.from_numpy(gamma).to(dt), torch.from_numpy(beta).to(dt)).numpy()
            for dt in (torch.float64, torch.float32)]
    got = _sal().instance_norm_relu(torch.from_numpy(x).cuda(), torch.from_numpy(gamma).cuda(), torch.from_numpy(beta).cuda()).cpu().numpy()
    return got, want


# (the last four: 49 and 113 slabs of 4096 voxels = 49 and 113 partials per value, where reduce_partials.h runs its unrolled loop once and twice;
#  C = 5 on the float path, C = 8 on the 16-byte one)
@pytest.mark.parametrize("V, C", [(1, 5), (400, 3), (400, 64), (5000, 1), (9001, 70), (4097, 130), (196609, 5), (196609, 8), (458753, 5), (458753, 8)])
def test_instance_norm_relu_values(V, C):
    rng = np.random.default_rng(V + C)
    x = (rng.standard_normal((2, V, C)) * rng.uniform(0.5, 3.0, C) + rng.standard_normal(C)).astype(np.float32)
    gamma, beta = rng.uniform(0.5, 1.5, C).astype(np.float32), (rng.standard_normal(C) * 0.2).astype(np.float32)
    got, want = _norm_case(x, gamma, beta)
    if V == 1:  # variance 0: ReLU(beta), exactly
        assert np.array_equal(got, np.broadcast_to(np.maximum(beta, 0), got.shape))
    _bar(got, want[0], want[1], "instance_norm_relu V=%d C=%d" % (V, C))


def test_instance_norm_relu_constant_channel():
    rng = np.random.default_rng(5)
    x = rng.standard_normal((2, 400, 4)).astype(np.float32)
    x[:, :, 2] = 3.7
    x[1, :, 0] = -1e3
    gamma, beta = np.array([1.0, 0.5, 2.0, 1.5], np.float32), np.array([0.1, -0.2, 0.3, 0.0], np.float32)
    got, want = _norm_case(x, gamma, beta)
    assert np.isfinite(got).all()
    assert np.array_equal(got[:, :, 2], np.full((2, 400), np.float32(0.3))) and np.array_equal(got[1, :, 0], np.full(400, np.float32(0.1)))
    _bar(got, want[0], want[1], "instance_norm_relu constant channel")


def test_instance_norm_relu_cancellation():
    """Mean 50, deviation 1 over 131 072 voxels: fp32 E[x^2] - E[x]^2 loses the variance, the float64 partial sums do not."""
    rng = np.random.default_rng(6)
    x = (50.0 + rng.standard_normal((1, 131072, 3))).astype(np.float32)
    gamma, beta = np.ones(3, np.float32), np.full(3, 1.5, np.float32)
    got, want = _norm_case(x, gamma, beta)
    err = float(np.abs(got - want[0]).max())
    print("instance_norm_relu cancellation: kernel %.3e, torch-CPU float32 %.3e" % (err, np.abs(want[1] - want[0]).max()))
    assert err <= 1e-4


def test_instance_norm_relu_determinism():
    sal = _sal()
    rng = np.random.default_rng(7)
    x = torch.from_numpy(rng.standard_normal((2, 20000, 24)).astype(np.float32)).cuda()
    g, b = torch.from_numpy(rng.uniform(0.5, 1.5, 24).astype(np.float32)).cuda(), torch.zeros(24).cuda()
    assert torch.equal(sal.instance_norm_relu(x, g, b), sal.instance_norm_relu(x, g, b))


# ---- 7. the whole network -----------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _net_case(shape, cin):
    """(params, patch, float64 logits, float64 taps, float32 logits), computed once per shape and left unchanged."""
    params = _sal().init_params(cin, 2, seed=11)
    x = np.random.default_rng(12).standard_normal((1,) + shape + (cin,)).astype(np.float32)
    taps = {}
    l64 = ref.forward(params, x, torch.float64, taps)
    l32 = ref.forward(params, x, torch.float32)
    return params, x, l64, taps, l32


@pytest.mark.parametrize("shape, cin", [((16, 32, 32), 1), ((16, 32, 48), 4), ((32, 32, 32), 1)])
def test_network_against_float64(shape, cin):
    params, x, l64, taps, l32 = _net_case(shape, cin)
    net = _sal().SaliencyNet(params, cin, 2)
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
    print("network %s x %d: logits %.3e (torch-CPU float32 %.3e, max |logit| %.2f), probabilities %.3e; taps %s"
          % (shape, cin, lerr, np.abs(l32 - l64).max(), np.abs(l64).max(), perr, ", ".join("%s %.3e of %.2f" % r for r in report)))
    for name, err, mag in report:
        assert err <= 1e-4 * mag, name
    assert lerr <= 1e-4
    assert perr <= 5e-5
    assert np.abs(probs.sum(-1) - 1.0).max() <= 1e-6
    # the entry points that write one result each give the same bytes, and so does a second run
    assert torch.equal(net.forward(xd), out["logits"]) and torch.equal(net.probs(xd), out["probs"])
    assert torch.equal(net.forward(xd), out["logits"])


def test_network_batch_of_two_equals_two_single_runs():
    params, x, _, _, _ = _net_case((16, 32, 32), 1)
    net = _sal().SaliencyNet(params, 1, 2)
    a = torch.from_numpy(x).cuda()
    b = torch.from_numpy(np.random.default_rng(13).standard_normal(x.shape).astype(np.float32) * 2.0 + 0.5).cuda()
    both = net.forward(torch.cat([a, b], 0))
    la, lb = net.forward(a), net.forward(b)
    assert not torch.equal(la, lb)
    assert torch.equal(both[0:1], la) and torch.equal(both[1:2], lb)


@pytest.mark.parametrize("classes", [3, 4])
def test_network_softmax_load_forms(classes):
    """The forward's softmax moves a voxel's logits as floats (3 classes) or in 16-byte accesses (4); two classes, everywhere else in this
    file, take the 8-byte form.  The probabilities against the host's softmax of the device's own logits."""
    from point_unet_amd import _lib
    sal = _sal()
    params = sal.init_params(1, classes, seed=31)
    net = sal.SaliencyNet(params, 1, classes)
    assert _lib.lib().ps_saliency_weight_count(1, classes) == sum(int(np.prod(s)) for s in sal.param_shapes(1, classes).values()) == net.weights.numel()
    x = torch.from_numpy(np.random.default_rng(32).standard_normal((1, 16, 16, 16, 1)).astype(np.float32)).cuda()
    out = net.forward_taps(x)
    logits = out["logits"].cpu().numpy()
    assert logits.shape == (1, 16, 16, 16, classes) and logits.dtype == np.float32
    _bar(out["probs"].cpu().numpy(), ref.softmax(logits.astype(np.float64)), ref.softmax(logits), "softmax of %d classes" % classes)
    assert torch.equal(net.probs(x), out["probs"])


# ---- 8., 9. the window average -----------------------------------------------------------------------------------------------------------------

PATCH, STEPS = (16, 32, 32), (12, 24, 24)


@functools.lru_cache(maxsize=None)
def _map_case():
    sal = _sal()
    params = sal.init_params(1, 2, seed=21)
    vol = np.random.default_rng(22).standard_normal((23, 40, 50)).astype(np.float32)
    net = sal.SaliencyNet(params, 1, 2)
    got = sal.saliency_map(torch.from_numpy(vol).cuda(), net, PATCH, STEPS)
    return params, vol, net, got


def test_saliency_map_values():
    params, vol, net, got_d = _map_case()
    got = got_d.cpu().numpy()
    assert got_d.is_cuda and got.shape == (23, 40, 50, 2) and got.dtype == np.float32
    seen = []

    def device_probs(window):
        seen.append(window.shape)
        return net.probs(torch.from_numpy(window).cuda()).cpu().numpy()

    own, count = ref.overlapping_inference(vol[None], device_probs, PATCH, STEPS, 2)
    assert len(seen) == 8 and count.min() == 1 and count.max() == 8
    for n, c, s, want in zip(vol.shape, PATCH, STEPS, ([0, 12], [0, 24], [0, 24])):
        assert _sal().window_origins(n, c, s) == want == ref.window_origins(n, c, s).tolist()
    e_own = float(np.abs(got - own).max())
    full, _ = ref.overlapping_inference(vol[None], lambda w: ref.softmax(ref.forward(params, w, torch.float64)), PATCH, STEPS, 2)
    e_full = float(np.abs(got - full).max())
    print("saliency_map: %.3e from the restatement on the device's own window probabilities, %.3e from the all-float64 restatement" % (e_own, e_full))
    assert e_own <= 1e-6
    assert e_full <= 5e-5
    assert np.abs(got.sum(-1) - 1.0).max() <= 1e-6


def test_saliency_map_counts_are_exact():
    """A window sum of ones over a count of ones: the accumulate / finish pair alone, every voxel's count exact."""
    from point_unet_amd import _lib, runtime
    D, H, W = 23, 40, 50
    total = torch.zeros((D, H, W, 2), dtype=torch.float32, device="cuda")
    count = torch.zeros((D, H, W), dtype=torch.int32, device="cuda")
    ones = torch.ones(PATCH + (2,), dtype=torch.float32, device="cuda")
    ctx = runtime.default_context(0)
    ctx.use_torch_stream()
    want = np.zeros((D, H, W), np.int32)
    for o0 in (0, 12):
        for o1 in (0, 24):
            for o2 in (0, 24):
                _lib.check(_lib.lib().ps_saliency_accumulate(ctx.handle, runtime.ptr(ones), *PATCH, 2, o0, o1, o2, D, H, W, runtime.ptr(total),
                                                             runtime.ptr(count)))
                want[o0:o0 + 16, o1:o1 + 32, o2:o2 + 32] += 1
    assert np.array_equal(count.cpu().numpy(), want) and np.array_equal(total.cpu().numpy(), np.repeat(want[..., None], 2, -1).astype(np.float32))
    out = torch.empty_like(total)
    _lib.check(_lib.lib().ps_saliency_finish(ctx.handle, runtime.ptr(total), runtime.ptr(count), D, H, W, 2, runtime.ptr(out)))
    assert torch.equal(out, torch.ones_like(out))


def test_saliency_map_volume_smaller_than_the_patch():
    params, vol, net, _ = _map_case()
    small = vol[:10, :20, :30]
    got = _sal().saliency_map(torch.from_numpy(np.ascontiguousarray(small)).cuda(), net, PATCH, STEPS)
    window = np.zeros((1,) + PATCH + (1,), np.float32)
    window[0, :10, :20, :30, 0] = small
    want = net.probs(torch.from_numpy(window).cuda())[0, :10, :20, :30]
    assert got.shape == (10, 20, 30, 2) and torch.equal(got, want)  # one window, count 1: x / 1


def test_saliency_map_feeds_pancreas_mask():
    from point_unet_amd import prepare
    _, _, _, got = _map_case()
    probs = got.permute(2, 1, 0, 3)  # [X, Y, Z, C], still on the device
    mask = prepare.pancreas_mask(probs=probs, threshold=0.5)
    assert mask.is_cuda and mask.dtype == torch.uint8 and tuple(mask.shape) == (50, 40, 23)
    want = (got.cpu().numpy()[..., 1] >= np.float32(0.5)).astype(np.uint8).transpose(2, 1, 0)
    assert np.array_equal(mask.cpu().numpy(), want) and 0 < want.sum() < want.size
