"""include/pointseg_saliency_step.h on the device: ps_saliency_sgd_update against the numpy restatement (saliency_step_ref) bit for bit;
ps_saliency_backward against the op-by-op path (TrainableSaliencyNet: loss and logits byte-equal) and against float64 torch.autograd on the
CPU through saliency_train_ref, under test_gpu_saliency.py's bar (4 x the torch-CPU float32 error + 1e-6 * max|expected|, the ReLU masks the
device's own); ps_saliency_train_step against backward + the restated update by hand, with and without a collective callback; the argument
errors; and train_saliency(engine="native").

Every direct call gives its results between guard bands of 4096 sentinel floats and scratch of exactly the reported size between two more."""
import ctypes
import functools
import time

import numpy as np
import pytest

import saliency_step_ref as sref
import saliency_train_ref as tref
from test_gpu_saliency import _bar
from test_gpu_saliency_train import F32, F64, LEARN_SEED, _banded, _check_bands, _ctx, _cuda, _graph_case, _np, graph_inputs

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def _sal():
    from point_unet_amd import saliency
    return saliency


def _ptr(t):
    from point_unet_amd import runtime
    return runtime.ptr(t)


# ---- the update ----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cin, classes", [(1, 2), (4, 4)])
def test_update_equals_the_restatement(cin, classes):
    from point_unet_amd import _lib
    sal = _sal()
    decay = sref.decay_mask(sal.param_shapes(cin, classes))
    n = decay.size
    assert n == _lib.lib().ps_saliency_weight_count(cin, classes)
    rng = np.random.default_rng(11 + cin)
    w, a = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    bands = []
    dw, dg, da = (_banded((n,), bands) for _ in range(3))
    dw.copy_(_cuda(w)), da.copy_(_cuda(a))
    for lr, scale in ((0.01, 1.0), (0.003, 0.5)):
        g = rng.standard_normal(n).astype(np.float32)
        dg.copy_(_cuda(g))
        _lib.check(_lib.lib().ps_saliency_sgd_update(_ctx().handle, _ptr(dw), _ptr(dg), _ptr(da), cin, classes, n, lr, 0.9, 1e-5, scale))
        w, a = sref.sgd_update(w, g, a, decay, lr, 0.9, 1e-5, scale)
        assert torch.equal(dw, _cuda(w)) and torch.equal(da, _cuda(a)) and torch.equal(dg, _cuda(g)), (lr, scale)
    _check_bands(bands)


def test_update_of_unaligned_buffers_and_every_tail():
    """Buffers 4 bytes off a 16-byte boundary take the float-at-a-time form: the same values."""
    from point_unet_amd import _lib
    sal = _sal()
    decay = sref.decay_mask(sal.param_shapes(1, 2))  # (the one-channel layers' vectors: segments and length are no multiples of 4)
    n = decay.size
    assert n % 4
    rng = np.random.default_rng(2)
    w, g, a = (rng.standard_normal(n).astype(np.float32) for _ in range(3))
    want = sref.sgd_update(w, g, a, decay, 0.01)
    for shift in (0, 1):
        bands = []
        bufs = [_banded((n + 4,), bands) for _ in range(3)]
        dw, dg, da = (b[shift:shift + n] for b in bufs)
        for b in bufs:
            b.fill_(7.0)
        dw.copy_(_cuda(w)), dg.copy_(_cuda(g)), da.copy_(_cuda(a))
        _lib.check(_lib.lib().ps_saliency_sgd_update(_ctx().handle, _ptr(dw), _ptr(dg), _ptr(da), 1, 2, n, 0.01, 0.9, 1e-5, 1.0))
        assert torch.equal(dw, _cuda(want[0])) and torch.equal(da, _cuda(want[1])), shift
        for b in bufs:  # the elements around the shifted view
            assert bool((b[:shift] == 7.0).all()) and bool((b[shift + n:] == 7.0).all())
        _check_bands(bands)


# ---- the backward --------------------------------------------------------------------------------------------------------------------------------

def _c_backward(params, x, labels, weight, cin, classes, want_logits=True):
    """ps_saliency_backward called directly on banded buffers: (loss, logits, flat gradients, scratch bytes)."""
    from point_unet_amd import _lib
    sal = _sal()
    flat = _cuda(sal.flatten_params(params, cin, classes))
    B, D, H, W, _ = x.shape
    bands = []
    grads, loss = _banded((flat.numel(),), bands), _banded((), bands)
    logits = _banded((B, D, H, W, classes), bands) if want_logits else None
    fn = _lib.lib().ps_saliency_backward
    call = lambda ctx, s, n: fn(ctx, _ptr(x), _ptr(labels), _ptr(weight), B, D, H, W, cin, classes, _ptr(flat), flat.numel(), _ptr(grads), _ptr(loss),
                                _ptr(logits), s, n)
    need = ctypes.c_int64(0)
    _lib.check(call(None, None, ctypes.byref(need)))
    scratch = _banded((need.value,), bands, torch.uint8)
    _lib.check(call(_ctx().handle, _ptr(scratch), ctypes.byref(need)))
    _check_bands(bands)
    return loss, logits, grads, need.value


def _by_name(flat, cin, classes):
    out, off = {}, 0
    for name, shape in _sal().param_shapes(cin, classes).items():
        n = int(np.prod(shape))
        out[name] = flat[off:off + n].reshape(shape)
        off += n
    assert off == flat.numel()
    return out


def _bar_between(a, b, want64, want32, what):
    """|a - b| under the bar that want64 / want32 set for either of them."""
    err = float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max())
    cpu = float(np.abs(want32.astype(np.float64) - want64).max())
    bar = 4.0 * cpu + 1e-6 * float(np.abs(want64).max())
    print("%s: one call against op by op %.3e, bar %.3e" % (what, err, bar))
    assert err <= bar, what


@functools.lru_cache(maxsize=None)
def _native_case():
    inputs = _graph_case()[0]
    params, x, labels, weight = inputs
    return _c_backward(params, _cuda(x), _cuda(labels), _cuda(weight), 1, 2)


def test_backward_loss_and_logits_equal_the_op_by_op_path():
    inputs, (net, loss, logits, grads, masks), _, _ = _graph_case()
    nloss, nlogits, _, _ = _native_case()
    assert torch.equal(nloss, loss) and torch.equal(nlogits, logits)


def test_backward_gradients_of_every_parameter():
    """[2, 32, 16, 16, 1], 2 classes: two slabs at full resolution, two voxels at the bottom level."""
    inputs, (net, loss, logits, grads, masks), want64, want32 = _graph_case()
    _, _, flat, _ = _native_case()
    got = _by_name(flat, 1, 2)
    assert len(got) == 158 and list(got) == list(grads)
    for n in got:
        _bar(_np(got[n]), want64[2][n], want32[2][n], "one call: d %s" % n)
        _bar_between(_np(got[n]), _np(grads[n]), want64[2][n], want32[2][n], "d %s" % n)


def test_backward_is_deterministic_and_logits_are_optional():
    inputs = _graph_case()[0]
    params, x, labels, weight = inputs
    loss, logits, flat, need = _native_case()
    loss2, none, flat2, need2 = _c_backward(params, _cuda(x), _cuda(labels), _cuda(weight), 1, 2, want_logits=False)
    assert none is None and need2 == need and need % 256 == 0
    assert torch.equal(loss, loss2) and torch.equal(flat, flat2)
    # the Python surface: the same bytes, the gradients by name
    tr = _sal().SaliencyTrainer(params, 1, 2)
    before = tr.flat.clone()
    ploss, plogits = tr.backward(_cuda(x), _cuda(labels), _cuda(weight), want_logits=True)
    assert torch.equal(ploss, loss) and torch.equal(plogits, logits) and torch.equal(tr.grad, flat) and torch.equal(tr.flat, before)
    assert tr.scratch_bytes == need
    named = tr.named_gradients()
    assert list(named) == list(_sal().param_shapes(1, 2)) and all(torch.equal(named[k], v) for k, v in _by_name(flat, 1, 2).items())
    assert all(np.array_equal(v, params[k]) for k, v in tr.export().items())


def test_backward_one_voxel_at_the_bottom():
    """[1, 16, 16, 16, 1]: the bottom level's instance norm has variance 0 and sends no gradient back."""
    params, x, labels, weight = graph_inputs((1, 16, 16, 16), seed=1)
    _, _, flat, _ = _c_backward(params, _cuda(x), _cuda(labels), _cuda(weight), 1, 2)
    got = _by_name(flat, 1, 2)
    assert all(bool(torch.isfinite(g).all()) for g in got.values())
    for i in (0, 1):
        assert not bool(got[tref.SCOPE + "down4_conv_%d/kernel" % i].any())
    assert bool(got[tref.SCOPE + "down3_conv_1/kernel"].any()) and bool(got[tref.SCOPE + "final/kernel"].any())


def test_backward_four_channels_four_classes_no_weight():
    """[1, 16, 16, 16, 4], 4 classes, weight NULL: the BraTS form, the 16-byte class path of the loss."""
    sal = _sal()
    rng = np.random.default_rng(7)
    params = sal.init_params(4, 4, seed=7)
    x = rng.standard_normal((1, 16, 16, 16, 4)).astype(np.float32)
    labels = rng.integers(0, 4, (1, 16, 16, 16)).astype(np.int32)
    net = sal.TrainableSaliencyNet(params, 4, 4)
    masks = {}
    with torch.no_grad():
        logits = net.logits(_cuda(x), masks)
        loss = sal.softmax_dice_loss(logits, _cuda(labels), None)[0]
    nloss, nlogits, flat, _ = _c_backward(params, _cuda(x), _cuda(labels), None, 4, 4)
    assert torch.equal(nloss, loss) and torch.equal(nlogits, logits)
    want = {}
    for dt in (F64, F32):
        P = tref.leaves(params, dt)
        ref_loss = tref.softmax_dice_loss(tref.graph(P, torch.from_numpy(x).to(dt), masks), torch.from_numpy(labels), None)
        want[dt] = (_np(ref_loss), dict(zip(P, (_np(g) for g in torch.autograd.grad(ref_loss, list(P.values()))))))
    _bar(_np(nloss), want[F64][0], want[F32][0], "4 channels, 4 classes: loss")
    got = _by_name(flat, 4, 4)
    for n in got:
        _bar(_np(got[n]), want[F64][1][n], want[F32][1][n], "4 channels, 4 classes: d %s" % n)


# ---- the step ------------------------------------------------------------------------------------------------------------------------------------

def _reference_losses(inputs, dt, steps=3, lr=0.01):
    """test_gpu_saliency_train.reference_losses in a given dtype: the losses before each reference_optimizer step and after the last, on
    the CPU with free ReLUs."""
    params, x, labels, weight = inputs
    net = torch.nn.Module()
    for k, v in params.items():
        net.register_parameter(k, torch.nn.Parameter(torch.tensor(v, dtype=dt)))  # (a copy: in float32 from_numpy would train the caller's arrays)
    opt = _sal().reference_optimizer(net, lr)
    xt, lt, wt = torch.from_numpy(x).to(dt), torch.from_numpy(labels), torch.from_numpy(weight).to(dt)
    out = []
    for step in range(steps + 1):
        loss = tref.softmax_dice_loss(tref.graph(dict(net.named_parameters()), xt), lt, wt)
        out.append(float(loss.detach()))
        if step < steps:
            opt.zero_grad()
            loss.backward()
            opt.step()
    return out


def _three_steps(inputs, **kw):
    params, x, labels, weight = inputs
    tr = _sal().SaliencyTrainer(params, 1, 2)
    xd, ld, wd = _cuda(x), _cuda(labels), _cuda(weight)
    losses = [float(tr.step(xd, ld, wd, 0.01, **kw)) for _ in range(3)]
    losses.append(float(tr.backward(xd, ld, wd)))
    return tr, losses


@functools.lru_cache(maxsize=None)
def _learn_case():
    inputs = graph_inputs((1, 16, 16, 16), seed=LEARN_SEED)
    return inputs, _three_steps(inputs)


def test_three_train_steps_follow_the_reference():
    """One [1, 16, 16, 16, 1] patch, seed 2, lr 0.01: the float64 CPU reference gives 0.41998, 0.38144, 0.37318, 0.38652."""
    inputs, (tr, losses) = _learn_case()
    t0 = time.time()
    cpu64, cpu32 = _reference_losses(inputs, F64), _reference_losses(inputs, F32)
    print("three steps: device %s, CPU float64 %s, float32 %s (%.1f s)" % (losses, cpu64, cpu32, time.time() - t0))
    assert np.allclose(cpu64, [0.41998, 0.38144, 0.37318, 0.38652], rtol=0, atol=5e-6)
    _bar(np.asarray(losses, np.float32), np.asarray(cpu64), np.asarray(cpu32, np.float32), "three steps: the losses")
    tr2, losses2 = _three_steps(inputs)
    assert losses2 == losses and torch.equal(tr2.flat, tr.flat) and torch.equal(tr2.accum, tr.accum)


def test_train_step_is_backward_and_the_restated_update():
    inputs, (tr, losses) = _learn_case()
    params, x, labels, weight = inputs
    sal = _sal()
    decay = sref.decay_mask(sal.param_shapes(1, 2))
    hand = sal.SaliencyTrainer(params, 1, 2)
    xd, ld, wd = _cuda(x), _cuda(labels), _cuda(weight)
    w, a = _np(hand.flat), np.zeros(hand.flat.numel(), np.float32)
    for step in range(3):
        assert float(hand.backward(xd, ld, wd)) == losses[step]
        w, a = sref.sgd_update(w, _np(hand.grad), a, decay, 0.01)
        hand.flat.copy_(_cuda(w))
    assert torch.equal(tr.flat, _cuda(w)) and torch.equal(tr.accum, _cuda(a))
    # backward + ps_saliency_sgd_update: the same
    two = sal.SaliencyTrainer(params, 1, 2)
    for step in range(3):
        two.backward(xd, ld, wd)
        two.update(0.01)
    assert torch.equal(two.flat, tr.flat) and torch.equal(two.accum, tr.accum)


def test_collective_callback():
    from point_unet_amd import _lib
    inputs, (plain, _) = _learn_case()
    params, x, labels, weight = inputs
    xd, ld, wd = _cuda(x), _cuda(labels), _cuda(weight)
    seen = []

    class _Raw:
        def __init__(self, ptr, count):
            self.__cuda_array_interface__ = {"shape": (int(count),), "typestr": "<f4", "data": (int(ptr), False), "version": 2}

    def double(user, buf, count, dtype, stream):  # the sum over two ranks that hold the same gradient
        seen.append((buf, count, dtype))
        torch.as_tensor(_Raw(buf, count), device="cuda").mul_(2.0)
        return 0

    fn = _lib.PS_ALLREDUCE_FN(double)
    tr = _sal().SaliencyTrainer(params, 1, 2)
    for step in range(3):
        tr.step(xd, ld, wd, 0.01, allreduce=fn, world_size=2)
        assert len(seen) == step + 1 and seen[-1] == (tr.grad.data_ptr(), tr.flat.numel(), 0)  # once, the whole buffer, float32
    assert torch.equal(tr.flat, plain.flat) and torch.equal(tr.accum, plain.accum)  # (2 g) / 2 is g, exactly
    # world_size 1: never called
    one = _sal().SaliencyTrainer(params, 1, 2)
    one.step(xd, ld, wd, 0.01, allreduce=fn, world_size=1)
    assert len(seen) == 3
    # a failing callback: a status, and the parameters stay
    failing = _lib.PS_ALLREDUCE_FN(lambda user, buf, count, dtype, stream: 1)
    bad = _sal().SaliencyTrainer(params, 1, 2)
    before = bad.flat.clone()
    with pytest.raises(_lib.PointSegError, match="all-reduce callback failed with code 1"):
        bad.step(xd, ld, wd, 0.01, allreduce=failing, world_size=2)
    torch.cuda.synchronize()
    assert torch.equal(bad.flat, before) and not bool(bad.accum.any())


# ---- argument errors -------------------------------------------------------------------------------------------------------------------------------

def test_argument_errors_enqueue_nothing():
    from point_unet_amd import _lib
    lib = _lib.lib()
    n = lib.ps_saliency_weight_count(1, 2)
    ctx = _ctx().handle
    x = torch.zeros((1, 16, 16, 16, 1), device="cuda")
    labels = torch.zeros((1, 16, 16, 16), dtype=torch.int32, device="cuda")
    buf = torch.full((3 * n,), 0xA5, dtype=torch.uint8, device="cuda").repeat(4).view(torch.float32)  # weights | grads | accum, all sentinel
    weights, grads, accum = buf[:n], buf[n:2 * n], buf[2 * n:]
    loss = torch.full((1,), -7.0, device="cuda")
    need = ctypes.c_int64(0)
    _lib.check(lib.ps_saliency_backward(None, None, None, None, 1, 16, 16, 16, 1, 2, None, n, None, None, None, None, ctypes.byref(need)))
    scratch = torch.full((need.value,), 0xA5, dtype=torch.uint8, device="cuda")

    def backward(**kw):
        a = dict(ctx=ctx, x=_ptr(x), labels=_ptr(labels), weight=None, B=1, D=16, H=16, W=16, C_in=1, K=2, weights=_ptr(weights), count=n, grads=_ptr(grads),
                 loss=_ptr(loss), logits=None, scratch=_ptr(scratch))
        a.update(kw)
        return lib.ps_saliency_backward(*a.values(), ctypes.byref(ctypes.c_int64(need.value)))

    def step(**kw):
        a = dict(ctx=ctx, x=_ptr(x), labels=_ptr(labels), weight=None, B=1, D=16, H=16, W=16, C_in=1, K=2, params=_ptr(weights), count=n, grads=_ptr(grads),
                 accum=_ptr(accum), lr=0.01, options=None, loss=_ptr(loss), logits=None, scratch=_ptr(scratch))
        a.update(kw)
        return lib.ps_saliency_train_step(*a.values(), ctypes.byref(ctypes.c_int64(need.value)))

    err = lib.ps_last_error
    for call in (backward, step):
        for kw, word in ((dict(D=24), b"multiple of 16"), (dict(W=8), b"multiple of 16"), (dict(count=n - 1), b"weight_count"),
                         (dict(grads=_ptr(weights[4:])), b"must not overlap"), (dict(x=None), b"NULL"), (dict(labels=None), b"NULL"), (dict(grads=None), b"NULL"),
                         (dict(loss=None), b"NULL"), (dict(ctx=None), b"NULL")):
            assert call(**kw) == 1 and word in err(), (call.__name__, kw, err())
    assert step(accum=None) == 1 and b"NULL" in err() and step(accum=_ptr(grads)) == 1 and b"must not overlap" in err()
    assert lib.ps_saliency_sgd_update(ctx, _ptr(weights), _ptr(grads), _ptr(accum), 1, 2, n + 1, 0.01, 0.9, 1e-5, 1.0) == 1 and b"weight_count" in err()
    assert lib.ps_saliency_sgd_update(ctx, _ptr(weights), _ptr(weights), _ptr(accum), 1, 2, n, 0.01, 0.9, 1e-5, 1.0) == 1 and b"must not overlap" in err()
    torch.cuda.synchronize()
    raw = buf.view(torch.uint8)
    assert bool((raw == 0xA5).all()) and bool((scratch == 0xA5).all()) and float(loss) == -7.0  # nothing ran


# ---- train_saliency(engine="native") -----------------------------------------------------------------------------------------------------------------

def test_train_saliency_native_engine():
    """Three steps at patch (16, 16, 16), B = 2 on a two-volume bank: the batches of the autograd engine, drawn by hand, through
    SaliencyTrainer.step."""
    from point_unet_amd import saliency_data as sd
    from test_gpu_saliency_data import _pancreas_bank
    sal = _sal()
    bank = _pancreas_bank(((20, 24, 18), (18, 20, 22)), seed=9)
    params = sal.init_params(1, 2, seed=5)
    P = (16, 16, 16)
    tr = sal.SaliencyTrainer(params, 1, 2)
    losses = sd.train_saliency(tr, bank, 3, P, batch_size=2, lr=0.01, seed=3, engine="native")
    assert isinstance(losses, torch.Tensor) and losses.is_cuda and tuple(losses.shape) == (3,)
    hand = sal.SaliencyTrainer(params, 1, 2)
    auto = list(bank.epoch_batches(2, P, 0, 3)) + list(bank.epoch_batches(2, P, 1, 3)) + list(bank.epoch_batches(2, P, 2, 3))  # what the autograd engine draws
    assert len(auto) == 3
    for epoch in range(3):  # two volumes, batches of two: one batch per epoch
        (_, cand, s), = sd.epoch_plan(2, 2, epoch, seed=3, tries=8)
        batch = bank.sample(cand, P, s, "one_positive")
        assert all(torch.equal(batch[k], auto[epoch][k]) for k in ("images", "labels", "weights"))
        assert torch.equal(hand.step(batch["images"], batch["labels"], batch["weights"], 0.01), losses[epoch])
    assert torch.equal(hand.flat, tr.flat) and torch.equal(hand.accum, tr.accum)
    with pytest.raises(ValueError):
        sd.train_saliency(tr, bank, 1, P, engine="autograd")
    with pytest.raises(ValueError):
        sd.train_saliency(sal.TrainableSaliencyNet(params, 1), bank, 1, P, engine="native")
