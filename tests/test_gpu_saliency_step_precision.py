"""include/pointseg_saliency_step_precision.h on the device: ps_saliency_backward_prec and ps_saliency_train_step_prec, the one-call step
with one precision per role of its convolutions (forward, data gradient, weight gradient).

The yardstick is the op-by-op path at the SAME precisions (TrainableSaliencyNet(precision=...)), not float64: the step runs the same op
entries on the same operands in the same order, so it owes that path bytes -- loss and logits torch.equal, every gradient within the
fp32-rounding scale of test_gpu_saliency_step._bar_between (the two paths can differ only in the order of the float32 sums of gradients) --
and PS_PREC_FP32 three times owes the older entries their bytes.  That each role reaches its own call site is shown without a numeric
reference: a rounded role moves exactly the results behind it and leaves the others' bytes alone.

Every direct call gives its results between guard bands of 4096 sentinel floats and scratch of exactly the reported size between two more."""
import ctypes
import functools

import numpy as np
import pytest

import saliency_step_ref as sref
import saliency_train_ref as tref
from test_gpu_saliency_step import _bar_between, _by_name, _c_backward, _native_case
from test_gpu_saliency_train import LEARN_SEED, _banded, _check_bands, _ctx, _cuda, _graph_case, _np, graph_inputs

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

MIXED = ("bf16x3", "bf16", "fp32")
COMBOS = ["bf16x3", "bf16", MIXED]
IDS = ["bf16x3", "bf16", "bf16x3-bf16-fp32"]
EINVAL = 1


def _sal():
    from point_unet_amd import saliency
    return saliency


def _ptr(t):
    from point_unet_amd import runtime
    return runtime.ptr(t)


def _modes(precision, soft=0):
    """(soft_labels, precision_forward, precision_data_grad, precision_weight_grad) as the C entries take them."""
    return (int(soft),) + tuple(_sal()._precision("test", precision))


def _c_backward_prec(params, x, labels, weight, cin, classes, precision, soft=0, want_logits=True, entry="ps_saliency_backward_prec", modes=None):
    """`entry` called directly on banded buffers: (loss, logits, flat gradients, scratch bytes).  modes: the four trailing arguments (from
    `precision` and `soft` unless given; () for an entry that has none)."""
    from point_unet_amd import _lib
    flat = _cuda(_sal().flatten_params(params, cin, classes))
    B, D, H, W, _ = x.shape
    bands = []
    grads, loss = _banded((flat.numel(),), bands), _banded((), bands)
    logits = _banded((B, D, H, W, classes), bands) if want_logits else None
    fn = getattr(_lib.lib(), entry)
    modes = _modes(precision, soft) if modes is None else modes
    call = lambda ctx, s, n: fn(ctx, _ptr(x), _ptr(labels), _ptr(weight), B, D, H, W, cin, classes, _ptr(flat), flat.numel(), _ptr(grads), _ptr(loss),
                                _ptr(logits), s, n, *modes)
    need = ctypes.c_int64(0)
    _lib.check(call(None, None, ctypes.byref(need)))
    scratch = _banded((need.value,), bands, torch.uint8)
    _lib.check(call(_ctx().handle, _ptr(scratch), ctypes.byref(need)))
    _check_bands(bands)
    return loss, logits, grads, need.value


def _op_by_op(params, x, labels, weight, cin, classes, precision):
    """TrainableSaliencyNet(precision=...) under torch.autograd: (loss, logits, gradients by name)."""
    net = _sal().TrainableSaliencyNet(params, cin, classes, precision=precision)
    logits = net.logits(x)
    loss = _sal().differentiable_softmax_dice_loss(logits, labels, weight)
    loss.backward()
    return loss.detach(), logits.detach(), {n: p.grad for n, p in net.named_parameters()}


def _device_inputs():
    params, x, labels, weight = _graph_case()[0]  # graph_inputs((2, 32, 16, 16)): two slabs at full resolution, two voxels at the bottom
    return params, _cuda(x), _cuda(labels), _cuda(weight)


@functools.lru_cache(maxsize=None)
def _one_call(precision):
    """The one call at [2, 32, 16, 16, 1], once per session and precision."""
    params, x, labels, weight = _device_inputs()
    return _c_backward_prec(params, x, labels, weight, 1, 2, precision)


@functools.lru_cache(maxsize=None)
def _graph(precision):
    params, x, labels, weight = _device_inputs()
    return _op_by_op(params, x, labels, weight, 1, 2, precision)


def _all_equal(a, b):
    return all(torch.equal(a[k], b[k]) for k in a)


# ---- 1, 2: the one call against the op-by-op path at the same precisions ----------------------------------------------------------------------------

@pytest.mark.parametrize("precision", COMBOS, ids=IDS)
def test_loss_and_logits_are_the_op_by_op_bytes(precision):
    nloss, nlogits, _, _ = _one_call(precision)
    loss, logits, _ = _graph(precision)
    assert torch.equal(nloss, loss) and torch.equal(nlogits, logits)


@pytest.mark.parametrize("precision", COMBOS, ids=IDS)
def test_gradients_of_every_parameter_against_the_op_by_op_path(precision):
    """All 158, in param_shapes order, each within _bar_between's fp32-rounding scale of the op-by-op gradient at the same precisions."""
    _, _, want64, want32 = _graph_case()
    _, _, flat, _ = _one_call(precision)
    _, _, grads = _graph(precision)
    got = _by_name(flat, 1, 2)
    assert len(got) == 158 and list(got) == list(grads) == list(_sal().param_shapes(1, 2))
    equal = sum(1 for n in got if torch.equal(got[n], grads[n]))
    print("%s: %d of 158 gradients byte-equal to the op-by-op path" % (precision, equal))
    for n in got:
        _bar_between(_np(got[n]), _np(grads[n]), want64[2][n], want32[2][n], "%s: d %s" % (precision, n))


# ---- 3: fp32 is today's bytes --------------------------------------------------------------------------------------------------------------------------

def _same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and a[3] == b[3]


def test_fp32_three_times_is_the_older_entries_bytes():
    params, x, labels, weight = _device_inputs()
    assert _same(_one_call("fp32"), _native_case())  # ps_saliency_backward
    # the soft pair, on mixed rows
    sparams, sx, slabels, sweight = graph_inputs((1, 16, 16, 16), seed=4)
    other = np.random.default_rng(16).integers(0, 2, slabels.shape)
    rows = (0.34 * np.eye(2, dtype=np.float32)[slabels] + 0.66 * np.eye(2, dtype=np.float32)[other]).astype(np.float32)
    sx, rows, sweight = _cuda(sx), _cuda(rows), _cuda(sweight)
    old = _c_backward_prec(sparams, sx, rows, sweight, 1, 2, None, entry="ps_saliency_backward_soft", modes=())
    assert _same(_c_backward_prec(sparams, sx, rows, sweight, 1, 2, "fp32", soft=1), old)
    assert not torch.equal(old[2], _c_backward_prec(sparams, sx, _cuda(slabels), sweight, 1, 2, "fp32")[2])  # (the rows are mixed: another loss)
    # the Python surface: the default is "fp32", and both are the older entry's bytes
    sal = _sal()
    for tr in (sal.SaliencyTrainer(params, 1, 2), sal.SaliencyTrainer(params, 1, 2, precision="fp32")):
        assert tr.precision == "fp32"
        ploss, plogits = tr.backward(x, labels, weight, want_logits=True)
        assert _same((ploss, plogits, tr.grad, tr.scratch_bytes), _native_case())


# ---- 4: the modes are on, and each role reaches its own call site ------------------------------------------------------------------------------------

def _conv_kernels(names):
    return [n for n in names if n.endswith("/kernel") and "_dense_" not in n]


def test_weight_gradient_role_moves_the_convolution_kernels_gradients_alone():
    loss, logits, flat, _ = _one_call("fp32")
    bloss, blogits, bflat, _ = _one_call(("fp32", "fp32", "bf16"))
    assert torch.equal(bloss, loss) and torch.equal(blogits, logits)
    a, b = _by_name(flat, 1, 2), _by_name(bflat, 1, 2)
    fixed = [n for n in a if n.endswith("/gamma") or n.endswith("/beta") or "_dense_" in n]  # every dy is unchanged and those ops are fp32
    assert len(fixed) == 2 * (len(_conv_kernels(a)) - 1) + 4 and sum(1 for n in fixed if "_dense_" in n) == 4  # (`final` has no norm)
    for n in fixed:
        assert torch.equal(a[n], b[n]), n
    for n in _conv_kernels(a):
        assert not torch.equal(a[n], b[n]), n


def test_data_gradient_role_leaves_the_last_layer_alone_and_reaches_the_first():
    loss, logits, flat, _ = _one_call("fp32")
    bloss, blogits, bflat, _ = _one_call(("fp32", "bf16", "fp32"))
    assert torch.equal(bloss, loss) and torch.equal(blogits, logits)
    a, b = _by_name(flat, 1, 2), _by_name(bflat, 1, 2)
    for n in ("final/kernel", "final/bias"):  # their dy comes from the loss alone
        assert torch.equal(a[tref.SCOPE + n], b[tref.SCOPE + n]), n
    assert not torch.equal(a[tref.SCOPE + "init_conv/kernel"], b[tref.SCOPE + "init_conv/kernel"])


def test_forward_role_moves_the_logits():
    assert not torch.equal(_one_call(("bf16", "fp32", "fp32"))[1], _one_call("fp32")[1])


def test_bf16_gradient_distance_from_fp32_is_reported():
    a, b = _one_call("fp32")[2].double(), _one_call("bf16")[2].double()
    print("bf16 against fp32, the whole gradient: relative L2 distance %.3f" % float((a - b).norm() / a.norm()))  # (no bound exists: DESIGN.md 4.16)
    assert bool(torch.isfinite(b).all())


# ---- 5: determinism, optional logits, scratch -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["bf16x3", "bf16"])
def test_two_runs_are_byte_equal_logits_are_optional_and_the_scratch_is_fp32s(precision):
    params, x, labels, weight = _device_inputs()
    first = _one_call(precision)
    assert _same(_c_backward_prec(params, x, labels, weight, 1, 2, precision), first)
    loss, none, flat, need = _c_backward_prec(params, x, labels, weight, 1, 2, precision, want_logits=False)
    assert none is None and torch.equal(loss, first[0]) and torch.equal(flat, first[2])
    assert need == first[3] == _native_case()[3] and need % 256 == 0  # (the guard bands are checked inside every call)


# ---- 6: the step ------------------------------------------------------------------------------------------------------------------------------------------

def _c_step_prec(state, x, labels, weight, lr, precision, options=None):
    """ps_saliency_train_step_prec on the banded buffers of `state` = (params, grads, accum, loss, bands): one step in place."""
    from point_unet_amd import _lib
    params, grads, accum, loss, bands = state
    B, D, H, W, _ = x.shape
    fn = _lib.lib().ps_saliency_train_step_prec
    call = lambda ctx, s, n: fn(ctx, _ptr(x), _ptr(labels), _ptr(weight), B, D, H, W, 1, 2, _ptr(params), params.numel(), _ptr(grads), _ptr(accum), lr,
                                ctypes.byref(options) if options is not None else None, _ptr(loss), None, s, n, *_modes(precision))
    need = ctypes.c_int64(0)
    _lib.check(call(None, None, ctypes.byref(need)))
    scratch = _banded((need.value,), bands, torch.uint8)
    _lib.check(call(_ctx().handle, _ptr(scratch), ctypes.byref(need)))
    _check_bands(bands)
    del bands[-2:]


def _step_state(params):
    flat = _sal().flatten_params(params, 1, 2)
    bands = []
    w, g, a, loss = _banded((flat.size,), bands), _banded((flat.size,), bands), _banded((flat.size,), bands), _banded((), bands)
    w.copy_(_cuda(flat)), a.zero_()
    return w, g, a, loss, bands


@pytest.mark.parametrize("precision", ["bf16x3", "bf16"])
def test_train_step_is_backward_and_the_restated_update(precision):
    from point_unet_amd import _lib
    sal = _sal()
    params, x, labels, weight = graph_inputs((1, 16, 16, 16), seed=LEARN_SEED)
    xd, ld, wd = _cuda(x), _cuda(labels), _cuda(weight)
    decay = sref.decay_mask(sal.param_shapes(1, 2))
    state = _step_state(params)
    w, a = sal.flatten_params(params, 1, 2), np.zeros(decay.size, np.float32)
    for step in range(2):  # (the second step has a momentum to carry)
        hand = _c_backward_prec(sal.unflatten_params(w, 1, 2), xd, ld, wd, 1, 2, precision)
        _c_step_prec(state, xd, ld, wd, 0.01, precision)
        assert torch.equal(state[3], hand[0]) and torch.equal(state[1], hand[2]), step
        w, a = sref.sgd_update(w, _np(hand[2]), a, decay, 0.01)
        assert torch.equal(state[0], _cuda(w)) and torch.equal(state[2], _cuda(a)), step
    assert bool(state[2].any())

    # a collective of two ranks that hold the same gradient: called once with the whole buffer, and (2 g) / 2 is g exactly
    seen = []

    class _Raw:
        def __init__(self, ptr, count):
            self.__cuda_array_interface__ = {"shape": (int(count),), "typestr": "<f4", "data": (int(ptr), False), "version": 2}

    def double(user, buf, count, dtype, stream):
        seen.append((buf, count, dtype))
        torch.as_tensor(_Raw(buf, count), device="cuda").mul_(2.0)
        return 0

    fn = _lib.PS_ALLREDUCE_FN(double)
    two = _step_state(params)
    opt = _lib.PsSaliencyStepOptions(fn, None, 2, 0.9, 1e-5)
    for step in range(2):
        _c_step_prec(two, xd, ld, wd, 0.01, precision, opt)
        assert len(seen) == step + 1 and seen[-1] == (two[1].data_ptr(), decay.size, 0)
    assert torch.equal(two[0], state[0]) and torch.equal(two[2], state[2])  # grad_scale is 0.5
    assert torch.equal(two[1], 2.0 * state[1])  # (the summed gradient stays in `grads`)


# ---- 7: the BraTS form and soft labels ---------------------------------------------------------------------------------------------------------------------

def test_four_channels_four_classes_no_weight_in_bf16():
    """[1, 16, 16, 16, 4], 4 classes, weight NULL: one sample and the same order -- every gradient is the op-by-op path's, byte for byte."""
    sal = _sal()
    rng = np.random.default_rng(7)
    params = sal.init_params(4, 4, seed=7)
    x = _cuda(rng.standard_normal((1, 16, 16, 16, 4)).astype(np.float32))
    labels = _cuda(rng.integers(0, 4, (1, 16, 16, 16)).astype(np.int32))
    loss, logits, grads = _op_by_op(params, x, labels, None, 4, 4, "bf16")
    nloss, nlogits, flat, _ = _c_backward_prec(params, x, labels, None, 4, 4, "bf16")
    assert torch.equal(nloss, loss) and torch.equal(nlogits, logits)
    got = _by_name(flat, 4, 4)
    assert list(got) == list(grads)
    differ = [n for n in got if not torch.equal(got[n], grads[n])]
    assert not differ, differ
    assert not torch.equal(nlogits, _c_backward_prec(params, x, labels, None, 4, 4, "fp32")[1])  # (and the mode is on)


def test_soft_one_hot_rows_are_the_hard_labels_in_bf16x3():
    params, x, labels, weight = graph_inputs((1, 16, 16, 16), seed=4)
    xd, wd = _cuda(x), _cuda(weight)
    hard = _c_backward_prec(params, xd, _cuda(labels), wd, 1, 2, "bf16x3")
    soft = _c_backward_prec(params, xd, _cuda(np.eye(2, dtype=np.float32)[labels]), wd, 1, 2, "bf16x3", soft=1)
    assert _same(soft, hard)


# ---- 8: argument errors ------------------------------------------------------------------------------------------------------------------------------------

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
    logits = torch.full((1, 16, 16, 16, 2), -7.0, device="cuda")
    need = ctypes.c_int64(0)
    _lib.check(lib.ps_saliency_backward_prec(None, None, None, None, 1, 16, 16, 16, 1, 2, None, n, None, None, None, None, ctypes.byref(need), 0, 2, 1, 0))
    scratch = torch.full((need.value,), 0xA5, dtype=torch.uint8, device="cuda")

    def backward(modes, run):
        got = ctypes.c_int64(need.value if run else -7)
        rc = lib.ps_saliency_backward_prec(ctx if run else None, _ptr(x), _ptr(labels), None, 1, 16, 16, 16, 1, 2, _ptr(weights), n, _ptr(grads), _ptr(loss),
                                           _ptr(logits), _ptr(scratch) if run else None, ctypes.byref(got), *modes)
        return rc, got.value

    def step(modes, run):
        got = ctypes.c_int64(need.value if run else -7)
        rc = lib.ps_saliency_train_step_prec(ctx if run else None, _ptr(x), _ptr(labels), None, 1, 16, 16, 16, 1, 2, _ptr(weights), n, _ptr(grads), _ptr(accum),
                                             0.01, None, _ptr(loss), _ptr(logits), _ptr(scratch) if run else None, ctypes.byref(got), *modes)
        return rc, got.value

    bad = [(2, 0, 0, 0)] + [tuple(v if i == role else 0 for i in range(4)) for role in (1, 2, 3) for v in (3, -1)]
    for call in (backward, step):
        for modes in bad:
            word = b"soft_labels" if modes[0] else b"precision"
            assert call(modes, False) == (EINVAL, -7) and word in lib.ps_last_error(), (call.__name__, modes)  # the sizing call: *scratch_bytes untouched
            assert call(modes, True) == (EINVAL, need.value) and word in lib.ps_last_error(), (call.__name__, modes)
    torch.cuda.synchronize()
    assert bool((buf.view(torch.uint8) == 0xA5).all()) and bool((scratch == 0xA5).all()) and float(loss) == -7.0 and bool((logits == -7.0).all())  # nothing ran
    params = _sal().init_params(1, 2, seed=0)
    for wrong in ("fp16", ("bf16x3", "bf16"), ("bf16x3", "bf16", "fp16")):
        with pytest.raises(ValueError, match="precision"):
            _sal().SaliencyTrainer(params, 1, 2, precision=wrong)


# ---- 9: the Python surface ------------------------------------------------------------------------------------------------------------------------------------

def test_trainer_backward_is_the_direct_call():
    params, x, labels, weight = _device_inputs()
    triple = ("bf16x3", "bf16", "bf16")
    tr = _sal().SaliencyTrainer(params, 1, 2, precision=triple)
    assert tr.precision == triple
    before = tr.flat.clone()
    ploss, plogits = tr.backward(x, labels, weight, want_logits=True)
    assert _same((ploss, plogits, tr.grad, tr.scratch_bytes), _one_call(triple)) and torch.equal(tr.flat, before)
    assert not torch.equal(tr.grad, _one_call("bf16x3")[2])  # (the second and third names are heard)
    net = _sal().TrainableSaliencyNet(params, 1, 2, precision=triple)  # the op-by-op surface takes the same triple
    assert net.export(precision="forward").precision == "bf16x3" and set(net.export()) == set(params)
    assert torch.equal(_graph(triple)[1], _one_call(triple)[1]) and torch.equal(_graph(triple)[1], _graph("bf16x3")[1])  # the forward hears the first


def test_train_saliency_native_engine_carries_the_trainers_precision():
    """Two steps at patch (16, 16, 16), B = 2 on a two-volume bank, as test_gpu_saliency_step.test_train_saliency_native_engine builds it: the
    losses are those of two trainer.step calls on the same batches, bit for bit."""
    from point_unet_amd import saliency_data as sd
    from test_gpu_saliency_data import _pancreas_bank
    sal = _sal()
    bank = _pancreas_bank(((20, 24, 18), (18, 20, 22)), seed=9)
    params = sal.init_params(1, 2, seed=5)
    P = (16, 16, 16)
    tr = sal.SaliencyTrainer(params, 1, 2, precision="bf16")
    losses = sd.train_saliency(tr, bank, 2, P, batch_size=2, lr=0.01, seed=3, engine="native")
    assert isinstance(losses, torch.Tensor) and tuple(losses.shape) == (2,) and bool(torch.isfinite(losses).all())
    hand, fp32 = sal.SaliencyTrainer(params, 1, 2, precision="bf16"), sal.SaliencyTrainer(params, 1, 2)
    for epoch in range(2):  # two volumes, batches of two: one batch per epoch
        (_, cand, s), = sd.epoch_plan(2, 2, epoch, seed=3, tries=8)
        batch = bank.sample(cand, P, s, "one_positive")
        assert torch.equal(hand.step(batch["images"], batch["labels"], batch["weights"], 0.01), losses[epoch])
        if epoch == 0:
            assert not torch.equal(fp32.step(batch["images"], batch["labels"], batch["weights"], 0.01), losses[0])  # (not the fp32 step)
    assert torch.equal(hand.flat, tr.flat) and torch.equal(hand.accum, tr.accum)
