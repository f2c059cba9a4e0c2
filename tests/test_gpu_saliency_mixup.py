"""include/pointseg_saliency_mixup.h on the device: the mixed gather byte-equal to its numpy restatement (saliency_mixup_ref.py) and to
ps_patch_sample mixed with torch; the soft-label Dice loss byte-equal to the hard-label op on one-hot rows and under the project's bar
against float64 autograd on genuinely soft ones; the step on soft labels against the op-by-op path; train_saliency(mixup=...) in both
engines."""
import ctypes
import functools

import numpy as np
import pytest

import saliency_data_ref as dref
import saliency_mixup_ref as ref
import saliency_train_ref as tref
import test_gpu_saliency_data as tdata
from test_gpu_saliency import _bar
from test_gpu_saliency_step import _bar_between, _by_name, _c_backward, _ptr
from test_gpu_saliency_train import F32, F64, _banded, _c_loss, _c_loss_bwd, _check_bands, _ctx, _cuda, _np, _two_call, graph_inputs, loss_inputs

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

GAMMAS = (0.0, 1.0, 1.0 - 2.0 ** -30, 0.34029683942911143, 0.77, 1e-12)
SHAPES = ((9, 20, 23), (4, 6, 30), (17, 33, 19))  # odd extents: source rows start at any byte


def _sal():
    from point_unet_amd import saliency
    return saliency


def _sd():
    from point_unet_amd import saliency_data
    return saliency_data


# ---- the mixed gather against the restatement -------------------------------------------------------------------------------------------------

def _direct(bank, cand, P, seed, mode, K, gamma, shift=0):
    """ps_patch_sample_mixup itself, every output `shift` bytes past a 256-byte boundary between guard bands.  Returns (outputs as numpy,
    the raw output bytes)."""
    from point_unet_amd import _lib, runtime
    cand = np.ascontiguousarray(cand, dtype=np.int32)
    B, T = cand.shape[0] - 1, cand.shape[1]
    C = bank.channels
    gamma = np.ascontiguousarray(gamma, np.float64)
    shapes = {"images": ((B,) + tuple(P) + (C,), np.float32), "weights": ((B,) + tuple(P), np.float32), "soft": ((B,) + tuple(P) + (K,), np.float32),
              "info": ((B + 1, 8), np.int32)}
    bufs = {k: tdata._banded(4 * int(np.prod(s)), shift) for k, (s, _) in shapes.items()}
    images, labels, weights, dims, n = bank.c_tables()
    bank.ctx.use_torch_stream()
    rc = _lib.lib().ps_patch_sample_mixup(bank.ctx.handle, images, labels, weights, dims, n, C, cand.ctypes.data_as(_lib.c_i32p), B, T, (ctypes.c_int64 * 3)(*P),
                                          seed, tdata.MODE_ID[mode], K, gamma.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                          *[runtime.ptr(bufs[k][1]) for k in ("images", "weights", "soft", "info")])
    assert rc == 0, _lib.lib().ps_last_error()
    torch.cuda.synchronize()
    band = tdata.BAND
    assert all(bool((full[:band + shift] == 0xA5).all()) and bool((full[band + shift + part.numel():] == 0xA5).all()) for full, part in bufs.values()), \
        "a guard band was written"
    raw = {k: _np(part).copy() for k, (_, part) in bufs.items()}
    return {k: raw[k].view(dt).reshape(s) for k, (s, dt) in shapes.items()}, raw


def _equal_to_the_rule(vols, bank, cand, P, seed, mode, K, gamma, cache, shift=0):
    got, raw = _direct(bank, cand, P, seed, mode, K, gamma, shift)
    images, weights, soft, info = ref.sample_mixup(vols, cand, P, seed, mode, K, gamma, cache)
    assert np.array_equal(got["info"], info), (got["info"], info)
    assert np.array_equal(got["weights"].view(np.uint32), weights.view(np.uint32))
    assert np.array_equal(got["soft"].view(np.uint32), soft.view(np.uint32))
    assert np.array_equal(got["images"].view(np.uint32), images.view(np.uint32))
    return info, raw


def _cands(n, B, T):
    """Candidate tables [B + 1, T] over the bank of test_gpu_saliency_data._make_bank (labelled volumes 0 .. n-1, empty ones n .. 2n-1)."""
    c = tdata._cands(n, B + 1, T)  # (its "late" makes only the LAST sample's last try positive: under the mixed rule nobody asks for it)
    forced = c["none"].copy()
    forced[B - 1, T - 1] = 0       # the forced sample B - 1 finds its positive on its last try ...
    forced[B, T - 1] = 1           # ... and sample B, which has one there too, stays on try 0
    c["forced"] = forced
    return c


CASES = [(C, P) for P in ((5, 6, 7), (8, 8, 8), (16, 16, 16)) for C in (1, 4)]


@pytest.mark.parametrize("C, P", CASES, ids=["C%d-P%d" % (c, p[0]) for c, p in CASES])
def test_mixed_sampler_equals_the_rule_bit_for_bit(C, P):
    """(5, 6, 7): P2 * C % 4 != 0 at C = 1; (8, 8, 8): row-aligned, overhang and fill on the (4, 6, 30) volume; (16, 16, 16): larger than two
    of the volumes.  K = 2, 3, 4: the paired, the scalar and the 16-byte soft rows (labels go up to 3: K = 2 and 3 see labels >= K)."""
    vols, bank = tdata._make_bank(C, SHAPES, seed=300 + C + P[0])
    n = len(SHAPES)
    seen = {}
    call = 0
    for B, T, classes in ((1, 1, (2,)), (1, 4, (3,)), (3, 1, (4,)), (3, 4, (2, 3, 4))):
        cands, cache, seed = _cands(n, B, T), {}, 7 + 13 * B + T
        for K in classes:
            for mode in dref.MODES:
                for name in ("mixed", "none", "late", "late_all", "first", "forced"):
                    if T == 1 and name not in ("mixed", "none"):
                        continue
                    gamma = [GAMMAS[(call + b) % len(GAMMAS)] for b in range(B)]
                    call += 1
                    info, _ = _equal_to_the_rule(vols, bank, cands[name], P, seed, mode, K, gamma, cache)
                    seen[(mode, name, B, T)] = (tuple(info[:, 0]), tuple(info[:, 6]))
    assert call >= len(GAMMAS)  # every gamma, the ends of [0, 1] and float32(gamma) == 1 with h > 0 among them, was used
    # each branch of the mixed choice was taken: the forced sample is B - 1 = 2, sample 3 stays on try 0
    assert seen[("one_positive", "forced", 3, 4)] == ((0, 0, 3, 0), (1, 1, 1, 1))
    assert seen[("one_positive", "none", 3, 4)] == ((0, 0, 3, 0), (1, 1, 0, 1)) == seen[("one_positive", "late", 3, 4)]
    assert seen[("one_positive", "first", 3, 4)] == ((0, 0, 0, 0), (1, 1, 1, 1))
    assert seen[("all_positive", "late_all", 3, 4)] == ((3, 3, 3, 3), (1, 1, 1, 1)) and seen[("all_positive", "none", 3, 4)] == ((3, 3, 3, 3), (0, 0, 0, 0))
    assert seen[("random", "none", 3, 4)] == ((0, 0, 0, 0), (1, 1, 1, 1))
    assert seen[("one_positive", "forced", 1, 4)] == ((3, 0), (1, 1)) and seen[("one_positive", "none", 1, 4)] == ((3, 0), (0, 1))  # B = 1: sample 0
    assert seen[("one_positive", "none", 3, 1)] == ((0, 0, 0, 0), (1, 1, 0, 1))
    # outputs 4 or 8 bytes past a 16-byte boundary take the narrower stores: the same bytes.  Two runs give the same bytes.
    cands, cache = _cands(n, 3, 4), {}
    for K in (2, 3, 4):
        gamma = [GAMMAS[3], GAMMAS[2], GAMMAS[4]]
        _, raw = _equal_to_the_rule(vols, bank, cands["mixed"], P, 5, "one_positive", K, gamma, cache)
        for shift in (4, 8):
            _, shifted = _equal_to_the_rule(vols, bank, cands["mixed"], P, 5, "one_positive", K, gamma, cache, shift=shift)
            assert all(np.array_equal(raw[k], shifted[k]) for k in raw)
        _, again = _direct(bank, cands["mixed"], P, 5, "one_positive", K, gamma)
        assert all(np.array_equal(raw[k], again[k]) for k in raw)


@pytest.mark.parametrize("mode", ["random", "all_positive"])
def test_mixed_sampler_is_the_plain_sampler_mixed_with_torch(mode):
    """For the modes whose choice does not single out a sample, the mixed batch is ps_patch_sample at B + 1 slots on the same cand, mixed by
    eager torch ops (two products and a sum, each its own kernel: no fused multiply-add)."""
    K = 4
    for C, P in ((1, (5, 6, 7)), (4, (8, 8, 8))):
        vols, bank = tdata._make_bank(C, SHAPES, seed=41)
        cand = _cands(len(SHAPES), 3, 4)["late_all" if mode == "all_positive" else "mixed"]
        gamma = np.array([GAMMAS[3], GAMMAS[2], GAMMAS[4]])
        plain = bank.sample(cand, P, 21, mode)
        mixed = bank.sample(cand, P, 21, mode, mixup=K, gamma=gamma)
        assert set(mixed) == {"images", "weights", "labels", "info", "gamma"} and np.array_equal(mixed["gamma"], gamma)
        assert mixed["labels"].dtype == torch.float32 and tuple(mixed["labels"].shape) == (3,) + P + (K,) and tuple(mixed["info"].shape) == (4, 8)
        assert torch.equal(mixed["info"], plain["info"])
        g = _cuda(gamma.astype(np.float32))
        h = _cuda((1.0 - gamma).astype(np.float32))

        def mix(t):
            shape = (3,) + (1,) * (t.dim() - 1)
            a, b = g.reshape(shape) * t[:-1], h.reshape(shape) * t[1:]
            return a + b

        hot = torch.nn.functional.one_hot(plain["labels"].long(), K).to(torch.float32)
        assert torch.equal(mixed["images"], mix(plain["images"])) and torch.equal(mixed["labels"], mix(hot))
        assert torch.equal(mixed["weights"], ((plain["weights"][:-1] != 0) | (plain["weights"][1:] != 0)).to(torch.float32))
    # gamma drawn from the seed on the host: Beta(0.4, 0.4) of numpy's default generator
    drawn = bank.sample(cand, P, 21, mode, mixup=K)
    assert np.array_equal(drawn["gamma"], np.random.default_rng(21).beta(0.4, 0.4, 3))
    assert all(torch.equal(drawn[k], bank.sample(cand, P, 21, mode, mixup=K, gamma=drawn["gamma"])[k]) for k in ("images", "weights", "labels", "info"))


# ---- the soft-label loss ------------------------------------------------------------------------------------------------------------------------

def _c_soft_loss(logits, soft, weight):
    from point_unet_amd import _lib, runtime
    p = runtime.ptr
    B, V, C = logits.shape
    bands = []
    loss, sums = _banded((), bands), _banded((B, C, 3), bands, torch.float64)
    fn = _lib.lib().ps_softmax_dice_soft_loss
    _two_call(bands, lambda ctx, s, n: fn(ctx, p(logits), p(soft), p(weight), B, V, C, p(loss), p(sums), s, n))
    _check_bands(bands)
    return loss, sums


def _c_soft_loss_bwd(logits, soft, weight, sums, dloss=None, in_place=False):
    from point_unet_amd import _lib, runtime
    p = runtime.ptr
    B, V, C = logits.shape
    bands = []
    dlogits = _banded(logits.shape, bands)
    if in_place:
        logits = dlogits.copy_(logits)
    _lib.check(_lib.lib().ps_softmax_dice_soft_loss_bwd(_ctx().handle, p(logits), p(soft), p(weight), p(sums), p(dloss), B, V, C, p(dlogits)))
    _check_bands(bands)
    return dlogits


def _shifted(t, nbytes):
    """t's values in memory `nbytes` past a 256-byte boundary."""
    buf = torch.empty((t.numel() * 4 + 256,), dtype=torch.uint8, device="cuda")
    out = buf[nbytes:nbytes + t.numel() * 4].view(torch.float32).reshape(t.shape)
    return out.copy_(t)


@pytest.mark.parametrize("V, C", [(1, 2), (5, 2), (4097, 2), (9001, 4), (300, 16), (4500, 3)])
def test_soft_loss_on_one_hot_rows_is_byte_equal_to_the_hard_label_op(V, C):
    logits, labels, weight = (_cuda(a) for a in loss_inputs(V, C))
    soft = torch.nn.functional.one_hot(labels.long(), C).to(torch.float32)
    dl = torch.tensor(0.75, dtype=torch.float32, device="cuda")
    for w in (weight, None):
        loss, sums = _c_loss(logits, labels, w)
        sloss, ssums = _c_soft_loss(logits, soft, w)
        assert torch.equal(sloss, loss) and torch.equal(ssums, sums)
        want = _c_loss_bwd(logits, labels, w, sums, dl)
        assert torch.equal(_c_soft_loss_bwd(logits, soft, w, ssums, dl), want)
        # soft rows that are not 16- or 8-byte aligned are read a float at a time: the same values
        for nbytes in (4, 8):
            moved = _shifted(soft, nbytes)
            l2, s2 = _c_soft_loss(logits, moved, w)
            assert torch.equal(l2, loss) and torch.equal(s2, sums) and torch.equal(_c_soft_loss_bwd(logits, moved, w, s2, dl), want)


def soft_inputs(V, C, B=2, kind="plain"):
    """loss_inputs' logits and weight; the rows are convex mixes of two one-hots, as the sampler makes them (one gamma per sample)."""
    logits, labels, weight = loss_inputs(V, C, B, kind if kind in ("no weight", "zero weights", "saturated") else "plain")
    rng = np.random.default_rng(7 * V + C)
    other = rng.integers(0, C, (B, V))
    gamma = (0.34029683942911143, 0.77, 0.5)
    soft = np.stack([ref.mix(ref.one_hot(labels[b], C), ref.one_hot(other[b], C), gamma[b % 3]) for b in range(B)])
    assert soft.dtype == np.float32 and (V < 100 or ((soft > 0) & (soft < 1)).any())
    return logits, soft, weight


def soft_reference(inputs, dloss, dt):
    logits, soft, weight = inputs
    z = torch.from_numpy(logits).to(dt).requires_grad_()
    loss = ref.soft_dice_loss(z, torch.from_numpy(soft), None if weight is None else torch.from_numpy(weight).to(dt))
    (g,) = torch.autograd.grad(loss, z, torch.tensor(dloss, dtype=dt))
    return dict(loss=_np(loss), dlogits=_np(g))


def _soft_case(V, C, kind="plain", dloss=0.75):
    """test_gpu_saliency_train._loss_case on soft labels."""
    inputs = soft_inputs(V, C, kind=kind)
    logits, soft, weight = (_cuda(a) for a in inputs)
    loss, sums = _c_soft_loss(logits, soft, weight)
    dl = torch.tensor(dloss, dtype=torch.float32, device="cuda")
    got = dict(loss=loss, dlogits=_c_soft_loss_bwd(logits, soft, weight, sums, dl))
    want64, want32 = soft_reference(inputs, dloss, F64), soft_reference(inputs, dloss, F32)
    for k in want64:
        _bar(_np(got[k]), want64[k], want32[k], "soft dice V=%d C=%d %s: %s" % (V, C, kind, k))
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(got["dlogits"]).all()) and bool(torch.isfinite(sums).all())
    # dlogits is logits (in place); dloss NULL is 1; the Python wrappers take the float32 rows for soft labels; a second run
    assert torch.equal(_c_soft_loss_bwd(logits, soft, weight, sums, dl, in_place=True), got["dlogits"])
    one = torch.ones((), device="cuda")
    assert torch.equal(_c_soft_loss_bwd(logits, soft, weight, sums, None), _c_soft_loss_bwd(logits, soft, weight, sums, one))
    py = _sal().softmax_dice_loss(logits, soft, weight)
    assert py[0].dim() == 0 and py[0].is_cuda and torch.equal(py[0], loss) and torch.equal(py[1], sums)
    assert torch.equal(_sal().softmax_dice_loss_backward(logits, soft, weight, sums, dl), got["dlogits"])
    return inputs, got


# (the last four: 49 and 113 slabs per sample)
@pytest.mark.parametrize("V, C", [(1, 2), (5, 2), (4097, 2), (9001, 4), (300, 16), (4500, 3), (196609, 2), (196609, 4), (458753, 2), (458753, 4)])
def test_soft_loss_values(V, C):
    _soft_case(V, C)


def test_soft_loss_without_a_weight():
    _soft_case(4500, 3, "no weight")
    _soft_case(301, 2, "no weight")


def test_soft_loss_all_weights_zero():
    for V, C in ((4500, 3), (301, 2)):
        _, got = _soft_case(V, C, "zero weights")
        assert float(got["loss"]) == 1.0 and not bool(got["dlogits"].any())


def test_soft_loss_saturated_logits():
    for V, C in ((4500, 3), (301, 2), (64, 4)):
        _, got = _soft_case(V, C, "saturated")
        assert not bool(got["dlogits"][:, :V // 2].any())  # p exactly 0 or 1: exactly no gradient
        assert bool(got["dlogits"][:, V // 2:].any())


def test_soft_loss_autograd_function_and_python_argument_errors():
    sal = _sal()
    logits, soft, weight = (_cuda(a) for a in soft_inputs(300, 2))
    z = logits.clone().requires_grad_()
    loss = sal.differentiable_softmax_dice_loss(z, soft, weight)
    assert loss.dim() == 0 and loss.is_cuda
    (loss * 0.75).backward()  # the upstream gradient reaches the kernel as a device pointer
    _, sums = sal.softmax_dice_loss(logits, soft, weight)
    assert torch.equal(z.grad, sal.softmax_dice_loss_backward(logits, soft, weight, sums, torch.tensor(0.75, device="cuda")))
    # int32 labels behave as before; any other dtype or size raises
    hard = torch.zeros((2, 300), dtype=torch.int32, device="cuda")
    assert sal.softmax_dice_loss(logits, hard, weight)[1].shape == (2, 2, 3)
    for labels in (hard.long(), soft.double(), soft[:, :, 0].contiguous(), torch.zeros((2, 300, 2), dtype=torch.int32, device="cuda"), soft.cpu()):
        with pytest.raises(ValueError, match="labels"):
            sal.softmax_dice_loss(logits, labels, weight)
        with pytest.raises(ValueError, match="labels"):
            sal.softmax_dice_loss_backward(logits, labels, weight, sums)


# ---- the step on soft labels ----------------------------------------------------------------------------------------------------------------------

def _c_backward_soft(params, x, soft, weight, cin, classes):
    """ps_saliency_backward_soft called directly on banded buffers: (loss, logits, flat gradients, scratch bytes)."""
    from point_unet_amd import _lib
    flat = _cuda(_sal().flatten_params(params, cin, classes))
    B, D, H, W, _ = x.shape
    bands = []
    grads, loss, logits = _banded((flat.numel(),), bands), _banded((), bands), _banded((B, D, H, W, classes), bands)
    fn = _lib.lib().ps_saliency_backward_soft
    call = lambda ctx, s, n: fn(ctx, _ptr(x), _ptr(soft), _ptr(weight), B, D, H, W, cin, classes, _ptr(flat), flat.numel(), _ptr(grads), _ptr(loss),
                                _ptr(logits), s, n)
    need = ctypes.c_int64(0)
    _lib.check(call(None, None, ctypes.byref(need)))
    scratch = _banded((need.value,), bands, torch.uint8)
    _lib.check(call(_ctx().handle, _ptr(scratch), ctypes.byref(need)))
    _check_bands(bands)
    return loss, logits, grads, need.value


def _soft_graph_inputs(shape):
    params, x, labels, weight = graph_inputs(shape, seed=4)
    rng = np.random.default_rng(shape[1])
    other = rng.integers(0, 2, shape)
    soft = np.stack([ref.mix(ref.one_hot(labels[b], 2), ref.one_hot(other[b], 2), (0.34029683942911143, 0.77)[b % 2]) for b in range(shape[0])])
    return params, x, labels, weight, soft


def _soft_reference_graph(params, x, soft, weight, masks, dt):
    P = tref.leaves(params, dt)
    logits = tref.graph(P, torch.from_numpy(x).to(dt), masks)
    loss = ref.soft_dice_loss(logits, torch.from_numpy(soft), torch.from_numpy(weight).to(dt))
    grads = torch.autograd.grad(loss, list(P.values()))
    return {k: _np(g) for k, g in zip(P, grads)}


@functools.lru_cache(maxsize=None)
def _step_case(shape):
    """The op-by-op path and the one call on soft labels at `shape`, and the two CPU references of the gradients, once per session."""
    params, x, labels, weight, soft = _soft_graph_inputs(shape)
    net = _sal().TrainableSaliencyNet(params, 1, 2)
    masks = {}
    logits = net.logits(_cuda(x), masks)
    loss = _sal().differentiable_softmax_dice_loss(logits, _cuda(soft), _cuda(weight))
    loss.backward()
    grads = {n: p.grad for n, p in net.named_parameters()}
    native = _c_backward_soft(params, _cuda(x), _cuda(soft), _cuda(weight), 1, 2)
    want64, want32 = (_soft_reference_graph(params, x, soft, weight, masks, dt) for dt in (F64, F32))
    return (params, x, labels, weight, soft), (loss.detach(), logits.detach(), grads), native, want64, want32


STEP_SHAPES = [(1, 16, 16, 16), (2, 32, 16, 16)]


@pytest.mark.parametrize("shape", STEP_SHAPES, ids=["1x16x16x16", "2x32x16x16"])
def test_backward_soft_on_one_hot_labels_is_the_hard_label_backward(shape):
    params, x, labels, weight = graph_inputs(shape, seed=4)
    xd, wd = _cuda(x), _cuda(weight)
    hard = _c_backward(params, xd, _cuda(labels), wd, 1, 2)
    soft = _c_backward_soft(params, xd, _cuda(ref.one_hot(labels, 2)), wd, 1, 2)
    assert torch.equal(soft[0], hard[0]) and torch.equal(soft[1], hard[1]) and torch.equal(soft[2], hard[2]) and soft[3] == hard[3]


@pytest.mark.parametrize("shape", STEP_SHAPES, ids=["1x16x16x16", "2x32x16x16"])
def test_backward_soft_against_the_op_by_op_path(shape):
    (params, x, labels, weight, soft), (loss, logits, grads), native, want64, want32 = _step_case(shape)
    nloss, nlogits, flat, need = native
    assert torch.equal(nloss, loss) and torch.equal(nlogits, logits)
    got = _by_name(flat, 1, 2)
    assert len(got) == 158 and list(got) == list(grads)
    for n in got:
        _bar_between(_np(got[n]), _np(grads[n]), want64[n], want32[n], "soft labels: d %s" % n)
    again = _c_backward_soft(params, _cuda(x), _cuda(soft), _cuda(weight), 1, 2)
    assert all(torch.equal(a, b) for a, b in zip(again[:3], native[:3])) and again[3] == need
    # the Python surface: TrainableSaliencyNet.loss and SaliencyTrainer.backward take the soft rows
    tr = _sal().SaliencyTrainer(params, 1, 2)
    ploss, plogits = tr.backward(_cuda(x), _cuda(soft), _cuda(weight), want_logits=True)
    assert torch.equal(ploss, nloss) and torch.equal(plogits, nlogits) and torch.equal(tr.grad, flat)
    assert torch.equal(_sal().TrainableSaliencyNet(params, 1, 2).loss(_cuda(x), _cuda(soft), _cuda(weight)).detach(), loss)


@pytest.mark.parametrize("shape", STEP_SHAPES, ids=["1x16x16x16", "2x32x16x16"])
def test_train_step_soft_is_backward_soft_and_the_update(shape):
    params, x, labels, weight, soft = _soft_graph_inputs(shape)
    xd, sd, wd = _cuda(x), _cuda(soft), _cuda(weight)
    one, two = _sal().SaliencyTrainer(params, 1, 2), _sal().SaliencyTrainer(params, 1, 2)
    for _ in range(2):
        a = one.step(xd, sd, wd, 0.01).clone()
        b = two.backward(xd, sd, wd).clone()
        two.update(0.01)
        assert torch.equal(a, b) and torch.equal(one.grad, two.grad)
    assert torch.equal(one.flat, two.flat) and torch.equal(one.accum, two.accum) and bool(one.accum.any())


# ---- train_saliency(mixup=...) ----------------------------------------------------------------------------------------------------------------------

P16 = (16, 16, 16)


@functools.lru_cache(maxsize=None)
def _train_bank():
    return tdata._pancreas_bank(((20, 24, 18), (16, 16, 16), (18, 20, 22), (17, 19, 21)), seed=9)


def _train(engine, mixup, steps=3):
    sal, bank = _sal(), _train_bank()
    params = sal.init_params(1, 2, seed=5)
    net = sal.SaliencyTrainer(params, 1, 2) if engine == "native" else sal.TrainableSaliencyNet(params, 1, 2)
    losses = _sd().train_saliency(net, bank, steps, P16, batch_size=2, lr=0.01, seed=3, engine=engine, mixup=mixup)
    flat = net.flat.clone() if engine == "native" else torch.cat([p.detach().reshape(-1) for p in net.parameters()])
    return losses, flat


@pytest.mark.parametrize("engine", ["autograd", "native"])
def test_train_saliency_with_mixup(engine):
    losses, flat = _train(engine, 2)
    assert isinstance(losses, torch.Tensor) and losses.is_cuda and tuple(losses.shape) == (3,)
    assert bool(torch.isfinite(losses).all()) and bool(torch.isfinite(flat).all()) and 0 < float(losses.min()) and float(losses.max()) <= 1
    again, flat2 = _train(engine, 2)
    assert torch.equal(again, losses) and torch.equal(flat2, flat)  # the same seed: the same bytes
    # the batches are the mixed ones of epoch_batches: B + 1 = 3 of the four volumes per batch, one batch per epoch
    bank = _train_bank()
    (_, cand, s), = _sd().epoch_plan(4, 3, 0, seed=3, tries=8)
    batch = bank.sample(cand, P16, s, "one_positive", mixup=2)
    first, = list(bank.epoch_batches(2, P16, 0, 3, mixup=2))
    assert all(torch.equal(batch[k], first[k]) for k in ("images", "weights", "labels", "info")) and tuple(batch["labels"].shape) == (2,) + P16 + (2,)
    assert bool(((batch["labels"] > 0) & (batch["labels"] < 1)).any())  # genuinely soft rows
    with pytest.raises(ValueError, match="mixup"):
        _sd().train_saliency(_sal().SaliencyTrainer(_sal().init_params(1, 2, seed=5), 1, 2), bank, 1, P16, engine="native", mixup=3)


def test_train_saliency_with_mixup_engines_agree_on_the_first_step():
    assert torch.equal(_train("autograd", 2, steps=1)[0], _train("native", 2, steps=1)[0])


def test_train_saliency_without_mixup_is_unchanged():
    """mixup=None: both engines return what the unchanged call path -- epoch_plan, sample without the keyword, the loss or the step on int32
    labels -- gives, written out by hand."""
    sal, sd, bank = _sal(), _sd(), _train_bank()
    params = sal.init_params(1, 2, seed=5)
    batches = []
    for epoch in range(2):  # four volumes, batches of two: two batches per epoch
        for _, cand, s in sd.epoch_plan(4, 2, epoch, seed=3, tries=8):
            batches.append(bank.sample(cand, P16, s, "one_positive"))
    assert batches[0]["labels"].dtype == torch.int32 and set(batches[0]) == {"images", "weights", "labels", "info"}
    hand = sal.SaliencyTrainer(params, 1, 2)
    native = [hand.step(b["images"], b["labels"], b["weights"], 0.01).clone() for b in batches[:3]]
    losses, flat = _train("native", None)
    assert torch.equal(losses, torch.stack(native)) and torch.equal(flat, hand.flat)
    net = sal.TrainableSaliencyNet(params, 1, 2)
    opt = sal.reference_optimizer(net, lr=0.01)
    auto = []
    for b in batches[:3]:
        opt.zero_grad(set_to_none=True)
        loss = net.loss(b["images"], b["labels"], b["weights"])
        loss.backward()
        opt.step()
        auto.append(loss.detach())
    losses, flat = _train("autograd", None)
    assert torch.equal(losses, torch.stack(auto)) and torch.equal(flat, torch.cat([p.detach().reshape(-1) for p in net.parameters()]))
