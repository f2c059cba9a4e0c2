"""The point network's Dice losses and its step accuracy (include/pointseg_train_loss.h) on the GPU, against tests/point_loss_ref.py.

Op values: the bar is test_gpu_saliency.py's rule (`_bar`), per result: 4 x the error of the same computation in torch-CPU float32 against
float64, plus 1e-6 of the largest expected value.  The kernels hold their sums and coefficients in float64 and round once, so they sit well
inside it (the float32 restatement's relative gradient error on these inputs is about 1.5e-7, its loss error below 1e-7).  Counts and the
accuracy are exact.  The trainer tests use tests/test_gpu_train.py's own case and bars: loss relative 1e-5, logits 1e-4, every gradient
within 2e-3 of its own scale plus 2e-5 of the global scale; the data-parallel test the pattern and bars of
test_sync_bn_ranks_equal_one_rank_with_the_batch."""
import ctypes
import functools
import os

import numpy as np
import pytest

import netcase
import point_loss_ref as pref
from test_gpu_saliency import _bar

pytestmark = pytest.mark.gpu

ROWS = (1, 63, 64, 65, 257, 4095, 4096, 4097, 8193, 70001)  # a wave, a workgroup, one and two slabs (4096 rows), many slabs
CLASSES = (2, 4, 3, 5, 13, 16)                               # the 8-byte, the 16-byte and the scalar row modes, the register bound


def _weights(C):
    return np.linspace(4.0, 1.0, C).astype(np.float32)


def _inputs(R, C, ignored=0.0, scale=1.0, seed=None):
    rng = np.random.default_rng(1000 * C + R if seed is None else seed)
    z = (rng.standard_normal((R, C)) * scale).astype(np.float32)
    y = rng.integers(0, C, R).astype(np.int32)
    if ignored:
        y[rng.random(R) < ignored] = -1
    return z, y


@functools.lru_cache(maxsize=None)
def _expected(R, C, kind, ignored=0.0, scale=1.0):
    """(loss, gradient) in float64 and in torch-CPU float32, the sums and the counts: computed once per case, shared, left unchanged"""
    import torch
    z, y = _inputs(R, C, ignored, scale)
    w64 = pref.loss_and_grad(kind, z, y, _weights(C))
    w32 = pref.loss_and_grad(kind, z, y, _weights(C), dtype=torch.float32)
    return w64, w32, pref.sums_of(z, y)


def _p(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


def _check(kind, R, C, got, ignored=0.0, scale=1.0, what=""):
    (loss64, grad64), (loss32, grad32), sums = _expected(R, C, kind, ignored, scale)
    loss, acc, dlogits, dsums = got
    tag = "%s R=%d C=%d %s" % (kind, R, C, what)
    _bar(np.asarray(loss.cpu().numpy(), np.float32), np.asarray(loss64), np.asarray(loss32), tag + ": loss")
    _bar(dlogits.cpu().numpy(), grad64, grad32, tag + ": dlogits")
    s = dsums.cpu().numpy()
    assert np.array_equal(s[3 * C:], sums[3 * C:]), (tag, s[3 * C:], sums[3 * C:])  # n_valid, n_correct: exact
    assert np.array_equal(s[2:3 * C:3], sums[2:3 * C:3]), tag                        # S2: exact integers
    big = max(1.0, float(np.abs(sums[:3 * C]).max()))
    assert np.abs(s[:3 * C] - sums[:3 * C]).max() <= 1e-12 * big, tag                # S0, S1: float64 sums in another order
    n, k = int(sums[3 * C]), int(sums[3 * C + 1])
    assert acc.dtype.is_floating_point and float(acc) == (np.float32(k / n) if n else 0.0), tag


# ---- op values ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("C", CLASSES)
@pytest.mark.parametrize("R", ROWS)
def test_dice_values_against_float64(R, C):
    import torch
    from point_unet_amd.train import point_loss
    z, y = _inputs(R, C)
    dz, dy = torch.from_numpy(z).cuda(), torch.from_numpy(y).cuda()
    for kind in pref.KINDS:
        _check(kind, R, C, point_loss(dz, dy, kind, _weights(C)))


@pytest.mark.parametrize("C", [2, 4])
def test_a_logits_pointer_offset_by_one_float_takes_the_scalar_mode(C):
    import torch
    from point_unet_amd.train import point_loss
    R = 4097
    z, y = _inputs(R, C)
    buf = torch.zeros(R * C + 4, dtype=torch.float32, device="cuda")
    off = buf[1:1 + R * C].view(R, C)
    off.copy_(torch.from_numpy(z))
    assert off.data_ptr() % 8 == 4
    dy = torch.from_numpy(y).cuda()
    for kind in pref.KINDS:
        got = point_loss(off, dy, kind, _weights(C))
        _check(kind, R, C, got, what="offset pointer")
        ali = point_loss(torch.from_numpy(z).cuda(), dy, kind, _weights(C))
        for a, b in zip(got, ali):  # the vector mode moves the same values: the same bytes
            assert torch.equal(a, b)


@pytest.mark.parametrize("C", [2, 4, 5])
def test_dlogits_may_be_the_logits(lib, C):
    import torch
    from point_unet_amd import runtime
    R = 8193
    z, y = _inputs(R, C)
    h = runtime.default_context(0).handle
    runtime.default_context(0).use_torch_stream()
    dz, dy = torch.from_numpy(z).cuda(), torch.from_numpy(y).cuda()
    cw = torch.from_numpy(_weights(C)).cuda()
    sums = torch.empty(3 * C + 2, dtype=torch.float64, device="cuda")
    loss = torch.zeros((), dtype=torch.float32, device="cuda")
    assert lib.ps_op_dice_sums(h, _p(dz), _p(dy), R, C, _p(sums)) == 0
    assert lib.ps_op_dice_from_sums(h, 2, _p(dz), _p(dy), _p(cw), _p(sums), 1.0, R, C, _p(loss), _p(dz)) == 0
    acc = (sums[-1] / sums[-2]).float()
    _check("dice_weighted", R, C, (loss, acc, dz, sums), what="in place")


@pytest.mark.parametrize("what,ignored,scale", [("a third ignored", 1 / 3, 1.0), ("everything ignored", 1.0, 1.0), ("logits of 1e4", 0.0, 1e4)])
@pytest.mark.parametrize("R,C", [(4097, 4), (257, 2), (8193, 13)])
def test_edge_inputs(R, C, what, ignored, scale):
    import torch
    from point_unet_amd.train import point_loss
    z, y = _inputs(R, C, ignored, scale)
    if ignored == 1.0:
        assert (y < 0).all()
        z[::7] = np.inf  # (an ignored row's logits are never read into a sum or a gradient)
    dz, dy = torch.from_numpy(z).cuda(), torch.from_numpy(y).cuda()
    for kind in pref.KINDS:
        got = point_loss(dz, dy, kind, _weights(C))
        if ignored == 1.0:
            assert float(got[0]) == 1.0 and float(got[1]) == 0.0 and not got[2].any() and not got[3].any()
        else:
            _check(kind, R, C, got, ignored, scale, what)
            assert not got[2][dy < 0].any()


def test_loss_alone_and_gradient_alone(lib):
    import torch
    from point_unet_amd import runtime
    from point_unet_amd.train import point_loss
    R, C = 4097, 4
    z, y = _inputs(R, C)
    dz, dy = torch.from_numpy(z).cuda(), torch.from_numpy(y).cuda()
    want = point_loss(dz, dy, "dice", None)
    h = runtime.default_context(0).handle
    loss = torch.full((), 7.0, dtype=torch.float32, device="cuda")
    dl = torch.full_like(dz, 7.0)
    assert lib.ps_op_dice_from_sums(h, 1, _p(dz), _p(dy), None, _p(want[3]), 1.0, R, C, _p(loss), None) == 0
    assert lib.ps_op_dice_from_sums(h, 1, _p(dz), _p(dy), None, _p(want[3]), 1.0, R, C, None, _p(dl)) == 0
    assert torch.equal(loss, want[0]) and torch.equal(dl, want[2])


def test_two_runs_give_the_same_bytes():
    import torch
    from point_unet_amd.train import point_loss
    for R, C in ((70001, 4), (8193, 13)):
        z, y = _inputs(R, C, ignored=0.2)
        dz, dy = torch.from_numpy(z).cuda(), torch.from_numpy(y).cuda()
        for kind in pref.KINDS:
            a, b = point_loss(dz, dy, kind, _weights(C)), point_loss(dz, dy, kind, _weights(C))
            for u, v in zip(a, b):
                assert torch.equal(u, v)


@pytest.mark.parametrize("kind", pref.KINDS)
@pytest.mark.parametrize("R,C", [(8193, 4), (4097, 5)])
def test_split_rows_rule_of_the_collective(lib, R, C, kind):
    """What the trainer does with shared statistics: the sums of the two halves added, the from-sums pass with grad_scale = 2 on each half --
    the loss is the unsplit one, the gradients 2 x the rows of the unsplit call."""
    import torch
    from point_unet_amd import runtime
    from point_unet_amd.train import point_loss
    z, y = _inputs(R, C)
    (loss64, grad64), (loss32, grad32), _ = _expected(R, C, kind)
    dz, dy = torch.from_numpy(z).cuda(), torch.from_numpy(y).cuda()
    cw = torch.from_numpy(_weights(C)).cuda()
    h = runtime.default_context(0).handle
    half = R // 2
    parts = [(dz[:half].contiguous(), dy[:half].contiguous()), (dz[half:].contiguous(), dy[half:].contiguous())]
    sums = []
    for zz, yy in parts:
        s = torch.empty(3 * C + 2, dtype=torch.float64, device="cuda")
        assert lib.ps_op_dice_sums(h, _p(zz), _p(yy), zz.shape[0], C, _p(s)) == 0
        sums.append(s.cpu())
    total = sums[0].clone()
    total[:3 * C] += sums[1][:3 * C]  # (on the host, as an all-reduce would)
    total = total.cuda()
    grads = []
    for zz, yy in parts:
        loss = torch.zeros((), dtype=torch.float32, device="cuda")
        dl = torch.empty_like(zz)
        assert lib.ps_op_dice_from_sums(h, 1 if kind == "dice" else 2, _p(zz), _p(yy), _p(cw), _p(total), 2.0, zz.shape[0], C, _p(loss), _p(dl)) == 0
        _bar(np.asarray(loss.cpu().numpy()), np.asarray(loss64), np.asarray(loss32), "%s split R=%d C=%d: loss" % (kind, R, C))
        grads.append(dl.cpu().numpy())
    _bar(np.concatenate(grads), 2 * grad64, 2 * grad32, "%s split R=%d C=%d: dlogits" % (kind, R, C))
    assert int(sums[0][3 * C] + sums[1][3 * C]) == R


def test_accuracy_is_the_numpy_rule_exactly(lib):
    import torch
    from point_unet_amd.train import point_loss
    for R, C in ((4097, 4), (70001, 13), (257, 2), (300, 40)):
        rng = np.random.default_rng(R)
        z = np.round(rng.standard_normal((R, C)) * 2).astype(np.float32) / 2  # (coarse values: many ties)
        y = rng.integers(-1, C, R).astype(np.int32)
        z[1, :] = 0.5                      # a constructed tie of all classes: correct
        y[1] = C - 1
        z[2, y[2] if y[2] >= 0 else 0] = np.nan  # a NaN target: never correct
        y[2] = max(y[2], 0)
        z[3, :] = -1.0
        z[3, 0] = np.nan                   # a NaN elsewhere is not larger
        y[3] = 1
        n, k = pref.top1_counts(z, y)
        assert 0 < k < n
        dz, dy = torch.from_numpy(z).cuda(), torch.from_numpy(y).cuda()
        kinds = ("ce",) if C > 16 else ("ce", "dice")
        for kind in kinds:
            loss, acc, _, sums = point_loss(dz, dy, kind)
            assert sums[-2:].cpu().tolist() == [n, k], (kind, R, C)
            assert acc.dtype == torch.float32 and float(acc) == float(pref.accuracy(z, y)), (kind, R, C)


# ---- the trainer ---------------------------------------------------------------------------------------------------------------------------

def _train_case():
    cfg, xyz, feats = netcase.small_deep(1500, seed=2, B=2)
    cfg.d_out = [16, 32, 64, 32, 16]
    return cfg, xyz, feats


def _check_step(tr, loss, want, red_labels):
    assert abs(float(loss) - want["loss"]) <= 1e-5 * max(1.0, abs(want["loss"])), (float(loss), want["loss"])
    logits = tr.last_logits.cpu().numpy()
    assert np.abs(logits.reshape(want["logits"].shape) - want["logits"]).max() < 1e-4
    gscale = max(np.abs(g).max() for g in want["grads"].values())
    worst = []
    for name in tr.names:
        got, ref = tr.G[name].cpu().numpy(), want["grads"][name]
        tol = 2e-3 * np.abs(ref).max() + 2e-5 * gscale
        worst.append((float(np.abs(got - ref).max() / tol), name))
    worst.sort(reverse=True)
    print("worst gradient / tolerance:", worst[:3])
    assert worst[0][0] <= 1.0, worst[:5]
    assert float(tr.last_accuracy) == float(pref.accuracy(logits, red_labels))


@functools.lru_cache(maxsize=None)
def _yardstick(kind, ignored):
    from oracle import bindings as ob
    from oracle import randla_oracle as ro
    from point_unet_amd import weights
    cfg, xyz, feats = _train_case()
    params = weights.init_params(cfg, seed=3, randomize_bn=True)
    rng = np.random.default_rng(3)
    labels = rng.integers(0, cfg.num_classes + (1 if ignored else 0), xyz.shape[:2]).astype(np.int32)
    red = pref.reduce_labels(labels.reshape(-1), cfg.num_classes, [0] if ignored else [])
    cw = np.linspace(1.0, 2.0, cfg.num_classes).astype(np.float32)
    pts, nbr, pool, up = ro.build_pyramid(lambda s, q, k: ob.knn_batch(s, q, k), xyz, cfg.k_n, cfg.sub_sampling_ratio)
    want = pref.train_step_with_loss(kind, params, cfg.num_layers, pts, nbr, pool, up, feats, red, cw)
    return labels, red, want


@pytest.mark.parametrize("ignored", [False, True], ids=["all-labels", "ignored-label-0"])
@pytest.mark.parametrize("kind", pref.KINDS)
def test_one_training_step_matches_autograd(oracle, kind, ignored):
    import torch
    import test_gpu_train as T
    cfg, xyz, feats = _train_case()
    labels, red, want = _yardstick(kind, ignored)
    kw = dict(ignored_label_inds=[0]) if ignored else {}
    tr, pyr, _, _, _, _ = T._setup(cfg, xyz, feats, labels=labels, oracle_pyramid=False, loss=kind, **kw)
    assert tr.loss == kind
    with pytest.raises(AttributeError):
        tr.loss = "ce"
    loss = tr.train_step(pyr, torch.from_numpy(feats).cuda(), torch.from_numpy(labels).cuda())
    torch.cuda.synchronize()
    _check_step(tr, loss, want, red)
    # backward_only: the same gradients, no optimiser step
    flat = tr.flat.clone()
    tr.backward_only(pyr, torch.from_numpy(feats).cuda(), torch.from_numpy(labels).cuda())
    assert torch.equal(flat, tr.flat) and tr.last_accuracy is not None
    tr.close()


def test_python_engine_agrees_with_the_native_one(oracle):
    import torch
    import test_gpu_train as T
    cfg, xyz, feats = _train_case()
    labels, red, want = _yardstick("dice", False)
    runs = {}
    for engine in ("native", "python"):
        tr, pyr, _, _, _, _ = T._setup(cfg, xyz, feats, labels=labels, oracle_pyramid=False, loss="dice", engine=engine)
        loss = tr.train_step(pyr, torch.from_numpy(feats).cuda(), torch.from_numpy(labels).cuda())
        torch.cuda.synchronize()
        _check_step(tr, loss, want, red)
        runs[engine] = (float(loss), tr.last_logits.cpu().numpy().copy(), {n: tr.G[n].cpu().numpy().copy() for n in tr.names}, float(tr.last_accuracy))
        tr.close()
    a, b = runs["native"], runs["python"]
    assert abs(a[0] - b[0]) <= 1e-5 * max(1.0, abs(b[0]))
    assert np.abs(a[1] - b[1]).max() < 1e-4
    gscale = max(np.abs(g).max() for g in b[2].values())
    for n in b[2]:
        assert np.abs(a[2][n] - b[2][n]).max() <= 2e-3 * np.abs(b[2][n]).max() + 2e-5 * gscale, n
    assert a[3] == b[3]


def _raw_step(lib, tr, pyr, feats, labels, entry, kind=None, accuracy=None):
    """Trainer._train_step's single-rank plumbing around one of the four step entries"""
    import torch
    from point_unet_amd import _lib
    tr.ctx.use_torch_stream()
    _lib.check(lib.ps_trainer_set_collective(tr._h, _lib.PS_ALLREDUCE_FN(), None, 1, 0, 0))
    _lib.check(lib.ps_trainer_set_options(tr._h, ctypes.byref(tr._options())))
    _lib.check(lib.ps_trainer_set_step(tr._h, tr.step))
    f = feats.reshape(-1, feats.shape[-1]).contiguous()
    lab = labels.reshape(-1).to(torch.int32).contiguous()
    loss = torch.zeros(1, dtype=torch.float32, device="cuda")
    logits = torch.empty((f.shape[0], tr.cfg.num_classes), dtype=torch.float32, device="cuda")
    head = (tr._h, ctypes.byref(pyr.struct), _p(f), _p(lab), _p(tr.class_weights))
    if kind is None:
        rc = getattr(lib, entry)(*head, _p(loss), _p(logits))
    else:
        rc = getattr(lib, entry)(*head, kind, _p(loss), _p(accuracy), _p(logits))
    torch.cuda.synchronize()
    return rc, loss, logits


def test_the_old_entries_are_the_cross_entropy_calls_of_the_new(lib):
    """From equal initial state ps_randla_train_step and ps_randla_train_step_loss(PS_LOSS_CE) -- without and with the accuracy -- leave the
    same bytes: parameters, gradients, moving statistics, loss, logits.  Any other loss_kind is refused before anything runs."""
    import torch
    import test_gpu_train as T
    cfg, xyz, feats = _train_case()
    d_feats = torch.from_numpy(feats).cuda()
    out = []
    for entry, kind, with_acc in (("ps_randla_train_step", None, False), ("ps_randla_train_step_loss", 0, False), ("ps_randla_train_step_loss", 0, True)):
        tr, pyr, _, labels, _, _ = T._setup(cfg, xyz, feats, oracle_pyramid=False)
        d_lab = torch.from_numpy(labels).cuda()
        acc = torch.full((), -1.0, dtype=torch.float32, device="cuda") if with_acc else None
        if kind is not None:
            before = tr.flat.clone()
            for bad in (3, -1):
                rc, _, _ = _raw_step(lib, tr, pyr, d_feats, d_lab, entry, bad, acc)
                assert rc == 1 and b"loss_kind" in lib.ps_last_error()
            assert torch.equal(before, tr.flat)
        rc, loss, logits = _raw_step(lib, tr, pyr, d_feats, d_lab, entry, kind, acc)
        assert rc == 0
        out.append((tr.flat.clone(), tr.grad.clone(), tr.flat_buffers.clone(), loss, logits))
        if with_acc:
            assert float(acc) == float(pref.accuracy(logits.cpu().numpy(), labels.reshape(-1)))
        tr.close()
    for other in out[1:]:
        for a, b in zip(out[0], other):
            assert torch.equal(a, b)


def test_two_ranks_with_shared_statistics_equal_one_rank_with_the_batch(tmp_path):
    """test_gpu_train.py's sync_bn test under loss="dice_weighted": two gloo ranks on this one GPU, one cloud each, against one rank with
    the batch of two -- the ONE Dice over both clouds.  With shared statistics the step makes exactly one more all-reduce call than the
    cross-entropy step, of 8 * 3 C more bytes; without them exactly one.  (The parent and the two workers: 3 processes on the GPU.)"""
    import socket
    import subprocess
    import sys
    import torch
    import test_gpu_train as T
    world, kind = 2, "dice_weighted"
    cfg, xyz, feats = T.syncbn_case(world)
    labels = T.syncbn_labels(cfg, xyz)
    tr, pyr, _, _, _, _ = T._setup(cfg, xyz, feats, labels=labels, oracle_pyramid=False, loss=kind)
    loss = tr.train_step(pyr, torch.from_numpy(feats).cuda(), torch.from_numpy(labels).cuda())
    torch.cuda.synchronize()
    want_grad, want_loss = tr.grad.cpu().numpy(), float(loss)
    tr.close()
    del tr, pyr
    torch.cuda.empty_cache()
    out = str(tmp_path / "dice")
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "point_loss_worker.py")
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, worker, out, kind], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    logs = [p.communicate(timeout=900)[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(l[-2000:] for l in logs)
    got = [np.load(out + ".rank%d.npz" % r) for r in range(world)]
    gscale = np.abs(want_grad).max()
    for g in got:
        diff = g["grad"] - want_grad
        print("gradient: relative L2 %.3e, max entry %.3e of the scale; loss %.8f against %.8f"
              % (np.linalg.norm(diff) / np.linalg.norm(want_grad), np.abs(diff).max() / gscale, float(g["loss"]), want_loss))
        assert np.linalg.norm(diff) <= 2e-3 * np.linalg.norm(want_grad)
        assert np.abs(diff).max() <= 2e-2 * gscale
        assert abs(float(g["loss"]) - want_loss) <= 1e-5 * max(1.0, abs(want_loss))  # every rank returns the one loss
    assert np.array_equal(got[0]["grad"], got[1]["grad"]) and np.array_equal(got[0]["flat"], got[1]["flat"])
    assert float(got[0]["loss"]) == float(got[1]["loss"])
    C = cfg.num_classes
    for r, g in enumerate(got):
        assert int(g["calls_ce"]) == 74
        assert int(g["calls_dice"]) == int(g["calls_ce"]) + 1 and int(g["bytes_dice"]) == int(g["bytes_ce"]) + 8 * 3 * C
        assert int(g["calls_local"]) == 1 and int(g["bytes_local"]) == 4 * want_grad.size
        # the accuracy is the rank's own
        assert float(g["accuracy"]) == float(pref.accuracy(g["logits"], labels[r].reshape(-1)))
