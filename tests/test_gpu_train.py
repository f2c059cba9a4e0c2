"""GPU parity of the training step (BASELINE configs 3/4 path): forward in training mode, class-weighted CE, backward
and one Adam step on the HIP tape vs the torch-CPU float64 autograd restatement (oracle/randla_train_oracle.py).
Bars: loss relative 1e-5; every gradient max-abs error <= 2e-3 of that gradient's max magnitude (fp32 vs float64);
updated parameters after one Adam step."""
import numpy as np
import pytest

import netcase

pytestmark = pytest.mark.gpu


def _setup(cfg, xyz, feats, seed=3, lr=1e-3, keep_prob=1.0, labels=None, sync_bn=False, oracle_pyramid=True, mlp_dtype="fp32", **trainer_kw):
    import torch
    from oracle import bindings as ob
    from oracle import randla_oracle as ro
    from point_unet_amd import weights
    from point_unet_amd.pyramid import build_pyramid
    from point_unet_amd.train import Trainer
    params = weights.init_params(cfg, seed=seed, randomize_bn=True)
    rng = np.random.default_rng(seed)
    if labels is None:
        labels = rng.integers(0, cfg.num_classes, xyz.shape[:2]).astype(np.int32)
    cw = np.linspace(1.0, 2.0, cfg.num_classes).astype(np.float32)
    tr = Trainer(cfg, params=params, learning_rate=lr, class_weights=cw, keep_prob=keep_prob, sync_bn=sync_bn, mlp_dtype=mlp_dtype, **trainer_kw)
    pyr = build_pyramid(torch.from_numpy(xyz).cuda(), cfg)
    host_pyr = None
    if oracle_pyramid:
        host_pyr = ro.build_pyramid(lambda s, q, k: ob.knn_batch(s, q, k), xyz, cfg.k_n, cfg.sub_sampling_ratio)
    return tr, pyr, params, labels, cw, host_pyr


def syncbn_case(B=2):
    # 12000 points: the deepest level still has more points (23) than K, so no BatchNorm column is constant over its rows
    # (a constant column puts every row of it exactly on the leaky-ReLU kink, where the summation order decides the branch)
    cfg, xyz, feats = netcase.small_deep(12000, seed=8, B=B)
    cfg.d_out = [16, 32, 64, 32, 16]
    return cfg, xyz, feats


def syncbn_labels(cfg, xyz):
    return np.random.default_rng(11).integers(0, cfg.num_classes, xyz.shape[:2]).astype(np.int32)


@pytest.mark.parametrize("world,merged,op_by_op", [(2, True, False), (8, True, False), (2, False, False), (2, True, True)],
                         ids=["2", "8", "2-unmerged", "2-opbyop"])
def test_sync_bn_ranks_equal_one_rank_with_the_batch(tmp_path, world, merged, op_by_op):
    """BASELINE configs[3] semantics: `world` ranks with one cloud each and shared BatchNorm statistics take the same
    optimisation step as one rank with the batch of `world` clouds -- at 2 and at the 8 ranks of the node configs[3] names.  The ranks are
    processes on this one GPU joined by gloo (the collective is backend-agnostic; RCCL carries it on the 8-GPU node).  Also asserted at
    that world size: the number of all-reduce calls a step makes (ps_trainer_collective_stats) -- one for the flat gradient buffer plus
    two per BatchNorm layer with shared statistics (89 for the five-layer network's 44 layers) MINUS the merged ones: the independent
    pairs share a call (mlp2 || shortcut in both directions, mlp1 || LocSE-mlp1 forward: 15 calls less, 74) --, exactly one with per-GPU
    statistics.  Unmerged (the worker sets train_merge_syncbn = 0 on its context before its trainer is created): the same step, 89 calls.
    Op by op (fused_locse=False on the one-rank trainer and on the workers): the LocSE convolution as GEMM + BatchNorm, whose sums share
    ONE float all-reduce with mlp1's -- the pair saves the same forward call per level as the fused form, so 74 again."""
    import os
    import subprocess
    import sys
    import torch
    cfg, xyz, feats = syncbn_case(world)
    labels = syncbn_labels(cfg, xyz)
    trainer_kw = {"fused_locse": False} if op_by_op else {}
    tr, pyr, params, _, cw, _ = _setup(cfg, xyz, feats, labels=labels, oracle_pyramid=False, **trainer_kw)
    loss = tr.train_step(pyr, torch.from_numpy(feats).cuda(), torch.from_numpy(labels).cuda())
    torch.cuda.synchronize()
    want_grad, want_flat, want_loss = tr.grad.cpu().numpy(), tr.flat.cpu().numpy(), float(loss)
    n_bn = sum(1 for name in tr.names if name.endswith("gamma"))
    del tr, pyr
    torch.cuda.empty_cache()
    out = str(tmp_path / "syncbn")
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "syncbn_worker.py")
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    flags = ([] if merged else ["--unmerged"]) + (["--op-by-op"] if op_by_op else [])
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, worker, out] + flags, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    logs = [p.communicate(timeout=900)[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(l[-2000:] for l in logs)
    got = [np.load(out + ".rank%d.npz" % r) for r in range(world)]
    gscale = np.abs(want_grad).max()
    # every rank holds the same averaged gradient and takes the same Adam step.  The two runs sum the statistics in a different
    # order (per-rank partials first), which moves a handful of activations that sit within an ulp of a leaky-ReLU kink to the
    # other side -- a discontinuity of the gradient: single entries move by 2e-4..5e-3 of the gradient scale depending on which
    # activations happen to sit on a kink.  So the bar is on the whole vector (relative L2 <= 2e-3) with a loose cap on single
    # entries (2e-2 of the scale); a wrong row count or a missing reduction shows up at 1e-1 in both.
    for g in got:
        diff = g["grad"] - want_grad
        assert np.linalg.norm(diff) <= 2e-3 * np.linalg.norm(want_grad), np.linalg.norm(diff) / np.linalg.norm(want_grad)
        assert np.abs(diff).max() <= 2e-2 * gscale, np.abs(diff).max() / gscale
    for g in got[1:]:
        assert np.array_equal(got[0]["grad"], g["grad"]) and np.array_equal(got[0]["flat"], g["flat"])
    assert abs(float(np.mean([float(g["loss"]) for g in got])) - want_loss) <= 1e-5 * max(1.0, abs(want_loss))
    big = np.abs(want_grad) > 5e-2 * gscale  # Adam normalises rounding-noise gradients to O(lr): compare where g is signal
    assert np.abs(got[0]["flat"] - want_flat)[big].max() <= 2e-4
    # collectives of one step at this world size
    assert n_bn == 44, n_bn
    for g in got:
        assert 1 + 2 * n_bn == 89 and int(g["calls_sync_bn"]) == (89 - 15 if merged else 89), int(g["calls_sync_bn"])
        assert int(g["calls_local_bn"]) == 1, int(g["calls_local_bn"])
        assert int(g["bytes_local_bn"]) == 4 * want_grad.size


def test_one_training_step_matches_autograd(oracle):
    import torch
    from oracle import randla_train_oracle as rto
    cfg, xyz, feats = netcase.small_deep(1500, seed=2, B=2)
    cfg.d_out = [16, 32, 64, 32, 16]
    tr, pyr, params, labels, cw, (pts, nbr, pool, up) = _setup(cfg, xyz, feats)
    loss = tr.train_step(pyr, torch.from_numpy(feats).cuda(), torch.from_numpy(labels).cuda())
    torch.cuda.synchronize()
    want = rto.train_step(params, cfg.num_layers, pts, nbr, pool, up, feats, labels, cw, lr=1e-3, step=1)
    assert abs(float(loss) - want["loss"]) <= 1e-5 * max(1.0, abs(want["loss"])), (float(loss), want["loss"])
    assert np.abs(tr.last_logits.cpu().numpy().reshape(want["logits"].shape) - want["logits"]).max() < 1e-4
    # Tolerance: 2e-3 of the parameter's own gradient scale plus 2e-5 of the global gradient scale.  The second term
    # covers parameters whose true gradient is (near) zero -- biases in front of a BatchNorm (exactly 0) and the deepest
    # level, whose gradient passes a BatchNorm over a few dozen rows and comes out ~1e-6 after heavy cancellation.
    gscale = max(np.abs(g).max() for g in want["grads"].values())
    worst = []
    for name in tr.names:
        got = tr.G[name].cpu().numpy()
        ref = want["grads"][name]
        tol = 2e-3 * np.abs(ref).max() + 2e-5 * gscale
        worst.append((float(np.abs(got - ref).max() / tol), name))
    worst.sort(reverse=True)
    assert worst[0][0] <= 1.0, worst[:5]
    # moving statistics (the reference's extra_update_ops)
    new = tr.export_params()
    for k, v in want["new_params"].items():
        if k.endswith(("moving_mean", "moving_variance")):
            assert np.abs(new[k] - v).max() <= 1e-5 * max(1.0, np.abs(v).max()), k
    # one Adam step: the first step moves every weight by about lr * sign(g), so entries whose gradient is rounding noise
    # (|g| far below the global scale, e.g. biases in front of a BatchNorm) are excluded -- Adam normalises noise to O(lr)
    checked = 0
    for name in tr.names:
        ref_g = want["grads"][name]
        mask = np.abs(ref_g) > 1e-3 * gscale
        if mask.any():
            checked += int(mask.sum())
            assert np.abs(new[name] - want["new_params"][name])[mask].max() <= 2e-5, name
    assert checked > 1000


def _bf16_rule(kind, cin, cout):
    """Which GEMMs of Trainer(mlp_dtype="bf16") run on bf16-rounded operands (csrc/ops.hip: ps_op_conv1x1_ex takes the bf16 kernel
    when its K axis is a multiple of 16 -- for the input-gradient GEMM dy . W^T that axis is cout --; the weight-gradient kernel
    rounds every shape).  The LocSE convolution (cin = 10: relative_pos_encoding -> conv 10 -> h, RandLANet.py:324-325) is not one of
    the "bf16 MLPs": fp32 operands in all three GEMMs (its fused form, csrc/locse_train.hip, computes in fp32)."""
    if cin == 10:
        return False
    return True if kind == "wgrad" else ((cin if kind == "fwd" else cout) % 16 == 0)


def _act_rule(h):
    """Which levels of Trainer(mlp_dtype="bf16") STORE their [N*K, h] LFA rows as bfloat16 (ps_train_options.act_bf16, csrc/trainer.hip:
    where the fused LocSE branch, the recompute-form convolution and the split-source pooling kernels all apply: h a multiple of 8 up
    to 64)."""
    return h % 8 == 0 and h <= 64


def _grad_stats(got, ref, names):
    """(relative L2 over the whole gradient, worst per-tensor max error in units of 3e-2 of the tensor's own max + 1e-4 of the global max)"""
    gscale = max(np.abs(ref[n]).max() for n in names)
    num = den = 0.0
    worst = []
    for n in names:
        d = np.asarray(got[n], np.float64) - ref[n]
        num += float((d ** 2).sum())
        den += float((ref[n] ** 2).sum())
        worst.append((float(np.abs(d).max() / (3e-2 * np.abs(ref[n]).max() + 1e-4 * gscale)), n))
    worst.sort(reverse=True)
    return (num / den) ** 0.5, worst


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_training_step_at_the_true_width_ladder(oracle, mode):
    """BASELINE configs[2] at the real widths d_out = 16, 64, 128, 256, 512 (two clouds of 6 000 points: no level has fewer rows
    than K): loss, logits, EVERY gradient and the Adam update of one step against the torch-CPU float64 autograd oracle.

    fp32.  Bars: loss 2e-5 relative, logits 1e-4; every gradient tensor max |diff| <= 3e-2 of its own max + 1e-4 of the global max;
    relative L2 over the whole flat gradient <= 5e-3.  Measured: loss 1.2e-7, logits 3.6e-5, rel L2 2.3e-3, worst tensor 1.5e-2 of its
    own max (one entry of a BatchNorm beta of the decoder: a sum over 186 rows in which ONE leaky-ReLU decision on a pre-activation
    within rounding noise of zero changes a term by a factor of five).  For scale: torch-CPU float32 autograd against its own float64
    run on the same inputs gives rel L2 2.9e-4 and an outlier of the same kind at 0.7e-2.

    mlp_dtype="bf16".  The yardstick is the float64 oracle with the operands of exactly the GEMMs the product rounds (see _bf16_rule)
    rounded to bfloat16.  That MODEL is itself sensitive at the 1e-1 level: an activation within rounding noise of a bf16 boundary
    rounds the other way, a 4e-3 relative change that flips max-pool / leaky-ReLU decisions downstream -- evaluating the same rounded
    model in float32 instead of float64 moves its gradient by rel L2 0.125 and its logits by 0.18 (of 15.5).  So the bar is that
    spread, measured in the test: the product may differ from the float64 evaluation by at most 2x what the float32 evaluation of the
    same model differs by (plus 1e-3), for the loss, the logits and the whole gradient.
    CAVEAT -- what this bar does NOT show: with a measured spread of rel L2 0.125 the whole-step bar would still pass a bf16-mode
    gradient that is ~25 % off.  It only shows that the step behaves like the rounded model within that model's own chaos.  The
    evidence that the bf16 arithmetic itself is right is the GEMM-level test (test_bf16_mlp_mode_rounds_operands_and_accumulates_in_fp32:
    every product within 2e-5 of a float64 GEMM of the rounded operands) plus the fp32 leg of THIS test, which runs the same tape,
    the same kernels and the same gradient plumbing against float64 autograd at 5e-3."""
    import torch
    from oracle import randla_train_oracle as rto
    cfg, xyz, feats = netcase.small_deep(6000, seed=12, B=2)
    assert list(cfg.d_out) == [16, 64, 128, 256, 512]
    tr, pyr, params, labels, cw, (pts, nbr, pool, up) = _setup(cfg, xyz, feats, mlp_dtype=mode)
    loss = tr.train_step(pyr, torch.from_numpy(feats).cuda(), torch.from_numpy(labels).cuda())
    torch.cuda.synchronize()
    rule = _bf16_rule if mode == "bf16" else None
    arule = _act_rule if mode == "bf16" else None
    want = rto.train_step(params, cfg.num_layers, pts, nbr, pool, up, feats, labels, cw, lr=1e-3, step=1, bf16_rule=rule, act_rule=arule)
    got = {n: tr.G[n].cpu().numpy() for n in tr.names}
    rel_loss = abs(float(loss) - want["loss"]) / max(1.0, abs(want["loss"]))
    logit_err = float(np.abs(tr.last_logits.cpu().numpy().reshape(want["logits"].shape) - want["logits"]).max())
    rel_l2, worst = _grad_stats(got, want["grads"], tr.names)
    print("mode %s: loss rel %.2e, logits %.2e, grad rel L2 %.2e, worst tensors %s" % (mode, rel_loss, logit_err, rel_l2, worst[:3]))
    gscale = max(np.abs(g).max() for g in want["grads"].values())
    new = tr.export_params()
    if mode == "fp32":
        assert rel_loss <= 2e-5 and logit_err < 1e-4
        assert worst[0][0] <= 1.0, worst[:5]
        assert rel_l2 <= 5e-3
        checked = 0
        for name in tr.names:  # one Adam step where the gradient is signal (Adam normalises rounding noise to O(lr))
            mask = np.abs(want["grads"][name]) > 2e-2 * gscale
            if mask.any():
                checked += int(mask.sum())
                assert np.abs(new[name] - want["new_params"][name])[mask].max() <= 5e-5, name
        assert checked > 1000
    else:
        alt = rto.train_step(params, cfg.num_layers, pts, nbr, pool, up, feats, labels, cw, lr=1e-3, step=1, bf16_rule=rule, act_rule=arule, dtype=torch.float32)
        s_loss = abs(alt["loss"] - want["loss"]) / max(1.0, abs(want["loss"]))
        s_logit = float(np.abs(alt["logits"] - want["logits"]).max())
        s_l2, _ = _grad_stats(alt["grads"], want["grads"], tr.names)
        print("model sensitivity (float32 vs float64 evaluation of the rounded model): loss %.2e, logits %.2e, grad rel L2 %.2e" % (s_loss, s_logit, s_l2))
        assert rel_loss <= 2 * s_loss + 1e-3
        assert logit_err <= 2 * s_logit + 1e-3
        assert rel_l2 <= 2 * s_l2 + 1e-3
        # and the mode is not a no-op: the fp32 oracle is further away than the rounded one
        full = rto.train_step(params, cfg.num_layers, pts, nbr, pool, up, feats, labels, cw, lr=1e-3, step=1)
        assert _grad_stats(got, full["grads"], tr.names)[0] > 0.5 * _grad_stats(want["grads"], full["grads"], tr.names)[0]


def test_one_full_size_cloud_training_step_against_float64_autograd(oracle):
    """The per-rank work of BASELINE configs[3] (and one eighth of configs[2]) at its real size: ONE 180 000-point BraTS-shaped
    cloud, ConfigBraTS widths, Trainer(mlp_dtype="fp32"): loss, logits, EVERY gradient tensor and the moving statistics of one step
    against torch-CPU float64 autograd (about 25 s and 14 GB on 8 cores).  At this size the tape takes the branches the bench times:
    the >= 16 384-row gemm_b3 / wgrad_b3 products, the 2.9 M-row recomputed conv + BatchNorm passes, the radix-sorted inverse index
    (RandLANet.py:62-90 through :110-152).  Bars as in the width-ladder test: loss 2e-5 relative, logits 1e-4, every gradient tensor
    within 3e-2 of its own max + 1e-4 of the global max, relative L2 of the whole gradient 5e-3."""
    import torch
    from conftest import brats_cloud
    from oracle import randla_train_oracle as rto
    from point_unet_amd.helper_tool import ConfigBraTS as cfg
    n0 = 180000
    xyz = brats_cloud(n0, 0)[None]
    rng = np.random.default_rng(9)
    feats = np.concatenate([xyz, rng.standard_normal((1, n0, 4)).astype(np.float32)], -1)
    tr, pyr, params, labels, cw, (pts, nbr, pool, up) = _setup(cfg, xyz, feats, lr=1e-4)
    for i in range(cfg.num_layers):
        assert np.array_equal(pyr.neigh_idx[i].cpu().numpy(), nbr[i]) and np.array_equal(pyr.interp_idx[i].cpu().numpy(), up[i])
    loss = tr.train_step(pyr, torch.from_numpy(feats).cuda(), torch.from_numpy(labels).cuda())
    torch.cuda.synchronize()
    want = rto.train_step(params, cfg.num_layers, pts, nbr, pool, up, feats, labels, cw, lr=1e-4, step=1)
    got = {n: tr.G[n].cpu().numpy() for n in tr.names}
    rel_loss = abs(float(loss) - want["loss"]) / max(1.0, abs(want["loss"]))
    logit_err = float(np.abs(tr.last_logits.cpu().numpy().reshape(want["logits"].shape) - want["logits"]).max())
    rel_l2, worst = _grad_stats(got, want["grads"], tr.names)
    print("180 000 points: loss rel %.2e, logits %.2e, grad rel L2 %.2e, worst tensors %s" % (rel_loss, logit_err, rel_l2, worst[:3]))
    assert rel_loss <= 2e-5 and logit_err < 1e-4
    assert worst[0][0] <= 1.0, worst[:5]
    assert rel_l2 <= 5e-3
    new = tr.export_params()
    for k, v in want["new_params"].items():
        if k.endswith(("moving_mean", "moving_variance")):
            assert np.abs(new[k] - v).max() <= 1e-5 * max(1.0, np.abs(v).max()), k
    tr.close()


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_full_size_config3_step_properties(mode):
    """BASELINE configs[2] at FULL size: batch 8 x 180 000-point BraTS-shaped clouds, true widths, one training step (the oracle cannot
    run this size, so size-independent properties): (1) the loss is finite and equals the class-weighted cross-entropy re-evaluated
    on the host in float64 from the step's own logits (1e-5 relative); (2) the logits of two runs from the same state are
    bit-identical (no float atomics in the forward); (3) the flat gradient buffer of the two runs is BIT-IDENTICAL (torch.equal: the
    default step has no float atomics anywhere -- fixed-order partial sums and gather-reductions over inverse indices) and is
    non-trivial (no NaN, norm > 0); the float-atomics variant (deterministic=False) agrees with it to summation order; (4) after Adam every parameter moved by at most lr * (1 + 1e-3) (|m / sqrt(v)| = 1 at step 1)."""
    import torch
    from conftest import brats_cloud
    from point_unet_amd import weights
    from point_unet_amd.helper_tool import ConfigBraTS as cfg
    from point_unet_amd.pyramid import build_pyramid
    from point_unet_amd.train import Trainer
    B, n0 = 8, 180000
    xyz = np.stack([brats_cloud(n0, 50 + b) for b in range(B)])
    rng = np.random.default_rng(9)
    feats = np.concatenate([xyz, rng.standard_normal((B, n0, 4)).astype(np.float32)], -1)
    labels = rng.integers(0, cfg.num_classes, (B, n0)).astype(np.int32)
    cw = np.array([1.0, 2.5, 0.7, 1.8], np.float32)
    params = weights.init_params(cfg, seed=2)
    d_xyz, d_f, d_l = torch.from_numpy(xyz).cuda(), torch.from_numpy(feats).cuda(), torch.from_numpy(labels).cuda()
    pyr = build_pyramid(d_xyz, cfg)
    runs = []
    for _ in range(2):
        tr = Trainer(cfg, params=params, learning_rate=1e-4, class_weights=cw, keep_prob=1.0, mlp_dtype=mode)
        before = tr.flat.clone()
        loss = tr.train_step(pyr, d_f, d_l)
        torch.cuda.synchronize()
        runs.append((float(loss), tr.last_logits.clone(), tr.grad.clone(), (tr.flat - before).abs().max().item()))
        del tr
    loss, logits, grad, step = runs[0]
    assert np.isfinite(loss)
    z = logits.double().reshape(-1, cfg.num_classes)
    y = d_l.reshape(-1).long()
    ce = torch.nn.functional.cross_entropy(z, y, reduction="none") * torch.from_numpy(cw).cuda().double()[y]
    assert abs(loss - float(ce.mean())) <= 1e-5 * max(1.0, abs(loss))
    assert torch.equal(runs[1][1], logits) and runs[1][0] == loss
    assert bool(torch.isfinite(grad).all()) and float(grad.norm()) > 0
    rel = float((runs[1][2].double() - grad.double()).norm() / grad.double().norm())
    print("config3 %s: loss %.5f, grad norm %.4e, run-to-run rel L2 %.2e, max |step| %.3e" % (mode, loss, float(grad.norm()), rel, step))
    # the default step is DETERMINISTIC: weight / bias gradients and BatchNorm sums are fixed-order partial sums, every scatter-add of the
    # backward pass a gather-reduction over an inverse index in ascending row order (csrc/invidx.hip) -- two runs, bit-identical gradients
    assert torch.equal(runs[1][2], grad), rel
    assert 0 < step <= 1e-4 * (1 + 1e-3)
    # ... and the float-atomics form of the scatter-adds (Trainer(deterministic=False)) computes the same gradients to summation order
    tr = Trainer(cfg, params=params, learning_rate=1e-4, class_weights=cw, keep_prob=1.0, mlp_dtype=mode, deterministic=False)
    loss_a = tr.train_step(pyr, d_f, d_l)
    torch.cuda.synchronize()
    rel_a = float((tr.grad.double() - grad.double()).norm() / grad.double().norm())
    print("atomic scatter-adds against the deterministic ones: rel L2 %.2e" % rel_a)
    assert float(loss_a) == loss and rel_a <= (1e-5 if mode == "fp32" else 2e-3)


def test_ignored_labels_leave_the_loss_and_its_mean(oracle):
    """RandLANet.py:62-84: points whose label is in ignored_label_inds are dropped before the loss (mean over the valid ones) and
    the remaining raw labels are renumbered 0..C-1.  Trainer(ignored_label_inds=[0]) on raw labels 0..4 against the oracle fed the
    renumbered labels with -1 for the ignored points; the op alone against torch; an out-of-range label is ignored, never indexed."""
    import ctypes
    import torch
    from oracle import randla_train_oracle as rto
    from point_unet_amd import _lib, runtime, weights
    from point_unet_amd.pyramid import build_pyramid
    from point_unet_amd.train import Trainer
    from oracle import bindings as ob
    from oracle import randla_oracle as ro
    cfg, xyz, feats = netcase.small_deep(1500, seed=2, B=2)
    cfg.d_out = [16, 32, 64, 32, 16]
    params = weights.init_params(cfg, seed=3, randomize_bn=True)
    rng = np.random.default_rng(4)
    raw = rng.integers(0, cfg.num_classes + 1, xyz.shape[:2]).astype(np.int32)  # 0 = unlabeled, 1..4 = classes
    cw = np.linspace(1.0, 2.0, cfg.num_classes).astype(np.float32)
    tr = Trainer(cfg, params=params, learning_rate=1e-3, class_weights=cw, keep_prob=1.0, ignored_label_inds=[0])
    pyr = build_pyramid(torch.from_numpy(xyz).cuda(), cfg)
    loss = tr.train_step(pyr, torch.from_numpy(feats).cuda(), torch.from_numpy(raw).cuda())
    torch.cuda.synchronize()
    pts, nbr, pool, up = ro.build_pyramid(lambda s, q, k: ob.knn_batch(s, q, k), xyz, cfg.k_n, cfg.sub_sampling_ratio)
    want = rto.train_step(params, cfg.num_layers, pts, nbr, pool, up, feats, raw - 1, cw, lr=1e-3, step=1)
    assert abs(float(loss) - want["loss"]) <= 1e-5 * max(1.0, abs(want["loss"]))
    gscale = max(np.abs(g).max() for g in want["grads"].values())
    for name in ("fc/weights", "fc1/weights", "Encoder_layer_0mlp1/weights", "decoder_0/weights"):
        ref = want["grads"][name]
        assert np.abs(tr.G[name].cpu().numpy() - ref).max() <= 2e-3 * np.abs(ref).max() + 2e-5 * gscale, name
    # the op alone, labels outside [0, C) in both directions
    L, h = _lib.lib(), runtime.default_context(0).handle
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    g = torch.Generator().manual_seed(0)
    z = torch.randn(1001, 4, generator=g).cuda()
    y = torch.randint(-2, 7, (1001,), generator=g).int().cuda()
    w = torch.tensor([1.0, 2.0, 0.5, 3.0]).cuda()
    out, dz = torch.zeros(1).cuda(), torch.empty_like(z)
    _lib.check(L.ps_op_weighted_ce(h, p(z), p(y), p(w), 1001, 4, p(out), p(dz)))
    keep = (y >= 0) & (y < 4)
    zd = z.double().requires_grad_(True)
    ref = (torch.nn.functional.cross_entropy(zd[keep], y[keep].long(), reduction="none") * w.double()[y[keep].long()]).mean()
    ref.backward()
    assert abs(float(out) - float(ref)) < 1e-5 and (dz.double() - zd.grad).abs().max() < 1e-6
    assert float(dz[~keep].abs().max()) == 0.0
    out2 = torch.zeros(1).cuda()
    _lib.check(L.ps_op_weighted_ce(h, p(z), p(y), p(w), 1001, 4, p(out2), None))
    assert float(out2) == float(out)  # no float atomics: bit-identical from run to run


def test_training_forward_is_run_to_run_identical(oracle):
    """The forward pass has no float atomics (two-stage BatchNorm statistics with a fixed merge order): logits and loss
    inputs are bit-identical between runs, so which side of a leaky-ReLU kink / max-pool tie an activation falls on --
    and with it the gradient -- cannot flip from run to run.  Gradients (atomic weight-gradient sums) agree to ~1e-6."""
    import torch
    cfg, xyz, feats = netcase.small_deep(1500, seed=2, B=2)
    cfg.d_out = [16, 32, 64, 32, 16]
    outs = []
    for _ in range(3):
        tr, pyr, params, labels, cw, _ = _setup(cfg, xyz, feats)
        tr.train_step(pyr, torch.from_numpy(feats).cuda(), torch.from_numpy(labels).cuda())
        outs.append((tr.last_logits.cpu().numpy().copy(), tr.grad.cpu().numpy().copy()))
    for lg, g in outs[1:]:
        assert np.array_equal(lg, outs[0][0])
        assert np.abs(g - outs[0][1]).max() <= 2e-5 * np.abs(outs[0][1]).max()


def test_loss_decreases_over_a_few_steps(oracle):
    import torch
    cfg, xyz, feats = netcase.small_deep(3000, seed=5)
    cfg.d_out = [16, 32, 32, 16, 16]
    tr, pyr, params, labels, cw, _ = _setup(cfg, xyz, feats, lr=5e-3, keep_prob=0.5)
    # learnable target: label = sign pattern of the first modality
    labels = (feats[..., 3] > 0).astype(np.int32) + 2 * (feats[..., 4] > 0).astype(np.int32)
    f, l = torch.from_numpy(feats).cuda(), torch.from_numpy(labels).cuda()
    losses = [float(tr.train_step(pyr, f, l)) for _ in range(30)]
    assert np.isfinite(losses).all()
    assert np.mean(losses[-5:]) < 0.8 * np.mean(losses[:3]), losses


def test_training_ops_against_torch(oracle):
    """Op-level checks of the backward kernels on random tensors (shapes with awkward sizes)."""
    import ctypes
    import torch
    from point_unet_amd import _lib, runtime
    L, ctx = _lib.lib(), runtime.default_context(0)
    h = ctx.handle
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    g = torch.Generator().manual_seed(0)
    # wgrad
    for R, cin, cout in [(1000, 10, 8), (777, 24, 32), (301, 96, 128), (5000, 16, 16)]:
        x = torch.randn(R, cin, generator=g).cuda()
        dy = torch.randn(R, cout, generator=g).cuda()
        dW = torch.empty(cin, cout).cuda()
        db = torch.empty(cout).cuda()
        _lib.check(L.ps_op_linear_wgrad(h, p(x), p(dy), R, cin, cout, p(dW), p(db)))
        ref = x.double().T @ dy.double()
        assert (dW.double() - ref).abs().max() <= 1e-4 * ref.abs().max()
        assert (db.double() - dy.double().sum(0)).abs().max() <= 1e-4 * dy.double().sum(0).abs().max() + 1e-4
    # bn forward/backward
    R, C = 4097, 32
    x = (torch.randn(R, C, generator=g) * 2 + 0.5).cuda().requires_grad_(True)
    gamma = torch.rand(C, generator=g).cuda() + 0.5
    beta = torch.randn(C, generator=g).cuda()
    y = torch.empty(R, C).cuda()
    st = torch.empty(5, C).cuda()
    _lib.check(L.ps_op_bn_train_fwd(h, p(x), p(gamma), p(beta), R, C, 1e-6, 1, p(y), p(st[0]), p(st[1]), p(st[2]), p(st[3])))
    xd = x.detach().double().requires_grad_(True)
    ref = torch.nn.functional.leaky_relu((xd - xd.mean(0)) / torch.sqrt(xd.var(0, unbiased=False) + 1e-6) * gamma.double() + beta.double(), 0.2)
    assert (y.double() - ref).abs().max() < 1e-4
    dy = torch.randn(R, C, generator=g).cuda()
    ref.backward(dy.double())
    dx = torch.empty(R, C).cuda()
    dg = torch.empty(C).cuda()
    dbt = torch.empty(C).cuda()
    _lib.check(L.ps_op_bn_train_bwd(h, p(dy), p(x), p(gamma), p(beta), p(st[0]), p(st[1]), R, C, 1, p(dx), p(dg), p(dbt)))
    assert (dx.double() - xd.grad).abs().max() < 1e-4
    # softmax pool
    Rr, K, d = 333, 16, 24
    f = torch.randn(Rr, K, d, generator=g).cuda()
    s = torch.randn(Rr, K, d, generator=g).cuda()
    fd, sd = f.double().requires_grad_(True), s.double().requires_grad_(True)
    ref = (fd * torch.softmax(sd, 1)).sum(1)
    probs = torch.empty_like(f)
    agg = torch.empty(Rr, d).cuda()
    _lib.check(L.ps_op_softmax_pool_fwd(h, p(f), p(s), Rr, K, d, p(probs), p(agg)))
    assert (agg.double() - ref).abs().max() < 1e-5
    da = torch.randn(Rr, d, generator=g).cuda()
    ref.backward(da.double())
    df, ds = torch.empty_like(f), torch.empty_like(f)
    _lib.check(L.ps_op_softmax_pool_bwd(h, p(da), p(f), p(probs), Rr, K, d, p(df), p(ds)))
    assert (df.double() - fd.grad).abs().max() < 1e-5 and (ds.double() - sd.grad).abs().max() < 1e-5
    # weighted CE
    z = torch.randn(999, 4, generator=g).cuda()
    yl = torch.randint(0, 4, (999,), generator=g).int().cuda()
    cw = torch.tensor([1.0, 2.0, 0.5, 3.0]).cuda()
    loss = torch.zeros(1).cuda()
    dz = torch.empty_like(z)
    _lib.check(L.ps_op_weighted_ce(h, p(z), p(yl), p(cw), 999, 4, p(loss), p(dz)))
    zd = z.double().requires_grad_(True)
    ref = (torch.nn.functional.cross_entropy(zd, yl.long(), reduction="none") * cw.double()[yl.long()]).mean()
    ref.backward()
    assert abs(float(loss) - float(ref)) < 1e-5 and (dz.double() - zd.grad).abs().max() < 1e-6


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_fused_attentive_pooling_forward_backward(mode):
    """ps_op_att_pool_train_fwd / _bwd (score product + softmax over K + weighted sum in one kernel per direction; the backward
    recomputes scores and probabilities) against torch float64 autograd of  agg = sum_K softmax_K(F.W) * F  -- for the bf16 mode with
    the operands of the three products rounded exactly as the kernel rounds them (F, W for the scores; dS, W^T for dF; F, dS for dW).
    Strided input (a column block of a wider buffer), ragged point counts down to a single point, d = 16 / 32 / 64 (and 128 in the bf16
    mode); at R = 37 also the plain form's per-element store path (a row pitch of d + 2), bit-identical to the row stores.  Bars: agg 2e-6 (fp32) / 2e-5 (bf16) of its
    max; dF and dW 2e-5 of their max in fp32; in the bf16 mode 2e-3 / 1e-3: dS is rounded to bfloat16 from its fp32 value in the
    kernel and from its float64 value here, and an element within fp32 noise of a rounding boundary lands on the neighbouring
    bfloat16 (a 4e-3 relative change of that one term).  The weight gradient is bit-identical from run to run (fixed summation order)."""
    import ctypes
    import torch
    from point_unet_amd import _lib, runtime
    L, ctx = _lib.lib(), runtime.default_context(0)
    h = ctx.handle
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    g = torch.Generator().manual_seed(11)
    rb = (lambda t: t.float().bfloat16().double()) if mode == "bf16" else (lambda t: t)
    K = 16
    try:
        _lib.check(L.ps_set_train_gemm_bf16(h, 1 if mode == "bf16" else 0))
        shapes = [(1000, 16, 16), (4097, 16, 32), (777, 32, 32), (2049, 64, 64), (300, 64, 128)]
        # tiny point counts: one point (seven of a workgroup's eight waves idle), four, and 37 (the last workgroup ends mid-way)
        shapes += [(1, 16, 16), (4, 16, 16), (37, 16, 32), (1, 32, 32), (4, 32, 32), (37, 32, 48)]
        if mode == "bf16":  # d = 128 (level 2) exists on the bf16 matrix pipe only: both weight orientations as bfloat16 in LDS
            shapes += [(1500, 128, 128), (333, 128, 192)]
            # (the column-split backward: one live group of three / a second workgroup with one live group / a ragged end)
            shapes += [(1, 128, 128), (4, 128, 128), (37, 128, 160)]
        for R, d, wide in shapes:
            assert L.ps_op_att_pool_train_supported_ex(K, d, 1 if mode == "bf16" else 0) == 1
            buf = torch.randn(R * K, wide, generator=g).cuda()
            F = buf[:, wide - d:]
            W = (torch.randn(d, d, generator=g) / d ** 0.5).cuda()
            dagg = torch.randn(R, d, generator=g).cuda()
            agg = torch.empty(R, d).cuda()
            _lib.check(L.ps_op_att_pool_train_fwd(h, p(F), wide, p(W), R, K, d, p(agg)))
            dF = torch.empty(R * K, d).cuda()
            dW, dW2 = torch.empty(d, d).cuda(), torch.empty(d, d).cuda()
            _lib.check(L.ps_op_att_pool_train_bwd(h, p(F), wide, p(W), p(dagg), R, K, d, p(dF), d, p(dW)))
            _lib.check(L.ps_op_att_pool_train_bwd(h, p(F), wide, p(W), p(dagg), R, K, d, p(dF), d, p(dW2)))
            assert torch.equal(dW, dW2)
            if R == 37:
                # a row pitch that is no multiple of four floats takes the per-element store path of the plain form (at d = 128: the
                # one-wave backward): same accumulators, same grid, another store instruction -- the written columns and dW are
                # bit-identical, the padding columns untouched
                dFp, dWp = torch.full((R * K, d + 2), -7.5).cuda(), torch.empty(d, d).cuda()
                _lib.check(L.ps_op_att_pool_train_bwd(h, p(F), wide, p(W), p(dagg), R, K, d, p(dFp), d + 2, p(dWp)))
                assert torch.equal(dFp[:, :d], dF), (R, d)
                assert bool((dFp[:, d:] == -7.5).all()), (R, d)
                assert torch.equal(dWp, dW), (R, d)
            Fd, Wd = F.double().reshape(R, K, d), W.double()
            S = rb(Fd) @ rb(Wd)
            P = torch.softmax(S, 1)
            ref = (P * Fd).sum(1)
            assert (agg.double() - ref).abs().max() <= (2e-6 if mode == "fp32" else 2e-5) * ref.abs().max(), (R, d)
            gd = dagg.double()[:, None, :]
            dS = P * gd * (Fd - ref[:, None, :])
            dF_ref = P * gd + rb(dS) @ rb(Wd).T
            dW_ref = rb(Fd).reshape(-1, d).T @ rb(dS).reshape(-1, d)
            assert (dF.double().reshape(R, K, d) - dF_ref).abs().max() <= (2e-5 if mode == "fp32" else 2e-3) * dF_ref.abs().max(), (R, d)
            assert (dW.double() - dW_ref).abs().max() <= (2e-5 if mode == "fp32" else 1e-3) * dW_ref.abs().max(), (R, d)
            if mode == "fp32":  # and the closed form agrees with autograd
                Fa, Wa = F.double().reshape(R, K, d).clone().requires_grad_(True), W.double().clone().requires_grad_(True)
                ((torch.softmax(Fa @ Wa, 1) * Fa).sum(1) * dagg.double()).sum().backward()
                assert (dF_ref - Fa.grad).abs().max() < 1e-10 and (dW_ref - Wa.grad).abs().max() < 1e-9
        assert L.ps_op_att_pool_train_supported(K, 128) == 0 and L.ps_op_att_pool_train_supported(32, 16) == 0
        assert L.ps_op_att_pool_train_supported_ex(K, 128, 0) == 0 and L.ps_op_att_pool_train_supported_ex(K, 128, 1) == 1
    finally:
        _lib.check(L.ps_set_train_gemm_bf16(h, 0))
    torch.cuda.synchronize()


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_wide_level_attentive_pooling_on_the_gemm_frame(mode):
    """ps_op_att_pool_gemm_fwd / _bwd (csrc/attpool_gemm.hip: the score product, the softmax over K, the weighted sum and -- backward --
    dS and dF = p g + dS . W^T with the scores only in accumulator registers; d = 128 / 256 / 512, the backward of 512 as two launches over
    halves of the dF columns) against torch float64
    autograd of  agg = sum_K softmax_K(F.W) * F  (RandLANet.py:394-398), the bf16 mode with the operands of the products rounded as the
    kernel rounds them.  Strided input (a column block of a wider buffer), ragged point counts (the last workgroup holds an odd number
    of points / waves without rows), accumulation into an existing dF, and the weight gradient through ps_op_linear_wgrad_ex over
    (F, dS).  Bars as the narrow-level kernels: agg 2e-6 / 2e-5 of its max, dF and dW 2e-5 (fp32) and 2e-3 / 1e-3 (bf16: dS within
    fp32 noise of a bfloat16 rounding boundary lands on the neighbour).  Transposes would show: W is not symmetric, rows are random."""
    import ctypes
    import torch
    from point_unet_amd import _lib, runtime
    L, ctx = _lib.lib(), runtime.default_context(0)
    h = ctx.handle
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    g = torch.Generator().manual_seed(23)
    rb = (lambda t: t.float().bfloat16().double()) if mode == "bf16" else (lambda t: t)
    K = 16
    try:
        _lib.check(L.ps_set_train_gemm_bf16(h, 1 if mode == "bf16" else 0))
        for R, d, wide, bwd in [(1000, 128, 128, True), (1033, 128, 160, True), (7, 128, 128, True), (1500, 256, 256, True), (333, 256, 320, True),
                                (1, 256, 256, True), (515, 512, 512, True), (130, 512, 544, True)]:
            assert L.ps_op_att_pool_gemm_supported(K, d) == 1
            buf = torch.randn(R * K, wide, generator=g).cuda()
            F = buf[:, wide - d:]
            W = (torch.randn(d, d, generator=g) / d ** 0.5).cuda()
            dagg = torch.randn(R, d, generator=g).cuda()
            agg = torch.full((R + 1, d), 7.0).cuda()
            _lib.check(L.ps_op_att_pool_gemm_fwd(h, p(F), wide, p(W), R, K, d, p(agg)))
            assert bool((agg[R] == 7.0).all()), "wrote past the last point"
            Fd, Wd = F.double().reshape(R, K, d), W.double()
            S = rb(Fd) @ rb(Wd)
            P = torch.softmax(S, 1)
            ref = (P * Fd).sum(1)
            assert (agg[:R].double() - ref).abs().max() <= (2e-6 if mode == "fp32" else 2e-5) * ref.abs().max(), (R, d)
            if not bwd:
                continue
            seed = torch.randn(R * K + 16, d, generator=g).cuda()
            dF, dF2 = torch.full((R * K + 16, d), 3.0).cuda(), seed.clone()
            dS = torch.full((R * K + 16, d + 4), 5.0).cuda()
            _lib.check(L.ps_op_att_pool_gemm_bwd(h, p(F), wide, p(W), p(dagg), R, K, d, p(dF), d, 0, p(dS), d + 4))
            _lib.check(L.ps_op_att_pool_gemm_bwd(h, p(F), wide, p(W), p(dagg), R, K, d, p(dF2), d, 1, p(dS), d + 4))
            assert bool((dF[R * K:] == 3.0).all()) and bool((dS[R * K:] == 5.0).all()) and bool((dS[:, d:] == 5.0).all()), "wrote past the last row"
            gd = dagg.double()[:, None, :]
            dS_ref = P * gd * (Fd - ref[:, None, :])
            dF_ref = P * gd + rb(dS_ref) @ rb(Wd).T
            bar = 2e-5 if mode == "fp32" else 2e-3
            assert (dS[:R * K, :d].double().reshape(R, K, d) - rb(dS_ref)).abs().max() <= (2e-5 if mode == "fp32" else 8e-3) * dS_ref.abs().max(), (R, d)
            assert (dF[:R * K].double().reshape(R, K, d) - dF_ref).abs().max() <= bar * dF_ref.abs().max(), (R, d)
            assert ((dF2[:R * K] - seed[:R * K]).double().reshape(R, K, d) - dF_ref).abs().max() <= 2 * bar * dF_ref.abs().max(), (R, d)
            dW = torch.empty(d, d).cuda()
            _lib.check(L.ps_op_linear_wgrad_ex(h, p(F), wide, p(dS), d + 4, R * K, d, d, p(dW), None))
            dW_ref = rb(Fd).reshape(-1, d).T @ rb(dS_ref).reshape(-1, d)
            assert (dW.double() - dW_ref).abs().max() <= (2e-5 if mode == "fp32" else 2e-3) * dW_ref.abs().max(), (R, d)
            if mode == "fp32" and R <= 1100:  # and the closed form agrees with autograd
                Fa, Wa = F.double().reshape(R, K, d).clone().requires_grad_(True), W.double().clone().requires_grad_(True)
                ((torch.softmax(Fa @ Wa, 1) * Fa).sum(1) * dagg.double()).sum().backward()
                assert (dF_ref - Fa.grad).abs().max() < 1e-10 and (dW_ref - Wa.grad).abs().max() < 1e-9
        assert L.ps_op_att_pool_gemm_supported(K, 64) == 0 and L.ps_op_att_pool_gemm_supported(32, 128) == 0
    finally:
        _lib.check(L.ps_set_train_gemm_bf16(h, 0))
    torch.cuda.synchronize()


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_wide_level_split_source_forms_equal_the_materialised_ones(mode):
    """ps_op_att_pool_gemm_fwd_split / _bwd_split and ps_op_linear_wgrad_split (gather_neighbour + concat folded into the wide-level fused
    pooling and into the loader of the split-bf16 weight-gradient kernel, RandLANet.py:326-333) against the SAME kernels fed the
    materialised concat buffer: same products in the same order, so agg, both halves of dF, dS and dW are bit-identical; the f_xyz half
    is also checked in its accumulate form.  Two clouds (the gathered rows are cloud-local), 650 of 700 points queried, d = 128 / 256;
    and three clouds of 37 queried points out of 40: 111 points are an odd number (the last wave with rows holds ONE point, the fourth
    wave of the workgroup none) and a cloud ends inside a wave's pair of points (each point takes its own cloud's rows)."""
    import ctypes
    import torch
    from point_unet_amd import _lib, runtime
    L, ctx = _lib.lib(), runtime.default_context(0)
    h = ctx.handle
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    g = torch.Generator().manual_seed(29)
    K = 16
    try:
        _lib.check(L.ps_set_train_gemm_bf16(h, 1 if mode == "bf16" else 0))
        for B, N, M, d in [(2, 700, 650, 128), (2, 700, 650, 256), (3, 40, 37, 128), (3, 40, 37, 256)]:
            hh = d // 2
            fsrc = torch.randn(B * N, hh, generator=g).cuda()
            fx = torch.randn(B * M * K, hh, generator=g).cuda()
            idx = torch.randint(0, N, (B, M, K), generator=g, dtype=torch.int32).cuda()
            W = (torch.randn(d, d, generator=g) / d ** 0.5).cuda()
            dagg = torch.randn(B * M, d, generator=g).cuda()
            cat = torch.empty(B * M * K, d).cuda()
            _lib.check(L.ps_op_gather_neighbour_ex(h, p(fsrc), p(idx), B, N, M, K, hh, p(cat), d))
            cat[:, hh:] = fx
            agg0, dcat, dS0, dW0 = torch.empty(B * M, d).cuda(), torch.empty(B * M * K, d).cuda(), torch.empty(B * M * K, d).cuda(), torch.empty(d, d).cuda()
            _lib.check(L.ps_op_att_pool_gemm_fwd(h, p(cat), d, p(W), B * M, K, d, p(agg0)))
            _lib.check(L.ps_op_att_pool_gemm_bwd(h, p(cat), d, p(W), p(dagg), B * M, K, d, p(dcat), d, 0, p(dS0), d))
            _lib.check(L.ps_op_linear_wgrad_ex(h, p(cat), d, p(dS0), d, B * M * K, d, d, p(dW0), None))
            agg1, rows, dfx, dS1, dW1 = (torch.empty(B * M, d).cuda(), torch.empty(B * M * K, hh).cuda(), torch.empty(B * M * K, hh).cuda(),
                                         torch.empty(B * M * K, d).cuda(), torch.empty(d, d).cuda())
            _lib.check(L.ps_op_att_pool_gemm_fwd_split(h, p(fsrc), hh, p(idx), B, N, M, p(fx), hh, p(W), K, d, p(agg1)))
            _lib.check(L.ps_op_att_pool_gemm_bwd_split(h, p(fsrc), hh, p(idx), B, N, M, p(fx), hh, p(W), p(dagg), K, d, p(rows), hh, p(dfx), hh, 0, p(dS1), d))
            assert torch.equal(agg0, agg1), (B, d)
            assert torch.equal(dcat[:, :hh].contiguous(), rows) and torch.equal(dcat[:, hh:].contiguous(), dfx) and torch.equal(dS0, dS1), (B, d)
            if B * M * K >= 16384:  # (the split-source weight-gradient product takes 16 384 rows or more)
                _lib.check(L.ps_op_linear_wgrad_split(h, p(fsrc), hh, p(idx), B, N, M, K, p(fx), hh, p(dS1), d, d, d, p(dW1)))
                assert torch.equal(dW0, dW1), (B, d)
            seed = torch.randn(B * M * K, hh, generator=g).cuda()
            acc = seed.clone()
            _lib.check(L.ps_op_att_pool_gemm_bwd_split(h, p(fsrc), hh, p(idx), B, N, M, p(fx), hh, p(W), p(dagg), K, d, p(rows), hh, p(acc), hh, 1, p(dS1), d))
            assert torch.equal(acc, seed + dfx), (B, d)
    finally:
        _lib.check(L.ps_set_train_gemm_bf16(h, 0))
    torch.cuda.synchronize()


def test_bf16_storage_of_the_lfa_rows_changes_only_the_format():
    """ps_set_train_act_bf16 (ps_train_options.act_bf16; BASELINE configs[2]): the [N*K, h] rows of the LFA branch STORED as bfloat16.
    A storage format, not another algorithm -- so every op is held to that: with the flag on,
      * ps_op_locse_train_apply and ps_op_conv_bn_train_apply write exactly bfloat16(RNE) of what they write with the flag off;
      * ps_op_conv_bn_train_sums / _apply / _bwd_sums2 / _bwd_apply_w fed bfloat16 rows x, and ps_op_att_pool_train_fwd_split /
        _bwd_split_rows fed bfloat16 rows fr, return bit for bit what they return for the same values handed over as fp32 rows;
      * the GRADIENT rows of those tensors travel in the same format: dz into (and dx out of, plain or accumulating) the convolution's
        backward, dz into ps_op_locse_train_bwd, dfr out of the pooling's backward -- bfloat16(RNE) of the fp32 form's values.
    h = 8 (one thread per row), 32 and 64 (tile kernels); d = 2h = 16 (per-point kernels), 64 (attpool_gemm.hip's attg64), 128 (the
    column-split bf16 kernel).  Two clouds, 600 points, bf16-MLP mode on."""
    import ctypes
    import torch
    from point_unet_amd import _lib, runtime
    L, ctx = _lib.lib(), runtime.default_context(0)
    hd = ctx.handle
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    g = torch.Generator().manual_seed(41)
    B, N, K = 2, 600, 16
    R = B * N * K
    xyz = torch.rand(B * N, 3, generator=g).cuda()
    idx = torch.randint(0, N, (B, N, K), generator=g, dtype=torch.int32).cuda()

    def act(on):
        _lib.check(L.ps_set_train_act_bf16(hd, 1 if on else 0))
    try:
        _lib.check(L.ps_set_train_gemm_bf16(hd, 1))
        for h in (8, 32, 64):
            d = 2 * h
            # -- LocSE apply: the output format
            W1 = (torch.randn(10, h, generator=g) * 0.5).cuda(); b1 = (torch.randn(h, generator=g) * 0.1).cuda()
            mean, scale, beta = (0.1 * torch.randn(h, generator=g)).cuda(), (1 + 0.2 * torch.rand(h, generator=g)).cuda(), (0.1 * torch.randn(h, generator=g)).cuda()
            y32 = torch.empty(R, h).cuda(); y16 = torch.empty(R, h, dtype=torch.bfloat16).cuda()
            act(False); _lib.check(L.ps_op_locse_train_apply(hd, p(xyz), p(idx), B, N, K, p(W1), p(b1), h, p(mean), p(scale), p(beta), p(y32), h))
            act(True); _lib.check(L.ps_op_locse_train_apply(hd, p(xyz), p(idx), B, N, K, p(W1), p(b1), h, p(mean), p(scale), p(beta), p(y16), h))
            assert torch.equal(y16, y32.bfloat16()), h
            # -- LFA mlp2 in the recompute form: x as bfloat16 rows
            x16, xf = y16, y16.float()
            W2 = (torch.randn(h, h, generator=g) / h ** 0.5).cuda(); b2 = (torch.randn(h, generator=g) * 0.1).cuda()
            CP = max(h, 16)
            s_a, s_b = torch.zeros(3 * CP, dtype=torch.float64).cuda(), torch.zeros(3 * CP, dtype=torch.float64).cuda()
            act(False); _lib.check(L.ps_op_conv_bn_train_sums(hd, p(xf), h, p(W2), p(b2), R, h, p(s_a)))
            act(True); _lib.check(L.ps_op_conv_bn_train_sums(hd, p(x16), h, p(W2), p(b2), R, h, p(s_b)))
            assert torch.equal(s_a, s_b), h
            m2, inv2 = (0.1 * torch.randn(h, generator=g)).cuda(), (1 + 0.2 * torch.rand(h, generator=g)).cuda()
            sc2, be2 = (inv2 * 1.1).contiguous(), (0.1 * torch.randn(h, generator=g)).cuda()
            z32 = torch.empty(R, h).cuda(); z16 = torch.empty(R, h, dtype=torch.bfloat16).cuda()
            act(False); _lib.check(L.ps_op_conv_bn_train_apply(hd, p(xf), h, p(W2), p(b2), R, h, p(m2), p(sc2), p(be2), p(z32), h))
            act(True); _lib.check(L.ps_op_conv_bn_train_apply(hd, p(x16), h, p(W2), p(b2), R, h, p(m2), p(sc2), p(be2), p(z16), h))
            assert torch.equal(z16, z32.bfloat16()), h
            # (the gradient rows dz / dx have the format of the activation rows: bfloat16 dz in, bfloat16 dx out -- plain and accumulating)
            dz16 = torch.randn(R, h, generator=g).cuda().bfloat16(); dzf = dz16.float()
            old16 = torch.randn(R, h, generator=g).cuda().bfloat16()
            for accumulate in (0, 1):
                outs = {}
                for on, xx, dzz in ((False, xf, dzf), (True, x16, dz16)):
                    act(on)
                    s12 = torch.zeros(3 * h).cuda(); dw = torch.empty(h, h).cuda(); db = torch.empty(h).cuda()
                    dx = old16.clone() if on else old16.float()
                    _lib.check(L.ps_op_conv_bn_train_bwd_sums2(hd, p(xx), h, p(W2), p(b2), R, h, p(m2), p(inv2), p(sc2), p(be2), p(dzz), h, p(s12)))
                    _lib.check(L.ps_op_conv_bn_train_bwd_apply_w(hd, p(xx), h, p(W2), p(b2), R, h, p(m2), p(inv2), p(sc2), p(be2), p(s12), 1.0 / R, p(dzz), h,
                                                                 accumulate, p(dx), h, p(dw), p(db)))
                    outs[on] = (s12[:2 * h].clone(), dx if on else dx.bfloat16(), dw, db)
                for a_, b_ in zip(outs[False], outs[True]):
                    assert torch.equal(a_, b_), (h, accumulate)
            # -- LocSE backward: dz as bfloat16 rows
            sums = {}
            inv1 = (1 + 0.2 * torch.rand(h, generator=g)).cuda()
            for on, dzz in ((False, dzf), (True, dz16)):
                act(on)
                acc = torch.empty(23 * h + 16).cuda()
                _lib.check(L.ps_op_locse_train_bwd(hd, p(xyz), p(idx), B, N, K, p(W1), p(b1), h, p(scale), p(beta), p(mean), p(inv1), p(dzz), h, p(acc)))
                sums[on] = acc
            assert torch.equal(sums[False], sums[True]), h
            # -- the split-source pooling: fr as bfloat16 rows
            assert L.ps_op_att_pool_train_supported_ex(K, d, 1) == 1
            fsrc = torch.randn(B * N, h, generator=g).cuda()
            Wfc = (torch.randn(d, d, generator=g) / d ** 0.5).cuda(); dagg = torch.randn(B * N, d, generator=g).cuda()
            # (... and both halves of the gradient: dfr, and the gathered half's rows for the gather-reduction, as bfloat16 rows)
            res = {}
            for on, fr in ((False, xf), (True, x16)):
                act(on)
                agg = torch.empty(B * N, d).cuda(); dW = torch.empty(d, d).cuda()
                rows = torch.empty(R, h, dtype=torch.bfloat16 if on else torch.float32).cuda()
                dfr = torch.empty(R, h, dtype=torch.bfloat16 if on else torch.float32).cuda()
                _lib.check(L.ps_op_att_pool_train_fwd_split(hd, p(fsrc), h, p(idx), B, N, N, p(fr), h, p(Wfc), K, d, p(agg)))
                _lib.check(L.ps_op_att_pool_train_bwd_split_rows(hd, p(fsrc), h, p(idx), B, N, N, p(fr), h, p(Wfc), p(dagg), K, d, p(rows), h, p(dfr), h, p(dW)))
                res[on] = (agg, rows if on else rows.bfloat16(), dfr if on else dfr.bfloat16(), dW)
            for a_, b_ in zip(res[False], res[True]):
                assert torch.equal(a_, b_), (h, d)
            if d == 128:  # the forward on the frame of the large GEMMs (attpool_gemm.hip): the bfloat16 rows are operand fragments as loaded
                aggs = {}
                for on, fr in ((False, xf), (True, x16)):
                    act(on)
                    agg = torch.empty(B * N, d).cuda()
                    _lib.check(L.ps_op_att_pool_gemm_fwd_split(hd, p(fsrc), h, p(idx), B, N, N, p(fr), h, p(Wfc), K, d, p(agg)))
                    aggs[on] = agg
                assert torch.equal(aggs[False], aggs[True])
                assert (aggs[True] - res[True][0]).abs().max() <= 2e-5 * max(1.0, float(res[True][0].abs().max()))  # (and the per-point kernel's result)
            # -- the gather-reduction over bfloat16 rows: the sums of the same values handed over as fp32 rows, bit for bit
            act(False)
            off = torch.empty(B * N + 1, dtype=torch.int32, device="cuda"); src = torch.empty(R, dtype=torch.int32, device="cuda")
            ws = torch.empty(int(L.ps_op_inverse_index_workspace(B * N, R)), dtype=torch.int32, device="cuda")
            _lib.check(L.ps_op_inverse_index(hd, p(idx), B, N, N * K, p(off), p(src), p(ws)))
            rows16 = res[True][1]
            rows32 = rows16.float()
            perm = torch.stack([torch.randperm(N, generator=g) for _ in range(B)]).int().cuda()
            for accumulate in (0, 1):
                base = torch.randn(B * N, h, generator=g).cuda()
                want, got, got_o = base.clone(), base.clone(), base.clone()
                _lib.check(L.ps_op_gather_reduce_rows(hd, p(rows32), h, p(off), p(src), B * N, h, p(want), h, accumulate))
                act(True)
                _lib.check(L.ps_op_gather_reduce_rows(hd, p(rows16), h, p(off), p(src), B * N, h, p(got), h, accumulate))
                _lib.check(L.ps_op_gather_reduce_rows_ordered(hd, p(rows16), h, p(off), p(src), B * N, h, p(got_o), h, accumulate, p(perm), N))
                act(False)
                assert torch.equal(want, got) and torch.equal(want, got_o), (h, accumulate)
    finally:
        _lib.check(L.ps_set_train_act_bf16(hd, 0))
        _lib.check(L.ps_set_train_gemm_bf16(hd, 0))
    torch.cuda.synchronize()


def test_bf16_rows_of_the_level1_pooling_where_a_wave_takes_a_second_tile():
    """ps_op_att_pool_train_fwd_split / _bwd_split_rows at d = 64 (attpool_gemm.hip's attg64_kernel) fed bfloat16 rows fr, at a size where
    the persistent grid is capped (256 workgroups per resident workgroup of a CU) and waves walk on to a second tile: 2 x 3 100 points = 3 100
    tiles against 3 072 waves of the forward and 2 048 of the eight-wave backward -- the prefetch of the next tile's rows and of the index two
    tiles ahead.  The assertions of test_bf16_storage_of_the_lfa_rows_changes_only_the_format: bit for bit what the same values handed over
    as fp32 rows give, both halves of the gradient as bfloat16(RNE) of the fp32 form's values."""
    import ctypes
    import torch
    from point_unet_amd import _lib, runtime
    L, ctx = _lib.lib(), runtime.default_context(0)
    hd = ctx.handle
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    g = torch.Generator().manual_seed(43)
    B, N, K, h = 2, 3100, 16, 32
    R, d = B * N * K, 2 * h
    idx = torch.randint(0, N, (B, N, K), generator=g, dtype=torch.int32).cuda()
    fsrc = torch.randn(B * N, h, generator=g).cuda()
    x16 = torch.randn(R, h, generator=g).cuda().bfloat16()
    Wfc = (torch.randn(d, d, generator=g) / d ** 0.5).cuda(); dagg = torch.randn(B * N, d, generator=g).cuda()
    try:
        _lib.check(L.ps_set_train_gemm_bf16(hd, 1))
        assert L.ps_op_att_pool_train_supported_ex(K, d, 1) == 1
        res = {}
        for on, fr in ((False, x16.float()), (True, x16)):
            _lib.check(L.ps_set_train_act_bf16(hd, 1 if on else 0))
            agg = torch.empty(B * N, d).cuda(); dW = torch.empty(d, d).cuda()
            rows = torch.empty(R, h, dtype=torch.bfloat16 if on else torch.float32).cuda()
            dfr = torch.empty(R, h, dtype=torch.bfloat16 if on else torch.float32).cuda()
            _lib.check(L.ps_op_att_pool_train_fwd_split(hd, p(fsrc), h, p(idx), B, N, N, p(fr), h, p(Wfc), K, d, p(agg)))
            _lib.check(L.ps_op_att_pool_train_bwd_split_rows(hd, p(fsrc), h, p(idx), B, N, N, p(fr), h, p(Wfc), p(dagg), K, d, p(rows), h, p(dfr), h, p(dW)))
            res[on] = (agg, rows if on else rows.bfloat16(), dfr if on else dfr.bfloat16(), dW)
        for a_, b_ in zip(res[False], res[True]):
            assert torch.equal(a_, b_)
    finally:
        _lib.check(L.ps_set_train_act_bf16(hd, 0))
        _lib.check(L.ps_set_train_gemm_bf16(hd, 0))
    torch.cuda.synchronize()


def test_split_source_attentive_pooling_equals_gather_concat_attpool():
    """ps_op_att_pool_train_*_split (gather_neighbour + concat folded into the fused attention) against the materialised form through
    the SAME fused kernels: agg, the f_xyz half of the gradient and dWfc bit-identical (same arithmetic, fixed summation order); the
    gathered half, scatter-added with float atomics, equal to ps_op_scatter_add_rows of the materialised gradient within the atomics'
    summation-order noise (2e-6 of its max); it is ADDED to what the buffer held.  Two clouds, d = 16 / 32 / 64."""
    import ctypes
    import torch
    from point_unet_amd import _lib, runtime
    L, ctx = _lib.lib(), runtime.default_context(0)
    h = ctx.handle
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    g = torch.Generator().manual_seed(5)
    B, N, M, K = 2, 700, 650, 16
    for d in (16, 32, 64):
        hh = d // 2
        fsrc = torch.randn(B * N, hh, generator=g).cuda()
        idx = torch.randint(0, N, (B, M, K), generator=g, dtype=torch.int32).cuda()
        fx = torch.randn(B * M * K, hh, generator=g).cuda()
        W = (torch.randn(d, d, generator=g) / d ** 0.5).cuda()
        dagg = torch.randn(B * M, d, generator=g).cuda()
        # materialised reference
        cat = torch.empty(B * M * K, d).cuda()
        _lib.check(L.ps_op_gather_neighbour_ex(h, p(fsrc), p(idx), B, N, M, K, hh, p(cat), d))
        cat[:, hh:] = fx
        agg0, dcat, dW0 = torch.empty(B * M, d).cuda(), torch.empty(B * M * K, d).cuda(), torch.empty(d, d).cuda()
        _lib.check(L.ps_op_att_pool_train_fwd(h, p(cat), d, p(W), B * M, K, d, p(agg0)))
        _lib.check(L.ps_op_att_pool_train_bwd(h, p(cat), d, p(W), p(dagg), B * M, K, d, p(dcat), d, p(dW0)))
        dsrc0 = torch.ones(B * N, hh).cuda()
        _lib.check(L.ps_op_scatter_add_rows_ex(h, p(dcat), d, p(idx), B, N, M * K, hh, p(dsrc0)))
        # split-source form
        agg1, dfx, dW1 = torch.empty(B * M, d).cuda(), torch.empty(B * M * K, hh).cuda(), torch.empty(d, d).cuda()
        dsrc1 = torch.ones(B * N, hh).cuda()
        _lib.check(L.ps_op_att_pool_train_fwd_split(h, p(fsrc), hh, p(idx), B, N, M, p(fx), hh, p(W), K, d, p(agg1)))
        _lib.check(L.ps_op_att_pool_train_bwd_split(h, p(fsrc), hh, p(idx), B, N, M, p(fx), hh, p(W), p(dagg), K, d, p(dsrc1), hh, p(dfx), hh, p(dW1)))
        assert torch.equal(agg0, agg1), d
        # the float-atomic scatter form runs attpool_train.hip's per-point kernels at every width; the materialised form takes
        # attpool_gemm.hip's matrix-pipe kernel at d = 64: same values to fp32 rounding there, bit for bit elsewhere
        if d == 64:
            assert (dcat[:, hh:] - dfx).abs().max() <= 2e-5 * dfx.abs().max() and (dW0 - dW1).abs().max() <= 2e-5 * dW0.abs().max(), d
        else:
            assert torch.equal(dcat[:, hh:], dfx), d
            assert torch.equal(dW0, dW1), d
        assert (dsrc0 - dsrc1).abs().max() <= (2e-5 if d == 64 else 2e-6) * dsrc0.abs().max(), d
        # the row-output form (the deterministic step's): the same kernel as the materialised form at every width -- bit-identical, the
        # gathered half as plain rows equal to the left columns of the materialised gradient
        rows, dfx2, dW2 = torch.empty(B * M * K, hh).cuda(), torch.empty(B * M * K, hh).cuda(), torch.empty(d, d).cuda()
        _lib.check(L.ps_op_att_pool_train_bwd_split_rows(h, p(fsrc), hh, p(idx), B, N, M, p(fx), hh, p(W), p(dagg), K, d, p(rows), hh, p(dfx2), hh, p(dW2)))
        assert torch.equal(dcat[:, hh:], dfx2) and torch.equal(dcat[:, :hh].contiguous(), rows) and torch.equal(dW0, dW2), d
    torch.cuda.synchronize()


def test_fused_locse_branch_against_float64_autograd():
    """ps_op_locse_train_sums / _apply / _bwd (the LocSE branch recomputed from coordinates and indices, csrc/locse_train.hip) against
    torch float64 autograd of LeakyReLU(BN_train(enc10 . W + b)): batch statistics, output, and -- through the caller-side finishing
    arithmetic of Tape.locse_bn_act -- dW, db, dgamma, dbeta.  Two clouds, h = 8 / 16 / 32 / 64, strided output."""
    import torch
    from point_unet_amd import _lib, runtime
    from point_unet_amd.train import Tape, BN_EPS
    ctx = runtime.default_context(0)
    g = torch.Generator().manual_seed(3)
    B, N, K = 2, 900, 16
    xyz = torch.rand(B * N, 3, generator=g).cuda()
    idx = torch.randint(0, N, (B, N, K), generator=g, dtype=torch.int32).cuda()
    for h in (8, 16, 32, 64):
        assert _lib.lib().ps_op_locse_train_supported(K, h) == 1
        W = (torch.randn(10, h, generator=g) * 0.5).cuda()
        b = (torch.randn(h, generator=g) * 0.1).cuda()
        gamma, beta = (1 + 0.2 * torch.randn(h, generator=g)).cuda(), (0.1 * torch.randn(h, generator=g)).cuda()
        gW, gb, gg, gbt = torch.zeros_like(W), torch.zeros_like(b), torch.zeros_like(gamma), torch.zeros_like(beta)
        mm, mv = torch.zeros(h).cuda(), torch.ones(h).cuda()
        t = Tape(ctx, None)
        wide = torch.zeros(B * N * K, 2 * h).cuda()
        y = t.locse_bn_act(xyz, idx, B, W, b, gW, gb, gamma, beta, gg, gbt, mm, mv, out=wide[:, h:])
        dz = torch.randn(B * N * K, h, generator=g).cuda()
        t.backward(y, dz)
        torch.cuda.synchronize()
        # float64 reference
        X, I = xyz.double().reshape(B, N, 3), idx.long()
        nb = torch.stack([X[bb][I[bb]] for bb in range(B)])
        ctr = X[:, :, None, :].expand_as(nb)
        rel = ctr - nb
        enc = torch.cat([rel.pow(2).sum(-1, keepdim=True).sqrt(), rel, ctr, nb], -1).reshape(-1, 10)
        Wd, bd, gd, btd = [v.double().clone().requires_grad_(True) for v in (W, b, gamma, beta)]
        yy = enc @ Wd + bd
        mean, var = yy.mean(0), yy.var(0, unbiased=False)
        z = torch.nn.functional.leaky_relu((yy - mean) / torch.sqrt(var + BN_EPS) * gd + btd, 0.2)
        (z * dz.double()).sum().backward()
        errs = dict(out=(wide[:, h:].double() - z).abs().max().item() / z.abs().max().item(),
                    mean=(mm.double() / 0.01 - mean).abs().max().item(), var=((mv.double() - 0.99) / 0.01 - var).abs().max().item() / var.max().item(),
                    dW=(gW.double() - Wd.grad).abs().max().item() / Wd.grad.abs().max().item(),
                    dgamma=(gg.double() - gd.grad).abs().max().item() / gd.grad.abs().max().item(),
                    dbeta=(gbt.double() - btd.grad).abs().max().item() / btd.grad.abs().max().item(),
                    db=(gb.double() - bd.grad).abs().max().item() / Wd.grad.abs().max().item())
        print(h, errs)
        # measured: out 2.7e-7, mean 1e-7, var 6e-6 (read back through the fp32 moving-variance update), gradients 2e-6
        assert errs["out"] <= 2e-6 and errs["mean"] <= 2e-6 and errs["var"] <= 1e-4, (h, errs)
        assert errs["dW"] <= 2e-5 and errs["dgamma"] <= 2e-5 and errs["dbeta"] <= 2e-5 and errs["db"] <= 2e-5, (h, errs)


def test_large_fp32_gemms_on_split_bf16_mfma():
    """ps_op_conv1x1_ex at the matrix-pipe-bound shapes of the training step (>= 4096 rows -- 8192 in the bf16-MLP mode --, cin >= 128, cout % 128 == 0) runs on bf16 MFMA
    over exact three-way splits (csrc/gemm_b3.hip).  Against a float64 product: error no larger than the fp32-MFMA path's on the same
    inputs (+ 1e-6 of the output scale) -- measured 3e-7 both; ragged row count, strided input / output, bias + LeakyReLU, accumulate."""
    import ctypes
    import torch
    from point_unet_amd import _lib, runtime
    L, ctx = _lib.lib(), runtime.default_context(0)
    h = ctx.handle
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    g = torch.Generator().manual_seed(21)
    try:
        for R, K, N, leaky, acc in [(16384, 256, 128, 0, 0), (20001, 256, 256, 1, 0), (17500, 128, 256, 0, 1), (16385, 512, 512, 0, 0), (19000, 320, 256, 1, 1), (30000, 128, 128, 1, 0),
                                     (4097, 256, 128, 1, 0), (9001, 512, 256, 0, 1), (5624, 128, 384, 1, 1)]:  # (the last three: the 128-row workgroup form of few-row products)
            xw = torch.randn(R, K + 8, generator=g).cuda()
            x = xw[:, 4:K + 4]
            W = (torch.randn(K, N, generator=g) / K ** 0.5).cuda()
            b = torch.randn(N, generator=g).cuda()
            y0 = torch.randn(R, N + 4, generator=g).cuda()
            ref = x.double() @ W.double() + b.double()
            if leaky:
                ref = torch.where(ref >= 0, ref, 0.2 * ref)
            if acc:  # y += act(x . W + b)
                ref = ref + y0[:, :N].double()
            errs = {}
            for on in (1, 0):
                _lib.check(L.ps_set_train_gemm_b3(h, on))
                y = y0.clone()
                _lib.check(L.ps_op_conv1x1_ex(h, p(x), K + 8, p(W), p(b), R, K, N, leaky, acc, p(y), N + 4))
                errs[on] = ((y[:, :N].double() - ref).abs().max() / ref.abs().max()).item()
                assert torch.equal(y[:, N:], y0[:, N:])
            print(R, K, N, errs)
            assert errs[1] <= errs[0] + 1e-6 and errs[1] <= 2e-6, (R, K, N, errs)
    finally:
        _lib.check(L.ps_set_train_gemm_b3(h, 1))
    torch.cuda.synchronize()


def test_fused_square_conv_bn_branch_against_float64_autograd():
    """ps_op_conv_bn_train_* (conv c->c + BatchNorm(train) + LeakyReLU with the pre-BatchNorm product recomputed, csrc/smallconv_train.hip)
    through Tape.conv_bn_act against torch float64 autograd: output, batch statistics, dx, dW, db, dgamma, dbeta.  c = 8 / 16 / 32 / 64,
    ragged row count, strided input and output, input gradient written fresh and accumulated into an existing one."""
    import torch
    from point_unet_amd import runtime
    from point_unet_amd.train import Tape, BN_EPS
    ctx = runtime.default_context(0)
    g = torch.Generator().manual_seed(9)
    for C, R in ((8, 10007), (16, 4099), (32, 5003), (64, 3001)):
        wide_in = torch.randn(R, C + 8, generator=g).cuda()
        x = wide_in[:, 4:C + 4]
        x.requires_grad_flag = True
        W = (torch.randn(C, C, generator=g) / C ** 0.5).cuda()
        b = (0.1 * torch.randn(C, generator=g)).cuda()
        gamma, beta = (1 + 0.2 * torch.randn(C, generator=g)).cuda(), (0.1 * torch.randn(C, generator=g)).cuda()
        gW, gb, gg, gbt = torch.zeros_like(W), torch.zeros_like(b), torch.zeros_like(gamma), torch.zeros_like(beta)
        mm, mv = torch.zeros(C).cuda(), torch.ones(C).cuda()
        dz = torch.randn(R, C, generator=g).cuda()
        Xd = x.double().clone().requires_grad_(True)
        Wd, bd, gd, btd = [v.double().clone().requires_grad_(True) for v in (W, b, gamma, beta)]
        yy = Xd @ Wd + bd
        mean, var = yy.mean(0), yy.var(0, unbiased=False)
        z = torch.nn.functional.leaky_relu((yy - mean) / torch.sqrt(var + BN_EPS) * gd + btd, 0.2)
        (z * dz.double()).sum().backward()
        for prior in (False, True):
            t = Tape(ctx, None)
            wide_out = torch.zeros(R, 2 * C).cuda()
            y = t.conv_bn_act(x, W, b, gW, gb, gamma, beta, gg, gbt, mm.clone(), mv.clone(), out=wide_out[:, C:])
            extra = torch.randn(R, C, generator=g).cuda()
            if prior:
                t.grads[id(x)] = extra.clone()
            t.grads[id(y)] = dz
            for tt, bw in reversed(t.ops):
                gr = t.grads.pop(id(tt), None)
                if gr is not None:
                    bw(gr)
            dx = t.grads[id(x)]
            torch.cuda.synchronize()
            want_dx = Xd.grad + (extra.double() if prior else 0)
            rel = lambda a, r: (a.double() - r).abs().max().item() / r.abs().max().item()  # noqa: E731
            errs = dict(out=rel(wide_out[:, C:], z), dx=rel(dx, want_dx), dW=rel(gW, Wd.grad), dgamma=rel(gg, gd.grad), dbeta=rel(gbt, btd.grad),
                        db=(gb.double() - bd.grad).abs().max().item() / Wd.grad.abs().max().item())
            print(C, prior, errs)
            assert errs["out"] <= 2e-6 and errs["dx"] <= 2e-5 and errs["dW"] <= 2e-5 and errs["dgamma"] <= 2e-5 and errs["dbeta"] <= 2e-5 and errs["db"] <= 2e-5, (C, errs)
            assert torch.all(wide_out[:, :C] == 0)


def test_row_strided_variants_match_the_dense_ops():
    """ps_op_*_ex on column blocks of a wider tensor (the training step's concat buffers) give what the dense entry points give
    on contiguous copies; conv1x1_ex with accumulate adds in the epilogue."""
    import ctypes
    import torch
    from point_unet_amd import _lib, runtime
    L, ctx = _lib.lib(), runtime.default_context(0)
    h = ctx.handle
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    g = torch.Generator().manual_seed(5)
    for R, C, wide, off in [(4099, 16, 32, 16), (1237, 8, 16, 8), (530, 10, 23, 7), (2048, 64, 128, 64)]:
        buf = torch.randn(R, wide, generator=g).cuda()
        blk = buf[:, off:off + C]            # rows contiguous, row stride = wide
        dense = blk.contiguous()
        # conv1x1: strided input, strided output, then the accumulate epilogue
        cout = 24
        W = torch.randn(C, cout, generator=g).cuda()
        b = torch.randn(cout, generator=g).cuda()
        y_ref = torch.empty(R, cout).cuda()
        _lib.check(L.ps_op_conv1x1(h, p(dense), p(W), p(b), R, C, cout, 1, p(y_ref)))
        ybuf = torch.full((R, cout + 9), 7.0).cuda()
        yv = ybuf[:, 4:4 + cout]
        _lib.check(L.ps_op_conv1x1_ex(h, p(blk), wide, p(W), p(b), R, C, cout, 1, 0, p(yv), cout + 9))
        assert torch.equal(yv, y_ref) and float(ybuf[:, :4].min()) == 7.0 and float(ybuf[:, 4 + cout:].max()) == 7.0
        _lib.check(L.ps_op_conv1x1_ex(h, p(blk), wide, p(W), p(b), R, C, cout, 1, 1, p(yv), cout + 9))
        assert torch.allclose(yv, 2 * y_ref, rtol=0, atol=1e-6 * float(y_ref.abs().max()))
        # wgrad with both operands strided
        dybuf = torch.randn(R, cout + 5, generator=g).cuda()
        dyv = dybuf[:, 5:]
        dW, db = torch.empty(C, cout).cuda(), torch.empty(cout).cuda()
        _lib.check(L.ps_op_linear_wgrad_ex(h, p(blk), wide, p(dyv), cout + 5, R, C, cout, p(dW), p(db)))
        ref = dense.double().T @ dyv.double()
        assert (dW.double() - ref).abs().max() <= 1e-4 * ref.abs().max()
        assert (db.double() - dyv.double().sum(0)).abs().max() <= 1e-4 * dyv.double().sum(0).abs().max() + 1e-4
        # BatchNorm: y into a column block, dy read from a column block
        gamma, beta = torch.rand(C, generator=g).cuda() + 0.5, torch.randn(C, generator=g).cuda()
        x = (torch.randn(R, C, generator=g) * 2 + 0.5).cuda()
        st, st2 = torch.empty(5, C).cuda(), torch.empty(5, C).cuda()
        y_ref = torch.empty(R, C).cuda()
        _lib.check(L.ps_op_bn_train_fwd(h, p(x), p(gamma), p(beta), R, C, 1e-6, 1, p(y_ref), p(st[0]), p(st[1]), p(st[2]), p(st[3])))
        out = torch.zeros(R, wide).cuda()
        _lib.check(L.ps_op_bn_train_fwd_ex(h, p(x), p(gamma), p(beta), R, C, 1e-6, 1, p(out[:, off:off + C]), wide, p(st2[0]), p(st2[1]), p(st2[2]),
                                           p(st2[3])))
        assert torch.equal(out[:, off:off + C], y_ref) and torch.equal(st[:3], st2[:3])
        assert float(out[:, :off].abs().max()) == 0.0 and (off + C == wide or float(out[:, off + C:].abs().max()) == 0.0)
        dx_ref, dg_ref, db_ref = torch.empty(R, C).cuda(), torch.empty(C).cuda(), torch.empty(C).cuda()
        _lib.check(L.ps_op_bn_train_bwd(h, p(dense), p(x), p(gamma), p(beta), p(st[0]), p(st[1]), R, C, 1, p(dx_ref), p(dg_ref), p(db_ref)))
        dx, dg, dbt = torch.empty(R, C).cuda(), torch.empty(C).cuda(), torch.empty(C).cuda()
        _lib.check(L.ps_op_bn_train_bwd_ex(h, p(blk), wide, p(x), p(gamma), p(beta), p(st[0]), p(st[1]), R, C, 1, p(dx), p(dg), p(dbt)))
        assert torch.equal(dx, dx_ref) and torch.equal(dg, dg_ref) and torch.equal(dbt, db_ref)
    # gather into a column block / scatter-add from a column block
    B, N, M, K, d = 2, 300, 170, 5, 12
    pc = torch.randn(B * N, d, generator=g).cuda()
    idx = torch.randint(0, N, (B, M, K), generator=g).int().cuda()
    ref = torch.empty(B * M * K, d).cuda()
    _lib.check(L.ps_op_gather_neighbour(h, p(pc), p(idx), B, N, M, K, d, p(ref)))
    wide = torch.zeros(B * M * K, 2 * d).cuda()
    _lib.check(L.ps_op_gather_neighbour_ex(h, p(pc), p(idx), B, N, M, K, d, p(wide[:, :d]), 2 * d))
    assert torch.equal(wide[:, :d], ref) and float(wide[:, d:].abs().max()) == 0.0
    drows = torch.randn(B * M * K, 2 * d, generator=g).cuda()
    acc_ref, acc = torch.zeros(B * N, d).cuda(), torch.zeros(B * N, d).cuda()
    _lib.check(L.ps_op_scatter_add_rows(h, p(drows[:, d:].contiguous()), p(idx), B, N, M * K, d, p(acc_ref)))
    _lib.check(L.ps_op_scatter_add_rows_ex(h, p(drows[:, d:]), 2 * d, p(idx), B, N, M * K, d, p(acc)))
    assert torch.allclose(acc, acc_ref, rtol=0, atol=1e-5)
    torch.cuda.synchronize()


def test_bf16_mlp_mode_rounds_operands_and_accumulates_in_fp32():
    """ps_set_train_gemm_bf16: the GEMM ops equal a float64 GEMM of the bf16-rounded operands (so the only error left is the fp32
    accumulation), they differ from the fp32 result by bf16 rounding, and a whole training step in that mode stays close to the
    fp32 step (loss within 1 %, gradient direction cosine > 0.99)."""
    import ctypes
    import torch
    from point_unet_amd import _lib, runtime
    L, ctx = _lib.lib(), runtime.default_context(0)
    h = ctx.handle
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    g = torch.Generator().manual_seed(9)
    rb = lambda t: t.bfloat16().double()  # noqa: E731  (round-to-nearest-even, like v_cvt_pk_bf16_f32)
    try:
        _lib.check(L.ps_set_train_gemm_bf16(h, 1))
        for R, cin, cout in [(5000, 64, 64), (777, 128, 256), (333, 16, 32), (4099, 32, 16), (100, 512, 128)]:
            x, W = torch.randn(R, cin, generator=g).cuda(), (torch.randn(cin, cout, generator=g) / cin ** 0.5).cuda()
            b = torch.randn(cout, generator=g).cuda()
            y = torch.empty(R, cout).cuda()
            _lib.check(L.ps_op_conv1x1(h, p(x), p(W), p(b), R, cin, cout, 0, p(y)))
            ref = rb(x) @ rb(W) + b.double()
            assert (y.double() - ref).abs().max() <= 2e-5 * ref.abs().max(), (R, cin, cout)
            full = x.double() @ W.double() + b.double()
            assert 1e-5 * full.abs().max() < (y.double() - full).abs().max() < 3e-2 * full.abs().max()  # it IS a bf16 product
            dy = torch.randn(R, cout, generator=g).cuda()
            dW, db = torch.empty(cin, cout).cuda(), torch.empty(cout).cuda()
            _lib.check(L.ps_op_linear_wgrad(h, p(x), p(dy), R, cin, cout, p(dW), p(db)))
            ref = rb(x).T @ rb(dy)
            assert (dW.double() - ref).abs().max() <= 1e-4 * ref.abs().max(), (R, cin, cout)
            assert (db.double() - dy.double().sum(0)).abs().max() <= 1e-4 * dy.double().sum(0).abs().max() + 1e-4   # bias sums stay fp32
        # layers the bf16 kernel does not cover (channel count not a multiple of 16) stay exact fp32
        x, W = torch.randn(1000, 10, generator=g).cuda(), torch.randn(10, 8, generator=g).cuda()
        y = torch.empty(1000, 8).cuda()
        _lib.check(L.ps_op_conv1x1(h, p(x), p(W), None, 1000, 10, 8, 0, p(y)))
        assert (y.double() - x.double() @ W.double()).abs().max() < 1e-5
    finally:
        _lib.check(L.ps_set_train_gemm_bf16(h, 0))
    from point_unet_amd.train import Trainer
    cfg, xyz, feats = netcase.small_deep(12000, seed=4, B=1)
    labels = np.random.default_rng(3).integers(0, cfg.num_classes, xyz.shape[:2]).astype(np.int32)
    out = {}
    for mode in ("fp32", "bf16"):
        tr, pyr, params, _, cw, _ = _setup(cfg, xyz, feats, labels=labels, oracle_pyramid=False, mlp_dtype=mode)
        loss = tr.train_step(pyr, torch.from_numpy(feats).cuda(), torch.from_numpy(labels).cuda())
        torch.cuda.synchronize()
        out[mode] = (float(loss), tr.grad.double().cpu())
    assert abs(out["bf16"][0] - out["fp32"][0]) <= 1e-2 * abs(out["fp32"][0])
    cos = float((out["bf16"][1] * out["fp32"][1]).sum() / (out["bf16"][1].norm() * out["fp32"][1].norm()))
    assert cos > 0.99, cos
    assert not torch.equal(out["bf16"][1], out["fp32"][1])


def test_streaming_gemm_for_millions_of_rows():
    """The [N*K, d] GEMMs of the training step (>= 524 288 rows x column blocks, <= 128 input channels) run the persistent
    streaming kernel: fp32 and bf16 flavours, strided input, the accumulate epilogue, ragged last tile."""
    import ctypes
    import torch
    from point_unet_amd import _lib, runtime
    L, ctx = _lib.lib(), runtime.default_context(0)
    h = ctx.handle
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    g = torch.Generator(device="cuda").manual_seed(3)
    # (the last three: the thread-per-row kernel of the tiny level-0 convolutions, >= 2^20 rows, 8 / 16 channels; with 8 input channels the
    #  bf16 mode leaves the operands alone, like the MFMA flavours: their K axis is not a multiple of 16)
    for R, cin, cout, wide in [(600_007, 64, 64, 64), (530_001, 16, 16, 32), (300_011, 128, 128, 128), (540_000, 32, 64, 48),
                               (1_100_003, 8, 8, 12), (1_060_001, 16, 8, 16), (1_050_000, 8, 16, 8)]:
        buf = torch.randn(R, wide, generator=g, device="cuda")
        x = buf[:, wide - cin:]
        W = torch.randn(cin, cout, generator=g, device="cuda") / cin ** 0.5
        b = torch.randn(cout, generator=g, device="cuda")
        ref = x.double() @ W.double() + b.double()
        y = torch.empty(R, cout, device="cuda")
        _lib.check(L.ps_op_conv1x1_ex(h, p(x), wide, p(W), p(b), R, cin, cout, 0, 0, p(y), cout))
        assert (y.double() - ref).abs().max() <= 2e-5 * ref.abs().max(), (R, cin, cout)
        _lib.check(L.ps_op_conv1x1_ex(h, p(x), wide, p(W), p(b), R, cin, cout, 1, 1, p(y), cout))   # y += lrelu(...)
        want = ref + torch.nn.functional.leaky_relu(ref, 0.2)
        assert (y.double() - want).abs().max() <= 4e-5 * want.abs().max(), (R, cin, cout)
        try:
            _lib.check(L.ps_set_train_gemm_bf16(h, 1))
            _lib.check(L.ps_op_conv1x1_ex(h, p(x), wide, p(W), p(b), R, cin, cout, 0, 0, p(y), cout))
        finally:
            _lib.check(L.ps_set_train_gemm_bf16(h, 0))
        refb = (x.bfloat16().double() @ W.bfloat16().double() + b.double()) if cin % 16 == 0 else ref
        assert (y.double() - refb).abs().max() <= 2e-5 * refb.abs().max(), (R, cin, cout)
        del buf, x, y, ref, refb, want
    torch.cuda.synchronize()


def test_a_pooling_table_that_is_not_the_neighbour_prefix_still_gets_correct_gradients():
    """ps_randla_train_step accepts any caller-filled ps_pyramid.  The deterministic max-pool backward walks the PREFIX of the neighbour
    table's inverse index, which is only right when sub_idx[i] = neigh_idx[i][:, :M] (what ps_pyramid_build writes).  The trainer compares
    the two tables once per table and takes the float-atomic form for a pooling table that is something else: here level 0 pools over the
    neighbour rows of OTHER points, and the default (deterministic) trainer must agree with the all-atomic one to summation order."""
    import torch
    from point_unet_amd import weights
    from point_unet_amd.pyramid import build_pyramid
    from point_unet_amd.train import Trainer
    cfg, xyz, feats = netcase.small_deep(6000, seed=31, B=2)
    params = weights.init_params(cfg, seed=5, randomize_bn=True)
    labels = np.random.default_rng(3).integers(0, cfg.num_classes, xyz.shape[:2]).astype(np.int32)
    pyr = build_pyramid(torch.from_numpy(xyz).cuda(), cfg)
    assert pyr.struct.built != 0  # ps_pyramid_build vouches for its own tables ...
    pyr.struct.built = 0          # ... a caller that is about to rewrite one takes that back (include/pointseg.h, ps_pyramid.built)
    M = pyr.sub_idx[0].shape[1]
    prefix = pyr.sub_idx[0].clone()
    d_feats, d_lab = torch.from_numpy(feats).cuda(), torch.from_numpy(labels).cuda()
    grads = {}
    for det in (True, False):
        with Trainer(cfg, params=params, learning_rate=1e-3, keep_prob=1.0, deterministic=det) as tr:
            # first a pass over the pyramid as built (the table IS the prefix: the fixed-order form runs) ...
            pyr.sub_idx[0].copy_(prefix)
            tr.backward_only(pyr, d_feats, d_lab)
            # ... then the SAME buffers rewritten in place -- same pointers, same shapes: a remembered "is a prefix" would now be stale
            # (the gradients were silently wrong) -- pooling every output over some other point's neighbourhood
            pyr.sub_idx[0].copy_(pyr.neigh_idx[0][:, M:2 * M, :])
            loss = float(tr.backward_only(pyr, d_feats, d_lab))
            torch.cuda.synchronize()
            grads[det] = (loss, tr.grad.double().clone())
    assert grads[True][0] == grads[False][0]
    rel = float((grads[True][1] - grads[False][1]).norm() / grads[False][1].norm())
    assert rel <= 1e-5, rel


def test_weight_gradients_on_the_second_stream_change_nothing():
    """Trainer(overlap_wgrad=True) (ps_train_options.overlap_wgrad): the weight-gradient products run on a second HIP stream of the trainer
    behind events of the main one, their operands held until the step's reduction launch.  Same kernels on the same data: losses,
    gradients, parameters and moving statistics of three steps equal the one-stream step bit for bit."""
    import torch
    from point_unet_amd import weights
    from point_unet_amd.pyramid import build_pyramid
    from point_unet_amd.train import Trainer
    cfg, xyz, feats = netcase.small_deep(6000, seed=23, B=2)
    params = weights.init_params(cfg, seed=5, randomize_bn=True)
    labels = np.random.default_rng(3).integers(0, cfg.num_classes, xyz.shape[:2]).astype(np.int32)
    pyr = build_pyramid(torch.from_numpy(xyz).cuda(), cfg)
    d_feats, d_lab = torch.from_numpy(feats).cuda(), torch.from_numpy(labels).cuda()
    out = {}
    for side in (False, True):
        with Trainer(cfg, params=params, learning_rate=1e-3, keep_prob=0.5, overlap_wgrad=side) as tr:
            losses = []
            for _ in range(3):
                losses.append(float(tr.train_step(pyr, d_feats, d_lab)))
            torch.cuda.synchronize()
            out[side] = (losses, tr.flat.clone(), tr.grad.clone(), tr.flat_buffers.clone())
    assert out[True][0] == out[False][0]
    for a, b in zip(out[True][1:], out[False][1:]):
        assert torch.equal(a, b)


def test_rebinding_the_parameter_buffer_between_steps_drops_the_recorded_weight_images():
    """ps_trainer_bind with another parameter buffer (checkpoint reload, buffer swap) between two steps: the trainer replays its
    recorded weight-packing launches at the start of every step, over pointers into the parameter buffer of the step that recorded
    them -- a rebind must drop that recording.  Three steps with a rebind to fresh buffers after each (the old ones poisoned with NaN,
    standing in for freed memory) equal three steps of an undisturbed trainer bit for bit."""
    import torch
    from point_unet_amd import weights
    from point_unet_amd.pyramid import build_pyramid
    from point_unet_amd.train import Trainer
    cfg, xyz, feats = netcase.small_deep(6000, seed=21, B=2)
    params = weights.init_params(cfg, seed=5, randomize_bn=True)
    labels = np.random.default_rng(3).integers(0, cfg.num_classes, xyz.shape[:2]).astype(np.int32)
    pyr = build_pyramid(torch.from_numpy(xyz).cuda(), cfg)
    d_feats, d_lab = torch.from_numpy(feats).cuda(), torch.from_numpy(labels).cuda()
    out = {}
    for rebind in (False, True):
        with Trainer(cfg, params=params, learning_rate=1e-3, keep_prob=1.0) as tr:
            losses = []
            for _ in range(3):
                losses.append(float(tr.train_step(pyr, d_feats, d_lab)))
                torch.cuda.synchronize()
                if rebind:
                    for t in tr.rebind():
                        t.fill_(float("nan"))
            out[rebind] = (losses, tr.flat.clone(), tr.grad.clone(), tr.flat_buffers.clone())
    assert out[True][0] == out[False][0] and all(np.isfinite(out[True][0]))
    for a, b in zip(out[True][1:], out[False][1:]):
        assert torch.equal(a, b)


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_native_step_equals_the_python_tape(mode):
    """ps_randla_train_step (csrc/trainer.hip: tape, activation pool and moving-statistics updates in C++, ONE C-ABI call per step)
    against Trainer(engine="python") (the host-side tape of point-unet_amd/train.py recording the same op-level kernels): same
    parameters, same clouds, dropout ON (the mask is a counter hash of (element, step, rank): identical in both), two consecutive
    steps.  Same kernels in the same order; what differs is the [h]-sized finishing arithmetic of the LocSE BatchNorm (torch float ops
    there, one small kernel here: last-bit differences in mean / invstd) and the float atomics of the gradient sums, so the bars are:
    loss 2e-6 relative, logits 2e-5 of their magnitude, moving statistics 1e-5; gradients relative L2 5e-3 -- the bar of the fp32 step
    against float64 autograd: at 6 000 points the deepest BatchNorms see 23 rows and a last-bit change of an activation next to a
    leaky-ReLU kink moves the gradient by 1e-3 (measured between the engines: 2.7e-3) -- and parameters after Adam relative L2 1e-3
    (Adam moves a noise-level entry by up to 2 lr when its gradient's sign flips: max |diff| <= 2.1 lr)."""
    import torch
    from point_unet_amd import weights
    from point_unet_amd.pyramid import build_pyramid
    from point_unet_amd.train import Trainer
    cfg, xyz, feats = netcase.small_deep(6000, seed=21, B=2)
    params = weights.init_params(cfg, seed=5, randomize_bn=True)
    rng = np.random.default_rng(3)
    labels = rng.integers(0, cfg.num_classes, xyz.shape[:2]).astype(np.int32)
    cw = np.linspace(1.0, 2.0, cfg.num_classes).astype(np.float32)
    pyr = build_pyramid(torch.from_numpy(xyz).cuda(), cfg)
    d_feats, d_lab = torch.from_numpy(feats).cuda(), torch.from_numpy(labels).cuda()
    runs = {}
    for engine in ("native", "python"):
        tr = Trainer(cfg, params=params, learning_rate=1e-3, class_weights=cw, keep_prob=0.5, mlp_dtype=mode, engine=engine)
        assert tr.engine == engine and tr.num_params() == weights.num_params(cfg)
        out = []
        for _ in range(2):
            loss = tr.train_step(pyr, d_feats, d_lab)
            torch.cuda.synchronize()
            out.append(dict(loss=float(loss), logits=tr.last_logits.cpu().numpy().copy(), grad=tr.grad.cpu().numpy().copy(),
                            flat=tr.flat.cpu().numpy().copy(), buffers={k: v.cpu().numpy().copy() for k, v in tr.buffers.items()}))
        assert tr.step == 2
        runs[engine] = out
        if engine == "native":
            assert tr.pool_peak_bytes() > 0
        tr.close() if hasattr(tr, "close") else None
    for i, (a, b) in enumerate(zip(runs["native"], runs["python"])):
        # step 1 starts from identical parameters.  Step 2 starts from parameters that already differ by the first step's gradient noise
        # through Adam (lr 1e-3 moves a noise-level gradient entry by up to 2e-3 when its sign flips) and, at 6 000 points, runs
        # BatchNorms over 23 rows: it is only held to "the same training run" (loss 1 %, logits 5 % of their magnitude)
        if i == 0 and mode == "fp32":
            assert abs(a["loss"] - b["loss"]) <= 2e-6 * abs(b["loss"]), (a["loss"], b["loss"])
            assert np.abs(a["logits"].reshape(b["logits"].shape) - b["logits"]).max() <= 2e-5 * np.abs(b["logits"]).max()
            for k in b["buffers"]:
                assert np.abs(a["buffers"][k] - b["buffers"][k]).max() <= 1e-5 * max(1.0, np.abs(b["buffers"][k]).max()), k
            assert np.linalg.norm(a["grad"] - b["grad"]) <= 5e-3 * np.linalg.norm(b["grad"])
            assert np.abs(a["flat"] - b["flat"]).max() <= 2.1e-3
            assert np.linalg.norm(a["flat"] - b["flat"]) <= 1e-3 * np.linalg.norm(b["flat"])
        elif i == 0:
            # bf16 mode: a last-bit difference in a BatchNorm statistic moves activations across bfloat16 rounding boundaries -- the
            # rounded model's own sensitivity (test_training_step_at_the_true_width_ladder measures 0.125 on the gradient)
            assert abs(a["loss"] - b["loss"]) <= 1e-2 * abs(b["loss"]), (a["loss"], b["loss"])
            assert np.abs(a["logits"].reshape(b["logits"].shape) - b["logits"]).max() <= 0.1 * np.abs(b["logits"]).max()
            cos = float((a["grad"] * b["grad"]).sum() / (np.linalg.norm(a["grad"]) * np.linalg.norm(b["grad"])))
            assert cos >= 0.9, cos
        elif mode == "fp32":
            assert abs(a["loss"] - b["loss"]) <= 1e-2 * abs(b["loss"]), (a["loss"], b["loss"])
            assert np.abs(a["logits"].reshape(b["logits"].shape) - b["logits"]).max() <= 5e-2 * np.abs(b["logits"]).max()
            assert np.abs(a["flat"] - b["flat"]).max() <= 4.2e-3
        else:  # (bf16 mode, second step: two trajectories of a chaotic model -- only "still the same run")
            assert np.isfinite(a["loss"]) and abs(a["loss"] - b["loss"]) <= 5e-2 * abs(b["loss"]), (a["loss"], b["loss"])
            assert np.abs(a["flat"] - b["flat"]).max() <= 4.2e-3


def test_a_storage_flag_left_on_by_an_op_level_caller_does_not_reach_the_native_step():
    """ps_set_train_act_bf16 is a public setter of the op-level surface.  A flag left on for a SHARED context (an op-level
    experiment, a test that failed before its reset) must not leak into ps_randla_train_step, whose row reductions and split-source pooling
    read the flag directly outside the trainer's own scopes: the bf16-MLP step with the flag set beforehand is bit-identical to the step
    without it -- in both modes -- and the caller's flag is as it was afterwards."""
    import torch
    from point_unet_amd import _lib, runtime, weights
    from point_unet_amd.pyramid import build_pyramid
    from point_unet_amd.train import Trainer
    cfg, xyz, feats = netcase.small_deep(6000, seed=23, B=2)
    params = weights.init_params(cfg, seed=6, randomize_bn=True)
    labels = np.random.default_rng(4).integers(0, cfg.num_classes, xyz.shape[:2]).astype(np.int32)
    cw = np.linspace(1.0, 2.0, cfg.num_classes).astype(np.float32)
    pyr = build_pyramid(torch.from_numpy(xyz).cuda(), cfg)
    d_feats, d_lab = torch.from_numpy(feats).cuda(), torch.from_numpy(labels).cuda()
    L = _lib.lib()
    for mode in ("bf16", "fp32"):
        got = []
        for leaked in (0, 1):
            tr = Trainer(cfg, params=params, learning_rate=1e-3, class_weights=cw, keep_prob=1.0, mlp_dtype=mode)
            _lib.check(L.ps_set_train_act_bf16(tr.ctx.handle, leaked))
            try:
                loss = tr.train_step(pyr, d_feats, d_lab)
                torch.cuda.synchronize()
                got.append((float(loss), tr.grad.clone(), tr.flat.clone()))
            finally:
                _lib.check(L.ps_set_train_act_bf16(tr.ctx.handle, 0))
        assert got[0][0] == got[1][0], (mode, got[0][0], got[1][0])
        assert torch.equal(got[0][1], got[1][1]) and torch.equal(got[0][2], got[1][2]), mode


def test_backward_only_leaves_the_parameters_alone():
    """ps_randla_backward = the step without the collective and without Adam: gradients as train_step computes them, parameters and
    Adam moments untouched, moving statistics updated."""
    import torch
    from point_unet_amd import weights
    from point_unet_amd.pyramid import build_pyramid
    from point_unet_amd.train import Trainer
    cfg, xyz, feats = netcase.small_deep(3000, seed=4, B=1)
    params = weights.init_params(cfg, seed=6, randomize_bn=True)
    labels = np.random.default_rng(0).integers(0, cfg.num_classes, xyz.shape[:2]).astype(np.int32)
    pyr = build_pyramid(torch.from_numpy(xyz).cuda(), cfg)
    d_feats, d_lab = torch.from_numpy(feats).cuda(), torch.from_numpy(labels).cuda()
    a = Trainer(cfg, params=params, learning_rate=1e-3, keep_prob=1.0)
    b = Trainer(cfg, params=params, learning_rate=1e-3, keep_prob=1.0)
    before = a.flat.clone()
    la = a.backward_only(pyr, d_feats, d_lab)
    lb = b.train_step(pyr, d_feats, d_lab)
    torch.cuda.synchronize()
    assert abs(float(la) - float(lb)) <= 1e-6 * abs(float(lb))
    assert torch.equal(a.flat, before) and float(a.m.abs().max()) == 0.0 and a.step == 0
    assert not torch.equal(b.flat, before)
    assert np.linalg.norm((a.grad - b.grad).cpu().numpy()) <= 1e-4 * np.linalg.norm(b.grad.cpu().numpy())
    assert torch.allclose(a.flat_buffers, b.flat_buffers, rtol=1e-6, atol=1e-7)
    mm = a.buffers["Encoder_layer_0mlp1/batch_normalization/moving_mean"].cpu().numpy()
    assert not np.array_equal(mm, params["Encoder_layer_0mlp1/batch_normalization/moving_mean"])


def test_inverse_index_and_gather_reduction(oracle):
    """ps_op_inverse_index / ps_op_gather_reduce_rows / ps_op_random_sample_bwd_inv / ps_op_att_pool_train_bwd_split_rows (csrc/invidx.hip): the
    inverse of a gather table lists, per source row, the gathering rows in ASCENDING order; the gather-reduction over it equals the
    scatter-add (to summation order) and repeats bit for bit; duplicated indices inside one K-list (n < K clouds are padded with 0),
    rows nobody gathers, batches, strided gradient rows."""
    import ctypes
    import torch
    from point_unet_amd import _lib, runtime
    L, ctx = _lib.lib(), runtime.default_context(0)
    h = ctx.handle
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    g = torch.Generator().manual_seed(5)
    # (2, 700, ...) .. (1, 40, ...): the count / fill / sort form of small tables; from 65 536 rows on the bucket form (one stable bucket pass
    # + a sort inside every bucket): ragged bucket and tile counts, a 1-NN table, destinations nobody gathers, and "skew" = most rows gather
    # ONE destination (a bucket far beyond what is sorted through LDS).  The radix-sort form and the other bucket tiles run this list in
    # test_gpu_tuning_paths.py (knobs inv_bucket / inv_tile on a context of their own).
    for B, N, M, K, d, skew in [(2, 700, 700, 16, 8, 0), (1, 300, 1200, 1, 64, 0), (3, 500, 125, 16, 32, 0), (1, 40, 40, 16, 5, 0), (2, 40000, 40000, 16, 4, 0),
                                (3, 4133, 4133, 16, 8, 0), (2, 70001, 70001, 1, 4, 0), (1, 1000, 9000, 16, 4, 1), (5, 513, 1100, 16, 4, 0),
                                (1, 262144, 30000, 16, 4, 0), (1, 300000, 5000, 16, 4, 0)]:  # (the last: beyond 512 x 512 destinations per cloud -> the radix-sort form)
        idx = torch.randint(0, N, (B, M, K), generator=g).int()
        if skew:
            idx[:, M // 8:, 1:] = 77
        idx[:, : M // 7, K // 2:] = 0                       # zero padding / duplicates inside a list
        idx[idx == N - 1] = 0                                # a source row nobody gathers
        d_idx = idx.cuda()
        n_dst, rpc = B * N, M * K
        off = torch.empty(n_dst + 1, dtype=torch.int32, device="cuda")
        src = torch.empty(B * rpc, dtype=torch.int32, device="cuda")
        ws = torch.empty(int(L.ps_op_inverse_index_workspace(n_dst, B * rpc)), dtype=torch.int32, device="cuda")
        _lib.check(L.ps_op_inverse_index(h, p(d_idx), B, N, rpc, p(off), p(src), p(ws)))
        off_h, src_h = off.cpu().numpy(), src.cpu().numpy()
        flat = (idx.reshape(B, -1).numpy().astype(np.int64) + (np.arange(B) * N)[:, None]).reshape(-1)
        assert off_h[0] == 0 and off_h[-1] == B * rpc
        assert np.array_equal(np.diff(off_h), np.bincount(flat, minlength=n_dst))
        order = np.argsort(flat, kind="stable")              # ascending row inside every segment
        assert np.array_equal(src_h, order.astype(np.int32))
        # gather-reduction == scatter-add (float64 reference), strided rows, accumulate on and off
        wide = torch.randn(B * rpc, d + 4, generator=g).cuda()
        rows = wide[:, 2:d + 2]
        ref = torch.zeros(n_dst, d, dtype=torch.float64)
        ref.index_add_(0, torch.from_numpy(flat), rows.cpu().double())
        for acc in (0, 1):
            base = torch.randn(n_dst, d, generator=g).cuda()
            out = base.clone()
            _lib.check(L.ps_op_gather_reduce_rows(h, p(rows), d + 4, p(off), p(src), n_dst, d, p(out), d, acc))
            want = ref + (base.cpu().double() if acc else 0)
            assert (out.cpu().double() - want).abs().max() <= 1e-5 * max(1.0, want.abs().max())
            again = base.clone()
            _lib.check(L.ps_op_gather_reduce_rows(h, p(rows), d + 4, p(off), p(src), n_dst, d, p(again), d, acc))
            assert torch.equal(out, again)
            if d % 4 == 0:  # destinations walked in another order (the trainer: kd-tree leaf order, XCD by XCD): the same sums, bit for bit
                perm = torch.stack([torch.randperm(N, generator=g) for _ in range(B)]).int().cuda()
                walked = base.clone()
                _lib.check(L.ps_op_gather_reduce_rows_ordered(h, p(rows), d + 4, p(off), p(src), n_dst, d, p(walked), d, acc, p(perm), N))
                assert torch.equal(out, walked)
        # random_sample backward through the inverse index of the table whose first M2 rows per cloud are the pooling table (the pyramid's
        # sub_idx = neigh_idx[:, :M2]) == the atomics form on that prefix (ties included: quantised features)
        if K > 1 and M == N:
            M2 = max(1, M // 4)
            pool = idx[:, :M2].contiguous().cuda()
            feat = (torch.randint(0, 4, (B * N, d), generator=g).float() / 2).cuda()
            out = torch.empty(B * M2, d, device="cuda")
            _lib.check(L.ps_op_random_sample(h, p(feat), p(pool), B, N, M2, K, d, p(out)))
            dout = torch.randn(B * M2, d, generator=g).cuda()
            a = torch.zeros(B * N, d, device="cuda")
            _lib.check(L.ps_op_random_sample_bwd(h, p(dout), p(out), p(feat), p(pool), B, N, M2, K, d, p(a)))
            b = torch.zeros(B * N, d, device="cuda")
            share = torch.empty(B * M2, d, device="cuda")
            _lib.check(L.ps_op_random_sample_bwd_inv(h, p(dout), p(out), p(feat), p(pool), p(off), p(src), B, N, M2, K, d, None, p(share), p(b)))
            assert (a - b).abs().max() <= 5e-5 * max(1.0, float(a.abs().max()))
            if d % 4 == 0:  # the forward that leaves the tie counts: same output, and the backward without the recount pass
                out2 = torch.empty_like(out)
                ties = torch.empty((B * M2, d), dtype=torch.uint8, device="cuda")
                _lib.check(L.ps_op_random_sample_ties(h, p(feat), p(pool), B, N, M2, K, d, p(out2), p(ties)))
                assert torch.equal(out2, out) and int(ties.min()) >= 1
                b2 = torch.zeros(B * N, d, device="cuda")
                _lib.check(L.ps_op_random_sample_bwd_inv(h, p(dout), p(out), p(feat), p(pool), p(off), p(src), B, N, M2, K, d, p(ties), None, p(b2)))
                assert torch.equal(b2, b)
    torch.cuda.synchronize()


def test_weight_gradients_on_split_bf16_mfma():
    """ps_op_linear_wgrad_ex for many-row, 128-multiple shapes (>= 4096 rows -- 16384 in the bf16-MLP mode --, cin % 128 == 0, cout % 128 == 0) runs csrc/gemm_b3.hip's
    wgrad_b3_kernel: X^T . dY on bf16 MFMA over exact three-way splits, the row axis as K, per-slab partials summed in slab order.  Against
    a float64 product: error no larger than the fp32-MFMA kernel's on the same inputs (+ 1e-6 of the output scale); strided operands, ragged
    row counts, the bias gradient; two calls give bit-identical results (no float atomics)."""
    import ctypes
    import torch
    from point_unet_amd import _lib, runtime
    L, ctx = _lib.lib(), runtime.default_context(0)
    h = ctx.handle
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    g = torch.Generator().manual_seed(33)
    try:
        for R, cin, cout in [(16384, 128, 128), (20001, 256, 128), (17003, 128, 384), (40000, 128, 128), (4099, 256, 128), (5624, 128, 256)]:
            xw = torch.randn(R, cin + 8, generator=g).cuda()
            dw = torch.randn(R, cout + 4, generator=g).cuda()
            x, dy = xw[:, 4:cin + 4], dw[:, :cout]
            ref_w = x.double().t() @ dy.double()
            ref_b = dy.double().sum(0)
            errs, outs = {}, {}
            for on in (1, 0):
                _lib.check(L.ps_set_train_gemm_b3(h, on))
                gW = torch.full((cin, cout), 7.0, device="cuda")   # (overwritten, not accumulated into)
                gb = torch.full((cout,), 7.0, device="cuda")
                _lib.check(L.ps_op_linear_wgrad_ex(h, p(x), cin + 8, p(dy), cout + 4, R, cin, cout, p(gW), p(gb)))
                errs[on] = (((gW.double() - ref_w).abs().max() / ref_w.abs().max()).item(), ((gb.double() - ref_b).abs().max() / ref_b.abs().max()).item())
                outs[on] = (gW.clone(), gb.clone())
            _lib.check(L.ps_set_train_gemm_b3(h, 1))
            gW2, gb2 = torch.empty(cin, cout, device="cuda"), torch.empty(cout, device="cuda")
            _lib.check(L.ps_op_linear_wgrad_ex(h, p(x), cin + 8, p(dy), cout + 4, R, cin, cout, p(gW2), p(gb2)))
            print(R, cin, cout, errs)
            assert torch.equal(gW2, outs[1][0]) and torch.equal(gb2, outs[1][1])
            assert errs[1][0] <= errs[0][0] + 1e-6 and errs[1][0] <= 3e-6, (R, cin, cout, errs)
            assert errs[1][1] <= 1e-5, errs
    finally:
        _lib.check(L.ps_set_train_gemm_b3(h, 1))
    torch.cuda.synchronize()


def test_pyramid_prefetcher_feeds_the_same_pyramids():
    """PyramidPrefetcher (the next batch's pyramid built on its own stream while the current batch trains): three steps through it give the
    losses of three steps with the pyramid built in front of each step, bit for bit (deterministic step, same pyramids)."""
    import torch
    from point_unet_amd import weights
    from point_unet_amd.pipeline import PyramidPrefetcher
    from point_unet_amd.pyramid import build_pyramid
    from point_unet_amd.train import Trainer
    cfg, xyz, feats = netcase.small_deep(6000, seed=61, B=2)
    clouds = [torch.from_numpy(netcase.small_deep(6000, seed=61 + 3 * i, B=2)[1]).cuda() for i in range(3)]
    params = weights.init_params(cfg, seed=3, randomize_bn=True)
    labels = torch.from_numpy(np.random.default_rng(1).integers(0, cfg.num_classes, xyz.shape[:2]).astype(np.int32)).cuda()
    d_f = torch.from_numpy(feats).cuda()
    a = Trainer(cfg, params=params, learning_rate=1e-3, keep_prob=1.0)
    want = [float(a.train_step(build_pyramid(c, cfg), d_f, labels)) for c in clouds]
    b = Trainer(cfg, params=params, learning_rate=1e-3, keep_prob=1.0)
    pre = PyramidPrefetcher(cfg)
    pre.submit(clouds[0])
    got = []
    for i in range(3):
        if i + 1 < 3:
            pre.submit(clouds[i + 1])
        pyr, slot = pre.next()
        got.append(b.train_step(pyr, d_f, labels))
        pre.release(slot)
    torch.cuda.synchronize()
    pre.close()
    assert [float(g) for g in got] == want


def test_training_step_k32_two_classes(oracle):
    """The Pancreas shape family (BASELINE configs[4]: K = 32, 4 input channels, 2 classes; runPancreas.py:118,125) through the native
    training step: the fused attention / LocSE kernels are compiled for K = 16 only, so this runs the op-by-op forms at every level --
    loss, logits and gradients against torch-CPU float64 autograd at the bars of test_one_training_step_matches_autograd."""
    import torch
    from oracle import randla_train_oracle as rto
    # 9 000 points: the deepest level keeps 35 >= K of them (below K the neighbour lists are zero-padded and the BatchNorms of that level
    # see a couple of dozen rows: the float32 error of the logits then grows to several 1e-4)
    cfg, xyz, feats = netcase.small_deep(9000, seed=6, B=2, k_n=32, classes=2, mods=1)
    cfg.d_out = [16, 32, 64, 32, 16]
    tr, pyr, params, labels, cw, (pts, nbr, pool, up) = _setup(cfg, xyz, feats)
    loss = tr.train_step(pyr, torch.from_numpy(feats).cuda(), torch.from_numpy(labels).cuda())
    torch.cuda.synchronize()
    want = rto.train_step(params, cfg.num_layers, pts, nbr, pool, up, feats, labels, cw, lr=1e-3, step=1)
    assert abs(float(loss) - want["loss"]) <= 1e-5 * max(1.0, abs(want["loss"])), (float(loss), want["loss"])
    err = np.abs(tr.last_logits.cpu().numpy().reshape(want["logits"].shape) - want["logits"]).max()
    assert err <= 1e-4 * max(1.0, np.abs(want["logits"]).max() / 4), err
    gscale = max(np.abs(g).max() for g in want["grads"].values())
    worst = []
    for name in tr.names:
        got = tr.G[name].cpu().numpy()
        ref = want["grads"][name]
        worst.append((float(np.abs(got - ref).max() / (2e-3 * np.abs(ref).max() + 2e-5 * gscale)), name))
    worst.sort(reverse=True)
    print("K = 32 step: logits err %.2e, worst gradient tensors %s" % (err, worst[:3]))
    assert worst[0][0] <= 1.0, worst[:5]@pytest.mark.gpu
def test_square_conv_bn_passes_of_the_native_step_against_float64_autograd():
    """The form of the conv c->c + BatchNorm(train) + LeakyReLU recompute passes that csrc/trainer.hip drives (ps_op_conv_bn_train_sums /
    _apply / _bwd_sums2 / _bwd_apply_w: the weight and bias gradients come out of the apply pass as x^T dy and sum dy; c = 8 on the
    one-thread-per-row kernels of csrc/convbn_rows.hip, wider layers on the 16-row tiles) against torch float64 autograd: output, S1 / S2
    (= dbeta / dgamma), dx written fresh and added to an existing gradient, dW, db.  Ragged row counts; c = 8 also at a row count that
    makes every thread loop (> 2048 x 256 rows), and run twice for bit-identical results."""
    import ctypes
    import torch
    from point_unet_amd import runtime, _lib
    from point_unet_amd.train import BN_EPS
    ctx = runtime.default_context(0)
    L = _lib.lib()
    vp = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    g = torch.Generator().manual_seed(19)
    for C, R in ((8, 10007), (8, 600011), (16, 4099), (32, 5003), (64, 3001)):
        CP = max(C, 16)
        x = torch.randn(R, C, generator=g).cuda()
        W = (torch.randn(C, C, generator=g) / C ** 0.5).cuda()
        b = (0.1 * torch.randn(C, generator=g)).cuda()
        gamma, beta = (1 + 0.2 * torch.randn(C, generator=g)).cuda(), (0.1 * torch.randn(C, generator=g)).cuda()
        dz = torch.randn(R, C, generator=g).cuda()
        Xd = x.double().clone().requires_grad_(True)
        Wd, bd, gd, btd = [v.double().clone().requires_grad_(True) for v in (W, b, gamma, beta)]
        yy = Xd @ Wd + bd
        mean_d, var_d = yy.mean(0), yy.var(0, unbiased=False)
        z_d = torch.nn.functional.leaky_relu((yy - mean_d) / torch.sqrt(var_d + BN_EPS) * gd + btd, 0.2)
        (z_d * dz.double()).sum().backward()
        sums = torch.zeros(3 * CP, dtype=torch.float64).cuda()
        assert L.ps_op_conv_bn_train_sums(ctx.handle, vp(x), C, vp(W), vp(b), R, C, vp(sums)) == 0
        mean64 = sums[:C] / R
        var64 = (sums[CP:CP + C] / R - mean64 * mean64).clamp_min(0)
        assert (mean64 - mean_d.detach()).abs().max().item() <= 1e-6 and (var64 - var_d.detach()).abs().max().item() <= 1e-6 * var_d.max().item() + 1e-7
        assert (sums[2 * CP:2 * CP + C] - x.double().sum(0)).abs().max().item() <= 1e-6 * R ** 0.5 + 1e-4
        mean, var = mean64.float(), var64.float()
        invstd = torch.rsqrt(var + BN_EPS)
        scale = gamma * invstd
        z = torch.empty(R, C).cuda()
        assert L.ps_op_conv_bn_train_apply(ctx.handle, vp(x), C, vp(W), vp(b), R, C, vp(mean), vp(scale), vp(beta), vp(z), C) == 0
        rel = lambda a, r: (a.double() - r).abs().max().item() / r.abs().max().item()  # noqa: E731
        assert rel(z, z_d.detach()) <= 2e-6
        s12 = torch.zeros(3 * C).cuda()
        assert L.ps_op_conv_bn_train_bwd_sums2(ctx.handle, vp(x), C, vp(W), vp(b), R, C, vp(mean), vp(invstd), vp(scale), vp(beta), vp(dz), C, vp(s12)) == 0
        assert rel(s12[:C], btd.grad) <= 2e-5 and rel(s12[C:2 * C], gd.grad) <= 2e-5
        first = None
        for prior in (False, True, True):
            extra = torch.randn(R, C, generator=torch.Generator().manual_seed(5)).cuda()
            dx = extra.clone() if prior else torch.full((R, C), float("nan")).cuda()
            dw, db = torch.full((C, C), float("nan")).cuda(), torch.full((C,), float("nan")).cuda()
            assert L.ps_op_conv_bn_train_bwd_apply_w(ctx.handle, vp(x), C, vp(W), vp(b), R, C, vp(mean), vp(invstd), vp(scale), vp(beta), vp(s12),
                                                     ctypes.c_float(1.0 / R), vp(dz), C, 1 if prior else 0, vp(dx), C, vp(dw), vp(db)) == 0
            torch.cuda.synchronize()
            want_dx = Xd.grad + (extra.double() if prior else 0)
            errs = dict(dx=rel(dx, want_dx), dW=rel(dw, Wd.grad), db=(db.double() - bd.grad).abs().max().item() / Wd.grad.abs().max().item())
            print(C, R, prior, errs)
            assert errs["dx"] <= 2e-5 and errs["dW"] <= 2e-5 and errs["db"] <= 2e-5, (C, R, errs)
            if prior:
                if first is None:
                    first = (dx.clone(), dw.clone(), db.clone())
                else:
                    assert torch.equal(first[0], dx) and torch.equal(first[1], dw) and torch.equal(first[2], db)


@pytest.mark.gpu
def test_widening_conv_bn_passes_against_float64_autograd():
    """ps_op_convbn_train_* (csrc/rectconv_train.hip: conv cin -> cout + BatchNorm(train) [+ LeakyReLU] with the pre-BatchNorm product recomputed;
    Encoder mlp2 / shortcut and fc1 of the native step) against torch float64 autograd for every compiled (cin, cout): batch statistics,
    output with and without the activation, S1 / S2 (= dbeta / dgamma), dx fresh / added to an existing gradient / not asked for, dW, db;
    ragged row counts, strided x; the backward run twice for bit-identical results."""
    import ctypes
    import torch
    from point_unet_amd import runtime, _lib
    from point_unet_amd.train import BN_EPS
    ctx = runtime.default_context(0)
    L = _lib.lib()
    vp = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    g = torch.Generator().manual_seed(23)
    assert not L.ps_op_convbn_train_supported(32, 32) and not L.ps_op_convbn_train_supported(64, 32)
    for (CI, CO), R, leaky in (((8, 32), 10007, 0), ((16, 32), 70001, 1), ((32, 64), 5003, 1), ((32, 128), 3001, 0), ((64, 128), 4099, 0), ((64, 128), 777, 1)):
        assert L.ps_op_convbn_train_supported(CI, CO)
        wide = torch.randn(R, CI + 8, generator=g).cuda()
        x = wide[:, 4:CI + 4]
        ldx = CI + 8
        W = (torch.randn(CI, CO, generator=g) / CI ** 0.5).cuda()
        b = (0.1 * torch.randn(CO, generator=g)).cuda()
        gamma, beta = (1 + 0.2 * torch.randn(CO, generator=g)).cuda(), (0.1 * torch.randn(CO, generator=g)).cuda()
        dz = torch.randn(R, CO, generator=g).cuda()
        Xd = x.double().clone().requires_grad_(True)
        Wd, bd, gd, btd = [v.double().clone().requires_grad_(True) for v in (W, b, gamma, beta)]
        yy = Xd @ Wd + bd
        mean_d, var_d = yy.mean(0), yy.var(0, unbiased=False)
        z_d = (yy - mean_d) / torch.sqrt(var_d + BN_EPS) * gd + btd
        if leaky:
            z_d = torch.nn.functional.leaky_relu(z_d, 0.2)
        (z_d * dz.double()).sum().backward()
        sums = torch.zeros(2 * CO, dtype=torch.float64).cuda()
        assert L.ps_op_convbn_train_sums(ctx.handle, vp(x), ldx, vp(W), vp(b), R, CI, CO, vp(sums)) == 0
        mean64 = sums[:CO] / R
        var64 = (sums[CO:] / R - mean64 * mean64).clamp_min(0)
        assert (mean64 - mean_d.detach()).abs().max().item() <= 1e-6 and (var64 - var_d.detach()).abs().max().item() <= 1e-6 * var_d.max().item() + 1e-7
        mean, var = mean64.float(), var64.float()
        invstd = torch.rsqrt(var + BN_EPS)
        scale = gamma * invstd
        z = torch.empty(R, CO).cuda()
        assert L.ps_op_convbn_train_apply(ctx.handle, vp(x), ldx, vp(W), vp(b), R, CI, CO, vp(mean), vp(scale), vp(beta), leaky, vp(z), CO) == 0
        rel = lambda a, r: (a.double() - r).abs().max().item() / r.abs().max().item()  # noqa: E731
        assert rel(z, z_d.detach()) <= 2e-6, (CI, CO, rel(z, z_d.detach()))
        if not leaky:  # the residual sum of dilated_res_block inside the apply pass == the apply pass followed by ps_op_add_lrelu, bit for bit
            addw = torch.randn(R, CO + 4, generator=g).cuda()
            addend = addw[:, :CO]  # (a strided addend: ld_add = CO + 4)
            fused, two = torch.empty(R, CO).cuda(), torch.empty(R, CO).cuda()
            assert L.ps_op_convbn_train_apply_add(ctx.handle, vp(x), ldx, vp(W), vp(b), R, CI, CO, vp(mean), vp(scale), vp(beta), vp(addend), CO + 4, vp(fused),
                                                  CO) == 0
            ac = addend.contiguous()
            assert L.ps_op_add_lrelu(ctx.handle, vp(z), vp(ac), R * CO, vp(two)) == 0
            assert torch.equal(fused, two), (CI, CO)
        s12 = torch.zeros(2 * CO).cuda()
        assert L.ps_op_convbn_train_bwd_sums(ctx.handle, vp(x), ldx, vp(W), vp(b), R, CI, CO, vp(mean), vp(invstd), vp(scale), vp(beta), leaky, vp(dz), CO,
                                             vp(s12)) == 0
        assert rel(s12[:CO], btd.grad) <= 2e-5 and rel(s12[CO:], gd.grad) <= 2e-5
        first = None
        for prior in (0, 1, 1, None):
            extra = torch.randn(R, CI, generator=torch.Generator().manual_seed(5)).cuda()
            dx = None if prior is None else (extra.clone() if prior else torch.full((R, CI), float("nan")).cuda())
            dw, db = torch.full((CI, CO), float("nan")).cuda(), torch.full((CO,), float("nan")).cuda()
            assert L.ps_op_convbn_train_bwd_apply(ctx.handle, vp(x), ldx, vp(W), vp(b), R, CI, CO, vp(mean), vp(invstd), vp(scale), vp(beta), leaky, vp(s12),
                                                  ctypes.c_float(1.0 / R), vp(dz), CO, 1 if prior else 0, vp(dx), CI, vp(dw), vp(db)) == 0
            torch.cuda.synchronize()
            errs = dict(dW=rel(dw, Wd.grad), db=(db.double() - bd.grad).abs().max().item() / Wd.grad.abs().max().item())
            if dx is not None:
                errs["dx"] = rel(dx, Xd.grad + (extra.double() if prior else 0))
            print(CI, CO, R, leaky, prior, errs)
            assert max(errs.values()) <= 2e-5, (CI, CO, R, errs)
            if prior == 1:
                if first is None:
                    first = (dx.clone(), dw.clone(), db.clone())
                else:
                    assert torch.equal(first[0], dx) and torch.equal(first[1], dw) and torch.equal(first[2], db)


@pytest.mark.gpu
def test_native_step_with_recomputed_square_convolutions():
    """Trainer(fused_convbn=True) (ps_train_options.fused_convbn: LFA mlp2 of every level with h <= 64, and the widening shared MLPs -- Encoder
    mlp2 / shortcut of levels 0-1, fc1 --, in the recompute form) against the
    op-by-op native step: same parameters and clouds, one step.  fp32: loss 2e-6, logits 2e-5 of their magnitude, moving statistics 1e-5,
    gradients 5e-3 relative L2 (the bar between the two engines; the recompute form sums in a different order).  bf16-MLP mode: the
    tile kernels round the operands of their products like the GEMMs they replace (the h = 8 layer is fp32 in both forms) -- held to the
    bf16 bars of the engine test.
    Also: two runs of the fused step give bit-identical gradients."""
    import torch
    from point_unet_amd import weights
    from point_unet_amd.pyramid import build_pyramid
    from point_unet_amd.train import Trainer
    cfg, xyz, feats = netcase.small_deep(6000, seed=23, B=2)
    params = weights.init_params(cfg, seed=6, randomize_bn=True)
    rng = np.random.default_rng(4)
    labels = rng.integers(0, cfg.num_classes, xyz.shape[:2]).astype(np.int32)
    cw = np.linspace(1.0, 2.0, cfg.num_classes).astype(np.float32)
    pyr = build_pyramid(torch.from_numpy(xyz).cuda(), cfg)
    d_feats, d_lab = torch.from_numpy(feats).cuda(), torch.from_numpy(labels).cuda()
    for mode in ("fp32", "bf16"):
        runs = []
        for fused in (True, True, False):
            tr = Trainer(cfg, params=params, learning_rate=1e-3, class_weights=cw, keep_prob=0.5, mlp_dtype=mode, fused_convbn=fused)
            assert tr.engine == "native"
            loss = tr.train_step(pyr, d_feats, d_lab)
            torch.cuda.synchronize()
            runs.append(dict(loss=float(loss), logits=tr.last_logits.cpu().numpy().copy(), grad=tr.grad.cpu().numpy().copy(),
                             buffers={k: v.cpu().numpy().copy() for k, v in tr.buffers.items()}))
            tr.close()
        a, a2, b = runs
        assert a["loss"] == a2["loss"] and np.array_equal(a["grad"], a2["grad"]) and np.array_equal(a["logits"], a2["logits"])
        assert not np.array_equal(a["grad"], b["grad"])  # (the switch does switch something)
        if mode == "fp32":
            assert abs(a["loss"] - b["loss"]) <= 2e-6 * abs(b["loss"]), (a["loss"], b["loss"])
            assert np.abs(a["logits"] - b["logits"]).max() <= 2e-5 * np.abs(b["logits"]).max()
            for k in b["buffers"]:
                assert np.abs(a["buffers"][k] - b["buffers"][k]).max() <= 1e-5 * max(1.0, np.abs(b["buffers"][k]).max()), k
            assert np.linalg.norm(a["grad"] - b["grad"]) <= 5e-3 * np.linalg.norm(b["grad"])
        else:
            assert abs(a["loss"] - b["loss"]) <= 1e-2 * abs(b["loss"]), (a["loss"], b["loss"])
            assert np.abs(a["logits"] - b["logits"]).max() <= 0.1 * np.abs(b["logits"]).max()
            cos = float((a["grad"] * b["grad"]).sum() / (np.linalg.norm(a["grad"]) * np.linalg.norm(b["grad"])))
            assert cos >= 0.9, cos


@pytest.mark.gpu
def test_softmax_pool_backward_from_scores_equals_the_one_from_probabilities():
    """ps_op_softmax_pool_bwd_scores (the native step keeps no probabilities: the backward forms softmax_K(scores) again) against
    ps_op_softmax_pool_bwd fed the probabilities the forward wrote: same arithmetic, so bit-identical dfset / dscores; K = 16, 32 (register
    forms) and 5 (loop form); the forward with probs = NULL returns the same agg; dscores written over the scores in place."""
    import ctypes
    import torch
    from point_unet_amd import runtime, _lib
    ctx = runtime.default_context(0)
    L = _lib.lib()
    vp = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    g = torch.Generator().manual_seed(31)
    for R, K, d in ((1003, 16, 128), (257, 32, 64), (300, 5, 24)):
        fset = torch.randn(R * K, d, generator=g).cuda()
        scores = (3 * torch.randn(R * K, d, generator=g)).cuda()
        dagg = torch.randn(R, d, generator=g).cuda()
        probs, agg, agg2 = torch.empty_like(fset), torch.empty(R, d).cuda(), torch.empty(R, d).cuda()
        assert L.ps_op_softmax_pool_fwd(ctx.handle, vp(fset), vp(scores), R, K, d, vp(probs), vp(agg)) == 0
        assert L.ps_op_softmax_pool_fwd(ctx.handle, vp(fset), vp(scores), R, K, d, None, vp(agg2)) == 0
        want = (torch.softmax(scores.double().view(R, K, d), 1) * fset.double().view(R, K, d)).sum(1)
        assert torch.equal(agg, agg2) and (agg.double() - want).abs().max().item() <= 1e-5
        df1, ds1, df2, ds2 = (torch.empty_like(fset) for _ in range(4))
        assert L.ps_op_softmax_pool_bwd(ctx.handle, vp(dagg), vp(fset), vp(probs), R, K, d, vp(df1), vp(ds1)) == 0
        assert L.ps_op_softmax_pool_bwd_scores(ctx.handle, vp(dagg), vp(fset), vp(scores), R, K, d, vp(df2), vp(ds2)) == 0
        assert torch.equal(df1, df2) and torch.equal(ds1, ds2)
        inplace = scores.clone()
        assert L.ps_op_softmax_pool_bwd_scores(ctx.handle, vp(dagg), vp(fset), vp(inplace), R, K, d, vp(df2), vp(inplace)) == 0
        torch.cuda.synchronize()
        assert torch.equal(inplace, ds1)



