"""Every step of a native trainer after its first.  From the second step on ps_randla_train_step no longer packs each weight image
where a product uses it: it replays a recorded list with one batched launch per source file at the start of the step (PackCache:
csrc/common.h, ops.hip pack_cache_replay / pack_slot, trainer.hip run_step), a call that does not match the recording packs call by call
for the rest of that step and the next step records again; the activation pool has grown to its size, the inverse indices are cached
per step.  None of that may change a number: the default step is deterministic (no float atomics), so EVERY call of a long-lived
trainer must equal, bit for bit, the same call made as the FIRST call of a fresh trainer that was handed the same state -- only the
fresh one packs call by call.  tests/test_gpu_train_gated_rows.py and test_training_step_at_the_true_width_ladder tie a fresh
trainer's first step to the float64 oracle; together with this file every step of a run is tied to it."""
import numpy as np
import pytest

import netcase

pytestmark = pytest.mark.gpu

LR = 1e-3


def _batch(cfg, xyz, feats, seed):
    import torch
    from point_unet_amd.pyramid import build_pyramid
    labels = np.random.default_rng(seed).integers(0, cfg.num_classes, xyz.shape[:2]).astype(np.int32)
    return build_pyramid(torch.from_numpy(xyz).cuda(), cfg), torch.from_numpy(feats).cuda(), torch.from_numpy(labels).cuda()


def _second_size():
    """Q: ONE cloud of 33 000 points (P: two of 6 000) with the ladder's network: 33 000 / 8 250 / 2 062 / 515 / 128 points per level.
    Larger per cloud and in total than P, so the activation pool grows again in its first step; and the decoder layer of level 1
    (384 -> 128 on 8 250 rows) is a gemm_b3 product in both modes (>= 4 096 rows fp32, >= 8 192 one plane), whose weight image is
    another kind than the one P's 3 000 rows record there -- a step on Q after steps on P does not match P's recording."""
    from conftest import brats_cloud
    xyz = brats_cloud(33000, 77, grid=(64, 64, 48))[None]
    feats = np.random.default_rng(78).standard_normal((1, 33000, 4)).astype(np.float32)
    return xyz, np.concatenate([xyz, feats], -1)


class _State:
    def __init__(self, tr):
        self.flat, self.buffers, self.m, self.v, self.step = tr.flat.clone(), tr.flat_buffers.clone(), tr.m.clone(), tr.v.clone(), tr.step


def _fresh(cfg, params, cw, mode, keep_prob, s):
    """A new trainer in state s: never stepped, so it records nothing it could replay and packs every weight image at its product."""
    from point_unet_amd.train import Trainer
    tr = Trainer(cfg, params=params, learning_rate=LR, class_weights=cw, keep_prob=keep_prob, mlp_dtype=mode)
    tr.rebind(flat=s.flat.clone(), m=s.m.clone(), v=s.v.clone(), flat_buffers=s.buffers.clone())
    tr.step = s.step
    return tr


def _call(tr, kind, batch):
    """(loss, logits, grad, flat, buffers, m, v, step, op_conv1x1 launches) of one call; the stage count shows what the pack cache did."""
    import torch
    tr.ctx.timing_begin()
    loss = (tr.train_step if kind == "step" else tr.backward_only)(*batch)
    torch.cuda.synchronize()
    rows = tr.ctx.timing_end()
    packs = sum(n for name, _, n in rows if name == "op_conv1x1")
    return (loss.clone(), tr.last_logits.clone(), tr.grad.clone(), tr.flat.clone(), tr.flat_buffers.clone(), tr.m.clone(), tr.v.clone(), tr.step), packs


_WHAT = ("loss", "logits", "gradient", "parameters", "moving statistics", "Adam m", "Adam v")


def _walk(cfg, mode, keep_prob, calls, seed=5):
    """Trainer A makes `calls` [(name, kind, batch)]; before each, its state goes to a fresh trainer B that makes the same call first.
    Returns [op_conv1x1 launches of A - of B] and A's pool peak after each call."""
    import torch
    from point_unet_amd import weights
    from point_unet_amd.train import Trainer
    params = weights.init_params(cfg, seed=seed, randomize_bn=True)
    cw = np.linspace(1.0, 2.0, cfg.num_classes).astype(np.float32)
    extra, peaks = [], []
    with Trainer(cfg, params=params, learning_rate=LR, class_weights=cw, keep_prob=keep_prob, mlp_dtype=mode) as a:
        for i, (name, kind, batch) in enumerate(calls):
            s = _State(a)
            with _fresh(cfg, params, cw, mode, keep_prob, s) as b:
                want, packs_b = _call(b, kind, batch)
            got, packs_a = _call(a, kind, batch)
            where = "call %d: %s(%s), %s, keep_prob %g" % (i + 1, kind, name, mode, keep_prob)
            assert bool(torch.isfinite(got[0]).all()) and bool(torch.isfinite(got[2]).all()), where
            assert got[-1] == want[-1] == s.step + (1 if kind == "step" else 0), where
            for what, x, y in zip(_WHAT, got, want):
                assert torch.equal(x, y), "%s: the %s differs from a fresh trainer's first call (max |diff| %.3e)" % (
                    where, what, float((x.double() - y.double()).abs().max()))
            if kind == "step":
                assert not torch.equal(got[3], s.flat) and float(got[2].abs().max()) > 0, where
            else:  # backward_only: gradients as the step computes them, parameters and moments untouched, moving statistics updated
                assert torch.equal(got[3], s.flat) and torch.equal(got[5], s.m) and torch.equal(got[6], s.v), where
                assert not torch.equal(got[4], s.buffers) and float(got[2].abs().max()) > 0, where
            extra.append(packs_a - packs_b)
            peaks.append(a.pool_peak_bytes())
    return extra, peaks


@pytest.fixture(scope="module")
def batches():
    cfg, xyz, feats = netcase.small_deep(6000, seed=21, B=2)
    P = _batch(cfg, xyz, feats, 3)
    qxyz, qfeats = _second_size()
    assert netcase.level_rows(cfg, qxyz.shape[1], 1)[0] == [33000, 8250, 2062, 515, 128]
    return cfg, P, _batch(cfg, qxyz, qfeats, 4)


@pytest.mark.parametrize("mode,keep_prob", [("fp32", 1.0), ("bf16", 1.0), ("fp32", 0.5)])
def test_every_later_call_equals_a_fresh_trainers_first(batches, mode, keep_prob):
    """A walks step(P), step(P), step(Q), step(Q), step(Q), backward_only(P), step(P), step(P) -- P the ladder case (2 x 6 000 points), Q one
    cloud of 33 000 (_second_size).  Each call must equal the first call of a fresh trainer in A's state (flat parameters, BatchNorm
    buffers, Adam m / v, step counter) with torch.equal: loss, logits, flat gradient, parameters and moments after Adam, moving
    statistics.  keep_prob = 0.5: the dropout mask is a hash of (element, step, rank), equal once the counters agree.
    What the pack cache did shows in the launches of stage op_conv1x1: a step that starts from a recording makes the two batched packing
    launches on top of what the fresh trainer makes.  Expected: 0 (records), 2 (replays), 2 (replays P's list, which Q's products do not
    match: packs call by call, drops the recording), 0 (records Q), 2, 2 (Q's list against P: dropped again), 0, 2.  The pool grows
    again at the first step on Q (a larger peak) and serves P from the larger pool afterwards."""
    cfg, P, Q = batches
    calls = [("P", "step", P), ("P", "step", P), ("Q", "step", Q), ("Q", "step", Q), ("Q", "step", Q), ("P", "backward_only", P), ("P", "step", P),
             ("P", "step", P)]
    extra, peaks = _walk(cfg, mode, keep_prob, calls)
    print("%s keep_prob %g: extra op_conv1x1 launches per call %s, pool peak MB %s" % (mode, keep_prob, extra, [p >> 20 for p in peaks]))
    assert extra == [0, 2, 2, 0, 2, 2, 0, 2], extra
    # (ps_trainer_pool_peak_bytes is the last call's peak: the same for the same batch whatever the pool held before, larger for Q)
    assert peaks[0] == peaks[1] == peaks[5] == peaks[6] == peaks[7] < peaks[2] == peaks[3] == peaks[4], peaks


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_replayed_steps_at_gated_rows_equal_a_fresh_trainers_first(mode):
    """Two plain steps on the wide-row case (netcase.wide_rows): the second replays the image kinds only many-row products have -- the
    split-bf16 planes of gemm_b3 (fp32), its one RNE plane (bf16-MLP mode: the 17 000-row decoder layer and the 33 984-row score product
    of level 4) and the accumulator-order images of the wide-level attentive pooling, split-source form included (bf16-MLP mode, level
    3) -- and must equal a fresh trainer's first step bit for bit."""
    cfg, xyz, feats = netcase.wide_rows()
    W = _batch(cfg, xyz, feats, 3)
    extra, _ = _walk(cfg, mode, 1.0, [("W", "step", W), ("W", "step", W)], seed=3)
    assert extra == [0, 2], extra
