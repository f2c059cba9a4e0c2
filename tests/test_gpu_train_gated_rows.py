"""The native training step (csrc/trainer.hip, ps_randla_train_step) at the row counts where it and the ops it calls switch kernels, against
the float64 autograd oracle (oracle/randla_train_oracle.py).  The other step tests run the width-ladder case (2 x 6 000 points), which
stays below the floor of the split-source wide pooling (16 384 [N*K] rows), of the many-row gemm_b3 form and of the one-plane wgrad_b3
(16 384 rows); netcase.wide_rows crosses every one of them in both modes (tests/test_wide_rows_case.py holds the row counts and the
thresholds).  The op-level tests show that each of those kernels agrees with its materialised form; these show that the STEP built from
them -- add_in_place into the gradient of f_xyz, gathered_grad, the split weight-gradient slabs, the one-plane packed images -- is right.

A test that silently took the default path would be the defect this file closes, so every variant carries a proof that its branch ran:
stage launch counts (ctx.timing_begin / timing_end) where a stage separates the forms, a bit-different gradient where none does."""
import numpy as np
import pytest

import netcase
from tuning import tuned_context

pytestmark = pytest.mark.gpu

LR = 1e-3
NO_B3 = {"gemm_b3_min_rows": 1 << 40, "wgrad_b3_min_rows": 1 << 40}  # (no row count reaches gemm_b3 / wgrad_b3: the fp32 / bf16 MFMA kernels everywhere)

# (id, mode, knobs of the trainer's context, Trainer keywords)
VARIANTS = [
    ("fp32-default", "fp32", {}, {}),
    ("fp32-att_gemm_split=1", "fp32", {"train_att_gemm_split": 1}, {}),
    ("fp32-fused_att=False", "fp32", {}, {"fused_att": False}),
    ("fp32-deterministic=False", "fp32", {}, {"deterministic": False}),
    ("fp32-no_b3", "fp32", NO_B3, {}),
    ("bf16-default", "bf16", {}, {}),
    ("bf16-att_gemm_split=0", "bf16", {"train_att_gemm_split": 0}, {}),
    ("bf16-fused_att=False", "bf16", {}, {"fused_att": False}),
    ("bf16-att_gemm=0", "bf16", {"train_att_gemm": 0}, {}),
    ("bf16-no_b3", "bf16", NO_B3, {}),
]
_BY_ID = {v[0]: v for v in VARIANTS}


class _Case:
    """One network case: inputs, parameters, the oracle's pyramid, the oracle step per mode (computed once, kept unchanged) and the native
    step per variant (one run each, shared between the tests that compare variants)."""

    def __init__(self, oracle, cfg, xyz, feats, with_oracle):
        from oracle import randla_oracle as ro
        from point_unet_amd import weights
        self.cfg, self.xyz, self.feats = cfg, xyz, feats
        self.params = weights.init_params(cfg, seed=3, randomize_bn=True)
        self.labels = np.random.default_rng(3).integers(0, cfg.num_classes, xyz.shape[:2]).astype(np.int32)
        self.cw = np.linspace(1.0, 2.0, cfg.num_classes).astype(np.float32)
        self.host_pyr = ro.build_pyramid(lambda s, q, k: oracle.knn_batch(s, q, k), xyz, cfg.k_n, cfg.sub_sampling_ratio) if with_oracle else None
        self._want, self._runs = {}, {}

    def want(self, mode):
        """(float64 oracle step, float32 evaluation of the same rounded model or None) -- the bf16 mode's model rounds the operands of the
        GEMMs the product rounds (test_gpu_train._bf16_rule) and the stored LFA rows (_act_rule)."""
        if mode not in self._want:
            import torch
            import test_gpu_train as T
            from oracle import randla_train_oracle as rto
            pts, nbr, pool, up = self.host_pyr
            kw = dict(lr=LR, step=1)
            if mode == "bf16":
                kw.update(bf16_rule=T._bf16_rule, act_rule=T._act_rule)
            want = rto.train_step(self.params, self.cfg.num_layers, pts, nbr, pool, up, self.feats, self.labels, self.cw, **kw)
            alt = None
            if mode == "bf16":
                alt = rto.train_step(self.params, self.cfg.num_layers, pts, nbr, pool, up, self.feats, self.labels, self.cw, dtype=torch.float32, **kw)
            self._want[mode] = (want, alt)
        return self._want[mode]

    def run(self, vid):
        """One native step of a fresh trainer on a fresh context with the variant's knobs (set before the trainer is created)."""
        if vid not in self._runs:
            import torch
            from point_unet_amd.pyramid import build_pyramid
            from point_unet_amd.train import Trainer
            _, mode, knobs, kw = _BY_ID[vid]
            with tuned_context(**knobs) as ctx:
                tr = Trainer(self.cfg, params=self.params, learning_rate=LR, class_weights=self.cw, keep_prob=1.0, mlp_dtype=mode, ctx=ctx, **kw)
                pyr = build_pyramid(torch.from_numpy(self.xyz).cuda(), self.cfg, ctx=ctx)
                if self.host_pyr is not None:
                    for i in range(self.cfg.num_layers):
                        assert np.array_equal(pyr.neigh_idx[i].cpu().numpy(), self.host_pyr[1][i]), i
                        assert np.array_equal(pyr.sub_idx[i].cpu().numpy(), self.host_pyr[2][i]), i
                        assert np.array_equal(pyr.interp_idx[i].cpu().numpy(), self.host_pyr[3][i]), i
                ctx.timing_begin()
                loss = tr.train_step(pyr, torch.from_numpy(self.feats).cuda(), torch.from_numpy(self.labels).cuda())
                torch.cuda.synchronize()
                stages = {}
                for name, _, n in ctx.timing_end():
                    stages[name] = stages.get(name, 0) + int(n)
                self._runs[vid] = dict(loss=float(loss), logits=tr.last_logits.cpu().numpy(), grads={n: tr.G[n].cpu().numpy() for n in tr.names},
                                       flat_grad=tr.grad.cpu().numpy().copy(), new=tr.export_params(), stages=stages)
                tr.close()
                del pyr
        return self._runs[vid]


@pytest.fixture(scope="module")
def wide(oracle):
    cfg, xyz, feats = netcase.wide_rows()
    return _Case(oracle, cfg, xyz, feats, True)


@pytest.fixture(scope="module")
def ladder():
    cfg, xyz, feats = netcase.small_deep(6000, seed=12, B=2)
    return _Case(None, cfg, xyz, feats, False)


def _errors(case, vid):
    import test_gpu_train as T
    mode = _BY_ID[vid][1]
    want, alt = case.want(mode)
    got = case.run(vid)
    names = list(got["grads"])
    e = dict(loss=abs(got["loss"] - want["loss"]) / max(1.0, abs(want["loss"])),
             logits=float(np.abs(got["logits"].reshape(want["logits"].shape) - want["logits"]).max()))
    e["l2"], e["worst"] = T._grad_stats(got["grads"], want["grads"], names)
    e["stats"] = max(float(np.abs(got["new"][k] - v).max() / max(1.0, np.abs(v).max())) for k, v in want["new_params"].items()
                     if k.endswith(("moving_mean", "moving_variance")))
    gscale = max(np.abs(g).max() for g in want["grads"].values())
    e["adam"], e["adam_checked"] = 0.0, 0
    for n in names:  # one Adam step where the gradient is signal (Adam normalises rounding noise to O(lr))
        mask = np.abs(want["grads"][n]) > 2e-2 * gscale
        if mask.any():
            e["adam_checked"] += int(mask.sum())
            e["adam"] = max(e["adam"], float(np.abs(got["new"][n] - want["new_params"][n])[mask].max()))
    if alt is not None:
        e["s_loss"] = abs(alt["loss"] - want["loss"]) / max(1.0, abs(want["loss"]))
        e["s_logits"] = float(np.abs(alt["logits"] - want["logits"]).max())
        e["s_l2"] = T._grad_stats(alt["grads"], want["grads"], names)[0]
    return e


def _hold_to_the_bar(case, vid):
    mode = _BY_ID[vid][1]
    e = _errors(case, vid)
    print("%s: loss rel %.2e, logits %.2e, grad rel L2 %.2e, worst tensors %s, moving statistics %.2e, Adam %.2e on %d entries" % (
        vid, e["loss"], e["logits"], e["l2"], [(round(w, 3), n) for w, n in e["worst"][:2]], e["stats"], e["adam"], e["adam_checked"]))
    if mode == "fp32":
        assert e["loss"] <= 2e-5 and e["logits"] < 1e-4, (e["loss"], e["logits"])
        assert e["worst"][0][0] <= 1.0, e["worst"][:5]
        assert e["l2"] <= 5e-3, e["l2"]
        assert e["stats"] <= 1e-5, e["stats"]
        assert e["adam_checked"] > 1000 and e["adam"] <= 5e-5, (e["adam_checked"], e["adam"])
    else:
        print("%s: spread of the rounded model (float32 against float64 evaluation): s_loss %.2e, s_logit %.2e, s_l2 %.2e" % (
            vid, e["s_loss"], e["s_logits"], e["s_l2"]))
        assert e["loss"] <= 2 * e["s_loss"] + 1e-3, (e["loss"], e["s_loss"])
        assert e["logits"] <= 2 * e["s_logits"] + 1e-3, (e["logits"], e["s_logits"])
        assert e["l2"] <= 2 * e["s_l2"] + 1e-3, (e["l2"], e["s_l2"])
    return e


def _n(case, vid, stage):
    return case.run(vid)["stages"].get(stage, 0)


def _prove_the_branch_ran(wide, vid):
    """What shows, from outside the step, that the variant's branch ran at the wide-row case."""
    mode = _BY_ID[vid][1]
    default = mode + "-default"
    stages, base = wide.run(vid)["stages"], wide.run(default)["stages"]
    print("%s stages: %s" % (vid, sorted(stages.items())))
    if "att_gemm_split" in vid or vid.endswith("default"):
        # the split-source pooling takes its gathered half through the index table: the two op_gather_neighbour launches of each wide level
        # (f_pc and f_agg into the concat buffers) are gone -- levels 2 and 3 in fp32 (d = 128, 256), level 3 in the bf16-MLP mode (d = 128
        # is one of the narrow levels there)
        on, off = ("fp32-att_gemm_split=1", "fp32-default") if mode == "fp32" else ("bf16-default", "bf16-att_gemm_split=0")
        gone = _n(wide, off, "op_gather_neighbour") - _n(wide, on, "op_gather_neighbour")
        assert gone == (4 if mode == "fp32" else 2), (gone, wide.run(on)["stages"], wide.run(off)["stages"])
        # ... and nothing else changes: the split-source kernels make the products of the materialised ones in the same order
        # (test_wide_level_split_source_forms_equal_the_materialised_ones), so the step wired from them -- rows for the gather-reduction,
        # the f_xyz half added in place, the split weight-gradient slabs -- must give the materialised step's bits
        assert np.array_equal(wide.run(on)["flat_grad"], wide.run(off)["flat_grad"]) and np.array_equal(wide.run(on)["logits"], wide.run(off)["logits"])
        assert {k: v for k, v in wide.run(on)["stages"].items() if k != "op_gather_neighbour"} == {
            k: v for k, v in wide.run(off)["stages"].items() if k != "op_gather_neighbour"}
    if vid.endswith("default"):
        # gemm_b3 / wgrad_b3: no stage separates them from the kernels they replace.  The step with both floors out of reach is held to the
        # same bar (variant no_b3) and must not give the same bits
        assert not np.array_equal(wide.run(vid)["flat_grad"], wide.run(mode + "-no_b3")["flat_grad"])
        assert not np.array_equal(wide.run(vid)["logits"], wide.run(mode + "-no_b3")["logits"])
        assert stages.get("train_inverse_index", 0) > 0 and stages.get("train_att_gemm_fwd", 0) > 0
    if vid.endswith("no_b3"):
        assert not np.array_equal(wide.run(vid)["flat_grad"], wide.run(default)["flat_grad"])
        if mode == "bf16":
            # the split-source pooling has no weight gradient but wgrad_b3's split form: with that floor out of reach level 3 must take the
            # materialised pooling (this step used to fail in its backward: "the split-source weight gradient does not apply")
            assert _n(wide, vid, "op_gather_neighbour") == _n(wide, "bf16-att_gemm_split=0", "op_gather_neighbour")
    if "fused_att=False" in vid:
        # op by op everywhere: no launch of the fused wide-level kernels, a softmax-pool pair at every level
        assert stages.get("train_att_gemm_fwd", 0) == 0 and stages.get("train_att_gemm_bwd", 0) == 0, stages
        assert stages.get("train_softpool_fwd", 0) == 2 * wide.cfg.num_layers > base.get("train_softpool_fwd", 0), (stages, base)
    if "deterministic=False" in vid:
        # float-atomic scatter-adds: no inverse index is built
        assert stages.get("train_inverse_index", 0) == 0 < base.get("train_inverse_index", 0), (stages, base)
        assert not np.array_equal(wide.run(vid)["flat_grad"], wide.run(default)["flat_grad"])
    if "att_gemm=0" in vid:
        assert stages.get("train_att_gemm_bwd", 0) == 0 < base.get("train_att_gemm_bwd", 0), (stages, base)
        assert stages.get("train_att_gemm_fwd", 0) < base.get("train_att_gemm_fwd", 0), (stages, base)


@pytest.mark.parametrize("vid", [v[0] for v in VARIANTS])
def test_step_at_gated_rows_against_float64_autograd(wide, vid):
    """One native step on netcase.wide_rows (2 x 17 000 points, ratios 2: [N] rows 34 000 / 17 000 / 8 500 / 4 250 / 2 124, [N*K] rows
    544 000 ... 33 984) against rto.train_step: loss, logits, every gradient tensor, moving statistics, parameters after Adam.

    fp32 variants -- default, train_att_gemm_split = 1, Trainer(fused_att=False) (what bench.py --no-fused-att times; with the native engine
    in no other test), Trainer(deterministic=False), and both gemm_b3 / wgrad_b3 floors out of reach -- at the bars of
    test_training_step_at_the_true_width_ladder and the full-size test: loss 2e-5 relative, logits 1e-4, every gradient tensor within
    3e-2 of its own max + 1e-4 of the global max, whole gradient 5e-3 relative L2, moving statistics 1e-5, Adam update 5e-5 where the
    gradient is signal.
    measured: default loss 4.8e-8, logits 2.0e-5, rel L2 8.8e-5, worst tensor at 0.028 of its bar (Encoder_layer_3mlp1/weights), moving
    statistics 9.1e-8, Adam 5.9e-8 on 32 849 entries; train_att_gemm_split = 1 the same bits; deterministic=False rel L2 8.8e-5; fused_att=False
    logits 2.0e-5, rel L2 4.2e-4, worst tensor 0.18 of its bar (Encoder_layer_3mlp2/weights); no b3 logits 2.2e-5, rel L2 3.3e-4, worst 0.18.
    (The deepest BatchNorm sees 1 062 rows here, 23 in the ladder case, whose fp32 step measures rel L2 2.3e-3.)

    bf16 variants -- default, train_att_gemm_split = 0, fused_att=False, train_att_gemm = 0, no b3 -- at the existing rule: the distance to the
    float64 oracle of the rounded model (_bf16_rule, _act_rule) is at most twice the distance of that model's own float32 evaluation,
    plus 1e-3, for loss, logits and the whole gradient (the caveat of test_training_step_at_the_true_width_ladder applies: this bar is as
    wide as the model is chaotic; the fp32 variants run the same plumbing at 5e-3).  fused_att=False stores no LFA rows as bfloat16
    (act16 needs the fused narrow pooling), the oracle's model does: that difference is inside the distance held to the bar.
    measured: spread of the rounded model s_loss 2.5e-5, s_logit 0.121, s_l2 0.026 (the ladder case: logits 0.18, rel L2 0.125 -- with 1 062
    rows under the deepest BatchNorm the model is five times less chaotic, and this bar five times tighter on the gradient); default and
    train_att_gemm_split = 0 (same bits) loss 4.6e-5, logits 0.129, rel L2 0.0263; fused_att=False 7.0e-6 / 0.197 / 0.0344; train_att_gemm = 0
    5.9e-5 / 0.130 / 0.0266; no b3 4.2e-5 / 0.127 / 0.0271.

    Each variant proves its branch ran (_prove_the_branch_ran): op_gather_neighbour launches for the split-source pooling, the fused
    stages' absence for fused_att=False / train_att_gemm = 0, no inverse index for deterministic=False, other bits for gemm_b3 / wgrad_b3."""
    _hold_to_the_bar(wide, vid)
    _prove_the_branch_ran(wide, vid)


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_the_split_knob_is_inert_at_the_ladder_size(ladder, mode):
    """Why the wide-row case exists: at the ladder size (levels 2 and 3 have 12 000 and 2 976 [N*K] rows, below att_gemm_split_ok's 16 384)
    train_att_gemm_split = 0 and 1 select the same kernels -- same launch counts in every stage, same bits -- so the two entries of
    tests/test_gpu_tuning_paths.py::_STEP_CASES that flip it test the default path."""
    import torch
    from point_unet_amd.pyramid import build_pyramid
    from point_unet_amd.train import Trainer
    out = []
    for split in (0, 1):
        with tuned_context(train_att_gemm_split=split) as ctx:
            tr = Trainer(ladder.cfg, params=ladder.params, learning_rate=LR, class_weights=ladder.cw, keep_prob=1.0, mlp_dtype=mode, ctx=ctx)
            pyr = build_pyramid(torch.from_numpy(ladder.xyz).cuda(), ladder.cfg, ctx=ctx)
            ctx.timing_begin()
            loss = tr.train_step(pyr, torch.from_numpy(ladder.feats).cuda(), torch.from_numpy(ladder.labels).cuda())
            torch.cuda.synchronize()
            stages = {}
            for name, _, n in ctx.timing_end():
                stages[name] = stages.get(name, 0) + int(n)
            out.append((float(loss), tr.grad.clone(), stages))
            tr.close()
            del pyr
    assert out[0][2] == out[1][2], (out[0][2], out[1][2])
    assert out[0][2].get("op_gather_neighbour", 0) > 0
    assert out[0][0] == out[1][0] and torch.equal(out[0][1], out[1][1])
