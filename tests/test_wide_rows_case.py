"""The "wide-row" training case (netcase.wide_rows) exists because the native training step and the ops it calls pick their kernels by
ROW COUNT, and the width-ladder case of the other step tests (netcase.small_deep(6000, B=2)) stays below several of those thresholds.
These CPU tests hold (1) the row counts of both cases, computed from their configs alone, against every threshold, and (2) the
thresholds themselves against the source text at the places the GPU tests rely on: a threshold that is moved later fails here instead
of silently un-covering tests/test_gpu_train_gated_rows.py and tests/test_gpu_train_replay.py.

Which products can take the row-gated forms at all (from the layer table of csrc/trainer.hip: build_layout).  gemm_b3 needs cin >= 128,
cin % 32 == 0 and cout % 128 == 0, wgrad_b3 cin % 128 == 0 and cout % 128 == 0.  With d_out = (16, 64, 128, 256, 512) those are
  [N] rows of level i >= 2:   att_pooling's mlp (d -> d), mlp2 (d -> 2d), the shortcut (d_in -> 2d), the decoder layer of that level;
  [N] rows of level 1:        its decoder layer (128 + 256 -> 128);
  [N*K] rows of level i >= 2: att_pooling's score product (d x d) where the pooling runs op by op (d = 512 always, d = 128 / 256 with
                              fused_att = False or train_att_gemm = 0) -- and the fused wide-level pooling (d = 128 / 256), whose
                              split-source form has its own floor."""
import os
import re

import netcase

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "point-unet_amd", "csrc")

# the thresholds as the GPU tests assume them (checked against the sources below)
SPLIT_MIN_ROWS = 16384        # trainer.hip: att_gemm_split_ok
GEMM_B3_MIN_ROWS = 4096       # gemm_b3.hip: gemm_b3_fits, three planes (fp32)
GEMM_B3_MIN_ROWS_ONE = 8192   # ... one plane (bf16-MLP mode)
GEMM_B3_SMALL_ROWS = 16384    # gemm_b3.hip: kB3SmallRows -- below: 128-row workgroups, from here on the kB3RT form
WGRAD_B3_MIN_ROWS = 4096      # gemm_b3.hip: wgrad_b3_fits, three planes
WGRAD_B3_MIN_ROWS_ONE = 16384  # ... one plane


def _b3_rows(cfg, n0, B):
    """Row counts at which a product of the b3-eligible shapes runs (see the module docstring)."""
    n_rows, nk_rows = netcase.level_rows(cfg, n0, B)
    return sorted(n_rows[1:] + nk_rows[2:])


def _split_rows(cfg, n0, B):
    """[N*K] rows of the levels whose fused pooling has a split-source form (d = 128 / 256)."""
    return [r for d, r in zip(cfg.d_out, netcase.level_rows(cfg, n0, B)[1]) if d in (128, 256)]


def _ladder():
    return netcase.make_cfg(5, (16, 64, 128, 256, 512), (4, 4, 4, 4, 2), 16), 6000, 2


def _wide():
    return netcase.make_cfg(5, (16, 64, 128, 256, 512), (2, 2, 2, 2, 2), 16), netcase.WIDE_ROWS_N0, netcase.WIDE_ROWS_B


def test_the_case_is_what_the_row_counts_below_assume():
    cfg, xyz, feats = netcase.wide_rows()
    want, n0, B = _wide()
    assert (list(cfg.d_out), list(cfg.sub_sampling_ratio), cfg.k_n, cfg.num_layers) == (list(want.d_out), list(want.sub_sampling_ratio), 16, 5)
    assert xyz.shape == (B, n0, 3) and feats.shape == (B, n0, cfg.in_channels) and cfg.in_channels == 7
    assert netcase.level_rows(cfg, n0, B) == ([34000, 17000, 8500, 4250, 2124], [544000, 272000, 136000, 68000, 33984])
    for b in range(B):  # (lattice voxels without replacement: no duplicate point, the K-NN tables of the two builders agree)
        assert len({tuple(p) for p in xyz[b].tolist()}) == n0
    lcfg, ln0, lB = _ladder()
    ref = netcase.small_deep(6000, seed=12, B=2)[0]
    assert (list(ref.d_out), list(ref.sub_sampling_ratio), ref.k_n) == (list(lcfg.d_out), list(lcfg.sub_sampling_ratio), lcfg.k_n)
    assert netcase.level_rows(lcfg, ln0, lB) == ([12000, 3000, 750, 186, 46], [192000, 48000, 12000, 2976, 736])


def test_the_wide_row_case_crosses_every_row_threshold_and_the_ladder_does_not():
    wide, ladder = _b3_rows(*_wide()), _b3_rows(*_ladder())
    # split-source wide pooling: both of its levels in the wide-row case, neither in the ladder
    assert all(r >= SPLIT_MIN_ROWS for r in _split_rows(*_wide())) and len(_split_rows(*_wide())) == 2
    assert all(r < SPLIT_MIN_ROWS for r in _split_rows(*_ladder())) and len(_split_rows(*_ladder())) == 2
    # gemm_b3 / wgrad_b3: a row count in every band between the thresholds, both sides of each one
    edges = sorted({GEMM_B3_MIN_ROWS, GEMM_B3_MIN_ROWS_ONE, GEMM_B3_SMALL_ROWS, WGRAD_B3_MIN_ROWS, WGRAD_B3_MIN_ROWS_ONE})
    assert edges == [4096, 8192, 16384]
    bands = [(0, 4096), (4096, 8192), (8192, 16384), (16384, 1 << 31)]
    for lo, hi in bands:
        assert any(lo <= r < hi for r in wide), (lo, hi, wide)
    assert [r for r in wide if 4096 <= r < 16384] == [4250, 8500]  # (256 -> 512 at 4 250 rows, 128 -> 256 at 8 500)
    # the ladder reaches the three-plane forms and the 128-row one-plane gemm_b3, but neither the many-row gemm_b3 form nor the one-plane
    # wgrad_b3 -- in the bf16-MLP mode, BASELINE configs[2], the step at the ladder size runs neither
    assert max(ladder) == 12000 and max(ladder) < min(GEMM_B3_SMALL_ROWS, WGRAD_B3_MIN_ROWS_ONE)
    assert any(r >= GEMM_B3_MIN_ROWS_ONE for r in ladder)


def _function(src, head):
    """The text of the function whose definition line contains `head`, up to the closing brace in column 0 (or 4, for a member)."""
    m = re.search(r"^( *)[^\n]*" + re.escape(head) + r"[^\n]*\n(?:.*\n)*?\1\}", src, re.M)
    assert m, "not found in the source: %s" % head
    return m.group(0)


def test_the_thresholds_are_where_the_tests_assume_them():
    trainer = open(os.path.join(CSRC, "trainer.hip")).read()
    b3 = open(os.path.join(CSRC, "gemm_b3.hip")).read()
    ok = _function(trainer, "bool att_gemm_split_ok(")
    assert re.search(r"rows = B \* M \* K;", ok) and re.search(r"&& rows >= %d &&" % SPLIT_MIN_ROWS, ok), ok
    assert "d <= 256" in ok and "d % 128 == 0" in ok
    # (the trainer asks per level, fp32: only with the knob; bf16-MLP: by default)
    assert "att_split_env < 0 ? opt.mlp_bf16 != 0 : att_split_env != 0" in trainer
    fits = _function(b3, "bool gemm_b3_fits(")
    assert "tn.gemm_b3_min_rows" in fits
    assert re.search(r"min_rows = env_rows > 0 \? env_rows : \(one_plane \? %d : %d\);" % (GEMM_B3_MIN_ROWS_ONE, GEMM_B3_MIN_ROWS), fits), fits
    assert "R >= min_rows && K >= 128 && K % 32 == 0 && N % 128 == 0" in fits
    wfits = _function(b3, "bool wgrad_b3_fits(")
    assert "tn.wgrad_b3_min_rows" in wfits
    assert re.search(r"min_rows = env_rows > 0 \? env_rows : \(one_plane \? %d : %d\);" % (WGRAD_B3_MIN_ROWS_ONE, WGRAD_B3_MIN_ROWS), wfits), wfits
    assert "R >= min_rows" in wfits and "cin % 128 == 0 && cout % 128 == 0" in wfits
    assert re.search(r"constexpr int64_t kB3SmallRows = %d;" % GEMM_B3_SMALL_ROWS, b3)
    assert "const bool small = R < kB3SmallRows;" in _function(b3, "int gemm_b3(ps_context* c")
    # the split-source weight gradient takes the one-plane floor in both modes
    assert "/*one_plane: the split form's own floor*/ true" in _function(b3, "bool wgrad_b3_split_fits(")
    # who passes one_plane: the bf16-MLP mode of the context
    ops = open(os.path.join(CSRC, "ops.hip")).read()
    assert "gemm_b3_fits(c->tune, R, cin, cout, x, ldx, c->train_bf16)" in ops
    assert "wgrad_b3_fits(c->tune, R, cin, cout, x, ldx, dy, lddy, c->train_bf16)" in open(os.path.join(CSRC, "ops_train.hip")).read()
