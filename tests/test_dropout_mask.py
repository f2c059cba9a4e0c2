"""Statistics of the dropout masks of the training step, on the numpy restatement of the kernel (dropout_ref.py; the GPU test
test_gpu_train_ops.py::test_dropout_mask_is_the_restatement_bit_for_bit ties it to ps_op_dropout): the keep rate overall and per column
of the [R, C] activations the trainer drops (fc0's output), independence of the masks of consecutive steps and of the ranks of a
data-parallel job, and the seed formula as both trainers write it."""
import os
import re

import numpy as np
import pytest

import dropout_ref as dr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = 20011  # rows (odd: the columns of a row-major [R, C] mask are not aligned with any power of two of the element index)


def _within(count, n, p, sigmas=6.0):
    return abs(count - n * p) <= sigmas * np.sqrt(n * p * (1.0 - p))


def test_the_seed_formula_is_the_one_both_trainers_use():
    native = open(os.path.join(ROOT, "point-unet_amd", "csrc", "trainer.hip")).read()
    tape = open(os.path.join(ROOT, "point-unet_amd", "train.py")).read()
    m = re.search(r"dropout\(f, opt\.keep_prob, \(uint32_t\)\((0x[0-9a-fA-F]+)u \* \(uint32_t\)\(step \+ 1\) \+ (0x[0-9a-fA-F]+)u \* \(uint32_t\)rank\)\)", native)
    assert m, "the seed expression of csrc/trainer.hip changed: update dropout_ref.py"
    assert (int(m.group(1), 16), int(m.group(2), 16)) == (dr.SEED_STEP, dr.SEED_RANK)
    m = re.search(r"t\.dropout\(f, self\.keep_prob, (0x[0-9a-fA-F]+) \* \(self\.step \+ 1\) \+ (0x[0-9a-fA-F]+) \* self\._rank\)", tape)
    assert m, "the seed expression of train.py changed: update dropout_ref.py"
    assert (int(m.group(1), 16), int(m.group(2), 16)) == (dr.SEED_STEP, dr.SEED_RANK)
    kernel = open(os.path.join(ROOT, "point-unet_amd", "csrc", "ops_train.hip")).read()
    assert "hash32((unsigned)e * %du ^ seed)" % dr.INDEX_MUL in kernel
    assert "x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;" in kernel


def test_hash32_known_values():
    # the mixer (a public 32-bit integer hash); values computed by hand in Python integers
    def ref(x):
        x ^= x >> 16
        x = (x * 0x7FEB352D) & 0xFFFFFFFF
        x ^= x >> 15
        x = (x * 0x846CA68B) & 0xFFFFFFFF
        return x ^ (x >> 16)
    xs = [0, 1, 2, 0xFFFFFFFF, 0x9E3779B9, 123456789]
    assert [int(v) for v in dr.hash32(np.array(xs, dtype=np.uint32))] == [ref(x) for x in xs]
    assert dr.step_seed(0) == 0x9E3779B9 and dr.step_seed(1, 1) == (2 * 0x9E3779B9 + 0x85EBCA6B) & 0xFFFFFFFF


@pytest.mark.parametrize("keep", [0.1, 0.5, 0.9])
@pytest.mark.parametrize("C", [32, 64])
def test_keep_rate_overall_and_per_column(keep, C):
    for step in (0, 1, 2, 63):
        for rank in (0, 3):
            k = dr.keep_mask(R * C, dr.step_seed(step, rank), keep).reshape(R, C)
            assert _within(int(k.sum()), R * C, keep), (step, rank)
            per_col = k.sum(0)
            bad = [c for c in range(C) if not _within(int(per_col[c]), R, keep)]
            assert not bad, (step, rank, bad, per_col[bad])


def test_the_mask_takes_only_zero_and_the_scale():
    for keep in (0.1, 0.5, 0.9, 1.0):
        m = dr.dropout_mask(100003, dr.step_seed(5), keep)
        scale = np.float32(1.0) / np.float32(keep)
        assert set(np.unique(m).tolist()) <= {0.0, float(scale)}
    assert dr.keep_mask(100003, dr.step_seed(5), 1.0).all()  # u < 1 always: keep_prob 1 drops nothing


@pytest.mark.parametrize("keep", [0.5, 0.9])
def test_masks_of_consecutive_steps_and_of_ranks_are_independent(keep):
    """Joint keep rate of (step s, step s+1) for s < 64 and of (rank 0, rank r) for r < 8 within 6 sigma of keep^2; no two masks equal."""
    n = R * 32
    p = keep * keep
    steps = [dr.keep_mask(n, dr.step_seed(s), keep) for s in range(65)]
    for s in range(64):
        both = int(np.count_nonzero(steps[s] & steps[s + 1]))
        assert _within(both, n, p), (s, both / n, p)
    ranks = [dr.keep_mask(n, dr.step_seed(7, r), keep) for r in range(8)]
    for r in range(1, 8):
        both = int(np.count_nonzero(ranks[0] & ranks[r]))
        assert _within(both, n, p), (r, both / n, p)
    seen = {}
    for name, k in [("step%d" % s, m) for s, m in enumerate(steps)] + [("rank%d" % r, m) for r, m in enumerate(ranks) if r]:
        key = np.packbits(k).tobytes()
        assert key not in seen, (name, seen.get(key))
        seen[key] = name
