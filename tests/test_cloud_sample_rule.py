"""The sampling rule of ps_cloud_sample on its numpy restatement (cloud_sample_ref.py; test_gpu_cloud_sample.py ties the kernels to it bit
for bit): S holds every positive point and N points in all, the background subset, the pairs of it and the output positions are uniform over
fixed seeds, a prefix of N/4 rows (the pyramid's next level) holds each chosen point with probability 1/4, and slots draw different
streams.  Bounds are explicit multiples of the binomial standard deviation (no scipy).  Also: CloudBank's epoch order and seeds."""
import os

import numpy as np
import pytest

import cloud_sample_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

n, P, N, SEEDS = 1000, 100, 400, 3000


def _labels():
    lab = np.zeros(n, np.int32)
    lab[np.random.default_rng(7).choice(n, P, replace=False)] = np.random.default_rng(8).integers(1, 4, P)
    return lab


@pytest.fixture(scope="module")
def draws():
    lab = _labels()
    return lab, np.stack([ref.sample_indices(lab, n, N, s, 0) for s in range(SEEDS)])


def test_every_positive_is_in_and_the_size_is_n(draws):
    lab, d = draws
    pos = np.flatnonzero(lab > 0)
    for row in d:
        assert len(row) == N and len(np.unique(row)) == N
        assert np.isin(pos, row).all()


def _check_binomial(counts, trials, p, sigmas=5.0):
    sd = np.sqrt(trials * p * (1 - p))
    assert np.abs(counts - trials * p).max() <= sigmas * sd, (counts.min(), counts.max(), trials * p, sd)


def test_background_inclusion_is_uniform(draws):
    lab, d = draws
    bg = np.flatnonzero(lab == 0)
    inc = np.zeros(n, np.int64)
    np.add.at(inc, d.reshape(-1), 1)
    p = (N - P) / (n - P)
    _check_binomial(inc[bg], SEEDS, p)  # 900 points at 5 sigma
    # the spread of the counts is that of a binomial (neither too regular nor too wide): variance within 20 % of n p (1 - p)
    var = inc[bg].var()
    assert 0.8 <= var / (SEEDS * p * (1 - p)) <= 1.2


def test_adjacent_background_pairs_are_co_included_at_the_uniform_rate(draws):
    lab, d = draws
    bg = np.flatnonzero(lab == 0)
    mask = np.zeros((SEEDS, n), bool)
    np.put_along_axis(mask, d, True, axis=1)
    a, b = bg[:-1], bg[1:]
    both = (mask[:, a] & mask[:, b]).sum()
    k, m = N - P, n - P
    p2 = k * (k - 1) / (m * (m - 1))
    trials = SEEDS * len(a)
    # (the pairs overlap, so the sum is not binomial; 6 sigma of the independent case is still a tight bar: 0.5 % of the mean)
    assert abs(both - trials * p2) <= 6 * np.sqrt(trials * p2), (both / trials, p2)


def test_output_position_is_uniform(draws):
    lab, d = draws
    pos = np.flatnonzero(lab > 0)
    # where positive point 0 and a background point land: uniform over 10 bins of 40 positions
    for pt in (pos[0], pos[1]):
        where = np.argmax(d == pt, axis=1)
        hist = np.bincount(where // (N // 10), minlength=10)
        _check_binomial(hist, SEEDS, 0.1)
    # every position holds a positive with probability P / N
    _check_binomial((lab[d] > 0).sum(0), SEEDS, P / N, sigmas=5.5)


def test_prefix_of_a_quarter_holds_each_chosen_point_with_probability_one_quarter(draws):
    lab, d = draws
    pos = np.flatnonzero(lab > 0)
    pre = np.zeros(n, np.int64)
    np.add.at(pre, d[:, :N // 4].reshape(-1), 1)
    _check_binomial(pre[pos], SEEDS, 0.25)  # positives are always chosen
    bg = np.flatnonzero(lab == 0)
    _check_binomial(pre[bg], SEEDS, 0.25 * (N - P) / (n - P))


def test_slots_and_seeds_draw_different_streams():
    lab = _labels()
    a = ref.sample_indices(lab, n, N, 5, 0)
    b = ref.sample_indices(lab, n, N, 5, 1)
    c = ref.sample_indices(lab, n, N, 6, 0)
    assert not np.array_equal(a, b) and not np.array_equal(a, c)
    # the background subsets differ too, not only the order
    assert len(np.setdiff1d(a, b)) > 50
    s = {ref.slot_seeds(7, k) for k in range(64)}
    assert len({x for pair in s for x in pair}) == 128
    assert np.array_equal(a, ref.sample_indices(lab, n, N, 5, 0))


def test_edge_cases_of_the_rule():
    lab = _labels()
    assert np.array_equal(np.sort(ref.sample_indices(lab, n, n, 3, 0)), np.arange(n))  # n = N: a permutation
    allpos = np.ones(50, np.int32)
    assert np.array_equal(np.sort(ref.sample_indices(allpos, 50, 50, 3, 0)), np.arange(50))
    assert len(ref.sample_indices(None, 50, 1, 3, 0)) == 1
    with pytest.raises(ValueError):
        ref.sample_indices(lab, n, P - 1, 0, 0)
    with pytest.raises(ValueError):
        ref.sample_indices(lab, n, n + 1, 0, 0)


def _dataset():
    import point_unet_amd  # noqa: F401  (the import shim)
    from point_unet_amd import dataset
    return dataset


def test_epoch_order_rank_split_and_seeds():
    ds = _dataset()
    plan = ds.epoch_plan(11, 2, epoch=3, seed=9)
    assert [ids for _, ids, _ in plan] == [[0, 1], [2, 3], [4, 5], [6, 7], [8, 9]]  # int(11 / 2) * 2 clouds, in order (runBraTS.py:82-97)
    assert [s for _, _, s in plan] == [ref.batch_seed(9, 3, j, 0) for j in range(5)]
    r0 = ds.epoch_plan(11, 2, 3, 9, rank=0, world=2)
    r1 = ds.epoch_plan(11, 2, 3, 9, rank=1, world=2)
    assert [j for j, _, _ in r0] == [0, 2, 4] and [j for j, _, _ in r1] == [1, 3]
    assert [ids for _, ids, _ in r1] == [[2, 3], [6, 7]]
    assert [s for _, _, s in r1] == [ref.batch_seed(9, 3, j, 1) for j in (1, 3)]
    seeds = {ds.batch_seed(0, e, j, r) for e in range(20) for j in range(50) for r in range(4)}
    assert len(seeds) == 4000
    assert ds.epoch_plan(1, 2, 0) == []
    with pytest.raises(ValueError):
        ds.epoch_plan(10, 2, 0, rank=2, world=2)
