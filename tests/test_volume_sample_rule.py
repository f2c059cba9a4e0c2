"""The sampling rule of ps_volume_sample on its numpy restatement (volume_sample_ref.py; test_gpu_volume_sample.py ties the kernels to it bit
for bit): every positive first and ascending in every draw, the background subset and its order uniform over fixed seeds, prefixes (the
pyramid's sub-samples) hold the mask first, loops and seeds draw different subsets; the restated dilation / threshold / statistics against
scipy and numpy; and the C surface: the prototype, the struct layout revision and the ctypes struct's size.  Bounds are explicit multiples
of the binomial standard deviation, as in test_cloud_sample_rule.py."""
import ctypes
import os

import numpy as np
import pytest

import volume_sample_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

n, P, N, SEEDS = 1000, 100, 400, 3000


def _mask():
    m = np.zeros(n, np.uint8)
    m[np.random.default_rng(7).choice(n, P, replace=False)] = 1
    return m


@pytest.fixture(scope="module")
def draws():
    m = _mask()
    return m, np.stack([ref.sample_indices(m, N, s, 0) for s in range(SEEDS)])


def _check_binomial(counts, trials, p, sigmas=5.0):
    sd = np.sqrt(trials * p * (1 - p))
    assert np.abs(counts - trials * p).max() <= sigmas * sd, (counts.min(), counts.max(), trials * p, sd)


def test_every_positive_comes_first_and_ascending(draws):
    m, d = draws
    pos = np.flatnonzero(m)
    for row in d:
        assert len(row) == N and len(np.unique(row)) == N
        assert np.array_equal(row[:P], pos)
        assert not m[row[P:]].any()


def test_background_inclusion_is_uniform(draws):
    m, d = draws
    bg = np.flatnonzero(m == 0)
    inc = np.zeros(n, np.int64)
    np.add.at(inc, d.reshape(-1), 1)
    p = (N - P) / (n - P)
    _check_binomial(inc[bg], SEEDS, p)
    var = inc[bg].var()
    assert 0.8 <= var / (SEEDS * p * (1 - p)) <= 1.2


def test_tail_position_of_a_background_point_is_uniform(draws):
    m, d = draws
    bg = np.flatnonzero(m == 0)
    for pt in bg[[0, 1, 200, 500, 899]]:
        hit = d[:, P:] == pt
        where = np.argmax(hit, axis=1)[hit.any(axis=1)]
        hist = np.bincount(where // ((N - P) // 10), minlength=10)
        _check_binomial(hist, len(where), 0.1)


def test_prefixes_hold_the_mask_first(draws):
    m, d = draws
    pos, bg = np.flatnonzero(m), np.flatnonzero(m == 0)
    pre = np.zeros(n, np.int64)
    np.add.at(pre, d[:, :N // 2].reshape(-1), 1)
    assert (pre[pos] == SEEDS).all()
    _check_binomial(pre[bg], SEEDS, (N // 2 - P) / (n - P))
    assert N // 4 == P  # at these sizes the quarter prefix is the mask and nothing else
    assert all(np.array_equal(row[:N // 4], pos) for row in d)


def test_loops_and_seeds_draw_different_subsets():
    m = _mask()
    a = ref.sample_indices(m, N, 5, 0)
    b = ref.sample_indices(m, N, 5, 1)
    c = ref.sample_indices(m, N, 6, 0)
    assert not np.array_equal(a, b) and not np.array_equal(a, c)
    assert len(np.setdiff1d(a, b)) > 50 and len(np.setdiff1d(a, c)) > 50
    assert np.array_equal(a, ref.sample_indices(m, N, 5, 0))


def test_edge_cases_of_the_rule():
    m = _mask()
    none = np.zeros(n, np.uint8)
    r = ref.sample_indices(none, N, 3, 0)  # P = 0
    assert len(np.unique(r)) == N
    assert np.array_equal(ref.sample_indices(m, P, 3, 0), np.flatnonzero(m))  # P = N: the mask alone
    full = ref.sample_indices(m, n, 3, 0)  # N = n
    assert np.array_equal(np.sort(full), np.arange(n)) and np.array_equal(full[:P], np.flatnonzero(m))
    assert len(ref.sample_indices(none, 0, 3, 0)) == 0  # N = 0
    assert ref.sample(np.zeros((2, 5, 100), np.int16), none, 0, 3, 1)["idx"].shape == (3, 0)
    with pytest.raises(ValueError):
        ref.sample_indices(m, P - 1, 0, 0)
    with pytest.raises(ValueError):
        ref.sample_indices(m, n + 1, 0, 0)


def test_restated_dilation_equals_scipy():
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(3)
    m = rng.random((13, 9, 17)) < 0.03
    m[0, 0, 0] = m[-1, -1, -1] = m[5, 0, 16] = True  # faces and corners
    for r in (1, 3):
        assert np.array_equal(ref.dilate(m, r), ndimage.binary_dilation(m, iterations=r))


def test_restated_threshold_and_statistics():
    t = np.float32(0.9)
    p = np.array([np.nextafter(t, np.float32(0)), t, np.nextafter(t, np.float32(1)), 0.0, 1.0], np.float32)
    probs = np.stack([1 - p, p], -1)
    assert np.array_equal(ref.threshold_mask(probs, 1, 0.9), probs[..., 1] >= 0.9)
    assert ref.threshold_mask(probs, 1, 0.9).tolist() == [False, True, True, False, True]
    rng = np.random.default_rng(4)
    vol = np.clip(rng.normal(-200, 400, (40, 36, 28)), -1024, 3000).astype(np.int16)
    mean, std = ref.statistics(vol)
    assert mean == vol.mean()
    assert abs(std - vol.std()) <= 1e-12 * vol.std()
    idx = np.arange(vol.size)
    want = ((vol - vol.mean()) / vol.std()).astype(np.float32).reshape(-1)  # the reference's expression (dataPreparePancreas.py:42-45)
    got = ref.values(vol, idx, mean, std)
    assert np.abs(got - want).max() <= 2e-7 * np.abs(want).max()
    origin, xyz = ref.rows(vol.shape, idx)
    g = np.stack(np.meshgrid(*[np.arange(s) for s in vol.shape], indexing="ij"), -1).reshape(-1, 3)
    assert np.array_equal(origin, g) and np.array_equal(xyz, g.astype(np.uint16).astype(np.float32) / np.array(vol.shape, np.float32))


# ---- the C surface: fails before the feature exists ------------------------------------------------------------------------------------------

def test_prototype_and_layout_revision():
    from point_unet_amd import _lib
    assert "ps_volume_sample" in _lib.PROTOTYPES
    assert _lib.PS_ABI_VERSION == 7


def test_ctypes_struct_matches_the_compiled_one(lib):
    from point_unet_amd import _lib
    dbg = ctypes.CDLL(os.path.join(ROOT, "point-unet_amd", "libpointseg_debug.so"))
    dbg.ps_debug_volume_sample_args_size.restype = ctypes.c_int
    assert dbg.ps_debug_volume_sample_args_size() == ctypes.sizeof(_lib.PsVolumeSampleArgs)
    assert not hasattr(lib, "ps_debug_volume_sample_args_size")


def test_argument_errors_need_no_gpu(lib):
    """Every argument error is found before any HIP call."""
    from point_unet_amd import _lib
    a = _lib.PsVolumeSampleArgs()
    assert lib.ps_volume_sample(None, ctypes.byref(a)) == 1 and b"NULL" in lib.ps_last_error()
