"""CPU tests that PIN the oracle: against every committed golden vector (generated from the real reference C++,
tests/golden/make_golden.py) and against the real reference itself on fresh inputs -- live where oracle/_ref is present, else
through the digests of its outputs in tests/golden/ref_digests.json."""
import glob
import hashlib
import json
import os

import numpy as np
import pytest

from conftest import brats_cloud, uniform_cloud

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def test_knn_oracle_matches_every_golden_vector(oracle):
    files = sorted(glob.glob(os.path.join(GOLD, "knn_*.npz")))
    assert len(files) >= 8
    for f in files:
        g = np.load(f)
        got = oracle.knn_batch(g["support"], g["queries"], int(g["K"]))
        assert np.array_equal(got, g["idx"]), f


def test_fewer_points_than_k_keeps_zeros(oracle):
    g = np.load(os.path.join(GOLD, "knn_fewer_than_k.npz"))
    assert np.all(g["idx"][:, :, 7:] == 0)  # knn.pyx:93: np.zeros, partially filled


def test_pyramid_golden(oracle):
    from oracle import randla_oracle as ro
    g = np.load(os.path.join(GOLD, "pyramid_brats6000.npz"))
    pts, nbr, pool, up = ro.build_pyramid(lambda s, q, k: oracle.knn_batch(s, q, k), g["xyz"], int(g["K"]), list(g["ratios"]))
    for i in range(5):
        assert np.array_equal(nbr[i], g["neigh_%d" % i])
        assert np.array_equal(pool[i], g["sub_%d" % i])
        assert np.array_equal(up[i], g["interp_%d" % i])


def test_grid_oracle_matches_golden_vectors(oracle):
    g = np.load(os.path.join(GOLD, "grid_all.npz"))
    p, f, l = oracle.canonical_rows(*oracle.grid_subsample(g["points"], g["features"], g["classes"], float(g["sampleDl"])))
    assert np.array_equal(p, g["out_points"]) and np.array_equal(f, g["out_features"]) and np.array_equal(l, g["out_classes"])
    g = np.load(os.path.join(GOLD, "grid_points_only.npz"))
    p, _, _ = oracle.canonical_rows(*oracle.grid_subsample(g["points"], None, None, float(g["sampleDl"])))
    assert np.array_equal(p, g["out_points"])
    g = np.load(os.path.join(GOLD, "grid_negative_coords.npz"))
    p, f, _ = oracle.canonical_rows(*oracle.grid_subsample(g["points"], g["features"], None, float(g["sampleDl"])))
    assert np.array_equal(p, g["out_points"]) and np.array_equal(f, g["out_features"])


def test_network_oracle_regression_pin(oracle):
    import netcase
    from oracle import randla_oracle as ro
    from point_unet_amd import weights
    g = np.load(os.path.join(GOLD, "net_config1.npz"))
    cfg, xyz, feats = netcase.config1()
    params = weights.init_params(cfg, seed=2, randomize_bn=True)
    pts, nbr, pool, up = ro.build_pyramid(lambda s, q, k: oracle.knn_batch(s, q, k), xyz, cfg.k_n, cfg.sub_sampling_ratio)
    assert np.array_equal(nbr[0][0, :256], g["neigh_0_rows"]) and np.array_equal(up[0][0, :256], g["interp_0_rows"])
    tap = {}
    logits = ro.inference(params, cfg.num_layers, pts, nbr, pool, up, feats, np.float64, tap=tap)
    assert np.abs(logits - g["logits"]).max() < 1e-5
    assert np.abs(tap["enc0"][0, :64] - g["enc0_rows"]).max() < 1e-5
    # the float32 evaluation of the same graph stays well inside the 1e-4 parity budget
    l32 = ro.inference(params, cfg.num_layers, pts, nbr, pool, up, feats, np.float32)
    assert np.abs(l32 - logits).max() < 5e-5


REF_DIGESTS = json.load(open(os.path.join(GOLD, "ref_digests.json")))  # the real reference's outputs on the inputs below (make_golden.py)


def digest(a):
    a = np.ascontiguousarray(a)
    return hashlib.sha256(("%s%s" % (a.dtype.str, a.shape)).encode() + a.tobytes()).hexdigest()


def same_as_reference(oracle, got, key, ref):
    """`got` equals what the real reference computes: its stored digest always, and the live output of oracle/_ref (`ref()`) where
    that could be built (it needs the reference sources)."""
    if oracle.have_ref():
        want = ref()
        assert digest(want) == REF_DIGESTS[key], key
        return np.array_equal(got, want)
    return digest(got) == REF_DIGESTS[key]


@pytest.mark.parametrize("K", [1, 16, 32])
def test_knn_oracle_vs_real_reference_fresh_inputs(oracle, K):
    for j, p in enumerate((uniform_cloud(9000, 21), brats_cloud(9000, 22, grid=(48, 48, 32)))):
        assert same_as_reference(oracle, oracle.knn_batch(p[None], p[None], K), "knn_k%d_cloud%d" % (K, j),
                                 lambda: oracle.ref_knn_batch(p[None], p[None], K))
        sub = p[:2250]
        assert same_as_reference(oracle, oracle.knn_batch(sub[None], p[None], 1), "upsample_cloud%d" % j,
                                 lambda: oracle.ref_knn_batch(sub[None], p[None], 1))


def test_knn_oracle_threading_variants_agree(oracle):
    rng = np.random.default_rng(5)
    s = rng.random((4, 2500, 3), dtype=np.float32)
    q = rng.random((4, 700, 3), dtype=np.float32)
    if oracle.have_ref():
        assert np.array_equal(oracle.ref_knn_batch(s, q, 16, omp=True), oracle.ref_knn_batch(s, q, 16, omp=False))
    for got in (oracle.knn_batch(s, q, 16, threads=4), oracle.knn_batch(s, q, 16, threads=3, qpar=True)):
        assert same_as_reference(oracle, got, "threading_k16", lambda: oracle.ref_knn_batch(s, q, 16, omp=False))


def test_grid_oracle_vs_real_reference_fresh_inputs(oracle):
    rng = np.random.default_rng(3)
    p = rng.random((30000, 3), dtype=np.float32)
    f = rng.standard_normal((30000, 3)).astype(np.float32)
    a = oracle.canonical_rows(*oracle.grid_subsample(p, f, None, 0.05))
    b = lambda: oracle.canonical_rows(*oracle.ref_grid_subsample(p, f, None, 0.05))  # noqa: E731
    assert same_as_reference(oracle, a[0], "grid_points", lambda: b()[0])
    assert same_as_reference(oracle, a[1], "grid_features", lambda: b()[1])
