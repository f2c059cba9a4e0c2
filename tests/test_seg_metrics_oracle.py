"""The test-side restatement of medpy's hd95 (tests/seg_metrics_oracle.py): its scipy form equals the brute force, and the committed
golden generator reproduces tests/golden/seg_metrics.npz.  No GPU."""
import os

import numpy as np
import pytest

import seg_metrics_oracle as so

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("shape,variant", [((24, 24, 24), 0), ((20, 24, 22), 1), ((9, 17, 13), 0), ((24, 7, 16), 2)])
@pytest.mark.parametrize("spacing", [(1.0, 1.0, 1.0), (0.8, 0.8, 2.5), (1.5, 0.7, 1.1)])
def test_scipy_restatement_equals_brute_force(shape, variant, spacing):
    pytest.importorskip("scipy")
    pred, truth = so.label_pair(shape, variant)
    a = so.region_metrics(pred, truth, so.BRATS_REGIONS, spacing)
    b = so.region_metrics(pred, truth, so.BRATS_REGIONS, spacing, brute=True)
    for r in so.BRATS_REGIONS:
        assert {k: a[r][k] for k in ("dice", "n_pred", "n_truth", "n_both")} == {k: b[r][k] for k in ("dice", "n_pred", "n_truth", "n_both")}
        assert a[r]["hd95"] == pytest.approx(b[r]["hd95"], rel=1e-12)


def test_borders_agree_and_touch_the_faces():
    pytest.importorskip("scipy")
    m = np.zeros((6, 7, 8), bool)
    m[:, 2:5, 3:] = True  # touches four faces
    assert np.array_equal(so.border_numpy(m), so.border_scipy(m))
    assert so.border_numpy(m)[0, 3, 5] and so.border_numpy(m)[3, 3, 7] and not so.border_numpy(m)[3, 3, 5]


def test_empty_mask_rules():
    z = np.zeros((4, 4, 4), bool)
    one = z.copy()
    one[1, 2, 3] = True
    assert so.hd95_brute(z, z) == 0.0 and so.dice(z, z) == 1.0
    assert so.hd95_brute(one, z) == float("inf") and so.dice(one, z) == 0.0
    assert so.hd95_brute(one, one) == 0.0


def test_golden_generator_reproduces_the_npz():
    pytest.importorskip("scipy")
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_seg_metrics_golden", os.path.join(HERE, "golden", "make_seg_metrics_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    got = gen.compute()
    want = np.load(os.path.join(HERE, "golden", "seg_metrics.npz"))
    assert set(got) == set(want.files)
    for k in want.files:
        if k.endswith("/counts"):
            assert np.array_equal(got[k], want[k]), k
        else:
            np.testing.assert_allclose(got[k], want[k], rtol=1e-12, err_msg=k)
