"""The rules of include/pointseg_saliency_data.h as far as they go without a GPU: the numpy restatement (saliency_data_ref.py) against the
reference's own functions (tests/golden/saliency_data.npz, written by tests/golden/make_saliency_data_golden.py) -- preparation, centre
ranges, windows --, the uniformity of the drawn centres, the choice of try on constructed cases, and the ABI: header, prototype table and
library agree, and every argument error is found before any HIP call."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import saliency_data_ref as ref
from dropout_ref import hash32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"ps_saliency_brats_measure", "ps_saliency_brats_apply", "ps_saliency_pancreas_prepare", "ps_patch_sample"}
HEADERS = ("pointseg.h", "pointseg_train_ops.h", "pointseg_prepare.h", "pointseg_postprocess.h", "pointseg_saliency.h", "pointseg_saliency_train.h",
           "pointseg_saliency_attention.h")
FAKE = ctypes.c_void_p(4096)  # non-NULL pointers no check dereferences: every case below fails before the device is touched
OUT = ctypes.c_void_p(8192)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "saliency_data.npz"))


def _declared(hname):
    src = open(os.path.join(ROOT, "include", hname)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return set(re.findall(r"\b(ps_[a-z0-9_]+)\s*\(", src))


# ---- preparation ---------------------------------------------------------------------------------------------------------------------------

def test_brats_preparation_equals_the_reference_functions(golden):
    """Box, weight and both label remaps exact; the z-score within 2e-7 max|x| (float64 sums in another order, then one cast: the bar of
    test_volume_to_cloud_against_the_reference_functions)."""
    g = golden
    for num_class, key in ((4, "label4"), (2, "label2")):
        out = ref.brats_prepare(g["raw"], g["seg"], num_class, int(g["margin"]))
        assert out["box"][0] == g["bbmin"].tolist() and out["box"][1] == g["bbmax"].tolist()
        assert out["image"].dtype == np.float32 and out["label"].dtype == np.uint8 and out["weight"].dtype == np.uint8
        assert np.array_equal(out["weight"], g["weight"]) and np.array_equal(out["label"], g[key])
        want = np.moveaxis(g["normalised"], 0, -1)
        assert out["image"].shape == want.shape
        assert np.abs(out["image"].astype(np.float64) - want).max() <= 2e-7 * np.abs(want).max()
        assert np.array_equal(out["image"] == 0, np.moveaxis(g["crop"], 0, -1) == 0)  # zeros stay zero, and nothing else becomes one
    assert g["bbmin"][0] == 0 and g["bbmax"][0] < g["raw"].shape[1] - 1  # the margin clamps at one face and not at the other
    assert (g["crop"] < 0).any() and (g["normalised"][g["crop"] < 0] != 0).all()  # negative voxels are normalised like the rest
    assert ref.brats_prepare(g["raw"], None)["label"].max() == 0


def test_brats_preparation_refuses_what_the_reference_cannot_normalise(golden):
    raw = golden["raw"].copy()
    with pytest.raises(ValueError, match="all zero"):
        ref.brats_prepare(np.concatenate([np.zeros_like(raw[:1]), raw[1:]]))
    raw[2] = -np.abs(raw[2])
    with pytest.raises(ValueError, match="modality 2 has no voxel above zero"):
        ref.brats_prepare(raw)
    raw[2] = np.where(raw[2] != 0, 1.0, 0.0)
    raw[2, 0, 6, 6] = 1.0
    with pytest.raises(ValueError, match="modality 2 has std 0"):
        ref.brats_prepare(raw)


def test_pancreas_preparation_equals_the_reference_function(golden):
    out = ref.pancreas_prepare(golden["ct"], (golden["ct"] > 0).astype(np.int64) * 3)
    assert np.array_equal(out["image"][..., 0], golden["ct_rescaled"].astype(np.float32))  # bit for bit
    assert out["weight"].min() == 1 and out["weight"].dtype == np.uint8
    assert np.array_equal(out["label"], (golden["ct"] > 0) * 3) and ref.pancreas_prepare(golden["ct"])["label"].max() == 0


# ---- centres and windows -------------------------------------------------------------------------------------------------------------------

def _pairs(g):
    for k in range(int(g["n_pairs"])):
        yield k, tuple(int(v) for v in g["in%d" % k]), tuple(int(v) for v in g["out%d" % k])


def test_centre_ranges_and_fixed_centres_are_the_recorded_ones(golden):
    """The ranges random.randint was called with inside get_random_roi_sampling_center, and the centres of the axes that draw nothing."""
    g = golden
    seen_fixed = seen_drawn = 0
    for k, n_in, n_out in _pairs(g):
        lo, hi, mid = g["centres%d" % k].tolist()
        for a in range(3):
            x0, x1 = ref.centre_range(n_in[a], n_out[a])
            rec = g["ranges%d" % k][a].tolist()
            if rec == [-1, -1]:
                assert x1 <= x0
                assert ref.centre_from_hash(n_in[a], n_out[a], 0x12345678) == lo[a] == hi[a] == mid[a]
                seen_fixed += 1
            else:
                assert x1 > x0 and [x0, x1] == rec
                assert ref.centre_from_hash(n_in[a], n_out[a], 0) == lo[a] == x0
                assert ref.centre_from_hash(n_in[a], n_out[a], 0xFFFFFFFF) == hi[a] == x1
                seen_drawn += 1
    assert seen_fixed >= 5 and seen_drawn >= 8
    assert g["ranges0"].tolist() == [[2, 7], [3, 17], [3, 20]]  # the issue's CPU run of the reference


def test_windows_equal_extract_roi_from_volume(golden):
    """Label and weight patches equal the reference's zero-fill extraction at the lowest, the highest and an interior centre; the image
    equals it inside the copied box and is the stated hash outside."""
    g = golden
    fill_rows = 0
    for k, n_in, n_out in _pairs(g):
        vol = {"image": g["vol%d" % k][..., None], "label": g["lab%d" % k], "weight": np.ones(n_in, np.uint8)}
        for i, c in enumerate(g["centres%d" % k].tolist()):
            s_fill = ref.fill_seed(1000 * k + i)
            image, weight, label, pos = ref.extract(vol, n_out, c, s_fill)
            inside = g["roi_one%d" % k][i] == 1
            assert image.dtype == np.float32 and weight.dtype == np.float32 and label.dtype == np.int32
            assert np.array_equal(weight, g["roi_one%d" % k][i]) and np.array_equal(label, g["roi_lab%d" % k][i])
            assert pos == int((g["roi_lab%d" % k][i] > 0).sum())
            assert np.array_equal(image[..., 0][inside], g["roi_vol%d" % k][i][inside])
            j = np.flatnonzero(~inside.reshape(-1)).astype(np.uint32)
            with np.errstate(over="ignore"):
                want = (hash32((j * np.uint32(2654435761)) ^ np.uint32(s_fill)) >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
            got = image.reshape(-1)[j]
            assert np.array_equal(got, want) and (got.size == 0 or (got.min() >= 0 and got.max() < 1))
            if k == 0 and i == 1:  # an odd extent (axes 0 and 2) at its highest centre: one row of fill at the far end
                assert not inside[-1].any() and not inside[:, :, -1].any() and inside[:-1, :, :-1].all()
                fill_rows += 1
    assert fill_rows == 1
    k = int(g["n_pairs"]) - 1  # patch (8, 8, 8) on (1, 1, 1): one voxel copied, to the patch's centre
    assert g["roi_one%d" % k][0].sum() == 1 and g["roi_one%d" % k][0][4, 4, 4] == 1


def test_drawn_centres_are_uniform_with_both_ends_included():
    """6000 draws over a span of 6 ([2, 7]: extent 9, patch 5): both ends are hit, each value within 5 binomial standard deviations of 1000."""
    T = 16
    draws = [ref.centres((9, 9, 9), (5, 5, 5), ref.try_seed(77, b, t, T)) for b in range(125) for t in range(T)]
    sd = math.sqrt(6000 * (1 / 6) * (5 / 6))
    flat = np.array([d[a] for d in draws for a in range(3)])  # 2000 tries x 3 axes
    assert flat.size == 6000 and flat.min() == 2 and flat.max() == 7
    counts = np.bincount(flat, minlength=8)
    assert counts[:2].sum() == 0 and counts.size == 8
    assert np.abs(counts[2:] - 1000).max() <= 5 * sd, counts


# ---- choice of try -------------------------------------------------------------------------------------------------------------------------

def test_choice_of_try_on_constructed_cases():
    Z = [0, 0, 0, 0]
    # one_positive: an earlier slot is positive -> the last slot keeps try 0 although it is empty
    assert ref.choose([[5, 0, 0, 0], Z, Z], "one_positive") == [(0, 1), (0, 1), (0, 1)]
    # only try 3 of the last slot is positive
    assert ref.choose([Z, Z, [0, 0, 0, 2]], "one_positive") == [(0, 1), (0, 1), (3, 1)]
    # an earlier slot's later tries do not count: only its try 0 was ever drawn
    assert ref.choose([[0, 9, 9, 9], [0, 7, 0, 0]], "one_positive") == [(0, 1), (1, 1)]
    # none positive: the flag, and the last try
    assert ref.choose([Z, Z], "one_positive") == [(0, 1), (3, 0)]
    # B = 1: the only slot is the last one
    assert ref.choose([[0, 0, 4, 4]], "one_positive") == [(2, 1)] and ref.choose([Z], "one_positive") == [(3, 0)]
    assert ref.choose([[1, 0, 0, 0]], "one_positive") == [(0, 1)]
    # all_positive: every slot on its own
    assert ref.choose([[0, 3, 0, 1], Z, [2, 0, 0, 0]], "all_positive") == [(1, 1), (3, 0), (0, 1)]
    # random: try 0, always ok
    assert ref.choose([Z, [0, 1, 1, 1]], "random") == [(0, 1), (0, 1)]
    assert ref.choose([[0], [0]], "one_positive") == [(0, 1), (0, 0)] and ref.choose([[0], [3]], "all_positive") == [(0, 0), (0, 1)]


def test_sample_follows_the_choice_end_to_end():
    """Two volumes of (6, 6, 6): 0 is empty, 1 is all label 2.  Patch (4, 4, 4)."""
    rng = np.random.default_rng(5)
    bank = [{"image": rng.random((6, 6, 6, 2), dtype=np.float32), "label": np.full((6, 6, 6), v, np.uint8), "weight": np.ones((6, 6, 6), np.uint8)}
            for v in (0, 2)]
    images, weights, labels, info = ref.sample(bank, [[0, 1, 1], [0, 0, 1]], (4, 4, 4), 9, "one_positive")
    assert info[:, 0].tolist() == [0, 2] and info[:, 1].tolist() == [0, 1] and info[:, 6].tolist() == [1, 1] and info[:, 7].tolist() == [0, 0]
    assert info[0, 5] == 0 and info[1, 5] == int((labels[1] > 0).sum()) > 0 and labels[0].max() == 0 and set(np.unique(labels[1])) <= {0, 2}
    assert images.shape == (2, 4, 4, 4, 2) and weights.shape == labels.shape == (2, 4, 4, 4)
    for b in range(2):  # the centre stands in info, and the copied box is where the weight is 1
        c = info[b, 2:5].tolist()
        assert c == ref.centres((6, 6, 6), (4, 4, 4), ref.try_seed(9, b, int(info[b, 0]), 3))
        w = ref.window((6, 6, 6), (4, 4, 4), c)
        dst, src = tuple(x[0] for x in w), tuple(x[1] for x in w)
        assert np.array_equal(images[b][dst], bank[info[b, 1]]["image"][src]) and weights[b][dst].min() == 1 and weights[b].sum() == weights[b][dst].size
    _, _, _, info = ref.sample(bank, [[0, 1, 1], [0, 0, 0]], (4, 4, 4), 9, "one_positive")
    assert info[1, [0, 5, 6]].tolist() == [2, 0, 0]
    _, _, _, info = ref.sample(bank, [[0, 1, 1], [0, 0, 0]], (4, 4, 4), 9, "all_positive")
    assert info[:, 0].tolist() == [1, 2] and info[:, 6].tolist() == [1, 0]
    a = ref.sample(bank, [[1, 0, 0], [1, 0, 0]], (4, 4, 4), 9, "random")
    assert not np.array_equal(a[3][0, 2:5], a[3][1, 2:5]) or not np.array_equal(a[0][0], a[0][1])  # the same volume in two slots: two draws


def test_epoch_plan_is_reproducible_and_differs_per_epoch_and_rank():
    from point_unet_amd import saliency_data as sd
    plan = sd.epoch_plan(7, 2, 3, seed=11, tries=4)
    assert [j for j, _, _ in plan] == [0, 1, 2] and all(c.shape == (2, 4) and c.dtype == np.int32 and c.min() >= 0 and c.max() < 7 for _, c, _ in plan)
    again = sd.epoch_plan(7, 2, 3, seed=11, tries=4)
    assert all(np.array_equal(a[1], b[1]) and a[2] == b[2] for a, b in zip(plan, again))
    for _, c, _ in plan:  # a slot's next try is the next datapoint of the stream
        assert np.array_equal(c[0, 1:], c[1, :-1])
    stream = [int(plan[0][1][0, t]) for t in range(4)] + [int(plan[0][1][1, 3])]
    assert sorted(sd.shuffled_ids(7, 123)) == list(range(7)) and len(set(stream)) == 5  # five positions of one shuffled pass
    other = sd.epoch_plan(7, 2, 4, seed=11, tries=4)
    assert any(not np.array_equal(a[1], b[1]) for a, b in zip(plan, other)) and all(a[2] != b[2] for a, b in zip(plan, other))
    r0, r1 = sd.epoch_plan(7, 2, 3, seed=11, tries=4, rank=0, world=2), sd.epoch_plan(7, 2, 3, seed=11, tries=4, rank=1, world=2)
    assert [j for j, _, _ in r0] == [0, 2] and [j for j, _, _ in r1] == [1]
    assert np.array_equal(r0[0][1], plan[0][1]) and np.array_equal(r1[0][1], plan[1][1]) and not np.array_equal(r0[0][1], r1[0][1])
    assert r1[0][2] != plan[1][2]  # the seed carries the rank
    with pytest.raises(ValueError):
        sd.epoch_plan(7, 2, 0, rank=2, world=2)


# ---- header, table, library ----------------------------------------------------------------------------------------------------------------

def test_header_table_and_library_agree(lib):
    from point_unet_amd import _lib
    assert _declared("pointseg_saliency_data.h") == set(_lib.SALIENCY_DATA_PROTOTYPES) == NAMES
    for table in (_lib.PROTOTYPES, _lib.PREPARE_PROTOTYPES, _lib.POSTPROCESS_PROTOTYPES, _lib.SALIENCY_PROTOTYPES, _lib.SALIENCY_TRAIN_PROTOTYPES,
                  _lib.SALIENCY_ATTENTION_PROTOTYPES):
        assert not NAMES & set(table)
    for h in HEADERS:
        assert not NAMES & _declared(h), h
    for name, (_, args) in _lib.SALIENCY_DATA_PROTOTYPES.items():
        assert len(getattr(lib, name).argtypes) == len(args)
    src = open(os.path.join(ROOT, "include", "pointseg_saliency_data.h")).read()
    assert '#include "pointseg.h"' in src
    for cite in ("utils.py:30-60", "utils.py:62-78", "data_sampler.py:169-214", "data_sampler.py:77-88", "utils.py:390-421"):
        assert cite in src, cite
    for name, value in (("PS_PATCH_MAX_B", _lib.PS_PATCH_MAX_B), ("PS_PATCH_MAX_T", _lib.PS_PATCH_MAX_T), ("PS_PATCH_MAX_C", _lib.PS_PATCH_MAX_C),
                        ("PS_PATCH_RANDOM", _lib.PS_PATCH_RANDOM), ("PS_PATCH_ALL_POSITIVE", _lib.PS_PATCH_ALL_POSITIVE),
                        ("PS_PATCH_ONE_POSITIVE", _lib.PS_PATCH_ONE_POSITIVE)):
        assert int(re.search(r"#define %s (\d+)" % name, src).group(1)) == value
    mk = open(os.path.join(ROOT, "point-unet_amd", "csrc", "Makefile")).read()
    assert "saliency_data.hip" in mk and "pointseg_saliency_data.h" in mk


# ---- argument checks -----------------------------------------------------------------------------------------------------------------------

def _ptrs(*vals):
    return (ctypes.c_void_p * len(vals))(*vals)


def _sample(lib, **kw):
    """ps_patch_sample on a bank of two fake volumes of (9, 20, 23); kw replaces arguments."""
    a = dict(ctx=FAKE, images=_ptrs(4096, 4096), labels=_ptrs(4096, 4096), weights=_ptrs(4096, 4096), dims=(ctypes.c_int64 * 6)(9, 20, 23, 9, 20, 23), n=2, C=1,
             cand=(ctypes.c_int32 * 6)(0, 1, 0, 1, 1, 0), B=3, T=2, P=(ctypes.c_int64 * 3)(5, 6, 7), seed=1, mode=2, out_images=OUT, out_weights=OUT,
             out_labels=OUT, out_info=OUT)
    a.update(kw)
    return lib.ps_patch_sample(*a.values())


def test_patch_sample_argument_checks(lib):
    err = lib.ps_last_error
    i64 = lambda *v: (ctypes.c_int64 * len(v))(*v)
    bad = [(dict(C=0), b"C = 0"), (dict(C=17), b"C = 17"), (dict(B=0), b"B = 0"), (dict(B=65), b"B = 65"), (dict(T=0), b"T = 0"), (dict(T=17), b"T = 17"),
           (dict(mode=3), b"mode = 3"), (dict(mode=-1), b"mode = -1"), (dict(n=0), b"n = 0"),
           (dict(images=None), b"NULL images"), (dict(labels=None), b"NULL images"), (dict(weights=None), b"NULL images"), (dict(dims=None), b"NULL images"),
           (dict(cand=None), b"NULL images"), (dict(P=None), b"NULL images"),
           (dict(out_images=None), b"NULL out_images"), (dict(out_weights=None), b"NULL out_images"), (dict(out_labels=None), b"NULL out_images"),
           (dict(out_info=None), b"NULL out_images"),
           (dict(P=i64(0, 6, 7)), b"P = [0, 6, 7]"), (dict(P=i64(5, 6, -1)), b"P = [5, 6, -1]"), (dict(P=i64(2048, 2048, 512)), b"P = ["),
           (dict(P=i64(1024, 1024, 512), C=4), b"P = ["),
           (dict(images=_ptrs(4096, None)), b"volume 1 has a NULL"), (dict(labels=_ptrs(None, 4096)), b"volume 0 has a NULL"),
           (dict(weights=_ptrs(4096, None)), b"volume 1 has a NULL"),
           (dict(dims=i64(9, 20, 23, 9, 0, 23)), b"dims of volume 1"), (dict(dims=i64(-1, 20, 23, 9, 20, 23)), b"dims of volume 0"),
           (dict(dims=i64(2048, 2048, 512, 9, 20, 23)), b"dims of volume 0"),
           (dict(cand=(ctypes.c_int32 * 6)(0, 1, 0, 2, 1, 0)), b"cand[1, 1] = 2"), (dict(cand=(ctypes.c_int32 * 6)(0, 1, 0, 1, -1, 0)), b"cand[2, 0] = -1"),
           (dict(n=1), b"cand[0, 1] = 1")]
    for kw, word in bad:  # with a context and without one: the context is looked at last
        for ctx in (FAKE, None):
            assert _sample(lib, ctx=ctx, **kw) == 1 and b"ps_patch_sample:" in err() and word in err(), (kw, err())
    assert _sample(lib, ctx=None) == 1 and b"ps_patch_sample:" in err() and b"context" in err()
    for mode in (0, 1, 2):
        assert _sample(lib, ctx=None, mode=mode, B=1, T=1) == 1 and b"context" in err()
    assert _sample(lib, ctx=None, B=64, T=16, C=16, cand=(ctypes.c_int32 * 1024)()) == 1 and b"context" in err()  # the limits themselves are legal


def test_preparation_argument_checks(lib):
    err = lib.ps_last_error
    box, stats = (ctypes.c_int64 * 6)(0, 1, 1, 9, 13, 12), (ctypes.c_double * 8)(*([1.0, 2.0] * 4))

    def measure(**kw):
        a = dict(ctx=FAKE, raw=FAKE, C=4, D=12, H=14, W=15, margin=5, box=box, stats=stats)
        a.update(kw)
        return lib.ps_saliency_brats_measure(*a.values())

    def apply(**kw):
        a = dict(ctx=FAKE, raw=FAKE, seg=FAKE, C=4, D=12, H=14, W=15, num_class=2, box=box, stats=stats, image=OUT, label=OUT, weight=OUT)
        a.update(kw)
        return lib.ps_saliency_brats_apply(*a.values())

    def pancreas(**kw):
        a = dict(ctx=FAKE, ct=FAKE, dtype=1, n=100, label=FAKE, image=OUT, out_label=OUT, weight=OUT)
        a.update(kw)
        return lib.ps_saliency_pancreas_prepare(*a.values())

    shape = [(dict(C=0), b"C = 0"), (dict(C=17), b"C = 17"), (dict(D=0), b"the volume is [0, 14, 15]"), (dict(W=-3), b"the volume is"),
             (dict(D=2048, H=2048, W=512), b"the volume is")]
    for call, who, more in ((measure, b"ps_saliency_brats_measure:", [(dict(margin=-1), b"margin = -1"), (dict(raw=None), b"NULL raw"), (dict(box=None), b"NULL raw"),
                                                                       (dict(stats=None), b"NULL raw")]),
                            (apply, b"ps_saliency_brats_apply:", [(dict(num_class=1), b"num_class = 1"), (dict(raw=None), b"NULL raw"), (dict(image=None), b"NULL raw"),
                                                                   (dict(label=None), b"NULL raw"), (dict(weight=None), b"NULL raw"), (dict(stats=None), b"NULL raw"),
                                                                   (dict(box=(ctypes.c_int64 * 6)(0, 1, 1, 12, 13, 12)), b"box axis 0 is [0, 12]"),
                                                                   (dict(box=(ctypes.c_int64 * 6)(0, 5, 1, 9, 4, 12)), b"box axis 1 is [5, 4]"),
                                                                   (dict(box=(ctypes.c_int64 * 6)(0, 1, -1, 9, 13, 12)), b"box axis 2"),
                                                                   (dict(stats=(ctypes.c_double * 8)(1, 2, 1, 0, 1, 2, 1, 2)), b"stats of modality 1"),
                                                                   (dict(stats=(ctypes.c_double * 8)(1, 2, 1, 2, math.nan, 2, 1, 2)), b"stats of modality 2"),
                                                                   (dict(stats=(ctypes.c_double * 8)(1, 2, 1, 2, 1, 2, 1, math.inf)), b"stats of modality 3")])):
        for kw, word in shape + more:
            for ctx in (FAKE, None):
                assert call(ctx=ctx, **kw) == 1 and who in err() and word in err(), (kw, err())
        assert call(ctx=None) == 1 and who in err() and b"context" in err()
    assert apply(ctx=None, seg=None) == 1 and b"context" in err()  # no segmentation is legal
    for kw, word in ((dict(dtype=3), b"dtype = 3"), (dict(dtype=0), b"dtype = 0"), (dict(n=0), b"n = 0"), (dict(n=1 << 31), b"n = 2147483648"),
                     (dict(ct=None), b"NULL ct"), (dict(image=None), b"NULL ct"), (dict(out_label=None), b"NULL ct"), (dict(weight=None), b"NULL ct")):
        for ctx in (FAKE, None):
            assert pancreas(ctx=ctx, **kw) == 1 and b"ps_saliency_pancreas_prepare:" in err() and word in err(), (kw, err())
    assert pancreas(ctx=None) == 1 and b"context" in err() and pancreas(ctx=None, label=None, dtype=2) == 1 and b"context" in err()


def test_python_surface_rejects_cpu_tensors_and_bad_arguments():
    torch = pytest.importorskip("torch")
    from point_unet_amd import saliency_data as sd
    with pytest.raises(ValueError, match="channels"):
        sd.PatchBank(17)
    bank = sd.PatchBank(1)
    with pytest.raises(ValueError, match="CPU tensor"):
        bank.add_pancreas(torch.zeros((4, 4, 4)))
    with pytest.raises(ValueError, match="CPU tensor"):
        sd.PatchBank(4).add_brats(torch.zeros((4, 4, 4, 4)))
    with pytest.raises(ValueError, match="one channel"):
        sd.PatchBank(4).add_pancreas(np.zeros((4, 4, 4), np.int16))
    with pytest.raises(ValueError, match="mode"):
        bank.sample([[0]], (4, 4, 4), mode="some_positive")
    with pytest.raises(ValueError, match="volume ids"):
        bank.sample([[0]], (4, 4, 4))  # an empty bank
    with pytest.raises(ValueError, match="integer"):
        bank.sample([[0.5]], (4, 4, 4))
    with pytest.raises(ValueError, match="TrainableSaliencyNet"):
        sd.train_saliency(torch.nn.Linear(1, 1), bank, 1, (16, 16, 16))
    assert len(bank) == 0 and set(sd.MODES) == set(ref.MODES)
