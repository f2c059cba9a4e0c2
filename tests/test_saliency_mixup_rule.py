"""The rules of include/pointseg_saliency_mixup.h as far as they go without a GPU: the numpy restatement's `mix` against the reference's own
mixup (tests/golden/saliency_mixup.npz, written by tests/golden/make_saliency_mixup_golden.py), the mixed batch's choice of try on
constructed cases, the torch soft loss against the hard-label restatement, and the ABI: header, prototype table and library agree, and every
argument error of the five entries is found before any HIP call."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import saliency_data_ref as dref
import saliency_mixup_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"ps_patch_sample_mixup", "ps_softmax_dice_soft_loss", "ps_softmax_dice_soft_loss_bwd", "ps_saliency_backward_soft", "ps_saliency_train_step_soft"}
HEADERS = ("pointseg.h", "pointseg_train_ops.h", "pointseg_prepare.h", "pointseg_postprocess.h", "pointseg_saliency.h", "pointseg_saliency_train.h",
           "pointseg_saliency_attention.h", "pointseg_saliency_data.h", "pointseg_saliency_step.h")
FAKE = ctypes.c_void_p(4096)  # non-NULL pointers no check dereferences: every case below fails before the device is touched
OUT = ctypes.c_void_p(8192)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "saliency_mixup.npz"))


def _declared(hname):
    src = open(os.path.join(ROOT, "include", hname)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return set(re.findall(r"\b(ps_[a-z0-9_]+)\s*\(", src))


# ---- mixing --------------------------------------------------------------------------------------------------------------------------------

def test_mix_equals_the_reference_mixup_bit_for_bit(golden):
    g = golden
    assert g["gammas"].tolist() == [0.0, 1.0, 0.5, 1.0 - 2.0 ** -30, 1e-12, 0.34029683942911143] and g["classes"].tolist() == [2, 4]
    sums = set()
    for K in (2, 4):
        a, b = g["image_a%d" % K], g["image_b%d" % K]
        assert a.dtype == np.float32 and (a < 0).any() and (a == 0).any() and g["hot_a%d" % K].shape == (a.size, K)
        assert set(np.unique(g["hot_a%d" % K])) == {0.0, 1.0} and (g["hot_a%d" % K].sum(1) == 1).all()
        for i, gamma in enumerate(g["gammas"]):
            image = ref.mix(a, b, gamma)
            hot = ref.mix(g["hot_a%d" % K], g["hot_b%d" % K], gamma)
            assert image.dtype == hot.dtype == np.float32
            assert np.array_equal(image.view(np.uint32), g["mix_image%d_%d" % (K, i)].view(np.uint32)), (K, gamma)
            assert np.array_equal(hot.view(np.uint32), g["mix_hot%d_%d" % (K, i)].view(np.uint32)), (K, gamma)
            assert g["mix_weight%d_%d" % (K, i)].dtype == np.bool_
            assert np.array_equal(ref.mix_weights(g["weight_a%d" % K], g["weight_b%d" % K]), g["mix_weight%d_%d" % (K, i)].astype(np.float32))
            # the values a soft label takes: 0, g, h and fl32(g + h)
            gf, hf = np.float32(gamma), np.float32(1.0 - gamma)
            assert set(np.unique(hot)) <= {np.float32(0), gf, hf, np.float32(gf + hf)}
            sums.add(float(np.float32(gf + hf)))
    # float32(gamma) is exactly 1 while float32(1 - gamma) is a tiny non-zero number: nothing may special-case g == 1
    assert np.float32(1.0 - 2.0 ** -30) == 1 and np.float32(2.0 ** -30) > 0 and np.float32(1e-12) > 0
    assert sums <= {1.0, float(np.nextafter(np.float32(1), np.float32(0)))} and 1.0 in sums  # fl32(g + h) is 1 or the float32 below it
    assert np.array_equal(ref.one_hot(np.array([0, 2, 5]), 3), np.array([[1, 0, 0], [0, 0, 1], [0, 0, 0]], np.float32))


# ---- choice of try -------------------------------------------------------------------------------------------------------------------------

def test_choice_of_try_of_the_mixed_batch_on_constructed_cases():
    Z = [0, 0, 0, 0]
    late = [0, 0, 0, 2]
    # B = 1 (two samples): no earlier sample, so sample 0 must be positive; sample 1, the last, stays on try 0 although it is empty
    assert ref.choose_mixup([late, Z], "one_positive") == [(3, 1), (0, 1)]
    assert ref.choose_mixup([[1, 0, 0, 0], Z], "one_positive") == [(0, 1), (0, 1)] and ref.choose_mixup([Z, late], "one_positive") == [(3, 0), (0, 1)]
    # B = 2 (three samples): sample 1 is the forced one, sample 2 is free
    assert ref.choose_mixup([Z, late, late], "one_positive") == [(0, 1), (3, 1), (0, 1)]
    assert ref.choose_mixup([[4, 0, 0, 0], Z, late], "one_positive") == [(0, 1), (0, 1), (0, 1)]  # an earlier sample is positive
    assert ref.choose_mixup([[0, 9, 9, 9], [0, 7, 0, 0], Z], "one_positive") == [(0, 1), (1, 1), (0, 1)]  # only an earlier sample's try 0 counts
    assert ref.choose_mixup([Z, Z, [5, 5, 5, 5]], "one_positive") == [(0, 1), (3, 0), (0, 1)]  # nothing qualifies: the flag, the last try
    # B = 3 (four samples): sample 2 is forced -- not sample 3, which ps_patch_sample's rule at four slots would force
    assert ref.choose_mixup([Z, Z, late, late], "one_positive") == [(0, 1), (0, 1), (3, 1), (0, 1)]
    assert dref.choose([Z, Z, late, late], "one_positive") == [(0, 1), (0, 1), (0, 1), (3, 1)]
    assert ref.choose_mixup([Z, [2, 0, 0, 0], late, Z], "one_positive") == [(0, 1)] * 4
    assert ref.choose_mixup([Z, Z, Z, [1, 1, 1, 1]], "one_positive") == [(0, 1), (0, 1), (3, 0), (0, 1)]  # the last sample does not count as earlier
    # all_positive: every sample on its own; random: try 0, always ok
    assert ref.choose_mixup([[0, 3, 0, 1], Z, [2, 0, 0, 0], late], "all_positive") == [(1, 1), (3, 0), (0, 1), (3, 1)]
    assert ref.choose_mixup([Z, [0, 1, 1, 1]], "random") == [(0, 1), (0, 1)]
    for B in (1, 2, 3):
        for mode in dref.MODES:
            assert len(ref.choose_mixup([Z] * (B + 1), mode)) == B + 1
    assert ref.choose_mixup([[0], [0]], "one_positive") == [(0, 0), (0, 1)] and ref.choose_mixup([[0], [3]], "all_positive") == [(0, 0), (0, 1)]
    with pytest.raises(ValueError):
        ref.choose_mixup([Z], "random")


def test_sample_mixup_follows_the_choice_end_to_end():
    """Two volumes of (6, 6, 6): 0 is empty, 1 is all label 1.  Patch (4, 4, 4), two classes."""
    rng = np.random.default_rng(5)
    bank = [{"image": rng.random((6, 6, 6, 2), dtype=np.float32), "label": np.full((6, 6, 6), v, np.uint8), "weight": np.ones((6, 6, 6), np.uint8)}
            for v in (0, 1)]
    gamma = np.array([0.25, 1.0])
    cand = [[0, 0, 0], [0, 1, 1], [0, 1, 1]]
    images, weights, soft, info = ref.sample_mixup(bank, cand, (4, 4, 4), 9, "one_positive", 2, gamma)
    assert images.shape == (2, 4, 4, 4, 2) and weights.shape == (2, 4, 4, 4) and soft.shape == (2, 4, 4, 4, 2) and info.shape == (3, 8)
    assert info[:, 0].tolist() == [0, 1, 0] and info[:, 6].tolist() == [1, 1, 1]  # sample B - 1 = 1 is forced, sample 2 stays on its empty try 0
    # sample 1 is the same drawn patch in slots 0 and 1
    plain = dref.extract(bank[1], (4, 4, 4), info[1, 2:5].tolist(), dref.fill_seed(dref.try_seed(9, 1, 1, 3)))
    first = dref.extract(bank[0], (4, 4, 4), info[0, 2:5].tolist(), dref.fill_seed(dref.try_seed(9, 0, 0, 3)))
    assert np.array_equal(images[0], ref.mix(first[0], plain[0], 0.25)) and np.array_equal(images[1], plain[0])  # gamma 1: sample 1 itself
    inside = plain[1] == 1
    assert np.array_equal(soft[1][inside], np.tile(np.float32([0, 1]), (inside.sum(), 1)))
    assert np.array_equal(soft[0][inside & (first[1] == 1)], np.tile(np.float32([0.25, 0.75]), ((inside & (first[1] == 1)).sum(), 1)))
    assert np.array_equal(weights[0], np.maximum(first[1], plain[1]))
    # outside both copied boxes: class 0 with weight g + h, the weight map 0
    both_out = (first[1] == 0) & (plain[1] == 0)
    if both_out.any():
        assert (soft[0][both_out] == np.float32([1, 0])).all() and (weights[0][both_out] == 0).all()


# ---- the soft loss -------------------------------------------------------------------------------------------------------------------------

def test_soft_loss_on_one_hot_labels_is_the_hard_label_loss():
    torch = pytest.importorskip("torch")
    import saliency_train_ref as tref
    rng = np.random.default_rng(3)
    for B, V, C, weighted in ((2, 37, 2, True), (1, 50, 4, False), (2, 20, 3, True)):
        logits = torch.from_numpy(rng.standard_normal((B, V, C)))
        labels = rng.integers(0, C, (B, V))
        weight = torch.from_numpy(rng.uniform(0.2, 3.0, (B, V))) if weighted else None
        soft = torch.from_numpy(ref.one_hot(labels, C)).double()
        a = ref.soft_dice_loss(logits, soft, weight)
        b = tref.softmax_dice_loss(logits, torch.from_numpy(labels), weight)
        assert a.dtype == torch.float64 and float(a) == float(b)
        assert ref.soft_dice_loss(logits.float(), soft, weight).dtype == torch.float32
    half = 0.5 * soft + 0.5 * soft.roll(1, -1)  # genuinely soft rows change the loss
    assert float(ref.soft_dice_loss(logits, half, weight)) != float(a)


# ---- header, table, library ----------------------------------------------------------------------------------------------------------------

def test_header_table_and_library_agree(lib):
    from point_unet_amd import _lib
    assert _declared("pointseg_saliency_mixup.h") == set(_lib.SALIENCY_MIXUP_PROTOTYPES) == NAMES
    for table in (_lib.PROTOTYPES, _lib.PREPARE_PROTOTYPES, _lib.POSTPROCESS_PROTOTYPES, _lib.SALIENCY_PROTOTYPES, _lib.SALIENCY_TRAIN_PROTOTYPES,
                  _lib.SALIENCY_ATTENTION_PROTOTYPES, _lib.SALIENCY_DATA_PROTOTYPES, _lib.SALIENCY_STEP_PROTOTYPES):
        assert not NAMES & set(table)
    for h in HEADERS:
        assert not NAMES & _declared(h), h
    for name, (_, args) in _lib.SALIENCY_MIXUP_PROTOTYPES.items():
        assert len(getattr(lib, name).argtypes) == len(args)
    src = open(os.path.join(ROOT, "include", "pointseg_saliency_mixup.h")).read()
    for cite in ("data_sampler.py:329-337", "data_sampler.py:90-96", "utils.py:511-527", "model.py:550-590, 602-612"):
        assert cite in src, cite
    mk = open(os.path.join(ROOT, "point-unet_amd", "csrc", "Makefile")).read()
    assert "pointseg_saliency_mixup.h" in mk
    for path in ("include/pointseg_saliency_data.h", "point-unet_amd/saliency_data.py"):  # the "not built" sentences lost mixup
        text = open(os.path.join(ROOT, path)).read()
        assert not re.search(r"Not built[^.]*mixup", text), path


# ---- argument checks -----------------------------------------------------------------------------------------------------------------------

def _ptrs(*vals):
    return (ctypes.c_void_p * len(vals))(*vals)


def _f64(*v):
    return (ctypes.c_double * len(v))(*v)


def _sample(lib, **kw):
    """ps_patch_sample_mixup on a bank of two fake volumes of (9, 20, 23): B = 2, so three rows of cand; kw replaces arguments."""
    a = dict(ctx=FAKE, images=_ptrs(4096, 4096), labels=_ptrs(4096, 4096), weights=_ptrs(4096, 4096), dims=(ctypes.c_int64 * 6)(9, 20, 23, 9, 20, 23), n=2, C=1,
             cand=(ctypes.c_int32 * 6)(0, 1, 0, 1, 1, 0), B=2, T=2, P=(ctypes.c_int64 * 3)(5, 6, 7), seed=1, mode=2, K=2, gamma=_f64(0.25, 1.0), out_images=OUT,
             out_weights=OUT, out_soft=OUT, out_info=OUT)
    a.update(kw)
    return lib.ps_patch_sample_mixup(*a.values())


def test_patch_sample_mixup_argument_checks(lib):
    err = lib.ps_last_error
    i64 = lambda *v: (ctypes.c_int64 * len(v))(*v)
    bad = [(dict(C=0), b"C = 0"), (dict(C=17), b"C = 17"), (dict(B=0), b"B = 0"), (dict(B=64), b"B = 64"), (dict(T=0), b"T = 0"), (dict(T=17), b"T = 17"),
           (dict(mode=3), b"mode = 3"), (dict(mode=-1), b"mode = -1"), (dict(n=0), b"n = 0"), (dict(K=1), b"num_classes = 1"), (dict(K=17), b"num_classes = 17"),
           (dict(images=None), b"NULL images"), (dict(labels=None), b"NULL images"), (dict(weights=None), b"NULL images"), (dict(dims=None), b"NULL images"),
           (dict(cand=None), b"NULL images"), (dict(P=None), b"NULL images"),
           (dict(out_images=None), b"NULL out_images"), (dict(out_weights=None), b"NULL out_images"), (dict(out_soft=None), b"NULL out_images"),
           (dict(out_info=None), b"NULL out_images"),
           (dict(gamma=None), b"NULL gamma"), (dict(gamma=_f64(0.5, math.nan)), b"gamma[1] = nan"), (dict(gamma=_f64(-0.1, 0.5)), b"gamma[0] = -0.1"),
           (dict(gamma=_f64(0.5, 1.5)), b"gamma[1] = 1.5"), (dict(gamma=_f64(math.inf, 0.5)), b"gamma[0] = inf"),
           (dict(P=i64(0, 6, 7)), b"P = [0, 6, 7]"), (dict(P=i64(5, 6, -1)), b"P = [5, 6, -1]"), (dict(P=i64(2048, 2048, 512)), b"P = ["),
           (dict(P=i64(1024, 1024, 512)), b"num_classes"), (dict(P=i64(512, 512, 512), K=16), b"must stay below 2^31"),
           (dict(images=_ptrs(4096, None)), b"volume 1 has a NULL"), (dict(dims=i64(9, 20, 23, 9, 0, 23)), b"dims of volume 1"),
           (dict(cand=(ctypes.c_int32 * 6)(0, 1, 0, 2, 1, 0)), b"cand[1, 1] = 2"), (dict(cand=(ctypes.c_int32 * 6)(0, 1, 0, 1, 1, -1)), b"cand[2, 1] = -1"),
           (dict(n=1), b"cand[0, 1] = 1")]
    for kw, word in bad:  # with a context and without one: the context is looked at last
        for ctx in (FAKE, None):
            assert _sample(lib, ctx=ctx, **kw) == 1 and b"ps_patch_sample_mixup:" in err() and word in err(), (kw, err())
    assert _sample(lib, ctx=None) == 1 and b"ps_patch_sample_mixup:" in err() and b"context" in err()
    for mode in (0, 1, 2):
        assert _sample(lib, ctx=None, mode=mode, B=1, T=1) == 1 and b"context" in err()
    for g in (0.0, 1.0, 1.0 - 2.0 ** -30, 1e-12):  # the ends of [0, 1] are legal
        assert _sample(lib, ctx=None, gamma=_f64(g, g)) == 1 and b"context" in err()
    # the limits themselves are legal: 63 mixed slots are 64 drawn samples
    assert _sample(lib, ctx=None, B=63, T=16, C=16, K=16, cand=(ctypes.c_int32 * 1024)(), gamma=_f64(*([0.5] * 63))) == 1 and b"context" in err()


def test_soft_loss_argument_checks(lib):
    err = lib.ps_last_error
    need = ctypes.c_int64(1 << 20)

    def loss(**kw):
        a = dict(ctx=FAKE, logits=FAKE, soft=FAKE, weight=None, B=2, V=100, C=2, loss=OUT, sums=OUT, scratch=OUT, bytes=ctypes.byref(need))
        a.update(kw)
        return lib.ps_softmax_dice_soft_loss(*a.values())

    def bwd(**kw):
        a = dict(ctx=FAKE, logits=FAKE, soft=FAKE, weight=None, sums=FAKE, dloss=None, B=2, V=100, C=2, dlogits=OUT)
        a.update(kw)
        return lib.ps_softmax_dice_soft_loss_bwd(*a.values())

    shape = [(dict(C=1), b"C = 1"), (dict(C=17), b"C = 17"), (dict(B=0), b"B = 0"), (dict(V=0), b"V = 0"), (dict(V=1 << 31), b"V = 2147483648")]
    for call, who, more in ((loss, b"ps_softmax_dice_soft_loss:", [(dict(logits=None), b"NULL logits or soft"), (dict(soft=None), b"NULL logits or soft"),
                                                                   (dict(loss=None), b"NULL loss or sums"), (dict(sums=None), b"NULL loss or sums")]),
                            (bwd, b"ps_softmax_dice_soft_loss_bwd:", [(dict(logits=None), b"NULL logits, soft or sums"), (dict(soft=None), b"NULL logits, soft or sums"),
                                                                      (dict(sums=None), b"NULL logits, soft or sums"), (dict(dlogits=None), b"NULL dlogits")])):
        for kw, word in shape + more:
            for ctx in (FAKE, None):
                assert call(ctx=ctx, **kw) == 1 and who in err() and word in err(), (kw, err())
        assert call(ctx=None) == 1 and who in err() and b"context" in err()
    assert loss(bytes=None) == 1 and b"NULL scratch_bytes" in err()
    # the sizing call needs no pointer and no context, and asks for what the hard-label op asks for
    soft_need, hard_need = ctypes.c_int64(0), ctypes.c_int64(0)
    assert lib.ps_softmax_dice_soft_loss(None, None, None, None, 2, 9001, 4, None, None, None, ctypes.byref(soft_need)) == 0
    assert lib.ps_softmax_dice_loss(None, None, None, None, 2, 9001, 4, None, None, None, ctypes.byref(hard_need)) == 0
    assert soft_need.value == hard_need.value > 0
    small = ctypes.c_int64(16)
    assert loss(bytes=ctypes.byref(small)) == 1 and b"ps_softmax_dice_soft_loss:" in err()  # scratch too small


def test_soft_step_argument_checks(lib):
    err = lib.ps_last_error
    n = lib.ps_saliency_weight_count(1, 2)
    need, hard = ctypes.c_int64(0), ctypes.c_int64(0)
    assert lib.ps_saliency_backward_soft(None, None, None, None, 1, 16, 16, 16, 1, 2, None, n, None, None, None, None, ctypes.byref(need)) == 0
    assert lib.ps_saliency_backward(None, None, None, None, 1, 16, 16, 16, 1, 2, None, n, None, None, None, None, ctypes.byref(hard)) == 0
    assert need.value == hard.value > 0  # scratch accounting is unchanged: the soft tensor is the caller's
    step_need = ctypes.c_int64(0)
    assert lib.ps_saliency_train_step_soft(None, None, None, None, 1, 16, 16, 16, 1, 2, None, n, None, None, 0.01, None, None, None, None,
                                           ctypes.byref(step_need)) == 0 and step_need.value == need.value
    W, G, A = ctypes.c_void_p(1 << 30), ctypes.c_void_p(2 << 30), ctypes.c_void_p(3 << 30)

    def backward(**kw):
        a = dict(ctx=FAKE, x=FAKE, soft=FAKE, weight=None, B=1, D=16, H=16, W=16, C_in=1, K=2, weights=W, count=n, grads=G, loss=OUT, logits=None, scratch=OUT)
        a.update(kw)
        return lib.ps_saliency_backward_soft(*a.values(), ctypes.byref(ctypes.c_int64(need.value)))

    def step(**kw):
        a = dict(ctx=FAKE, x=FAKE, soft=FAKE, weight=None, B=1, D=16, H=16, W=16, C_in=1, K=2, params=W, count=n, grads=G, accum=A, lr=0.01, options=None,
                 loss=OUT, logits=None, scratch=OUT)
        a.update(kw)
        return lib.ps_saliency_train_step_soft(*a.values(), ctypes.byref(ctypes.c_int64(need.value)))

    for call, who in ((backward, b"ps_saliency_backward_soft:"), (step, b"ps_saliency_train_step_soft:")):
        for kw, word in ((dict(D=24), b"multiple of 16"), (dict(W=8), b"multiple of 16"), (dict(count=n - 1), b"weight_count"), (dict(K=1), b"num_classes = 1"),
                         (dict(K=17), b"num_classes = 17"), (dict(grads=ctypes.c_void_p((1 << 30) + 16)), b"must not overlap"), (dict(x=None), b"NULL"),
                         (dict(soft=None), b"NULL"), (dict(grads=None), b"NULL"), (dict(loss=None), b"NULL"), (dict(ctx=None), b"NULL")):
            assert call(**kw) == 1 and who in err() and word in err(), (kw, err())
    assert step(accum=None) == 1 and b"NULL" in err() and step(accum=G) == 1 and b"must not overlap" in err()


# ---- the Python surface ----------------------------------------------------------------------------------------------------------------------

def test_python_surface_rejects_bad_mixup_arguments():
    torch = pytest.importorskip("torch")
    from point_unet_amd import saliency_data as sd
    bank = sd.PatchBank(1)
    for mixup in (1, 17, 2.5, True):
        with pytest.raises(ValueError, match="mixup"):
            bank.sample([[0], [0]], (4, 4, 4), mixup=mixup)
    with pytest.raises(ValueError, match="gamma"):
        bank.sample([[0], [0]], (4, 4, 4), gamma=[0.5])  # gamma without mixup
    with pytest.raises(ValueError, match="volume ids"):
        bank.sample([[0], [0]], (4, 4, 4), mixup=2)  # an empty bank
    bank._vols.append((None, torch.zeros((4, 4, 4), dtype=torch.uint8), None, None))  # (one volume's worth of shape: the checks below never reach the device)
    with pytest.raises(ValueError, match=r"\[B \+ 1, T\]"):
        bank.sample([[0]], (4, 4, 4), mixup=2)  # one row: no pair to mix
    with pytest.raises(ValueError, match=r"\[B \+ 1, T\]"):
        bank.sample(np.zeros((65, 1), np.int64), (4, 4, 4), mixup=2)
    for gamma in ([0.5, 0.5], [math.nan], [-0.1], [1.5], [[0.5]]):
        with pytest.raises(ValueError, match="gamma"):
            bank.sample([[0], [0]], (4, 4, 4), mixup=2, gamma=gamma)


def test_epoch_batches_plans_one_more_row_with_mixup(monkeypatch):
    from point_unet_amd import saliency_data as sd
    bank = sd.PatchBank(1)
    bank._vols = [None] * 7
    seen = []
    monkeypatch.setattr(sd.PatchBank, "sample", lambda self, cand, patch, seed, mode, mixup=None: seen.append((cand, seed, mode, mixup)) or len(seen))
    assert list(bank.epoch_batches(2, (4, 4, 4), 3, seed=11, tries=4, mixup=2)) == [1, 2]
    plan = sd.epoch_plan(7, 3, 3, seed=11, tries=4)
    assert len(plan) == 7 // 3 == len(seen)
    for (cand, seed, mode, mixup), (_, want, s) in zip(seen, plan):
        assert cand.shape == (3, 4) and np.array_equal(cand, want) and seed == s and mode == "one_positive" and mixup == 2
    del seen[:]
    assert list(bank.epoch_batches(2, (4, 4, 4), 3, seed=11, tries=4)) == [1, 2, 3]  # without mixup: today's plan
    plain = sd.epoch_plan(7, 2, 3, seed=11, tries=4)
    assert all(np.array_equal(c, w) and m is None for (c, _, _, m), (_, w, _) in zip(seen, plain)) and len(seen) == 3
