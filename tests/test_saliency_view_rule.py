"""include/pointseg_saliency_view.h without a GPU: the restated rule (saliency_view_ref.py) equals what the reference's own sampler3d gave
under the three config.DIRECTION values and with its flip switched on (tests/golden/saliency_view.npz, make_saliency_view_golden.py); the
restatement's index arithmetic (no copies) equals its defining identity (copies); header, prototype table and library agree and the old
entries still resolve; the argument errors that need no device; the Python surface's own checks."""
import ctypes
import os
import re

import numpy as np
import pytest

import saliency_data_ref as ref
import saliency_view_ref as vref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"ps_patch_sample_view", "ps_patch_sample_mixup_view"}
FAKE = ctypes.c_void_p(4096)  # non-NULL pointers no check dereferences: every case below fails before the device is touched
OUT = ctypes.c_void_p(8192)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "saliency_view.npz"))


# ---- the restatement against the reference's sampler3d ---------------------------------------------------------------------------------------

def test_restatement_equals_sampler3d_in_every_direction_and_flipped(golden):
    g = golden
    runs = flips = 0
    for k in range(int(g["n_cases"])):
        shape, P = tuple(int(v) for v in g["shape%d" % k]), tuple(int(v) for v in g["patch%d" % k])
        vol = {"image": g["image%d" % k], "label": g["label%d" % k], "weight": np.ones(shape, np.uint8)}
        assert len(set(shape)) == 3  # non-cubic: a wrong permutation has another shape or other extents
        for view in g["directions"]:
            seen = vref.to_view(vol, view)
            ext = seen["label"].shape
            assert ext == tuple(shape[a] for a in vref.AXES[view])
            for pick in g["picks"]:
                for flip in (0, 1):
                    key = "%d_%s_%s_%d" % (k, view, pick, flip)
                    if "centre_" + key not in g:
                        assert flip == 1
                        continue
                    centre = [int(c) for c in g["centre_" + key]]
                    # the ranges sampler3d drew from are the rule's, on the VIEW's extents
                    want = [ref.centre_range(ext[a], P[a]) for a in range(3)]
                    assert g["ranges_" + key].tolist() == [list(r) for r in want if r[1] > r[0]]
                    for a in range(3):
                        x0, x1 = want[a]
                        assert centre[a] == ((x0 + x1) // 2 if x1 <= x0 else {"lo": x0, "hi": x1, "mid": (x0 + x1) // 2}[str(pick)])
                    image, weight, label, _ = ref.extract(seen, P, centre, 12345)
                    if flip:
                        image, weight, label = np.flip(image, 2), np.flip(weight, 2), np.flip(label, 2)
                    box = g["weight_" + key] > 0
                    assert np.array_equal(weight, g["weight_" + key]) and np.array_equal(label, g["label_" + key])
                    assert np.array_equal((image * box[..., None]).view(np.uint32), g["image_" + key].view(np.uint32))
                    if flip:  # the golden tells a flipped patch from an unflipped one, in all three arrays
                        plain = "%d_%s_%s_0" % (k, view, pick)
                        assert np.array_equal(np.flip(g["image_" + plain], 2), g["image_" + key]) and not np.array_equal(g["image_" + plain], g["image_" + key])
                        assert not np.array_equal(g["label_" + plain], g["label_" + key])
                        flips += 1
                    runs += 1
    assert runs == 3 * 3 * 4 and flips == 9
    # an off-centre box: the flip of the weight is seen where an odd extent at its highest centre leaves fill at the far end
    assert any(not np.array_equal(g["weight_%d_%s_hi_0" % (k, v)], g["weight_%d_%s_hi_1" % (k, v)]) for k in range(3) for v in vref.VIEWS)


def _bank(C, shapes, seed):
    rng = np.random.default_rng(seed)
    return [{"image": rng.standard_normal(s + (C,)).astype(np.float32), "label": ((rng.random(s) < 0.3) * rng.integers(1, 4, s)).astype(np.uint8),
             "weight": (rng.random(s) < 0.7).astype(np.uint8)} for s in shapes]


@pytest.mark.parametrize("view", vref.VIEWS)
def test_index_arithmetic_equals_the_copies(view):
    """The header's rule as the kernels apply it -- the box in view and in volume axes (saliency_view_ref.box), the volume never permuted --
    equals the defining identity on permuted copies, flip and info included; hard and mixed."""
    bank = _bank(2, ((9, 20, 23), (4, 6, 30), (1, 1, 1), (3, 2, 4)), 5)
    ax = vref.AXES[view]
    P, seed, T = (5, 6, 7), 77, 2
    cand = np.array([[0, 1], [2, 3], [1, 0], [3, 2]])
    flip = [1, 0, 1, 1]
    images, weights, labels, info = vref.sample_view(bank, cand, P, seed, "random", view, flip)
    assert info[:, 7].tolist() == flip and info[:, 0].tolist() == [0] * 4
    for b in range(4):
        vol = bank[cand[b, 0]]
        s = ref.try_seed(seed, b, 0, T)
        h = [int(ref.hash32((s + ref.AXIS_MUL * (a + 1)) & ref.M32)) for a in range(3)]
        ext, c, lo, n, vsrc, vn = vref.box(vol["label"].shape, P, view, h)
        assert info[b, 2:5].tolist() == c and sorted(vn) == sorted(n)
        got = ref.uniform(int(np.prod(P)) * 2, ref.fill_seed(s)).reshape(P + (2,))
        src = tuple(slice(vsrc[a], vsrc[a] + vn[a]) for a in range(3))
        dst = tuple(slice(lo[a], lo[a] + n[a]) for a in range(3))
        got[dst] = np.transpose(vol["image"][src], ax + (3,))  # (a view of the box: no copy of the volume)
        lab = np.zeros(P, np.int32)
        lab[dst] = np.transpose(vol["label"][src], ax)
        if flip[b]:
            got, lab = np.flip(got, 2), np.flip(lab, 2)
        assert np.array_equal(got.view(np.uint32), images[b].view(np.uint32)) and np.array_equal(lab, labels[b])
    # mixed: a flip on drawn sample 1 shows in slots 0 and 1, and nowhere else
    gamma = [0.25, 0.5, 0.75]
    base = vref.sample_mixup_view(bank, cand, P, seed, "random", 4, gamma, view)
    one = vref.sample_mixup_view(bank, cand, P, seed, "random", 4, gamma, view, [0, 1, 0, 0])
    changed = [not np.array_equal(base[0][b], one[0][b]) for b in range(3)]
    assert changed == [True, True, False] and one[3][:, 7].tolist() == [0, 1, 0, 0] and base[3][:, 7].tolist() == [0] * 4
    plain = vref.sample_view(bank, cand, P, seed, "random", view, [0, 1, 0, 0])
    assert np.array_equal(one[0][0], vref.mref.mix(plain[0][0], plain[0][1], 0.25)) and np.array_equal(one[3][:, :7], plain[3][:, :7])
    # the axial view without a flip is the old rule
    if view == "axial":
        old = ref.sample(bank, cand, P, seed, "one_positive")
        new = vref.sample_view(bank, cand, P, seed, "one_positive")
        assert all(np.array_equal(a, b) for a, b in zip(old, new))


# ---- header, table, library ----------------------------------------------------------------------------------------------------------------

def _declared(hname):
    src = open(os.path.join(ROOT, "include", hname)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return set(re.findall(r"\b(ps_[a-z0-9_]+)\s*\(", src))


C_TYPES = {"ps_context*": ctypes.c_void_p, "float*": ctypes.c_void_p, "int32_t*": ctypes.c_void_p, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64,
           "uint32_t": ctypes.c_uint32, "const int32_t*": ctypes.POINTER(ctypes.c_int32), "const int64_t*": ctypes.POINTER(ctypes.c_int64),
           "const double*": ctypes.POINTER(ctypes.c_double), "const float* const*": ctypes.POINTER(ctypes.c_void_p),
           "const uint8_t* const*": ctypes.POINTER(ctypes.c_void_p)}


def test_header_table_and_library_agree(lib):
    from point_unet_amd import _lib
    assert _declared("pointseg_saliency_view.h") == set(_lib.SALIENCY_VIEW_PROTOTYPES) == NAMES
    for h in os.listdir(os.path.join(ROOT, "include")):
        if h != "pointseg_saliency_view.h":
            assert not NAMES & _declared(h), h
    # the old headers and tables keep their names, and the old entries still resolve
    assert "ps_patch_sample" in _declared("pointseg_saliency_data.h") and "ps_patch_sample_mixup" in _declared("pointseg_saliency_mixup.h")
    assert "ps_patch_sample" in _lib.SALIENCY_DATA_PROTOTYPES and "ps_patch_sample_mixup" in _lib.SALIENCY_MIXUP_PROTOTYPES
    assert _lib.PS_ABI_VERSION == 7 and lib.ps_abi_version() == 7
    for name in ("ps_patch_sample", "ps_patch_sample_mixup"):
        assert getattr(lib, name).argtypes is not None
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pointseg_saliency_view.h")).read(), flags=re.S)
    for name, old in (("ps_patch_sample_view", _lib.SALIENCY_DATA_PROTOTYPES["ps_patch_sample"]),
                      ("ps_patch_sample_mixup_view", _lib.SALIENCY_MIXUP_PROTOTYPES["ps_patch_sample_mixup"])):
        args = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, src, flags=re.S).group(1)
        types = [C_TYPES[re.sub(r"\s*\b[A-Za-z_0-9]+$", "", a.strip())] for a in args.split(",")]
        res, want = _lib.SALIENCY_VIEW_PROTOTYPES[name]
        assert res is ctypes.c_int and types == want and len(getattr(lib, name).argtypes) == len(want) == len(old[1]) + 2
        assert want[:-6] == old[1][:-4] and want[-6:-4] == [ctypes.c_int32, ctypes.POINTER(ctypes.c_int32)]  # view and flip in front of the outputs
    text = open(os.path.join(ROOT, "include", "pointseg_saliency_view.h")).read()
    assert '#include "pointseg_saliency_mixup.h"' in text and '#include "pointseg_saliency_map.h"' in text
    for cite in ("data_sampler.py:169-214", "utils.py:80-104", "data_sampler.py:190-207"):
        assert cite in text, cite
    for sentence in ("byte-equal", "No permuted or mirrored copy", "before anything is enqueued", "info[7]"):
        assert sentence in text, sentence
    mk = open(os.path.join(ROOT, "point-unet_amd", "csrc", "Makefile")).read()
    assert "pointseg_saliency_view.h" in mk and "asan-sampler" in mk


def test_documents_name_the_entries():
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "ps_patch_sample_view" in readme and "pointseg_saliency_view.h" in readme
    assert "4.19" in open(os.path.join(ROOT, "DESIGN.md")).read()
    for path in ("README.md", os.path.join("include", "pointseg_saliency_data.h"), os.path.join("point-unet_amd", "saliency_data.py")):
        assert not re.search(r"Not built[^.]*DIRECTION", open(os.path.join(ROOT, path)).read()), path


# ---- argument checks -----------------------------------------------------------------------------------------------------------------------

def _ptrs(*vals):
    return (ctypes.c_void_p * len(vals))(*vals)


def _args(mixed, **kw):
    a = dict(ctx=FAKE, images=_ptrs(4096, 4096), labels=_ptrs(4096, 4096), weights=_ptrs(4096, 4096), dims=(ctypes.c_int64 * 6)(9, 20, 23, 9, 20, 23), n=2, C=1,
             cand=(ctypes.c_int32 * 6)(0, 1, 0, 1, 1, 0), B=2 if mixed else 3, T=2, P=(ctypes.c_int64 * 3)(5, 6, 7), seed=1, mode=2)
    if mixed:
        a.update(K=2, gamma=(ctypes.c_double * 2)(0.25, 0.5))
    a.update(view=0, flip=None, out_images=OUT, out_weights=OUT, out_labels=OUT, out_info=OUT)
    a.update(kw)
    return a


@pytest.mark.parametrize("mixed", [False, True], ids=["hard", "mixed"])
def test_view_argument_checks_need_no_device(lib, mixed):
    err = lib.ps_last_error
    fn = lib.ps_patch_sample_mixup_view if mixed else lib.ps_patch_sample_view
    who = b"ps_patch_sample_mixup_view:" if mixed else b"ps_patch_sample_view:"
    i32 = lambda *v: (ctypes.c_int32 * len(v))(*v)
    i64 = lambda *v: (ctypes.c_int64 * len(v))(*v)
    bad = [(dict(view=3), b"view = 3"), (dict(view=-1), b"view = -1"), (dict(flip=i32(0, 2, 0)), b"flip[1] = 2"), (dict(flip=i32(0, 0, -1)), b"flip[2] = -1"),
           (dict(view=1, flip=i32(1, 1, 7)), b"flip[2] = 7"),
           # the old entries' errors, through the new ones and on every view
           (dict(view=1, C=17), b"C = 17"), (dict(view=2, T=0), b"T = 0"), (dict(view=1, P=i64(5, 0, 7)), b"P = [5, 0, 7]"),
           (dict(view=2, dims=i64(9, 20, 23, 9, 0, 23)), b"dims of volume 1"), (dict(view=1, out_info=None), b"NULL out_images"),
           (dict(view=1, cand=i32(0, 1, 0, 2, 1, 0)), b"cand[1, 1] = 2"),
           # the sagittal grid: (slot, view row j) rows below 2^24
           (dict(view=1, P=i64(1, 1 << 23, 1)), b"sagittal")]
    for kw, word in bad:  # with a context and without one: the context is looked at last
        for ctx in (FAKE, None):
            assert fn(*_args(mixed, ctx=ctx, **kw).values()) == 1 and who in err() and word in err(), (kw, err())
    for view in (0, 1, 2):
        for flip in (None, i32(1, 0, 1)):
            assert fn(*_args(mixed, ctx=None, view=view, flip=flip).values()) == 1 and who in err() and b"context" in err()
    assert fn(*_args(mixed, ctx=None, view=2, P=i64(1, 1 << 23, 1)).values()) == 1 and b"context" in err()  # only the sagittal grid has that limit
    # the old entries keep their own name in their errors
    old = lib.ps_patch_sample_mixup if mixed else lib.ps_patch_sample
    a = _args(mixed, ctx=None)
    del a["view"], a["flip"]
    assert old(*a.values()) == 1 and (b"ps_patch_sample_mixup:" if mixed else b"ps_patch_sample:") in err() and b"context" in err()


def test_python_surface_refuses_bad_arguments():
    """PatchBank.sample(direction=, flip=) and train_saliency(direction=, flip=): the checks that come before anything touches a device."""
    import inspect
    from point_unet_amd import saliency_data as sd
    for fn in (sd.PatchBank.sample, sd.PatchBank.epoch_batches, sd.train_saliency):
        p = inspect.signature(fn).parameters
        assert p["direction"].default == "axial" and p["flip"].default is None
    bank = sd.PatchBank(1)
    view_args = lambda *a: bank._view_args("PatchBank.sample", *a)
    assert view_args("axial", None, 3, 0) == (0, None) and view_args("sagittal", None, 3, 0)[0] == 1 and view_args("coronal", None, 3, 0)[0] == 2
    view, bits = view_args("coronal", [1, 0, 1], 3, 0)
    assert list(bits) == [1, 0, 1]
    _, drawn = view_args("axial", "random", 5, 21)
    assert list(drawn) == np.random.default_rng(21).integers(0, 2, 5).tolist()
    for direction, flip, word in (("oblique", None, "direction"), ("axial", [0, 1], "flip"), ("axial", [0, 1, 2], "flip"), ("axial", "always", "flip"),
                                  ("axial", [[0, 1, 0]], "flip")):
        with pytest.raises(ValueError, match=word):
            view_args(direction, flip, 3, 0)
    assert "evaluate_saliency(bank, nets" in sd.__doc__ and "direction=view" in sd.__doc__
