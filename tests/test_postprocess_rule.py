"""The rules of include/pointseg_postprocess.h on their numpy restatement (postprocess_ref.py; test_gpu_postprocess.py ties the kernels
to it): the restatement against scipy's and the reference's recorded results (golden/postprocess.npz, written by
golden/make_postprocess_golden.py) and against a live scipy where one is installed, the scipy facts the design rests on, and the C
surface: the header's names, the ctypes table, the exported symbols and the argument checks that need no GPU.  Every comparison is exact:
all values are integers."""
import ctypes
import os
import re

import numpy as np
import pytest

import postprocess_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "postprocess.npz"))


# ---- the restatement against the recorded results --------------------------------------------------------------------------------------

def test_inputs_are_the_formulas(golden):
    assert np.array_equal(ref.blobs_and_specks(ref.GOLDEN_SHAPE), golden["blobs"])
    assert np.array_equal(ref.hole_cases(), golden["holes_in"])
    assert np.array_equal(ref.brats_weight(), golden["brats_weight"])
    for v in (0, 1):
        assert np.array_equal(ref.brats_pred(v), golden["brats_pred_%d" % v])
        assert np.array_equal(ref.two_blob_mask(bool(v)), golden["two_in_%d" % v])
    main, ext = ref.overlap_masks()
    assert np.array_equal(main, golden["overlap_main"]) and np.array_equal(ext, golden["overlap_ext"])


@pytest.mark.parametrize("c", (1, 2, 3))
def test_label_equals_golden(golden, c):
    labels, n, sizes, _ = ref.label(golden["blobs"], c)
    assert labels.dtype == np.int32 and np.array_equal(labels, golden["label_c%d" % c]) and n == int(golden["label_n_c%d" % c])
    assert np.array_equal(sizes, np.bincount(golden["label_c%d" % c].ravel())[1:])
    assert np.array_equal(ref.label(golden["blobs"], c, background=True)[0], golden["label_bg_c%d" % c])


@pytest.mark.parametrize("c", (1, 2, 3))
def test_morphology_equals_golden(golden, c):
    b = golden["blobs"]
    assert np.array_equal(ref.closing(b, c), golden["close_c%d" % c])
    assert np.array_equal(ref.opening(b, c), golden["open_c%d" % c])
    assert np.array_equal(ref.dilate(b, c, 2), golden["dilate2_c%d" % c])
    assert np.array_equal(ref.erode(b, c, 2), golden["erode2_c%d" % c])


def test_fill_holes_equals_golden(golden):
    got = ref.fill_holes(golden["holes_in"])
    assert np.array_equal(got, golden["holes_out"])
    # (1) enclosed, (2) open through a tunnel, (3) diagonal shell, (4) diagonal tunnel: inner voxel filled, outer not, (5) nested
    assert got[13, 5, 5] == 1 and got[3, 15, 5] == 0 and got[20, 5, 20] == 1 and got[1, 25, 5] == 1 and got[0, 26, 6] == 0
    assert got[12:23, 12:23, 20:31].all()


def test_selection_equals_the_reference(golden):
    for k in (0, 1):
        m = golden["two_in_%d" % k]
        assert np.array_equal(ref.keep_components(m, ref.KEEP_LARGEST_TWO, 2), golden["two_largest_%d" % k])
        assert np.array_equal(ref.keep_components(m, ref.KEEP_ABOVE, 2, 20), golden["two_above20_%d" % k])
    assert ref.label(golden["two_largest_1"], 2)[1] == 2 and ref.label(golden["two_largest_0"], 2)[1] == 1
    got = ref.keep_components(golden["overlap_ext"], ref.KEEP_OVERLAP, 2, main=golden["overlap_main"])
    assert np.array_equal(got, golden["overlap_out"])
    assert got[18:22, 20:24, 20:23].all(), "exactly half inside is kept"


def test_selection_edge_rules():
    one = np.zeros((3, 5, 7), np.uint8)
    one[1, 1:4, 2] = 1
    assert np.array_equal(ref.keep_components(one, ref.KEEP_ABOVE, 2, 1000), one), "a lone component is kept whatever its size"
    assert not ref.keep_components(np.zeros((3, 5, 7), np.uint8), ref.KEEP_ABOVE, 2, 0).any()
    tie = one.copy()
    tie[1, 1:4, 5] = 1
    tie[0, 0, 0] = 1
    got = ref.keep_components(tie, ref.KEEP_LARGEST_TWO, 2)
    assert got.sum() == 6 and got[0, 0, 0] == 0, "equal sizes: both kept (10 * 3 > 3), the single voxel is not"
    assert ref.keep_components(tie, ref.KEEP_ABOVE, 2, 2).sum() == 6


@pytest.mark.parametrize("v", (0, 1))
def test_chain_equals_the_reference(golden, v):
    pred = golden["brats_pred_%d" % v]
    with_w = ref.brats_post_processing(pred, golden["brats_weight"])
    assert np.array_equal(with_w, golden["brats_out_%d_w" % v])
    assert np.array_equal(ref.brats_post_processing(pred), golden["brats_out_%d_nw" % v])
    assert (4 in with_w) == (v == 0), "variant 1 loses its enhancing region to the < 100 rule"


# ---- a live scipy, where there is one ----------------------------------------------------------------------------------------------------

SHAPES = [(1, 1, 1), (1, 1, 37), (1, 40, 40), (3, 5, 7), (9, 17, 33), (16, 16, 16), (33, 34, 35)]


@pytest.mark.parametrize("shape", SHAPES)
def test_restatement_equals_live_scipy(shape):
    ndimage = pytest.importorskip("scipy.ndimage")
    for m in (ref.blobs_and_specks(shape), ref.checkerboard(shape), ref.serpentine(shape), np.ones(shape, np.uint8)):
        for c in (1, 2, 3):
            s = ndimage.generate_binary_structure(3, c)
            for bg in (False, True):
                want, n = ndimage.label((m == 0) if bg else m, s)
                got = ref.label(m, c, bg)
                assert np.array_equal(got[0], want) and got[1] == n
            assert np.array_equal(ref.closing(m, c), ndimage.binary_closing(m, structure=s))
            assert np.array_equal(ref.opening(m, c, 2), ndimage.binary_opening(m, structure=s, iterations=2))
            assert np.array_equal(ref.dilate(m, c, 2), ndimage.binary_dilation(m, structure=s, iterations=2))
            assert np.array_equal(ref.erode(m, c), ndimage.binary_erosion(m, structure=s))
        assert np.array_equal(ref.fill_holes(m), ndimage.binary_fill_holes(m))


def test_scipy_numbers_by_smallest_index():
    ndimage = pytest.importorskip("scipy.ndimage")
    for c in (1, 2, 3):
        lab, n = ndimage.label(ref.blobs_and_specks((9, 17, 33), 3), ndimage.generate_binary_structure(3, c))
        first = [int(np.flatnonzero(lab.ravel() == k)[0]) for k in range(1, n + 1)]
        assert n > 3 and first == sorted(first)


def test_scipy_closing_erodes_the_border():
    ndimage = pytest.importorskip("scipy.ndimage")
    s = ndimage.generate_binary_structure(3, 2)
    cube = ndimage.binary_closing(np.ones((3, 3, 3), np.uint8), structure=s)
    assert cube.sum() == 1 and cube[1, 1, 1]
    corner = np.zeros((3, 3, 3), np.uint8)
    corner[0, 0, 0] = 1
    assert not ndimage.binary_closing(corner, structure=s).any()
    assert ref.closing(np.ones((3, 3, 3)), 2).sum() == 1 and not ref.closing(corner, 2).any()


def test_scipy_fill_holes_is_the_face_rule():
    ndimage = pytest.importorskip("scipy.ndimage")
    m = np.ones((5, 5, 5), np.uint8)
    m[2, 2, 2] = 0
    assert ndimage.binary_fill_holes(m).all()
    m[2, 2, 0:2] = 0  # a tunnel to a face
    assert np.array_equal(ndimage.binary_fill_holes(m), m != 0)


# ---- the C surface: fails before the feature exists ----------------------------------------------------------------------------------------

def _declared(hname):
    src = open(os.path.join(ROOT, "include", hname)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return set(re.findall(r"\b(ps_[a-z0-9_]+)\s*\(", src))


NAMES = {"ps_label_components", "ps_binary_morph", "ps_keep_components", "ps_fill_holes", "ps_brats_postprocess"}


def test_header_matches_its_prototype_table():
    from point_unet_amd import _lib
    assert _declared("pointseg_postprocess.h") == set(_lib.POSTPROCESS_PROTOTYPES) == NAMES
    assert not set(_lib.POSTPROCESS_PROTOTYPES) & (set(_lib.PROTOTYPES) | set(_lib.PREPARE_PROTOTYPES))
    assert not NAMES & (_declared("pointseg.h") | _declared("pointseg_prepare.h") | _declared("pointseg_train_ops.h"))
    hdr = open(os.path.join(ROOT, "include", "pointseg_postprocess.h")).read()
    for name in ("PS_MORPH_DILATE", "PS_MORPH_ERODE", "PS_MORPH_CLOSE", "PS_MORPH_OPEN", "PS_KEEP_ABOVE", "PS_KEEP_LARGEST_TWO", "PS_KEEP_OVERLAP"):
        assert int(re.search(r"#define %s (\d+)" % name, hdr).group(1)) == getattr(_lib, name)
    assert (ref.KEEP_ABOVE, ref.KEEP_LARGEST_TWO, ref.KEEP_OVERLAP) == (_lib.PS_KEEP_ABOVE, _lib.PS_KEEP_LARGEST_TWO, _lib.PS_KEEP_OVERLAP)
    assert sorted(ref.MORPH) == [_lib.PS_MORPH_DILATE, _lib.PS_MORPH_ERODE, _lib.PS_MORPH_CLOSE, _lib.PS_MORPH_OPEN]


def test_library_exports_the_symbols(lib):
    from point_unet_amd import _lib
    for name, (_, args) in _lib.POSTPROCESS_PROTOTYPES.items():
        assert len(getattr(lib, name).argtypes) == len(args)


def _size_call(lib, name, dims, connectivity=1):
    """The first call of the two-call protocol, with no context and no volume: (status, bytes)."""
    need = ctypes.c_int64(-1)
    tail = (None, ctypes.byref(need))
    if name == "ps_label_components":
        rc = lib.ps_label_components(None, None, *dims, connectivity, 0, None, None, None, None, *tail)
    elif name == "ps_binary_morph":
        rc = lib.ps_binary_morph(None, None, *dims, 3, connectivity, 1, None, *tail)
    elif name == "ps_keep_components":
        rc = lib.ps_keep_components(None, None, *dims, connectivity, 1, 0, None, None, *tail)
    elif name == "ps_fill_holes":
        rc = lib.ps_fill_holes(None, None, *dims, None, *tail)
    else:
        rc = lib.ps_brats_postprocess(None, None, None, *dims, 2000, None, *tail)
    return rc, need.value


@pytest.mark.parametrize("name", sorted(NAMES))
def test_size_call_needs_no_gpu(lib, name):
    rc, need = _size_call(lib, name, (155, 240, 240))
    V = 155 * 240 * 240
    assert rc == 0 and need >= V and need % 256 == 0
    for dims in ((0, 4, 4), (4, 4, 0), (1 << 11, 1 << 10, 1 << 10), (1 << 31, 1, 1)):
        rc, _ = _size_call(lib, name, dims)
        assert rc == 1 and name.encode() in lib.ps_last_error(), dims
    if name in ("ps_label_components", "ps_binary_morph", "ps_keep_components"):
        for c in (0, 4):
            rc, _ = _size_call(lib, name, (4, 4, 4), c)
            assert rc == 1 and name.encode() in lib.ps_last_error() and b"connectivity" in lib.ps_last_error()


def test_bad_arguments_are_found_before_any_hip_call(lib):
    need = ctypes.c_int64(0)
    assert lib.ps_binary_morph(None, None, 4, 4, 4, 9, 1, 1, None, None, ctypes.byref(need)) == 1 and b"op" in lib.ps_last_error()
    assert lib.ps_binary_morph(None, None, 4, 4, 4, 1, 1, 0, None, None, ctypes.byref(need)) == 1 and b"iterations" in lib.ps_last_error()
    assert lib.ps_keep_components(None, None, 4, 4, 4, 2, 7, 0, None, None, None, ctypes.byref(need)) == 1 and b"rule" in lib.ps_last_error()
    assert lib.ps_keep_components(None, None, 4, 4, 4, 2, 1, -1, None, None, None, ctypes.byref(need)) == 1 and b"threshold" in lib.ps_last_error()
    assert lib.ps_label_components(None, None, 4, 4, 4, 1, 2, None, None, None, None, None, ctypes.byref(need)) == 1
    assert b"background" in lib.ps_last_error()
    assert lib.ps_brats_postprocess(None, None, None, 4, 4, 4, -5, None, None, ctypes.byref(need)) == 1 and b"wt_threshold" in lib.ps_last_error()
    assert lib.ps_fill_holes(None, None, 4, 4, 4, None, None, None) == 1 and b"NULL" in lib.ps_last_error()


def test_python_surface_rejects_cpu_tensors():
    torch = pytest.importorskip("torch")
    from point_unet_amd import postprocess as pp
    m = torch.zeros((3, 4, 5), dtype=torch.uint8)
    for fn in (pp.label_components, pp.fill_holes, pp.largest_two_components, pp.brats_post_processing, lambda t: pp.binary_closing(t, 2),
               lambda t: pp.remove_external_core(t, t)):
        with pytest.raises(ValueError):
            fn(m)
