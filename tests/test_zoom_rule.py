"""The rule of ps_volume_zoom on its numpy restatement (zoom_ref.py; test_gpu_volume_zoom.py ties the kernels to it): the restatement
against scipy's recorded results (golden/volume_zoom.npz, written by golden/make_zoom_golden.py) and against a live scipy where one is
installed, the Pancreas resampling chains of the reference's two scripts on the restatement, and the C surface: the new header's names,
the ctypes table, the exported symbol and the argument check that needs no GPU.

Bounds (the issue's): order 0 equal voxel for voxel; int16 order 3 equal except on rounding ties (zoom_ref.ties: the float64 value within
1e-6 of a tie), which may be at most 1 % of a case with a resampled axis shorter than 16 and none otherwise; float32 order 3 within
1e-9 * max|input| in float64, or one float32 ulp."""
import ctypes
import os
import re

import numpy as np
import pytest

import zoom_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "volume_zoom.npz"))


@pytest.mark.parametrize("k", range(ref.GOLDEN_CASES))
def test_restatement_equals_golden(golden, k):
    ct, f32, seg = ref.case_inputs(k)
    assert np.array_equal(ct, golden["in_i16_%d" % k]) and np.array_equal(seg, golden["in_u8_%d" % k])
    z = ref.CASES[k][1]
    assert np.array_equal(ref.zoom(seg, z, order=0), golden["u8_o0_%d" % k])
    ref.check_i16(ref.zoom(ct, z, order=3), golden["i16_o3_%d" % k], ct, k)
    ref.check_f32(ref.zoom(f32, z, order=3), golden["f32_o3_%d" % k], f32, k)


@pytest.mark.parametrize("k", range(len(ref.CASES)))
def test_restatement_equals_live_scipy(k):
    ndimage = pytest.importorskip("scipy.ndimage")
    ct, f32, seg = ref.case_inputs(k)
    z = ref.CASES[k][1]
    assert np.array_equal(ref.zoom(seg, z, order=0), ndimage.zoom(seg, z, order=0))
    assert np.array_equal(ref.zoom(ct, z, order=0), ndimage.zoom(ct, z, order=0))
    ref.check_i16(ref.zoom(ct, z, order=3), ndimage.zoom(ct, z, order=3), ct, k)
    ref.check_f32(ref.zoom(f32, z, order=3), ndimage.zoom(f32, z, order=3), f32, k)


def test_shapes_round_half_to_even():
    assert [ref.out_shape((n, n, n), 0.5)[0] for n in (29, 30, 31)] == [14, 15, 16]
    assert ref.out_shape((9, 16, 16), (2.5, 1, 1)) == (22, 16, 16)


def test_overshoot_plane_is_zero(golden):
    """30 -> 15: j = 14 maps to 29.000000000000004 > 29, and scipy zeroes that plane; 224 voxels of case 2."""
    cc, zero = ref.coords(30, 15)
    assert zero.tolist() == [False] * 14 + [True] and cc[14] > 29
    want = golden["i16_o3_2"]
    assert (want[:, 14, :] == 0).all() and want[:, 14, :].size == 224
    assert (ref.zoom(ref.case_inputs(2)[0], 0.5)[:, 14, :] == 0).all()


def test_mirror_and_taps():
    assert ref.mirror(np.arange(-2, 7), 4).tolist() == [2, 1, 0, 1, 2, 3, 2, 1, 0]
    assert ref.mirror(np.arange(-1, 4), 2).tolist() == [1, 0, 1, 0, 1]
    assert ref.mirror(np.arange(-1, 3), 1).tolist() == [0, 0, 0, 0]
    w, idx, zero = ref.taps(7, 5)  # t = 0.5 at j = 1, 3
    assert np.abs(w.sum(-1) - 1).max() < 1e-15 and w[1].tolist() == [1 / 48, 23 / 48, 23 / 48, 1 / 48]
    assert idx[0].tolist() == [1, 0, 1, 2] and idx[4].tolist() == [5, 6, 5, 4] and not zero.any()


def test_integer_output_rounds_half_away_and_saturates():
    v = np.array([0.5, -0.5, 1.49999, -2.5, 40000.0, -40000.0, 0.0])
    assert ref.to_dtype(v, np.int16).tolist() == [1, -1, 1, -3, 32767, -32768, 0]
    assert ref.to_dtype(v, np.uint8).tolist() == [1, 0, 1, 0, 255, 0, 0]


def test_chains_on_the_restatement_equal_golden(golden):
    ct, seg = golden["chain_ct"], golden["chain_seg"]
    lo, hi = (int(v) for v in golden["chain_clip"])
    kw = dict(spacing_z=float(golden["chain_spacing_z"]), down_scale=float(golden["chain_down_scale"]), lower=lo, upper=hi)
    c, s = ref.resample_chain(ct, seg, **kw)
    assert np.array_equal(c, golden["down_ct"]) and np.array_equal(s, golden["down_seg"])
    c, s = ref.resample_chain(ct, seg, flip_y=True, crop=[tuple(r) for r in golden["chain_crop"].tolist()], **kw)
    assert np.array_equal(c, golden["crop_ct"]) and np.array_equal(s, golden["crop_seg"])


# ---- the C surface: fails before the feature exists ---------------------------------------------------------------------------------------

def _declared(hname):
    src = open(os.path.join(ROOT, "include", hname)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return set(re.findall(r"\b(ps_[a-z0-9_]+)\s*\(", src))


def test_prepare_header_matches_its_prototype_table():
    from point_unet_amd import _lib
    assert _declared("pointseg_prepare.h") == set(_lib.PREPARE_PROTOTYPES) == {"ps_volume_zoom"}
    assert not set(_lib.PREPARE_PROTOTYPES) & set(_lib.PROTOTYPES)
    hdr = open(os.path.join(ROOT, "include", "pointseg_prepare.h")).read()
    assert int(re.search(r"#define PS_VOLUME_U8 (\d+)", hdr).group(1)) == _lib.PS_VOLUME_U8
    assert _lib.PS_VOLUME_U8 not in (_lib.PS_VOLUME_I16, _lib.PS_VOLUME_F32)


def test_library_exports_the_symbol(lib):
    assert hasattr(lib, "ps_volume_zoom")
    assert lib.ps_volume_zoom.argtypes is not None and len(lib.ps_volume_zoom.argtypes) == 17


def test_argument_errors_need_no_gpu(lib):
    """Every argument error is found before any HIP call."""
    need = ctypes.c_int64(0)
    assert lib.ps_volume_zoom(None, None, 1, 4, 4, 4, 3, 2, 2, 2, 0, 0, 0.0, 0.0, None, None, ctypes.byref(need)) == 1
    assert b"NULL" in lib.ps_last_error()
