"""include/pointseg_saliency_map.h without a GPU: the restated rule (saliency_map_ref.py) equals what the reference's own flip_lr,
transpose_volumes, overlapping_inference and segment_one_image gave (tests/golden/saliency_map_views.npz, make_saliency_map_golden.py);
the header's prototype is the ctypes table's; the library exports the entry, whose argument checks and sizing call touch no GPU."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import saliency_map_ref as mref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "saliency_map_views.npz")


def _model(window):
    """make_saliency_map_golden.py's model function: the probabilities depend on the voxel's value and on its place in the window."""
    _, p0, p1, p2, _ = window.shape
    i, j, k = np.meshgrid(np.arange(p0), np.arange(p1), np.arange(p2), indexing="ij")
    z = 1.3 * window[..., 0].astype(np.float64) + 0.013 * i - 0.007 * j + 0.003 * k + 0.0001 * i * k
    p = 1.0 / (1.0 + np.exp(-z))
    return np.stack([1.0 - p, p], -1)


@functools.lru_cache(maxsize=None)
def _case():
    g = np.load(GOLDEN)
    shape, patch, steps = (tuple(int(v) for v in g[k]) for k in ("shape", "patch", "steps"))
    vol = np.random.default_rng(int(g["seed"])).standard_normal(shape).astype(np.float32)[None]
    passes = {}
    for view in mref.VIEWS:
        m, count = mref.one_view(vol, _model, patch, steps, 2, view)
        assert count.shape == shape and count.min() >= 1
        passes[view, 0] = m
        passes[view, 1] = mref.flipped(vol, _model, patch, steps, 2, view)
    return g, vol, patch, steps, passes


def _at(g, m):
    p = g["positions"]
    return m[p[:, 0], p[:, 1], p[:, 2], 1]


def test_the_golden_case_has_seams_and_overhangs_in_every_view():
    g, vol, patch, steps, _ = _case()
    assert steps == (48, 118, 118)  # eval.py:108-109
    pos = g["positions"]
    assert 2000 <= len(pos) <= 5000 and len(np.unique(pos, axis=0)) == len(pos)
    D, H, W = vol.shape[1:]
    for corner in ((0, 0, 0), (D - 1, H - 1, W - 1), (0, H - 1, 0)):
        assert (pos == corner).all(1).any()
    for view in mref.VIEWS:
        n = mref.to_view(vol, view).shape[1:]
        origins = [mref.ref.window_origins(n[a], patch[a], steps[a]) for a in range(3)]
        assert sum(len(o) >= 2 for o in origins) >= 2
        assert any(o[-1] + patch[a] > n[a] for a, o in enumerate(origins) if len(o) >= 2)


@pytest.mark.parametrize("view", mref.VIEWS)
def test_restatement_equals_the_reference_per_view(view):
    g, _, _, _, passes = _case()
    assert np.abs(_at(g, passes[view, 0]) - g[view]).max() <= 1e-12
    both = (passes[view, 0] + passes[view, 1]) / 2.0
    assert np.abs(_at(g, both) - g[view + "_flip"]).max() <= 1e-12
    # what the golden can tell apart: the unflipped map, the flipped pass, and a pass that was not mirrored back
    assert np.abs(_at(g, passes[view, 1]) - g[view]).max() > 1e-3
    assert np.abs(_at(g, (passes[view, 0] + np.flip(passes[view, 1], 2)) / 2.0) - g[view + "_flip"]).max() > 1e-3
    assert np.abs(passes[view, 0].sum(-1) - 1.0).max() <= 1e-12


def test_restatement_equals_the_reference_fusion():
    g, vol, patch, steps, passes = _case()
    fused = [mref.fuse([passes[v, f] for v in mref.VIEWS]) for f in (0, 1)]
    assert np.abs(_at(g, fused[0]) - g["fused"]).max() <= 1e-12
    assert np.abs(_at(g, (fused[0] + fused[1]) / 2.0) - g["fused_flip"]).max() <= 1e-12
    # a view turned back the wrong way is seen (the coronal map through the sagittal permutation has another shape; swap two nets instead)
    wrong = mref.fuse([passes["axial", 0], passes["coronal", 0], passes["coronal", 0]])
    assert np.abs(_at(g, wrong) - g["fused"]).max() > 1e-3


def test_whole_rule_and_its_float32_fusion_on_a_small_case():
    """saliency_map (one function for the whole rule) against its own parts, and the float32-ordered fusion against the float64 one."""
    rng = np.random.default_rng(3)
    vol = rng.standard_normal((1, 13, 21, 18)).astype(np.float32)
    patch, steps = (8, 8, 8), (6, 5, 7)
    for views in (("axial",), ("sagittal",), ("coronal", "axial"), mref.VIEWS):
        for flip in (False, True):
            got = mref.saliency_map(vol, _model, patch, steps, 2, views, flip)
            parts = [mref.fuse([(mref.flipped(vol, _model, patch, steps, 2, v) if f else mref.one_view(vol, _model, patch, steps, 2, v)[0]) for v in views])
                     for f in ((0, 1) if flip else (0,))]
            want = (parts[0] + parts[1]) / 2.0 if flip else parts[0]
            assert got.shape == (13, 21, 18, 2) and np.array_equal(got, want)
            got32 = mref.saliency_map(vol, _model, patch, steps, 2, views, flip, f32=True)
            assert got32.dtype == np.float32 and np.abs(got32 - got).max() <= 4 * 2.0 ** -24
    # three views in float32: a correctly rounded division, which a multiplication by fl32(1/3) is not for every value
    x = np.float32(1.0) + np.arange(64, dtype=np.float32) * np.float32(2.0 ** -23)
    assert np.array_equal(mref.fuse32([x, 0 * x, 0 * x]), (x.astype(np.float64) / 3.0).astype(np.float32))
    assert not np.array_equal(x * np.float32(1.0 / 3.0), x / np.float32(3.0))
    # a step larger than the patch leaves holes, which give 0
    m, count = mref.one_view(vol, _model, (8, 8, 8), (10, 9, 8), 2, "sagittal")
    assert count.min() == 0 and (m[count == 0] == 0).all() and (m[count > 0].sum(-1) > 0.99).all()


# ---- the C surface ---------------------------------------------------------------------------------------------------------------------------------

def _header(hname="pointseg_saliency_map.h"):
    return open(os.path.join(ROOT, "include", hname)).read()


def _declared(hname):
    src = re.sub(r"/\*.*?\*/", "", _header(hname), flags=re.S)
    return set(re.findall(r"\b(ps_[a-z0-9_]+)\s*\(", src))


C_TYPES = {"ps_context*": ctypes.c_void_p, "const void*": ctypes.c_void_p, "void*": ctypes.c_void_p, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64,
           "const int32_t*": ctypes.POINTER(ctypes.c_int32), "const int64_t*": ctypes.POINTER(ctypes.c_int64), "int64_t*": ctypes.POINTER(ctypes.c_int64),
           "const void* const*": ctypes.POINTER(ctypes.c_void_p)}


def test_header_matches_its_prototype_table():
    from point_unet_amd import _lib
    assert _declared("pointseg_saliency_map.h") == set(_lib.SALIENCY_MAP_PROTOTYPES) == {"ps_saliency_map"}
    for other in ("pointseg.h", "pointseg_saliency.h", "pointseg_saliency_precision.h"):
        assert "ps_saliency_map" not in _declared(other)
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    ret, args = re.search(r"\b(int)\s+ps_saliency_map\s*\((.*?)\)\s*;", src, flags=re.S).groups()
    types = [C_TYPES[re.sub(r"\s*\b[A-Za-z_0-9]+$", "", a.strip())] for a in args.split(",")]
    res, want = _lib.SALIENCY_MAP_PROTOTYPES["ps_saliency_map"]
    assert res is ctypes.c_int and len(types) == len(want) == 20
    assert types == want
    assert re.search(r"PS_VIEW_AXIAL\s*=\s*0,\s*PS_VIEW_SAGITTAL\s*=\s*1,\s*PS_VIEW_CORONAL\s*=\s*2", src)
    assert re.search(r"PS_VOLUME_CDHW\s*=\s*0,\s*PS_VOLUME_DHWC\s*=\s*1", src)
    assert _lib.SALIENCY_VIEWS == {"axial": 0, "sagittal": 1, "coronal": 2} and (_lib.PS_VOLUME_CDHW, _lib.PS_VOLUME_DHWC) == (0, 1)


def test_library_exports_the_symbol(lib):
    from point_unet_amd import _lib
    for name, (_, args) in _lib.SALIENCY_MAP_PROTOTYPES.items():
        assert len(getattr(lib, name).argtypes) == len(args)


def _call(lib, need, **over):
    a = dict(ctx=None, volume=None, layout=0, C_in=1, D=23, H=40, W=50, K=2, n_views=1, views=(0,), weights=None, weight_count=None, patch=(16, 32, 32),
             step=(12, 24, 24), flip=0, batch=1, precision=0, out=None, scratch=None)
    a.update(over)
    if a["weight_count"] is None:
        a["weight_count"] = lib.ps_saliency_weight_count(1, 2)
    arr = lambda t, v: None if v is None else (t * len(v))(*v)
    return lib.ps_saliency_map(a["ctx"], a["volume"], a["layout"], a["C_in"], a["D"], a["H"], a["W"], a["K"], a["n_views"], arr(ctypes.c_int32, a["views"]),
                               a["weights"], a["weight_count"], arr(ctypes.c_int64, a["patch"]), arr(ctypes.c_int64, a["step"]), a["flip"], a["batch"],
                               a["precision"], a["out"], a["scratch"], need)


BAD = [("layout", dict(layout=2)), ("layout", dict(layout=-1)), ("n_views", dict(n_views=0)), ("n_views", dict(n_views=4, views=(0, 1, 2, 0))),
       ("views", dict(views=(3,))), ("views", dict(views=(-1,))), ("twice", dict(n_views=2, views=(1, 1))), ("twice", dict(n_views=3, views=(0, 2, 0))),
       ("flip", dict(flip=2)), ("flip", dict(flip=-1)), ("batch", dict(batch=0)), ("batch", dict(batch=9)), ("precision", dict(precision=3)),
       ("precision", dict(precision=-1)), ("multiple of 16", dict(patch=(16, 24, 32))), ("multiple of 16", dict(patch=(0, 32, 32))),
       ("at least 1", dict(step=(12, 0, 24))), ("C_in", dict(C_in=0)), ("C_in", dict(C_in=17)), ("num_classes", dict(K=1)), ("num_classes", dict(K=17)),
       ("weight_count", dict(weight_count=5)), ("2^31", dict(patch=(256, 256, 256))), ("2^31", dict(D=1 << 11, H=1 << 10, W=1 << 10)), ("volume", dict(D=0)),
       ("2^31", dict(step=(12, 24, (1 << 31) - 1))),
       ("NULL", dict(views=None)), ("NULL", dict(patch=None)), ("NULL", dict(step=None))]


@pytest.mark.parametrize("word, over", BAD)
def test_argument_errors_need_no_gpu(lib, word, over):
    """Every argument error, with a NULL context, in the call that sizes the scratch: PS_EINVAL, the size untouched."""
    need = ctypes.c_int64(-7)
    assert _call(lib, ctypes.byref(need), **over) == 1
    assert word.encode() in lib.ps_last_error(), lib.ps_last_error()
    assert need.value == -7


def test_sizing_call_counts_what_the_header_says(lib):
    assert _call(lib, None) == 1 and b"NULL" in lib.ps_last_error()
    # a NULL context is an error once there is a scratch to run on
    need = ctypes.c_int64(1 << 40)
    assert _call(lib, ctypes.byref(need), scratch=ctypes.c_void_p(256)) == 1 and b"NULL" in lib.ps_last_error()
    pad = lambda n: (n + 255) // 256 * 256
    n = lib.ps_saliency_weight_count(1, 2)
    for batch in (1, 3, 8):
        fwd = ctypes.c_int64(-1)
        assert lib.ps_saliency_forward(None, None, batch, 16, 32, 32, 1, 2, None, n, None, None, None, None, ctypes.byref(fwd)) == 0
        for n_views, views in ((1, (1,)), (2, (2, 0)), (3, (0, 1, 2))):
            for prec in (0, 1, 2):
                need = ctypes.c_int64(-1)
                assert _call(lib, ctypes.byref(need), n_views=n_views, views=views, batch=batch, precision=prec, flip=1) == 0, lib.ps_last_error()
                vox, win = 23 * 40 * 50, 16 * 32 * 32
                want = pad(vox * 2 * 4) * (2 if n_views > 1 else 1) + pad(vox * 4) + pad(batch * win * 4) + pad(batch * win * 2 * 4) + pad(fwd.value)
                assert need.value == want


def test_python_surface_refuses_bad_arguments():
    from point_unet_amd import saliency as sal

    class Net:  # (the checks below come before anything touches a device)
        in_channels, num_classes, _prec, precision = 1, 2, 0, "fp32"

    other = type("Other", (Net,), dict(num_classes=3))
    with pytest.raises(ValueError, match="direction"):
        sal.saliency_map(None, {"axial": Net()}, direction="sagittal")
    with pytest.raises(ValueError, match="views"):
        sal.saliency_map(None, Net(), direction="oblique")
    with pytest.raises(ValueError, match="views"):
        sal.saliency_map(None, {})
    with pytest.raises(ValueError, match="share"):
        sal.saliency_map(None, {"axial": Net(), "coronal": other()})
    with pytest.raises(ValueError, match="layout"):
        sal.saliency_map(None, Net(), layout="HWDC")


def test_documents_name_the_entry():
    assert re.search(r"ps_saliency_map", _header("pointseg_saliency.h"))
    hdr = _header()
    for cite in ("eval.py:103-193", "eval.py:254", "eval.py:355-411", "eval.py:461-463", "utils.py:15-28", "utils.py:80-104"):
        assert cite in hdr, cite
    for sentence in ("correctly rounded float32", "do not depend on `batch`", "No permuted or mirrored copy", "float32 where the reference's are float64"):
        assert sentence in hdr, sentence
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "ps_saliency_map" in readme and "pointseg_saliency_map.h" in readme
    assert "4.18" in open(os.path.join(ROOT, "DESIGN.md")).read()
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ("segment_one_image", "flip_lr", "transpose_volumes", "MULTI_VIEW"):
        assert name in integ, name
