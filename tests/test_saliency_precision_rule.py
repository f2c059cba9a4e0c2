"""include/pointseg_saliency_precision.h without a GPU: the restated rule (saliency_precision_ref.py) does what the header says, the
library exports the two entries, and their sizing call -- which touches no GPU -- gives ps_saliency_forward's size in every mode and
refuses a precision that does not exist."""
import ctypes
import os
import re

import numpy as np
import pytest

import saliency_precision_ref as pref
import saliency_ref as ref

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_split3_is_exact_and_its_pieces_are_bfloat16():
    rng = np.random.default_rng(0)
    x = np.concatenate([rng.standard_normal(4096) * 10.0 ** rng.integers(-20, 20, 4096), [0.0, -0.0, 1.0, -1.0, 3.4e38, 1.0 + 2.0 ** -23]]
                       ).astype(np.float32)
    p1, p2, p3 = pref.split3(x)
    for p in (p1, p2, p3):
        assert p.dtype == np.float32 and not (p.view(np.uint32) & 0xFFFF).any()  # a bfloat16: the low 16 bits are clear
        assert np.array_equal(pref.round_bf16(torch.from_numpy(p)).numpy(), p)
    s = p1.astype(np.float64) + p2.astype(np.float64) + p3.astype(np.float64)
    assert np.array_equal(s, x.astype(np.float64))
    assert np.array_equal((p1 + p2) + p3, x)  # also in float32, largest first
    # truncation, not rounding: 1 + 2^-8 + 2^-9 keeps 1 in the first piece
    p1, p2, p3 = pref.split3(np.float32(1.0 + 2.0 ** -8 + 2.0 ** -9))
    assert (p1, p2, p3) == (1.0, 2.0 ** -8 + 2.0 ** -9, 0.0)


def test_round_bf16_is_nearest_even():
    t = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, -(1.0 + 2.0 ** -9)], dtype=torch.float32)
    assert pref.round_bf16(t).tolist() == [1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7, -1.0]
    assert pref.round_bf16(t.double()).dtype == torch.float64


def test_rounded_convolution_differs_from_the_exact_one():
    g = torch.Generator().manual_seed(1)
    x, w, b = torch.randn((1, 5, 7, 9, 6), generator=g), torch.randn((3, 3, 3, 6, 10), generator=g) * 0.1, torch.randn(10, generator=g)
    exact = ref.conv3d_same(x.double(), w.double(), b.double())
    rounded = pref.conv3d_rounded(x, w, b)
    assert rounded.dtype == torch.float64 and rounded.shape == exact.shape
    d = float((rounded - exact).abs().max())
    assert 1e-4 < d < 1e-1
    # operands that are bfloat16 already: nothing to round
    xr, wr = pref.round_bf16(x), pref.round_bf16(w)
    assert torch.equal(pref.conv3d_rounded(xr, wr, b), ref.conv3d_same(xr.double(), wr.double(), b.double()))


def test_rounded_network_differs_from_the_exact_one():
    from point_unet_amd import saliency as sal
    params = sal.init_params(1, 2, seed=11)
    x = np.random.default_rng(12).standard_normal((1, 16, 16, 16, 1)).astype(np.float32)
    exact, rounded = ref.forward(params, x, torch.float64), pref.forward_rounded(params, x)
    assert rounded.shape == exact.shape == (1, 16, 16, 16, 2) and rounded.dtype == np.float64
    d = float(np.abs(rounded - exact).max())
    print("forward_rounded - forward on (16,16,16) x 1: %.3e (max |logit| %.2f)" % (d, np.abs(exact).max()))
    assert np.isfinite(rounded).all() and 1e-4 < d < 0.5 * float(np.abs(exact).max())


# ---- the C surface ---------------------------------------------------------------------------------------------------------------------------------

def _declared(hname):
    src = open(os.path.join(ROOT, "include", hname)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return set(re.findall(r"\b(ps_[a-z0-9_]+)\s*\(", src))


NAMES = {"ps_conv3d_prec", "ps_saliency_forward_prec"}


def test_header_matches_its_prototype_table():
    from point_unet_amd import _lib
    assert _declared("pointseg_saliency_precision.h") == set(_lib.SALIENCY_PRECISION_PROTOTYPES) == NAMES
    assert not NAMES & (_declared("pointseg_saliency.h") | _declared("pointseg.h") | _declared("pointseg_train_ops.h"))
    for new, old in (("ps_conv3d_prec", "ps_conv3d"), ("ps_saliency_forward_prec", "ps_saliency_forward")):
        assert _lib.SALIENCY_PRECISION_PROTOTYPES[new][1] == _lib.SALIENCY_PROTOTYPES[old][1] + [ctypes.c_int32]
    src = open(os.path.join(ROOT, "include", "pointseg_saliency_precision.h")).read()
    assert re.search(r"PS_PREC_FP32\s*=\s*0,\s*PS_PREC_BF16X3\s*=\s*1,\s*PS_PREC_BF16\s*=\s*2", src)
    assert (_lib.PS_PREC_FP32, _lib.PS_PREC_BF16X3, _lib.PS_PREC_BF16) == (0, 1, 2)
    assert _lib.SALIENCY_PRECISIONS == {"fp32": 0, "bf16x3": 1, "bf16": 2}


def test_library_exports_the_symbols(lib):
    from point_unet_amd import _lib
    for name, (_, args) in _lib.SALIENCY_PRECISION_PROTOTYPES.items():
        assert len(getattr(lib, name).argtypes) == len(args)


def test_sizing_call_is_the_same_in_every_mode_and_refuses_other_values(lib):
    err = lib.ps_last_error
    n = lib.ps_saliency_weight_count(1, 2)
    for B, shape in ((1, (16, 32, 32)), (2, (16, 32, 48)), (1, (64, 160, 160))):
        base = ctypes.c_int64(-1)
        assert lib.ps_saliency_forward(None, None, B, *shape, 1, 2, None, n, None, None, None, None, ctypes.byref(base)) == 0
        for prec in (0, 1, 2):
            need = ctypes.c_int64(-1)
            assert lib.ps_saliency_forward_prec(None, None, B, *shape, 1, 2, None, n, None, None, None, None, ctypes.byref(need), prec) == 0
            assert need.value == base.value > 0
    for prec in (3, -1):
        need = ctypes.c_int64(-7)
        assert lib.ps_saliency_forward_prec(None, None, 1, 16, 32, 32, 1, 2, None, n, None, None, None, None, ctypes.byref(need), prec) == 1  # PS_EINVAL
        assert b"precision" in err() and need.value == -7
    # the other checks are ps_saliency_forward's
    need = ctypes.c_int64(0)
    assert lib.ps_saliency_forward_prec(None, None, 1, 16, 24, 32, 1, 2, None, n, None, None, None, None, ctypes.byref(need), 2) == 1 and b"multiple of 16" in err()


def test_conv3d_prec_checks_its_arguments_before_any_hip_call(lib):
    err = lib.ps_last_error
    a = dict(ctx=None, x=None, x2=None, B=1, Ds=4, Hs=4, Ws=4, C1=4, C2=0, up=1, w=None, bias=None, kd=3, kh=3, kw=3, C_out=8, stride=1, dilation=1, y=None)
    for prec in (3, -1):
        assert lib.ps_conv3d_prec(*a.values(), prec) == 1 and b"precision" in err()
    for prec in (0, 1, 2):
        assert lib.ps_conv3d_prec(*a.values(), prec) == 1 and b"NULL" in err()
        assert lib.ps_conv3d_prec(*dict(a, kd=5).values(), prec) == 1 and b"kernel" in err()


def test_python_surface_refuses_an_unknown_precision():
    from point_unet_amd import saliency as sal
    params = sal.init_params(1, 2, seed=0)
    for bad in ("fp16", "BF16", 2, None):
        with pytest.raises(ValueError, match="precision"):
            sal.SaliencyNet(params, 1, 2, precision=bad)
        with pytest.raises(ValueError, match="precision"):
            sal.conv3d(None, None, precision=bad)
