"""include/pointseg_saliency_train_precision.h without a GPU: the restated rule (saliency_grad_precision_ref.py) does what the header says
on hand-written cases -- the stride's absent terms, the up-sampling's sum, the dilation's taps that never reach the input --, a rounded
gradient lies far enough from the exact one for the GPU test to tell "bf16" from a mode that silently ran fp32, and header, exported
symbols and ctypes table agree: the sizing call, which touches no GPU, gives the fp32 entries' size in every mode and refuses a precision
that does not exist."""
import ctypes
import os
import re

import numpy as np
import pytest

import saliency_grad_precision_ref as gref
import saliency_precision_ref as pref

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64


def _randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def _r(t):
    return pref.round_bf16(t).double().numpy()


# ---- the reference against hand-written cases ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("W", [5, 6])
def test_stride_2_on_an_odd_and_an_even_extent(W):
    """One axis, one channel, three taps: SAME padding puts one voxel in front of W = 5 and none in front of W = 6.  i = 2 o - pad + t, so
    an input voxel receives only the taps of its parity; the others are absent."""
    Wo, pad = 3, (1 if W == 5 else 0)
    dy, w, x = _randn((1, 1, 1, Wo, 1), 1), _randn((1, 1, 3, 1, 1), 2), _randn((1, 1, 1, W, 1), 3)
    dyr, wr, xr = _r(dy).reshape(Wo), _r(w).reshape(3), _r(x).reshape(W)
    dx, dw = np.zeros(W), np.zeros(3)
    for o in range(Wo):
        for t in range(3):
            i = 2 * o - pad + t
            if 0 <= i < W:
                dx[i] += dyr[o] * wr[t]
                dw[t] += xr[i] * dyr[o]
    got, none = gref.data_grad_rounded(dy, w, (1, 1, 1, W), stride=2)
    assert none is None and got.dtype == F64
    np.testing.assert_allclose(got.numpy().reshape(W), dx, rtol=0, atol=1e-14)
    np.testing.assert_allclose(gref.weight_grad_rounded(x, None, 1, dy, (1, 1, 3), stride=2).numpy().reshape(3), dw, rtol=0, atol=1e-14)
    if W == 6:  # no padding in front: tap 0 reaches only even voxels, and the last voxel (5 = 2 * 2 + 1) only tap 1
        assert dx[5] == dyr[2] * wr[1]


def test_upsampling_sums_the_virtual_voxels_and_the_concat_splits():
    """1 x 1 x 1 kernel behind a concat (1 + 1 channels) and up = 2: a source voxel's gradient is w[ci] times the sum of the rounded dy over
    its 8 virtual voxels; dw[ci] is the sum over all virtual voxels of the rounded source value times the rounded dy."""
    dy, w = _randn((1, 2, 4, 6, 1), 4), _randn((1, 1, 1, 2, 1), 5)
    x, x2 = _randn((1, 1, 2, 3, 1), 6), _randn((1, 1, 2, 3, 1), 7)
    dyr, wr = _r(dy)[0, ..., 0], _r(w).reshape(2)
    sums = dyr.reshape(1, 2, 2, 2, 3, 2).sum((1, 3, 5))
    dx, dx2 = gref.data_grad_rounded(dy, w, (1, 1, 2, 3), up=2, c1=1)
    np.testing.assert_allclose(dx.numpy()[0, ..., 0], wr[0] * sums, rtol=0, atol=1e-14)
    np.testing.assert_allclose(dx2.numpy()[0, ..., 0], wr[1] * sums, rtol=0, atol=1e-14)
    dw = gref.weight_grad_rounded(x, x2, 2, dy, (1, 1, 1)).numpy().reshape(2)
    np.testing.assert_allclose(dw, [(_r(x)[0, ..., 0] * sums).sum(), (_r(x2)[0, ..., 0] * sums).sum()], rtol=0, atol=1e-13)
    np.testing.assert_allclose(gref.bias_grad_rounded(dy).numpy(), [dyr.sum()], rtol=0, atol=1e-13)
    assert gref.bias_grad_rounded(dy, rounded=False).numpy()[0] == pytest.approx(float(dy.double().sum()), abs=1e-13)
    assert abs(float(gref.bias_grad_rounded(dy)[0]) - float(dy.double().sum())) > 1e-4  # the ROUNDED dy


def test_dilation_7_leaves_the_outer_taps_at_zero():
    """5 x 7 x 9 at dilation 7: the outer taps of the D (5) and H (7) axes never reach the input, their dw is exactly 0 and they send no
    gradient back; W = 9 is reached (0 + 7 < 9).  The centre line of taps is written out by hand."""
    x, dy, w = _randn((1, 5, 7, 9, 2), 8), _randn((1, 5, 7, 9, 3), 9), _randn((3, 3, 3, 2, 3), 10)
    dw = gref.weight_grad_rounded(x, None, 1, dy, (3, 3, 3), dilation=7).numpy()
    assert not dw[[0, 2]].any() and not dw[:, [0, 2]].any() and dw[1, 1].all()
    xr, dyr = _r(x)[0], _r(dy)[0]
    np.testing.assert_allclose(dw[1, 1, 1], np.einsum("dhwi,dhwo->io", xr, dyr), rtol=0, atol=1e-12)
    np.testing.assert_allclose(dw[1, 1, 0], np.einsum("dhwi,dhwo->io", xr[:, :, 0:2], dyr[:, :, 7:9]), rtol=0, atol=1e-12)  # in = o - 7
    np.testing.assert_allclose(dw[1, 1, 2], np.einsum("dhwi,dhwo->io", xr[:, :, 7:9], dyr[:, :, 0:2]), rtol=0, atol=1e-12)  # in = o + 7
    # the data gradient sees only the centre line: the outer kernel planes may hold anything
    w2 = w.clone()
    w2[[0, 2]] = 99.0
    w2[:, [0, 2]] = -99.0
    a, b = gref.data_grad_rounded(dy, w, (1, 5, 7, 9), dilation=7)[0], gref.data_grad_rounded(dy, w2, (1, 5, 7, 9), dilation=7)[0]
    assert torch.equal(a, b)
    wr = _r(w)
    want = np.einsum("dhwo,io->dhwi", dyr, wr[1, 1, 1])
    want[:, :, 0:2] += np.einsum("dhwo,io->dhwi", dyr[:, :, 7:9], wr[1, 1, 0])
    want[:, :, 7:9] += np.einsum("dhwo,io->dhwi", dyr[:, :, 0:2], wr[1, 1, 2])
    np.testing.assert_allclose(a.numpy()[0], want, rtol=0, atol=1e-12)


def test_unrounded_reference_is_plain_autograd():
    import saliency_ref as ref
    x, dy, w = _randn((2, 3, 4, 5, 3), 11), _randn((2, 2, 2, 3, 4), 12), _randn((3, 3, 3, 3, 4), 13)
    xl, wl = x.double().requires_grad_(), w.double().requires_grad_()
    gx, gw = torch.autograd.grad(ref.conv3d_same(xl, wl, None, 2, 1), [xl, wl], dy.double())
    assert torch.equal(gref.data_grad_rounded(dy, w, (2, 3, 4, 5), stride=2, rounded=False)[0], gx)
    assert torch.equal(gref.weight_grad_rounded(x, None, 1, dy, (3, 3, 3), stride=2, rounded=False), gw)
    assert gref.weight_grad_rounded(x, None, 1, dy, (3, 3, 3), stride=2, dtype=torch.float32).dtype == torch.float32


# ---- "bf16" is not silently fp32 ------------------------------------------------------------------------------------------------------------------

def _op_bar(want64, want32):
    """The project's op bar (_bar of test_gpu_saliency_grad.py): 4 x |torch-CPU float32 - float64 on the same operands| + 1e-6 max|expected|."""
    return 4.0 * float((want32.double() - want64).abs().max()) + 1e-6 * float(want64.abs().max())


def test_rounded_gradients_lie_more_than_100_bars_from_the_exact_ones():
    """5 x 7 x 9, 6 -> 10 channels, 3 x 3 x 3, standard-normal operands: the distance the GPU test asks of the "bf16" kernels, shown on the
    reference alone.  The bar is that of the ROUNDED operands, as the GPU test computes it."""
    x, dy, w = _randn((2, 5, 7, 9, 6), 14), _randn((2, 5, 7, 9, 10), 15), _randn((3, 3, 3, 6, 10), 16)
    cases = {
        "dx": lambda **kw: gref.data_grad_rounded(dy, w, (2, 5, 7, 9), **kw)[0],
        "dw": lambda **kw: gref.weight_grad_rounded(x, None, 1, dy, (3, 3, 3), **kw),
        "dbias": lambda **kw: gref.bias_grad_rounded(dy, **kw),
    }
    for name, fn in cases.items():
        round64, round32, exact64 = fn(), fn(dtype=torch.float32), fn(rounded=False)
        bar = _op_bar(round64, round32)
        off = float((round64 - exact64).abs().max())
        print("%s: rounded - exact %.3e, bar %.3e: %.0f bars" % (name, off, bar, off / bar))
        assert off > 100.0 * bar, name


# ---- the C surface -----------------------------------------------------------------------------------------------------------------------------------

def _declared(hname):
    src = open(os.path.join(ROOT, "include", hname)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return set(re.findall(r"\b(ps_[a-z0-9_]+)\s*\(", src))


NAMES = {"ps_conv3d_bwd_data_prec", "ps_conv3d_bwd_weight_prec"}
GEOMETRY = dict(B=2, Ds=5, Hs=7, Ws=9, C1=6, C2=3, up=2, kd=3, kh=3, kw=3, C_out=10, stride=1, dilation=1)


def test_header_matches_its_prototype_table():
    from point_unet_amd import _lib
    assert _declared("pointseg_saliency_train_precision.h") == set(_lib.SALIENCY_TRAIN_PRECISION_PROTOTYPES) == NAMES
    assert not NAMES & (_declared("pointseg_saliency_train.h") | _declared("pointseg_saliency_precision.h") | _declared("pointseg_saliency.h"))
    for new, old in (("ps_conv3d_bwd_data_prec", "ps_conv3d_bwd_data"), ("ps_conv3d_bwd_weight_prec", "ps_conv3d_bwd_weight")):
        assert _lib.SALIENCY_TRAIN_PRECISION_PROTOTYPES[new][1] == _lib.SALIENCY_TRAIN_PROTOTYPES[old][1] + [ctypes.c_int32]
    src = open(os.path.join(ROOT, "include", "pointseg_saliency_train_precision.h")).read()
    assert '#include "pointseg_saliency_precision.h"' in src and '#include "pointseg_saliency_train.h"' in src
    assert "pointseg_saliency_train_precision.h" in open(os.path.join(ROOT, "include", "pointseg_saliency_precision.h")).read()


def test_library_exports_the_symbols(lib):
    from point_unet_amd import _lib
    for name, (_, args) in _lib.SALIENCY_TRAIN_PRECISION_PROTOTYPES.items():
        assert len(getattr(lib, name).argtypes) == len(args)


def _calls(lib):
    """(new entry, old entry, the NULL arguments in front of and behind the geometry) of the two gradients."""
    return ((lib.ps_conv3d_bwd_data_prec, lib.ps_conv3d_bwd_data, (None,) * 3, (None,) * 3, b"ps_conv3d_bwd_data"),
            (lib.ps_conv3d_bwd_weight_prec, lib.ps_conv3d_bwd_weight, (None,) * 4, (None,) * 3, b"ps_conv3d_bwd_weight"))


def test_sizing_call_is_the_same_in_every_mode_and_refuses_other_values(lib):
    err = lib.ps_last_error
    for new, old, head, tail, who in _calls(lib):
        for geometry in (GEOMETRY, dict(GEOMETRY, up=1, stride=2, C2=0), dict(GEOMETRY, Ds=21, Hs=20, Ws=20, up=1)):
            base = ctypes.c_int64(-1)
            assert old(*head, *geometry.values(), *tail, ctypes.byref(base)) == 0
            for prec in (0, 1, 2):
                need = ctypes.c_int64(-1)
                assert new(*head, *geometry.values(), *tail, ctypes.byref(need), prec) == 0
                assert need.value == base.value > 0
        for prec in (3, -1):
            need = ctypes.c_int64(-7)
            assert new(*head, *GEOMETRY.values(), *tail, ctypes.byref(need), prec) == 1  # PS_EINVAL, also with scratch == NULL
            assert b"precision" in err() and who in err() and need.value == -7
            assert new(*head, *GEOMETRY.values(), None, None, ctypes.c_void_p(4096), ctypes.byref(need), prec) == 1 and b"precision" in err()


def test_prec_entries_check_their_arguments_before_any_hip_call(lib):
    err = lib.ps_last_error
    fake = ctypes.c_void_p(4096)
    for new, old, head, tail, who in _calls(lib):
        for prec in (0, 1, 2):
            need = ctypes.c_int64(1 << 40)
            assert new(*head, *dict(GEOMETRY, kd=5).values(), *tail, ctypes.byref(need), prec) == 1 and who in err() and b"kernel" in err()
            assert new(*head, *GEOMETRY.values(), None, None, fake, ctypes.byref(need), prec) == 1 and who in err() and b"NULL" in err()
            assert (who + b"_prec" in err()) == (prec != 0)  # PS_PREC_FP32 is the old entry, also by name


def test_python_surface_refuses_an_unknown_precision():
    from point_unet_amd import saliency as sal
    params = sal.init_params(1, 2, seed=0)
    for bad in ("fp16", "BF16", 2, None):
        with pytest.raises(ValueError, match="precision"):
            sal.TrainableSaliencyNet(params, 1, 2, precision=bad)
        with pytest.raises(ValueError, match="precision"):
            sal.conv3d_backward(None, None, None, precision=bad)
        with pytest.raises(ValueError, match="precision"):
            sal.differentiable_conv3d(None, None, precision=bad)
