"""include/pointseg_train_loss.h without a GPU: the header's closed form against autograd of the reference's expressions
(tests/point_loss_ref.py), hand-derived cases of the two Dice losses and of the accuracy rule, the header against its ctypes table and the
library's exports, the argument checks (all of them end before the device is touched), and the layout the issue fixed in advance: the two
pinned headers and the struct revision are the parent's, byte for byte."""
import ctypes
import hashlib
import os
import re

import numpy as np
import pytest

import point_loss_ref as pref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"ps_op_dice_sums", "ps_op_dice_from_sums", "ps_op_top1_counts", "ps_randla_backward_loss", "ps_randla_train_step_loss"}
FAKE = ctypes.c_void_p(4096)  # non-NULL pointers no check dereferences: every case below ends before the device is touched
PS_EINVAL = 1
# sha256 of the two headers tests/test_cabi.py pins, as the parent commit holds them
PINNED = {"pointseg.h": "c141a4b497c16f5efa72e84ab32e8dbf2ad129bf764a8b85599f5d069e2da829",
          "pointseg_train_ops.h": "232b96f46965d9629f04d5f9b7a2608e9f08139951609afd8b62dd4d69003e0d"}


def _case(R, C, ignored, seed):
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((R, C)).astype(np.float32)
    y = rng.integers(0, C, R).astype(np.int32)
    if ignored:
        y[rng.random(R) < 0.3] = -1
        y[0] = -1
    return z, y


# ---- the closed form is the gradient of the reference's expressions --------------------------------------------------------------------------

@pytest.mark.parametrize("kind", pref.KINDS)
@pytest.mark.parametrize("ignored", [False, True], ids=["all-valid", "ignored"])
@pytest.mark.parametrize("R,C", [(1, 2), (5, 4), (4097, 4), (70000, 13)])
def test_closed_form_equals_autograd_of_the_restatement(R, C, ignored, kind):
    z, y = _case(R, C, ignored, seed=R + C)
    cw = np.linspace(4.0, 1.0, C)
    for scale in (1.0, 2.0):
        want_loss, want_grad = pref.loss_and_grad(kind, z, y, cw, grad_scale=scale)
        loss, grad = pref.closed_form(kind, z, y, cw, grad_scale=scale)
        assert abs(loss - want_loss) <= 1e-12
        assert np.abs(grad - want_grad).max() <= 1e-12


# ---- hand-derived cases ---------------------------------------------------------------------------------------------------------------------------

def test_one_row():
    # z = (3, -1), y = 0: S0 = (3, 0), S1 = (9, 1), S2 = (1, 0); s_0 = 6 / (10 + 1e-5), s_1 = 0
    z, y = np.array([[3.0, -1.0]], np.float32), np.array([0], np.int32)
    D0, D1 = 10 + 1e-5, 1 + 1e-5
    s0 = 6 / D0
    loss, grad = pref.loss_and_grad("dice", z, y)
    assert abs(loss - (1 - s0 / 2)) <= 1e-15
    # a_c = 2 / (2 D_c), b_c = a_c s_c: d/dz_00 = b_0 3 - a_0, d/dz_01 = b_1 (-1) = 0
    assert np.abs(grad - np.array([[s0 / D0 * 3 - 1 / D0, 0.0]])).max() <= 1e-15
    assert np.array_equal(pref.sums_of(z, y), [3, 9, 1, 0, 1, 0, 1, 1])


def test_a_class_absent_scores_zero():
    z = np.array([[1.0, 2.0, 0.5], [0.25, -1.0, 4.0]], np.float32)
    y = np.array([0, 0], np.int32)
    loss, grad = pref.closed_form("dice", z, y)
    s0 = 2 * 1.25 / (1.0 + 0.0625 + 2 + 1e-5)
    assert abs(loss - (1 - s0 / 3)) <= 1e-15
    assert np.all(grad[:, 1:] == 0.0)  # b_c = a_c s_c = 0 and no row carries the class
    want = pref.loss_and_grad("dice", z, y)
    assert abs(loss - want[0]) <= 1e-15 and np.abs(grad - want[1]).max() <= 1e-15


@pytest.mark.parametrize("kind", pref.KINDS)
def test_everything_ignored(kind):
    z, y = np.ones((7, 4), np.float32), np.full(7, -1, np.int32)
    for loss, grad in (pref.closed_form(kind, z, y, pref.BRATS_WEIGHTS), pref.loss_and_grad(kind, z, y, pref.BRATS_WEIGHTS)):
        assert loss == 1.0 and np.all(grad == 0.0)
    assert pref.top1_counts(z, y) == (0, 0) and pref.accuracy(z, y) == 0.0


def test_an_out_of_range_label_is_an_ignored_row():
    z, y = _case(9, 4, False, seed=1)
    y2 = y.copy()
    y2[[2, 5]] = [4, -7]
    keep = np.ones(9, bool)
    keep[[2, 5]] = False
    loss, grad = pref.closed_form("dice_weighted", z, y2, pref.BRATS_WEIGHTS)
    want_loss, want_grad = pref.closed_form("dice_weighted", z[keep], y[keep], pref.BRATS_WEIGHTS)
    assert loss == want_loss and np.array_equal(grad[keep], want_grad) and np.all(grad[~keep] == 0.0)
    assert pref.top1_counts(z, y2) == pref.top1_counts(z[keep], y[keep])


def test_label_reduction_of_the_reference():
    # RandLANet.py:77-81 with ignored_label_inds = [0] and 4 classes: reducing_list = [0, 0, 1, 2, 3]; label 0 itself is an ignored row
    assert pref.reduce_labels([0, 1, 2, 3, 4, 5, -1], 4, [0]).tolist() == [-1, 0, 1, 2, 3, -1, -1]
    assert pref.reduce_labels([0, 1, 2, 3], 4, []).tolist() == [0, 1, 2, 3]


def test_top1_rule():
    z = np.array([[1.0, 1.0, 0.0],          # a tie with the target: correct, as in TensorFlow
                  [0.0, 2.0, 1.0],          # the target is the strict maximum
                  [0.0, 2.0, 3.0],          # a strictly larger class
                  [np.nan, 0.0, 0.0],       # a NaN target is never correct
                  [1.0, np.nan, 0.0],       # a NaN elsewhere is not larger
                  [np.inf, 0.0, 0.0],       # an infinite target is not finite
                  [5.0, 0.0, 0.0]], np.float32)  # ignored
    y = np.array([0, 1, 1, 0, 0, 0, -1], np.int32)
    assert pref.top1_counts(z, y) == (6, 3)
    assert pref.accuracy(z, y) == np.float32(3 / 6)


def test_brats_weights_reproduce_get_loss_dice_weight():
    import torch
    z, y = _case(200, 4, False, seed=5)
    zt, yt = torch.tensor(z, dtype=torch.float64), torch.tensor(y).long()
    # the function as the reference writes it, constant included
    one_hot = torch.nn.functional.one_hot(yt, 4).double()
    cw = torch.tensor([[4.0, 1.0, 1.0, 1.0]], dtype=torch.float64)
    num = 2.0 * (cw * one_hot * zt).sum(0)
    den = (cw * zt.square()).sum(0) + one_hot.sum(0)
    want = float(1 - (num / (den + 0.00001)).mean())
    assert abs(pref.closed_form("dice_weighted", z, y, [4, 1, 1, 1])[0] - want) <= 1e-15
    assert abs(float(pref.get_loss_dice_weight(zt, yt)) - want) == 0.0
    # and "dice" is the weights-of-one case
    assert abs(pref.closed_form("dice", z, y)[0] - pref.closed_form("dice_weighted", z, y, [1, 1, 1, 1])[0]) == 0.0


# ---- header, table, library ---------------------------------------------------------------------------------------------------------------------

def _declared(hname):
    src = open(os.path.join(ROOT, "include", hname)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return set(re.findall(r"\b(ps_[a-z0-9_]+)\s*\(", src))


def test_header_table_and_library_agree(lib):
    from point_unet_amd import _lib
    assert _declared("pointseg_train_loss.h") == set(_lib.TRAIN_LOSS_PROTOTYPES) == NAMES
    assert not NAMES & set(_lib.PROTOTYPES)
    for name, (_, args) in _lib.TRAIN_LOSS_PROTOTYPES.items():
        assert len(getattr(lib, name).argtypes) == len(args), name
    src = open(os.path.join(ROOT, "include", "pointseg_train_loss.h")).read()
    assert "enum { PS_LOSS_CE = 0, PS_LOSS_DICE = 1, PS_LOSS_DICE_WEIGHTED = 2 };" in src
    assert (_lib.PS_LOSS_CE, _lib.PS_LOSS_DICE, _lib.PS_LOSS_DICE_WEIGHTED) == (0, 1, 2)
    assert _lib.TRAIN_LOSSES == {"ce": 0, "dice": 1, "dice_weighted": 2}
    for cite in ("RandLANet.py:276-291", "RandLANet.py:293-312", "RandLANet.py:93-94", "NaN"):
        assert cite in src, cite


def test_the_pinned_layout_is_the_parents(lib):
    from point_unet_amd import _lib
    for hname, want in PINNED.items():
        got = hashlib.sha256(open(os.path.join(ROOT, "include", hname), "rb").read()).hexdigest()
        assert got == want, hname
    assert _lib.PS_ABI_VERSION == 7 and lib.ps_abi_version() == 7
    assert not NAMES & (_declared("pointseg.h") | _declared("pointseg_train_ops.h"))


# ---- argument checks: PS_EINVAL before anything is enqueued -------------------------------------------------------------------------------------

def _sums(lib, **kw):
    a = dict(ctx=FAKE, logits=FAKE, labels=FAKE, R=10, C=4, sums=FAKE)
    a.update(kw)
    return lib.ps_op_dice_sums(*a.values())


def _from_sums(lib, **kw):
    a = dict(ctx=FAKE, kind=1, logits=FAKE, labels=FAKE, cw=FAKE, sums=FAKE, scale=1.0, R=10, C=4, loss=FAKE, dlogits=FAKE)
    a.update(kw)
    return lib.ps_op_dice_from_sums(*a.values())


def _top1(lib, **kw):
    a = dict(ctx=FAKE, logits=FAKE, labels=FAKE, R=10, C=4, counts=FAKE)
    a.update(kw)
    return lib.ps_op_top1_counts(*a.values())


def test_op_argument_checks(lib):
    err = lib.ps_last_error
    for fn in (_sums, _from_sums):
        for bad in (dict(C=0), dict(C=17), dict(R=0), dict(R=1 << 31), dict(R=-1), dict(ctx=None), dict(logits=None), dict(labels=None)):
            assert fn(lib, **bad) == PS_EINVAL, (fn.__name__, bad)
    assert _sums(lib, sums=None) == PS_EINVAL
    assert _sums(lib, C=17) == PS_EINVAL and b"[1, 16]" in err()
    for kind in (3, -1, 0):  # (PS_LOSS_CE is not a Dice: ps_op_weighted_ce is its op)
        assert _from_sums(lib, kind=kind) == PS_EINVAL and b"kind" in err(), kind
    assert _from_sums(lib, sums=None) == PS_EINVAL
    assert _from_sums(lib, loss=None, dlogits=None) == PS_EINVAL and b"both NULL" in err()
    assert _from_sums(lib, kind=2, cw=None) == PS_EINVAL and b"class_weights" in err()
    for bad in (dict(C=0), dict(C=65), dict(R=0), dict(R=1 << 31), dict(ctx=None), dict(logits=None), dict(labels=None), dict(counts=None)):
        assert _top1(lib, **bad) == PS_EINVAL, bad


def test_step_argument_checks(lib):
    for fn in (lib.ps_randla_backward_loss, lib.ps_randla_train_step_loss):
        assert fn(None, None, FAKE, FAKE, FAKE, 0, FAKE, None, None) == PS_EINVAL and b"trainer is NULL" in lib.ps_last_error()


def test_trainer_rejects_an_unknown_loss_before_a_trainer_is_created():
    from point_unet_amd.train import Trainer, point_loss
    with pytest.raises(ValueError):
        Trainer(None, loss="softmax_dice")
    with pytest.raises(ValueError):
        point_loss(None, None, "generalised")
