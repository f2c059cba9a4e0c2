"""The rules of include/pointseg_saliency_attention.h as far as they go without a GPU: the header, the prototype table and the library
agree; every argument error of the six calls is found before any HIP call, the context last; the size queries look at the shapes alone;
hand-derived cases pin the yardstick of test_gpu_saliency_train.py itself -- float64 autograd through saliency_train_ref; and
reference_optimizer is the reference's momentum rule with its regulariser."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import saliency_train_ref as tref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"ps_channel_attention", "ps_channel_attention_bwd", "ps_spatial_gate", "ps_spatial_gate_bwd", "ps_softmax_dice_loss", "ps_softmax_dice_loss_bwd"}
FAKE = ctypes.c_void_p(4096)  # non-NULL pointers no check dereferences: every case below fails (or ends) before the device is touched
OUT = ctypes.c_void_p(8192)
HEADERS = ("pointseg.h", "pointseg_train_ops.h", "pointseg_prepare.h", "pointseg_postprocess.h", "pointseg_saliency.h", "pointseg_saliency_train.h")


def _declared(hname):
    src = open(os.path.join(ROOT, "include", hname)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return set(re.findall(r"\b(ps_[a-z0-9_]+)\s*\(", src))


# ---- header, table, library ------------------------------------------------------------------------------------------------------------------

def test_header_table_and_library_agree(lib):
    from point_unet_amd import _lib
    assert _declared("pointseg_saliency_attention.h") == set(_lib.SALIENCY_ATTENTION_PROTOTYPES) == NAMES
    for table in (_lib.PROTOTYPES, _lib.PREPARE_PROTOTYPES, _lib.POSTPROCESS_PROTOTYPES, _lib.SALIENCY_PROTOTYPES, _lib.SALIENCY_TRAIN_PROTOTYPES):
        assert not NAMES & set(table)
    for h in HEADERS:
        assert not NAMES & _declared(h), h
    for name, (_, args) in _lib.SALIENCY_ATTENTION_PROTOTYPES.items():
        assert len(getattr(lib, name).argtypes) == len(args)
    src = open(os.path.join(ROOT, "include", "pointseg_saliency_attention.h")).read()
    assert '#include "pointseg_saliency.h"' in src
    for cite in ("attention.py:166-174", "attention.py:148-152", "model.py:295", "model.py:491-548, 592-618"):
        assert cite in src, cite


# ---- argument checks -------------------------------------------------------------------------------------------------------------------------

def _need(need):
    return ctypes.byref(need if need is not None else ctypes.c_int64(1 << 40))


def _ca(lib, need=None, **kw):
    a = dict(ctx=None, x=None, B=2, V=10, C=8, Ch=2, w1=None, b1=None, w2=None, b2=None, mean=None, hidden=None, scale=None, y=None, scratch=None)
    a.update(kw)
    return lib.ps_channel_attention(*a.values(), _need(need))


def _ca_bwd(lib, need=None, **kw):
    a = dict(ctx=None, x=None, dy=None, mean=None, hidden=None, scale=None, w1=None, w2=None, B=2, V=10, C=8, Ch=2, dx=None, dw1=None, db1=None, dw2=None,
             db2=None, scratch=None)
    a.update(kw)
    return lib.ps_channel_attention_bwd(*a.values(), _need(need))


def _gate(lib, **kw):
    a = dict(ctx=None, a1=None, a2=None, a3=None, f=None, B=2, V=10, C=8, sa=None, y=None)
    a.update(kw)
    return lib.ps_spatial_gate(*a.values())


def _gate_bwd(lib, **kw):
    a = dict(ctx=None, dy=None, f=None, sa=None, B=2, V=10, C=8, df=None, da=None)
    a.update(kw)
    return lib.ps_spatial_gate_bwd(*a.values())


def _loss(lib, need=None, **kw):
    a = dict(ctx=None, logits=None, labels=None, weight=None, B=2, V=10, C=2, loss=None, sums=None, scratch=None)
    a.update(kw)
    return lib.ps_softmax_dice_loss(*a.values(), _need(need))


def _loss_bwd(lib, **kw):
    a = dict(ctx=None, logits=None, labels=None, weight=None, sums=None, dloss=None, B=2, V=10, C=2, dlogits=None)
    a.update(kw)
    return lib.ps_softmax_dice_loss_bwd(*a.values())


BAD_CA = ((dict(B=0), b"B"), (dict(B=65536), b"B"), (dict(C=0), b"C"), (dict(C=1025), b"C"), (dict(Ch=0), b"Ch"), (dict(Ch=257), b"Ch"), (dict(V=0), b"V"),
          (dict(V=1 << 31), b"V"), (dict(V=1 << 28), b"V"))
BAD_GATE = ((dict(B=0), b"B"), (dict(C=0), b"C"), (dict(C=1025), b"C"), (dict(V=0), b"V"), (dict(V=1 << 31), b"V"), (dict(V=1 << 27), b"V"))
BAD_LOSS = ((dict(B=0), b"B"), (dict(C=1), b"C"), (dict(C=17), b"C"), (dict(V=0), b"V"), (dict(V=1 << 31), b"V"))


def test_channel_attention_argument_checks(lib):
    err = lib.ps_last_error
    ins = dict(x=FAKE, w1=FAKE, b1=FAKE, w2=FAKE, b2=FAKE)
    for call, who, full in ((_ca, b"ps_channel_attention", dict(ins, mean=OUT, hidden=OUT, scale=OUT, y=OUT)),
                            (_ca_bwd, b"ps_channel_attention_bwd", dict(x=FAKE, dy=FAKE, mean=FAKE, hidden=FAKE, scale=FAKE, w1=FAKE, w2=FAKE, dx=OUT))):
        for kw, word in BAD_CA:  # found in the sizing call and in the second one, whatever else is given
            assert call(lib, **kw) == 1 and who + b":" in err() and word in err(), kw
            assert call(lib, scratch=FAKE, ctx=FAKE, **dict(full, **kw)) == 1 and who + b":" in err() and word in err(), kw
        assert call(lib, scratch=FAKE) == 1 and who + b":" in err() and b"NULL" in err()  # NULL tensors on the second call
        assert call(lib, scratch=FAKE, **full) == 1 and who + b":" in err() and b"context" in err()  # everything given: the context is last
    assert lib.ps_channel_attention(None, None, 2, 10, 8, 2, *([None] * 9), None) == 1 and b"ps_channel_attention:" in err() and b"scratch_bytes" in err()
    assert lib.ps_channel_attention_bwd(*([None] * 8), 2, 10, 8, 2, *([None] * 6), None) == 1 and b"ps_channel_attention_bwd:" in err()
    # forward: every input and the three kept vectors are needed, y alone may be NULL
    for name in ins:
        assert _ca(lib, scratch=FAKE, **dict(ins, mean=OUT, hidden=OUT, scale=OUT, **{name: None})) == 1 and b"NULL x, w1" in err(), name
    for name in ("mean", "hidden", "scale"):
        assert _ca(lib, scratch=FAKE, **dict(ins, **{n: OUT for n in ("mean", "hidden", "scale") if n != name})) == 1 and b"only y may be NULL" in err(), name
    assert _ca(lib, scratch=FAKE, mean=OUT, hidden=OUT, scale=OUT, **ins) == 1 and b"context" in err()
    # backward: not every result NULL, each alone is legal, dx must not be x
    bins = dict(x=FAKE, dy=FAKE, mean=FAKE, hidden=FAKE, scale=FAKE, w1=FAKE, w2=FAKE)
    for name in bins:
        assert _ca_bwd(lib, scratch=FAKE, dx=OUT, **dict(bins, **{name: None})) == 1 and b"NULL x, dy" in err(), name
    assert _ca_bwd(lib, scratch=FAKE, **bins) == 1 and b"ps_channel_attention_bwd:" in err() and b"every result is NULL" in err()
    for name in ("dx", "dw1", "db1", "dw2", "db2"):
        assert _ca_bwd(lib, scratch=FAKE, **dict(bins, **{name: OUT})) == 1 and b"context" in err(), name
    assert _ca_bwd(lib, scratch=FAKE, dx=FAKE, **bins) == 1 and b"dx must not overlap x" in err()
    # the scratch: too small, misaligned (behind the context, which these get)
    assert _ca(lib, ctypes.c_int64(16), scratch=FAKE, ctx=FAKE, mean=OUT, hidden=OUT, scale=OUT, **ins) == 1 and b"this call needs" in err()
    assert _ca_bwd(lib, scratch=ctypes.c_void_p(4100), ctx=FAKE, dx=OUT, **bins) == 1 and b"256-byte aligned" in err()


def test_spatial_gate_argument_checks(lib):
    err = lib.ps_last_error
    fwd = dict(a1=FAKE, a2=FAKE, a3=FAKE, f=FAKE, sa=OUT, y=OUT)
    bwd = dict(dy=FAKE, f=FAKE, sa=FAKE)
    for call, who, full in ((_gate, b"ps_spatial_gate", fwd), (_gate_bwd, b"ps_spatial_gate_bwd", dict(bwd, df=OUT, da=OUT))):
        for kw, word in BAD_GATE:
            assert call(lib, **kw) == 1 and who + b":" in err() and word in err(), kw
            assert call(lib, ctx=FAKE, **dict(full, **kw)) == 1 and who + b":" in err() and word in err(), kw
        assert call(lib) == 1 and who + b":" in err() and b"NULL" in err()
        assert call(lib, **full) == 1 and who + b":" in err() and b"context" in err()
    for name in fwd:
        assert _gate(lib, ctx=FAKE, **dict(fwd, **{name: None})) == 1 and b"NULL a1" in err(), name
    for name in bwd:
        assert _gate_bwd(lib, ctx=FAKE, df=OUT, **dict(bwd, **{name: None})) == 1 and b"NULL dy" in err(), name
    assert _gate_bwd(lib, ctx=FAKE, **bwd) == 1 and b"every result is NULL" in err()
    assert _gate_bwd(lib, df=OUT, **bwd) == 1 and b"context" in err() and _gate_bwd(lib, da=OUT, **bwd) == 1 and b"context" in err()
    assert _gate_bwd(lib, ctx=FAKE, df=FAKE, **bwd) == 1 and b"df must not overlap f" in err()


def test_softmax_dice_loss_argument_checks(lib):
    err = lib.ps_last_error
    fwd = dict(logits=FAKE, labels=FAKE, loss=OUT, sums=OUT)
    bwd = dict(logits=FAKE, labels=FAKE, sums=FAKE, dlogits=OUT)
    for kw, word in BAD_LOSS:
        assert _loss(lib, **kw) == 1 and b"ps_softmax_dice_loss:" in err() and word in err(), kw
        assert _loss(lib, scratch=FAKE, ctx=FAKE, **dict(fwd, **kw)) == 1 and b"ps_softmax_dice_loss:" in err() and word in err(), kw
        assert _loss_bwd(lib, **kw) == 1 and b"ps_softmax_dice_loss_bwd:" in err() and word in err(), kw
        assert _loss_bwd(lib, ctx=FAKE, **dict(bwd, **kw)) == 1 and b"ps_softmax_dice_loss_bwd:" in err() and word in err(), kw
    assert lib.ps_softmax_dice_loss(None, None, None, None, 2, 10, 2, None, None, None, None) == 1 and b"ps_softmax_dice_loss:" in err()
    assert _loss(lib, scratch=FAKE) == 1 and b"ps_softmax_dice_loss:" in err() and b"NULL logits" in err()
    for name in ("logits", "labels"):
        assert _loss(lib, scratch=FAKE, ctx=FAKE, **dict(fwd, **{name: None})) == 1 and b"NULL logits" in err(), name
    for name in ("loss", "sums"):
        assert _loss(lib, scratch=FAKE, ctx=FAKE, **dict(fwd, **{name: None})) == 1 and b"NULL loss or sums" in err(), name
    assert _loss(lib, scratch=FAKE, **fwd) == 1 and b"ps_softmax_dice_loss:" in err() and b"context" in err()  # weight NULL is legal
    assert _loss(lib, scratch=FAKE, weight=FAKE, **fwd) == 1 and b"context" in err()
    assert _loss(lib, ctypes.c_int64(8), scratch=FAKE, ctx=FAKE, **fwd) == 1 and b"this call needs" in err()
    assert _loss_bwd(lib) == 1 and b"ps_softmax_dice_loss_bwd:" in err() and b"NULL logits" in err()
    for name in ("logits", "labels", "sums"):
        assert _loss_bwd(lib, ctx=FAKE, **dict(bwd, **{name: None})) == 1 and b"NULL logits" in err(), name
    assert _loss_bwd(lib, ctx=FAKE, **dict(bwd, dlogits=None)) == 1 and b"NULL dlogits" in err()
    assert _loss_bwd(lib, **bwd) == 1 and b"context" in err()  # weight and dloss NULL are legal
    assert _loss_bwd(lib, weight=FAKE, dloss=FAKE, **bwd) == 1 and b"context" in err()


def test_size_queries_look_at_the_shapes_alone(lib):
    def size(call, **kw):
        need = ctypes.c_int64(-1)
        assert call(lib, need, **kw) == 0, lib.ps_last_error()
        assert need.value > 0 and need.value % 256 == 0
        return need.value

    for call, ptrs in ((_ca, dict(x=FAKE, w1=FAKE, mean=OUT, y=OUT, ctx=FAKE)), (_ca_bwd, dict(x=FAKE, dy=FAKE, dx=FAKE, ctx=FAKE)),
                       (_loss, dict(logits=FAKE, weight=FAKE, loss=OUT, ctx=FAKE))):
        base = size(call)
        assert size(call, **ptrs) == base  # NULL scratch: the pointers and the context are not looked at
        assert size(call, B=3) >= base and size(call, V=5000) >= base
    pad = lambda n: -(-n // 256) * 256
    # the documented sizes; 5000 voxels are two slabs of 4096
    assert size(_ca, V=5000) == pad(2 * 2 * 8 * 8) + pad(2 * 8 * 8)
    assert size(_ca_bwd, V=5000) == pad(2 * 2 * 8 * 8) + 2 * pad(2 * 8 * 8) + pad(2 * 2 * 8) + pad(2 * 8 * 4)
    assert size(_loss, V=5000) == pad(2 * 2 * 2 * 24) and size(_loss, V=5000, C=16) == pad(2 * 2 * 16 * 24)
    assert size(_ca, V=4096, C=64) == size(_ca, V=1, C=64) < size(_ca, V=4097, C=64)


# ---- the yardstick: float64 autograd through saliency_train_ref on cases small enough to derive by hand ----------------------------------------

torch = pytest.importorskip("torch")
EPS = 1e-5


def _dice(logits, labels, weight):
    """(loss, dlogits) of the reference for nested lists: logits [B][V][C], labels [B][V], weight [B][V] or None."""
    z = torch.tensor(logits, dtype=torch.float64, requires_grad=True)
    w = None if weight is None else torch.tensor(weight, dtype=torch.float64)
    loss = tref.softmax_dice_loss(z, torch.tensor(labels), w)
    return loss.item(), torch.autograd.grad(loss, z)[0].tolist()


def _close(got, want, tol=1e-13):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape and float(np.abs(got - want).max()) <= tol, (got, want)


def test_yardstick_dice_one_voxel():
    """V = 1, C = 2, logits (0, 0), label 0, weight w: p = (1/2, 1/2).  Class 0: num = w, D0 = w / 4 + w + eps; class 1: num = 0,
    D1 = w / 4 + eps.  G_0 = -(1/2)(2 w / D0 - 2 w . w . (1/2) / D0^2), G_1 = -(1/2)(0 - 0) = 0;
    dlogits_0 = p0 (G_0 - p0 G_0) = G_0 / 4, dlogits_1 = p1 (0 - p0 G_0) = -G_0 / 4."""
    for w in (1.0, 3.0):
        D0 = w / 4 + w + EPS
        G0 = -0.5 * (2 * w / D0 - 2 * w * w * 0.5 / D0 ** 2)
        loss, dz = _dice([[[0.0, 0.0]]], [[0]], [[w]])
        _close(loss, 1 - 0.5 * (w / D0))
        _close(dz[0][0], [G0 / 4, -G0 / 4])


def test_yardstick_dice_zero_weight_voxel_counts_for_nothing():
    """V = 2, the second voxel with weight 0: the loss and the first voxel's gradient are the one-voxel case's, the second voxel's is 0."""
    D0 = 1.25 + EPS
    G0 = -0.5 * (2 / D0 - 1 / D0 ** 2)
    loss, dz = _dice([[[0.0, 0.0], [2.0, -1.0]]], [[0, 1]], [[1.0, 0.0]])
    _close(loss, 1 - 0.5 / D0)
    _close(dz[0][0], [G0 / 4, -G0 / 4])
    assert dz[0][1] == [0.0, 0.0]


def test_yardstick_dice_absent_class_and_out_of_range_label():
    """V = 2, C = 2, both voxels labelled 0, logits (0, 0), no weight: class 1's score is 0 / (1/2 + eps) = 0, class 0's 2 / (1/2 + 2 + eps).
    A label outside [0, C) takes part in sum p^2 alone: with labels (0, 7) class 0 has num = 1, D0 = 1/2 + 1 + eps."""
    loss, dz = _dice([[[0.0, 0.0], [0.0, 0.0]]], [[0, 0]], None)
    D0, D1 = 2.5 + EPS, 0.5 + EPS
    _close(loss, 1 - 0.5 * (2 / D0))
    # G_v0 = -(1/2)(2 / D0 - 2 . 2 . (1/2) / D0^2), G_v1 = -(1/2)(0 - 0): class 1 sends nothing although D1 is small
    G0 = -0.5 * (2 / D0 - 2 / D0 ** 2)
    _close(dz[0], [[G0 / 4, -G0 / 4]] * 2)
    assert D1 < 1
    loss, dz = _dice([[[0.0, 0.0], [0.0, 0.0]]], [[0, 7]], None)
    D0 = 1.5 + EPS
    _close(loss, 1 - 0.5 * (1 / D0))
    Ga, Gb = -0.5 * (2 / D0 - 2 * 1 * 0.5 / D0 ** 2), -0.5 * (0 - 2 * 1 * 0.5 / D0 ** 2)  # the labelled voxel; the out-of-range one
    _close(dz[0], [[Ga / 4, -Ga / 4], [Gb / 4, -Gb / 4]])


def test_yardstick_dice_all_weights_zero():
    """Every sum is 0: each score is 0 / eps = 0, the loss exactly 1, the gradient 0 -- finite."""
    loss, dz = _dice([[[0.3, -0.2], [1.0, 2.0]], [[0.0, 5.0], [-1.0, 1.0]]], [[0, 1], [1, 1]], [[0.0, 0.0], [0.0, 0.0]])
    assert loss == 1.0
    assert all(v == 0.0 for s in dz for r in s for v in r)


def test_yardstick_dice_batch_mean():
    """Two samples: the loss is the mean of the two one-sample losses, and a sample's gradient is half its one-sample gradient."""
    one = [[[0.5, -0.5], [1.0, 0.0]]], [[1, 0]], [[2.0, 0.5]]
    two = [[[-1.0, 0.25], [0.0, 0.0]]], [[0, 0]], [[1.0, 1.5]]
    (l1, d1), (l2, d2) = _dice(*one), _dice(*two)
    loss, dz = _dice(one[0] + two[0], one[1] + two[1], one[2] + two[2])
    _close(loss, (l1 + l2) / 2)
    _close(dz[0], [[v / 2 for v in r] for r in d1[0]])
    _close(dz[1], [[v / 2 for v in r] for r in d2[0]])


@pytest.mark.parametrize("b1, live", [(0.5, True), (-5.0, False)])
def test_yardstick_channel_attention_both_sides_of_the_relu(b1, live):
    """V = 2, C = 2, Ch = 1: dx = dy . s + dmean / V with dmean_c = w1_c . dz1, dz1 = [z1 > 0] . sum_c w2_c . ds_c s_c (1 - s_c),
    ds_c = sum_v dy_vc x_vc.  With b1 = -5 the hidden unit is off: dmean = 0 and s = sigmoid(b2)."""
    x, dy = [[1.0, 2.0], [3.0, -1.0]], [[0.5, -1.0], [2.0, 0.25]]
    w1, w2, b2 = [0.3, -0.2], [0.7, -0.4], [0.1, -0.3]
    mean = [(x[0][c] + x[1][c]) / 2 for c in range(2)]
    z1 = mean[0] * w1[0] + mean[1] * w1[1] + b1
    assert (z1 > 0) == live
    h = max(z1, 0.0)
    s = [1 / (1 + math.exp(-(h * w2[c] + b2[c]))) for c in range(2)]
    ds = [dy[0][c] * x[0][c] + dy[1][c] * x[1][c] for c in range(2)]
    dz1 = sum(w2[c] * ds[c] * s[c] * (1 - s[c]) for c in range(2)) if live else 0.0
    want = [[dy[v][c] * s[c] + w1[c] * dz1 / 2 for c in range(2)] for v in range(2)]
    t = lambda a: torch.tensor(a, dtype=torch.float64)
    xt = t([x]).requires_grad_()
    pre = []
    y = tref.channel_attention(xt, t(w1).reshape(2, 1), t([b1]), t(w2).reshape(1, 2), t(b2), pre=pre)
    _close(pre[0].item(), z1)
    _close(y[0].tolist(), [[x[v][c] * s[c] for c in range(2)] for v in range(2)])
    _close(torch.autograd.grad(y, xt, t([dy]))[0][0].tolist(), want)
    # the mask in place of the ReLU gives the same
    xm = t([x]).requires_grad_()
    ym = tref.channel_attention(xm, t(w1).reshape(2, 1), t([b1]), t(w2).reshape(1, 2), t(b2), mask=torch.tensor([[live]]))
    _close(torch.autograd.grad(ym, xm, t([dy]))[0][0].tolist(), want)


def test_yardstick_gate():
    """One voxel, two channels: sa = sigmoid(a1 + a2 + a3), y = f sa, df = dy sa, da = sa (1 - sa) (dy_0 f_0 + dy_1 f_1), the same for each branch."""
    a, f, dy = [0.4, -1.0, 0.25], [2.0, -3.0], [0.5, 1.5]
    sa = 1 / (1 + math.exp(-((a[0] + a[1]) + a[2])))
    t = lambda v: torch.tensor(v, dtype=torch.float64).requires_grad_()
    a1, a2, a3, ft = t([[a[0]]]), t([[a[1]]]), t([[a[2]]]), t([[f]])
    y = tref.spatial_gate(a1, a2, a3, ft)
    _close(y[0, 0].tolist(), [f[0] * sa, f[1] * sa])
    g = torch.autograd.grad(y, (a1, a2, a3, ft), torch.tensor([[dy]], dtype=torch.float64))
    da = sa * (1 - sa) * (dy[0] * f[0] + dy[1] * f[1])
    for gi in g[:3]:
        _close(gi.item(), da)
    _close(g[3][0, 0].tolist(), [dy[0] * sa, dy[1] * sa])


# ---- the optimiser ---------------------------------------------------------------------------------------------------------------------------

def test_reference_optimizer_is_momentum_with_decay_on_kernels_only():
    """Two steps against the hand formula of train.py:50-56, 102-107: g' = g + 1e-5 w for kernels (g' = g elsewhere),
    accum = 0.9 accum + g', w -= lr accum."""
    from point_unet_amd import saliency as sal
    S, CA = sal.SCOPE, sal.SCOPE + "C345_ChannelWiseAttention_withcpfe"
    names = [S + "init_conv/kernel", S + "init_conv/bias", S + "init_conv/ins_norm/gamma", S + "init_conv/ins_norm/beta", CA + "_dense_1/kernel",
             CA + "_dense_1/bias", CA + "_dense_2/kernel", CA + "_dense_2/bias"]
    assert set(names) <= set(sal.param_shapes(1))
    net = torch.nn.Module()
    gen = torch.Generator().manual_seed(3)
    for n in names:
        net.register_parameter(n, torch.nn.Parameter(torch.randn(5, generator=gen, dtype=torch.float64) * 100))
    opt = sal.reference_optimizer(net, lr=0.01)
    assert isinstance(opt, torch.optim.SGD) and all(g["momentum"] == 0.9 and g["lr"] == 0.01 for g in opt.param_groups)
    P = dict(net.named_parameters())
    w = {n: p.detach().clone() for n, p in P.items()}
    accum = {n: torch.zeros(5, dtype=torch.float64) for n in names}
    for step in range(2):
        for n in names:
            g = torch.randn(5, generator=gen, dtype=torch.float64)
            P[n].grad = g.clone()
            accum[n] = 0.9 * accum[n] + (g + (1e-5 * w[n] if n.endswith("/kernel") else 0.0))
            w[n] = w[n] - 0.01 * accum[n]
        opt.step()
        for n in names:
            assert torch.allclose(P[n].detach(), w[n], rtol=0, atol=1e-12), (step, n)
    # no decay off the kernels: with a zero gradient a bias, a gamma and a beta stand still, every kernel (both dense ones too) moves
    net2 = torch.nn.Module()
    for n in names:
        net2.register_parameter(n, torch.nn.Parameter(torch.full((3,), 100.0, dtype=torch.float64)))
    opt2 = sal.reference_optimizer(net2)
    for p in net2.parameters():
        p.grad = torch.zeros(3, dtype=torch.float64)
    opt2.step()
    for n, p in net2.named_parameters():
        if n.endswith("/kernel"):
            assert torch.allclose(p.detach(), torch.full((3,), 100.0 - 0.01 * 1e-5 * 100.0, dtype=torch.float64), rtol=0, atol=1e-12), n
        else:
            assert torch.equal(p.detach(), torch.full((3,), 100.0, dtype=torch.float64)), n


def test_python_surface_rejects_cpu_tensors():
    from point_unet_amd import saliency as sal
    x = torch.zeros((1, 4, 8))
    with pytest.raises(ValueError):
        sal.channel_attention(x, torch.zeros(8, 2), torch.zeros(2), torch.zeros(2, 8), torch.zeros(8))
    with pytest.raises(ValueError):
        sal.spatial_gate(torch.zeros(1, 4), torch.zeros(1, 4), torch.zeros(1, 4), x)
    with pytest.raises(ValueError):
        sal.softmax_dice_loss(x, torch.zeros((1, 4), dtype=torch.int32))
    for f in (sal.ChannelAttentionFunction, sal.SpatialGateFunction, sal.SoftmaxDiceLossFunction):
        assert issubclass(f, torch.autograd.Function)
    assert issubclass(sal.TrainableSaliencyNet, torch.nn.Module)
