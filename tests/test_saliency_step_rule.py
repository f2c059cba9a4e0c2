"""The rules of include/pointseg_saliency_step.h as far as they go without a GPU: the numpy restatement of the update
(saliency_step_ref.py) against a hand-derived case and against torch.optim.SGD in float64; the header, the prototype table and the library
agree; the decay segments follow the layer table; every argument error is found before any HIP call."""
import ctypes
import os
import re

import numpy as np
import pytest

import saliency_step_ref as sref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"ps_saliency_backward", "ps_saliency_sgd_update", "ps_saliency_train_step"}
FAKE = ctypes.c_void_p(4096)  # non-NULL pointers no check dereferences: every case below fails (or ends) before the device is touched
F = np.float32


def _declared(hname):
    src = open(os.path.join(ROOT, "include", hname)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return set(re.findall(r"\b(ps_[a-z0-9_]+)\s*\(", src))


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------------

def test_restatement_two_steps_by_hand():
    """Two elements, the first in a kernel: with lr 0.5, momentum 0.5, l2 0.25 and values that are exact in float32 every step can be
    written down.  Step 1 (accum 0): kernel g' = 1 + 0.25 * 4 = 2, accum 2, w = 4 - 1 = 3; bias g' = 1, accum 1, w = 4 - 0.5 = 3.5.
    Step 2 with grad_scale 0.5 on gradient 2: kernel g = 1, g' = 1 + 0.25 * 3 = 1.75, accum = 1 + 1.75 = 2.75, w = 3 - 1.375 = 1.625;
    bias g' = 1, accum = 0.5 + 1 = 1.5, w = 3.5 - 0.75 = 2.75."""
    decay = np.array([True, False])
    w, a = sref.sgd_update([4.0, 4.0], [1.0, 1.0], [0.0, 0.0], decay, 0.5, 0.5, 0.25)
    assert w.tolist() == [3.0, 3.5] and a.tolist() == [2.0, 1.0]
    w, a = sref.sgd_update(w, [2.0, 2.0], a, decay, 0.5, 0.5, 0.25, grad_scale=0.5)
    assert w.tolist() == [1.625, 2.75] and a.tolist() == [2.75, 1.5]


def test_restatement_rounds_every_operation_on_its_own():
    """momentum * accum + g with a fused multiply-add would keep the product's low bits: a case where that shows."""
    m, a, g = F(0.9), F(1.0000001), F(-0.9)
    w, acc = sref.sgd_update([0.0], [g], [a], np.array([False]), 1.0, m, 0.0)
    assert acc[0] == F(F(m * a) + g)
    assert float(acc[0]) != float(np.float64(m) * np.float64(a) + np.float64(g))  # the unrounded product differs


def test_restatement_against_torch_sgd_in_float64():
    torch = pytest.importorskip("torch")
    from point_unet_amd import saliency as sal
    shapes = sal.param_shapes(1, 2)
    decay = sref.decay_mask(shapes)
    rng = np.random.default_rng(5)
    n = decay.size
    w0 = rng.standard_normal(n).astype(F)
    wk, wr = torch.from_numpy(w0[decay]).double().requires_grad_(), torch.from_numpy(w0[~decay]).double().requires_grad_()
    opt = torch.optim.SGD([{"params": [wk], "weight_decay": 1e-5}, {"params": [wr], "weight_decay": 0.0}], lr=0.01, momentum=0.9)
    w, a = w0, np.zeros(n, F)
    for _ in range(3):
        g = rng.standard_normal(n).astype(F)
        wk.grad, wr.grad = torch.from_numpy(g[decay]).double(), torch.from_numpy(g[~decay]).double()
        opt.step()
        w, a = sref.sgd_update(w, g, a, decay, 0.01)
    want = np.empty(n)
    want[decay], want[~decay] = wk.detach().numpy(), wr.detach().numpy()
    assert float(np.abs(w - want).max()) <= 1e-6 * float(np.abs(want).max())


# ---- header, table, library --------------------------------------------------------------------------------------------------------------------

def test_header_table_and_library_agree(lib):
    from point_unet_amd import _lib
    assert _declared("pointseg_saliency_step.h") == set(_lib.SALIENCY_STEP_PROTOTYPES) == NAMES
    for table in (_lib.PROTOTYPES, _lib.PREPARE_PROTOTYPES, _lib.POSTPROCESS_PROTOTYPES, _lib.SALIENCY_PROTOTYPES, _lib.SALIENCY_TRAIN_PROTOTYPES,
                  _lib.SALIENCY_ATTENTION_PROTOTYPES, _lib.SALIENCY_DATA_PROTOTYPES):
        assert not NAMES & set(table)
    for name, (_, args) in _lib.SALIENCY_STEP_PROTOTYPES.items():
        assert len(getattr(lib, name).argtypes) == len(args)
    src = open(os.path.join(ROOT, "include", "pointseg_saliency_step.h")).read()
    assert '#include "pointseg.h"' in src and "typedef int (*ps_allreduce_fn)" not in src  # pointseg.h's typedef, not a second one
    for cite in ("train.py:50-56, 83-110", "model.py:176-314, 491-548, 592-618"):
        assert cite in src, cite
    mk = open(os.path.join(ROOT, "point-unet_amd", "csrc", "Makefile")).read()
    assert "saliency_step.hip" in mk and "pointseg_saliency_step.h" in mk
    assert _lib.PS_ABI_VERSION == 7 and lib.ps_abi_version() == 7


@pytest.mark.parametrize("cin, classes", [(1, 2), (4, 4), (3, 3)])
def test_decay_segments_are_the_kernels(cin, classes):
    """The layer table gives the segments; they are the tensors whose name ends in /kernel, the two dense kernels included."""
    from point_unet_amd import saliency as sal
    shapes = sal.param_shapes(cin, classes)
    segments, off = [], 0
    for name, shape, bias, norm in sal.layer_table(cin, classes):
        n = int(np.prod(shape))
        segments.append((off, off + n))
        off += n + shape[-1] * (int(bias) + 2 * int(norm))
    mask = np.zeros(off, bool)
    for a, b in segments:
        mask[a:b] = True
    assert np.array_equal(mask, sref.decay_mask(shapes))
    names = [n for n in shapes if n.endswith("/kernel")]
    assert len(names) == len(segments) == 44 and sum(1 for n in names if "_dense_" in n) == 2


# ---- argument checks ---------------------------------------------------------------------------------------------------------------------------

def _count(lib, cin=1, classes=2):
    return lib.ps_saliency_weight_count(cin, classes)


def _backward(lib, need=None, **kw):
    a = dict(ctx=None, x=None, labels=None, weight=None, B=1, D=16, H=16, W=16, C_in=1, K=2, weights=None, count=_count(lib), grads=None, loss=None, logits=None,
             scratch=None)
    a.update(kw)
    return lib.ps_saliency_backward(*a.values(), ctypes.byref(need if need is not None else ctypes.c_int64(1 << 50)))


def _step(lib, need=None, **kw):
    a = dict(ctx=None, x=None, labels=None, weight=None, B=1, D=16, H=16, W=16, C_in=1, K=2, params=None, count=_count(lib), grads=None, accum=None, lr=0.01,
             options=None, loss=None, logits=None, scratch=None)
    a.update(kw)
    return lib.ps_saliency_train_step(*a.values(), ctypes.byref(need if need is not None else ctypes.c_int64(1 << 50)))


def _update(lib, **kw):
    a = dict(ctx=None, params=None, grads=None, accum=None, C_in=1, K=2, count=_count(lib), lr=0.01, momentum=0.9, l2=1e-5, grad_scale=1.0)
    a.update(kw)
    return lib.ps_saliency_sgd_update(*a.values())


BAD_SHAPES = ((dict(D=24), b"multiple of 16"), (dict(H=8), b"multiple of 16"), (dict(W=0), b"multiple of 16"), (dict(B=0), b"B"), (dict(C_in=0), b"C_in"),
              (dict(C_in=17), b"C_in"), (dict(K=1), b"num_classes"), (dict(K=17), b"num_classes"), (dict(count=5), b"weight_count"),
              (dict(B=8, D=256, H=256, W=256), b"2^31"))


def test_backward_and_step_argument_checks(lib):
    err = lib.ps_last_error
    n = _count(lib)
    far = lambda k: ctypes.c_void_p(1 << 20 | (k * 64 << 20))  # buffers that do not overlap
    for call, who, full in ((_backward, b"ps_saliency_backward", dict(x=FAKE, labels=FAKE, weights=far(1), grads=far(2), loss=FAKE)),
                            (_step, b"ps_saliency_train_step", dict(x=FAKE, labels=FAKE, params=far(1), grads=far(2), accum=far(3), loss=FAKE))):
        for kw, word in BAD_SHAPES:  # in the sizing call and in the second one, whatever else is given
            assert call(lib, **kw) == 1 and who + b":" in err() and word in err(), kw
            assert call(lib, scratch=FAKE, ctx=FAKE, **dict(full, **kw)) == 1 and who + b":" in err() and word in err(), kw
        assert call(lib, scratch=FAKE) == 1 and who + b":" in err() and b"NULL" in err()  # a scratch and no context
        for name in full:  # each needed pointer
            assert call(lib, scratch=FAKE, ctx=FAKE, **dict(full, **{name: None})) == 1 and who + b":" in err() and b"NULL" in err(), name
        assert call(lib, ctypes.c_int64(256), scratch=FAKE, ctx=FAKE, **full) == 1 and b"this call needs" in err()
        assert call(lib, scratch=ctypes.c_void_p(4100), ctx=FAKE, **full) == 1 and b"256-byte aligned" in err()
    where = far(1).value
    assert _backward(lib, scratch=FAKE, ctx=FAKE, x=FAKE, labels=FAKE, loss=FAKE, weights=far(1), grads=ctypes.c_void_p(where + 4 * n - 4)) == 1 \
        and b"grads must not overlap weights" in err()
    assert _step(lib, scratch=FAKE, ctx=FAKE, x=FAKE, labels=FAKE, loss=FAKE, params=far(1), grads=far(1), accum=far(3)) == 1 and b"must not overlap" in err()
    assert lib.ps_saliency_backward(*([None] * 4), 1, 16, 16, 16, 1, 2, None, n, *([None] * 5)) == 1 and b"ps_saliency_backward:" in err()
    # the options: a world of several ranks needs its callback
    from point_unet_amd import _lib
    opt = _lib.PsSaliencyStepOptions(_lib.PS_ALLREDUCE_FN(), None, 2, 0.9, 1e-5)
    assert _step(lib, options=ctypes.byref(opt)) == 1 and b"needs an all-reduce callback" in err()
    opt.world_size = 0
    assert _step(lib, options=ctypes.byref(opt)) == 1 and b"world_size" in err()


def test_update_argument_checks(lib):
    err = lib.ps_last_error
    far = lambda k: ctypes.c_void_p(1 << 20 | (k * 64 << 20))
    full = dict(params=far(1), grads=far(2), accum=far(3))
    for kw, word in ((dict(C_in=0), b"C_in"), (dict(K=17), b"num_classes"), (dict(count=7), b"weight_count")):
        assert _update(lib, ctx=FAKE, **dict(full, **kw)) == 1 and b"ps_saliency_sgd_update:" in err() and word in err(), kw
    for name in full:
        assert _update(lib, ctx=FAKE, **dict(full, **{name: None})) == 1 and b"NULL params" in err(), name
    assert _update(lib, ctx=FAKE, **dict(full, accum=far(2))) == 1 and b"must not overlap" in err()
    assert _update(lib, **full) == 1 and b"context" in err()  # everything given: the context is last


def test_size_query_looks_at_the_shapes_alone(lib):
    def size(call, **kw):
        need = ctypes.c_int64(-1)
        assert call(lib, need, **kw) == 0, lib.ps_last_error()
        assert need.value > 0 and need.value % 256 == 0
        return need.value

    base = size(_backward)
    assert size(_backward, x=FAKE, weights=FAKE, grads=FAKE, ctx=FAKE) == base == size(_step) == size(_step, params=FAKE, ctx=FAKE)
    assert size(_backward, B=2) > base and size(_backward, D=32) > base
    c4 = _count(lib, 4, 4)
    assert size(_backward, C_in=4, K=4, count=c4) > base
