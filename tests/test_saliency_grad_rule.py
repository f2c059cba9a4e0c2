"""The rules of include/pointseg_saliency_train.h as far as they go without a GPU: the header, the prototype table and the library
agree; every argument error is found before any HIP call; the size query looks at the shapes alone; and hand-derived cases pin the
yardstick of test_gpu_saliency_grad.py itself -- float64 autograd through saliency_ref."""
import ctypes
import os
import re

import pytest

import saliency_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"ps_conv3d_bwd_data", "ps_conv3d_bwd_weight", "ps_instance_norm_relu_bwd"}
FAKE = ctypes.c_void_p(4096)  # non-NULL pointers no check dereferences: every case below fails (or ends) before the device is touched
OUT = ctypes.c_void_p(8192)


def _declared(hname):
    src = open(os.path.join(ROOT, "include", hname)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return set(re.findall(r"\b(ps_[a-z0-9_]+)\s*\(", src))


# ---- header, table, library ------------------------------------------------------------------------------------------------------------------

def test_header_table_and_library_agree(lib):
    from point_unet_amd import _lib
    assert _declared("pointseg_saliency_train.h") == set(_lib.SALIENCY_TRAIN_PROTOTYPES) == NAMES
    assert not NAMES & (set(_lib.PROTOTYPES) | set(_lib.PREPARE_PROTOTYPES) | set(_lib.POSTPROCESS_PROTOTYPES) | set(_lib.SALIENCY_PROTOTYPES))
    for name, (_, args) in _lib.SALIENCY_TRAIN_PROTOTYPES.items():
        assert len(getattr(lib, name).argtypes) == len(args)
    src = open(os.path.join(ROOT, "include", "pointseg_saliency_train.h")).read()
    assert '#include "pointseg_saliency.h"' in src


# ---- argument checks -------------------------------------------------------------------------------------------------------------------------

def _data(lib, need=None, **kw):
    a = dict(ctx=None, dy=None, w=None, B=1, Ds=4, Hs=4, Ws=4, C1=4, C2=0, up=1, kd=3, kh=3, kw=3, C_out=8, stride=1, dilation=1, dx=None, dx2=None,
             scratch=None)
    a.update(kw)
    return lib.ps_conv3d_bwd_data(*a.values(), ctypes.byref(need if need is not None else ctypes.c_int64(1 << 40)))


def _weight(lib, need=None, **kw):
    a = dict(ctx=None, x=None, x2=None, dy=None, B=1, Ds=4, Hs=4, Ws=4, C1=4, C2=0, up=1, kd=3, kh=3, kw=3, C_out=8, stride=1, dilation=1, dw=None, dbias=None,
             scratch=None)
    a.update(kw)
    return lib.ps_conv3d_bwd_weight(*a.values(), ctypes.byref(need if need is not None else ctypes.c_int64(1 << 40)))


def _norm(lib, need=None, **kw):
    a = dict(ctx=None, x=None, y=None, dy=None, B=2, V=10, C=3, gamma=None, eps=1e-5, dx=None, dgamma=None, dbeta=None, scratch=None)
    a.update(kw)
    return lib.ps_instance_norm_relu_bwd(*a.values(), ctypes.byref(need if need is not None else ctypes.c_int64(1 << 40)))


BAD_GEOMETRY = ((dict(kd=5), b"kernel"), (dict(kw=2), b"kernel"), (dict(stride=3), b"stride"), (dict(stride=0), b"stride"), (dict(dilation=2), b"dilation"),
                (dict(up=0), b"up"), (dict(up=9), b"up"), (dict(C1=385), b"C1"), (dict(C1=300, C2=100), b"C1"), (dict(C_out=257), b"C_out"),
                (dict(C_out=0), b"C_out"), (dict(Ds=0), b"input"), (dict(Ds=1 << 12, Hs=1 << 12, Ws=1 << 12), b"input"), (dict(B=0), b"B"))


def test_conv_gradient_argument_checks(lib):
    err = lib.ps_last_error
    for call, who in ((_data, b"ps_conv3d_bwd_data"), (_weight, b"ps_conv3d_bwd_weight")):
        for kw, word in BAD_GEOMETRY:  # found in the sizing call and in the second one
            assert call(lib, **kw) == 1 and who in err() and word in err(), kw
            assert call(lib, scratch=FAKE, **kw) == 1 and who in err() and word in err(), kw
        assert call(lib, scratch=FAKE) == 1 and who in err() and b"NULL" in err()  # NULL tensors on the second call
    assert lib.ps_conv3d_bwd_data(None, None, None, 1, 4, 4, 4, 4, 0, 1, 3, 3, 3, 8, 1, 1, None, None, None, None) == 1 and b"ps_conv3d_bwd_data" in err()
    assert lib.ps_conv3d_bwd_weight(None, None, None, None, 1, 4, 4, 4, 4, 0, 1, 3, 3, 3, 8, 1, 1, None, None, None, None) == 1 and b"ps_conv3d_bwd_weight" in err()
    # data gradient: dx2 exactly with C2 > 0, not every result NULL, and only then the context
    assert _data(lib, scratch=FAKE, dy=FAKE, w=FAKE, dx=OUT, dx2=OUT) == 1 and b"ps_conv3d_bwd_data" in err() and b"dx2" in err()
    assert _data(lib, scratch=FAKE, dy=FAKE, w=FAKE) == 1 and b"ps_conv3d_bwd_data" in err() and b"every result is NULL" in err()
    assert _data(lib, scratch=FAKE, dy=FAKE, w=FAKE, C2=3) == 1 and b"every result is NULL" in err()
    assert _data(lib, scratch=FAKE, dy=FAKE, w=FAKE, C2=3, dx2=OUT) == 1 and b"context" in err()  # dx alone NULL is legal
    assert _data(lib, scratch=FAKE, dy=FAKE, w=FAKE, dx=OUT) == 1 and b"ps_conv3d_bwd_data" in err() and b"context" in err()
    assert _data(lib, scratch=FAKE, dy=FAKE, w=FAKE, dx=FAKE) == 1 and b"overlap" in err()
    # weight gradient: x2 exactly with C2 > 0
    assert _weight(lib, scratch=FAKE, x=FAKE, dy=FAKE, dw=FAKE, C2=4) == 1 and b"ps_conv3d_bwd_weight" in err() and b"x2" in err()
    assert _weight(lib, scratch=FAKE, x=FAKE, x2=FAKE, dy=FAKE, dw=FAKE) == 1 and b"ps_conv3d_bwd_weight" in err() and b"x2" in err()
    assert _weight(lib, scratch=FAKE, x=FAKE, dy=FAKE) == 1 and b"ps_conv3d_bwd_weight" in err() and b"every result is NULL" in err()
    assert _weight(lib, scratch=FAKE, x=FAKE, dy=FAKE, dbias=FAKE) == 1 and b"ps_conv3d_bwd_weight" in err() and b"context" in err()


def test_norm_gradient_argument_checks(lib):
    err = lib.ps_last_error
    who = b"ps_instance_norm_relu_bwd"
    for kw, word in ((dict(V=0), b"V"), (dict(B=0), b"B"), (dict(C=1025), b"C"), (dict(C=0), b"C"), (dict(eps=0.0), b"eps"), (dict(V=1 << 31), b"V")):
        assert _norm(lib, **kw) == 1 and who in err() and word in err(), kw
    assert lib.ps_instance_norm_relu_bwd(None, None, None, None, 2, 10, 3, None, 1e-5, None, None, None, None, None) == 1 and who in err() and b"NULL" in err()
    assert _norm(lib, scratch=FAKE) == 1 and who in err() and b"NULL" in err()
    assert _norm(lib, scratch=FAKE, x=FAKE, y=FAKE, dy=FAKE) == 1 and who in err() and b"NULL" in err()  # gamma
    assert _norm(lib, scratch=FAKE, x=FAKE, y=FAKE, dy=FAKE, gamma=FAKE) == 1 and who in err() and b"every result is NULL" in err()
    assert _norm(lib, scratch=FAKE, x=FAKE, y=FAKE, dy=FAKE, gamma=FAKE, dx=FAKE) == 1 and who in err() and b"dx must not overlap" in err()
    assert _norm(lib, scratch=FAKE, x=FAKE, y=FAKE, dy=FAKE, gamma=FAKE, dbeta=FAKE) == 1 and who in err() and b"context" in err()


def test_size_queries_look_at_the_shapes_alone(lib):
    def size(call, **kw):
        need = ctypes.c_int64(-1)
        assert call(lib, need, **kw) == 0, lib.ps_last_error()
        assert need.value > 0 and need.value % 256 == 0
        return need.value

    for call, ptrs in ((_data, dict(dy=FAKE, w=FAKE, dx=FAKE, ctx=FAKE)), (_weight, dict(x=FAKE, dy=FAKE, dw=FAKE, dbias=FAKE, ctx=FAKE)),
                       (_norm, dict(x=FAKE, y=FAKE, dy=FAKE, gamma=FAKE, dx=FAKE, dgamma=FAKE, ctx=FAKE))):
        base = size(call)
        assert size(call, **ptrs) == base  # NULL scratch: the pointers and the context are not looked at
        assert size(call, B=3) >= base
    for call in (_data, _weight):
        base = size(call, up=2, C2=3)
        assert size(call, up=2, C2=3, Ds=9) >= base and size(call, up=2, C2=3, Hs=40, Ws=40) >= base and size(call, up=2, C2=3, B=7) >= base
    # the documented sizes
    pad = lambda n: -(-n // 256) * 256
    assert size(_data) == pad(27 * 4 * 8 * 4) and size(_data, up=2, B=3) == pad(27 * 4 * 8 * 4) + pad(3 * 512 * 4 * 4)
    assert size(_weight, Ds=17, Hs=16, Ws=16, B=2) == pad(2 * 2 * (27 * 4 + 1) * 8 * 4)  # 4352 output voxels: two slabs of 4096 per sample
    assert size(_norm, V=5000) == pad(2 * 2 * 3 * 16) + 3 * pad(2 * 3 * 16)
    assert size(_norm, V=5000) <= size(_norm, V=9000) <= size(_norm, V=9000, C=70)


# ---- the yardstick: autograd through saliency_ref on cases small enough to derive by hand ------------------------------------------------------

torch = pytest.importorskip("torch")


def _grads(x, w, g, stride=1, dilation=1, up=1):
    x = torch.tensor(x, dtype=torch.float64).reshape(1, 1, 1, -1, 1).requires_grad_()
    w = torch.tensor(w, dtype=torch.float64).reshape(1, 1, -1, 1, 1).requires_grad_()
    y = ref.conv3d_same(ref.upsample(x, up) if up > 1 else x, w, None, stride, dilation)
    gy = torch.zeros_like(y)
    gy[0, 0, 0, :, 0] = torch.tensor(g, dtype=torch.float64)  # (with up > 1 the D and H axes are repeated too: dy is given on their first row only)
    dx, dw = torch.autograd.grad(y, (x, w), gy)
    return y.shape, dx.flatten().tolist(), dw.flatten().tolist()


def test_yardstick_stride_2_even_extent():
    """W axis, k = 3, stride 2, extent 4: pad 0 in front and 1 behind; o0 reads x0 x1 x2, o1 reads x2 x3 and the padding."""
    x, w, g = [2.0, 3.0, 5.0, 7.0], [11.0, 13.0, 17.0], [19.0, 23.0]
    shape, dx, dw = _grads(x, w, g, stride=2)
    assert tuple(shape) == (1, 1, 1, 2, 1)
    assert dx == [g[0] * w[0], g[0] * w[1], g[0] * w[2] + g[1] * w[0], g[1] * w[1]]
    assert dw == [g[0] * x[0] + g[1] * x[2], g[0] * x[1] + g[1] * x[3], g[0] * x[2]]


def test_yardstick_stride_2_odd_extent():
    """Extent 5: pad 1 and 1, three outputs; o0 reads (pad) x0 x1, o1 reads x1 x2 x3, o2 reads x3 x4 (pad)."""
    x, w, g = [2.0, 3.0, 5.0, 7.0, 11.0], [13.0, 17.0, 19.0], [23.0, 29.0, 31.0]
    shape, dx, dw = _grads(x, w, g, stride=2)
    assert tuple(shape) == (1, 1, 1, 3, 1)
    assert dx == [g[0] * w[1], g[0] * w[2] + g[1] * w[0], g[1] * w[1], g[1] * w[2] + g[2] * w[0], g[2] * w[1]]
    assert dw == [g[1] * x[1] + g[2] * x[3], g[0] * x[0] + g[1] * x[2] + g[2] * x[4], g[0] * x[1] + g[1] * x[3]]


def test_yardstick_upsampling_sums_the_repeated_voxels():
    """up = 2 behind a 1 x 1 x 1 kernel of 1, source extent 2: dx[i] = g[2 i] + g[2 i + 1]."""
    g = [2.0, 3.0, 5.0, 7.0]
    shape, dx, dw = _grads([1.0, 1.0], [1.0], g, up=2)
    assert tuple(shape) == (1, 2, 2, 4, 1)
    assert dx == [g[0] + g[1], g[2] + g[3]] and dw == [sum(g)]


def test_yardstick_dilation_7_only_the_centre_tap_reaches():
    x, w, g = [2.0, 3.0, 5.0, 7.0, 11.0], [13.0, 17.0, 19.0], [23.0, 29.0, 31.0, 37.0, 41.0]
    shape, dx, dw = _grads(x, w, g, dilation=7)
    assert tuple(shape) == (1, 1, 1, 5, 1)
    assert dx == [gi * w[1] for gi in g]
    assert dw[0] == 0.0 and dw[2] == 0.0 and dw[1] == sum(gi * xi for gi, xi in zip(g, x))


def test_python_surface_rejects_cpu_tensors_and_bad_requests():
    from point_unet_amd import saliency as sal
    x, w, dy = torch.zeros((1, 4, 4, 4, 2)), torch.zeros((3, 3, 3, 2, 4)), torch.zeros((1, 4, 4, 4, 4))
    with pytest.raises(ValueError):
        sal.conv3d_backward(dy, x, w)
    with pytest.raises(ValueError):
        sal.instance_norm_relu_backward(dy, dy, dy, torch.ones(4))
    assert issubclass(sal.Conv3dFunction, torch.autograd.Function) and issubclass(sal.InstanceNormReluFunction, torch.autograd.Function)
