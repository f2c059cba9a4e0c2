"""The rules of include/pointseg_saliency.h on their restatement (saliency_ref.py; test_gpu_saliency.py ties the kernels to it), and
the C surface as far as it goes without a GPU: the prototype table, the argument checks, the parameter layout."""
import ctypes
import os
import re

import numpy as np
import pytest

import saliency_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- SAME padding, against hand-derived cases -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n, k, stride, dilation, want", [
    (6, 3, 2, 1, (3, 0, 1)),    # even extent, stride 2: windows start at 0, 2, 4, the last one needs voxel 6 -- one voxel behind, none in front
    (5, 3, 2, 1, (3, 1, 1)),    # odd extent: (3 - 1) * 2 + 3 - 5 = 2, one each side
    (8, 3, 2, 1, (4, 0, 1)),
    (7, 3, 1, 1, (7, 1, 1)),
    (4, 3, 1, 7, (4, 7, 7)),    # dilation 7 on 4 voxels: the taps sit 7 apart, span 15, 14 to pad -- only the centre tap ever lands inside
    (4, 3, 1, 5, (4, 5, 5)),
    (2, 9, 1, 1, (2, 4, 4)),    # k = 9 on 2 voxels: 8 to pad
    (5, 9, 1, 1, (5, 4, 4)),
    (5, 1, 1, 1, (5, 0, 0)),
    (5, 1, 2, 1, (3, 0, 0)),    # a 1-tap kernel at stride 2 never pads: (3 - 1) * 2 + 1 - 5 = 0
])
def test_same_padding_rule(n, k, stride, dilation, want):
    assert ref.same_padding(n, k, stride, dilation) == want


def test_same_conv_reads_what_the_rule_says():
    """A ones kernel on a ramp: every output is the sum of the taps inside, which the padding rule fixes by hand."""
    torch = pytest.importorskip("torch")
    x = torch.arange(1.0, 7.0, dtype=torch.float64).reshape(1, 6, 1, 1, 1)
    w = torch.ones((3, 1, 1, 1, 1), dtype=torch.float64)
    # stride 2, even extent: windows [0, 1, 2], [2, 3, 4], [4, 5, pad]
    assert ref.conv3d_same(x, w, stride=2).flatten().tolist() == [6.0, 12.0, 11.0]
    # stride 2, odd extent 5: windows [pad, 0, 1], [1, 2, 3], [3, 4, pad]
    assert ref.conv3d_same(x[:, :5], w, stride=2).flatten().tolist() == [3.0, 9.0, 9.0]
    # dilation 7 on 4 voxels: only the centre tap lands inside
    assert ref.conv3d_same(x[:, :4], w, dilation=7).flatten().tolist() == [1.0, 2.0, 3.0, 4.0]
    # k = 9 on 2 voxels: both voxels under every window
    w9 = torch.ones((9, 1, 1, 1, 1), dtype=torch.float64)
    assert ref.conv3d_same(x[:, :2], w9).flatten().tolist() == [3.0, 3.0]


def test_instance_norm_is_the_biased_variance():
    torch = pytest.importorskip("torch")
    x = torch.tensor([1.0, 2.0, 3.0, 6.0], dtype=torch.float64).reshape(1, 4, 1)
    got = ref.instance_norm_relu(x, torch.tensor([2.0], dtype=torch.float64), torch.tensor([0.5], dtype=torch.float64), eps=0.0)
    want = np.maximum((np.array([1.0, 2.0, 3.0, 6.0]) - 3.0) / np.sqrt(3.5) * 2.0 + 0.5, 0.0)  # var = (4 + 1 + 0 + 9) / 4
    assert np.allclose(got.flatten().numpy(), want, rtol=0, atol=1e-15)


# ---- float32 against float64: the rule itself stays well inside the GPU bar of 1e-4 ----------------------------------------------------------------

@pytest.mark.parametrize("shape, cin", [((16, 32, 32), 1), ((16, 32, 48), 4)])
def test_float32_restatement_against_float64(shape, cin):
    torch = pytest.importorskip("torch")
    from point_unet_amd import saliency as sal
    params = sal.init_params(cin, 2, seed=3)
    x = np.random.default_rng(4).standard_normal((1,) + shape + (cin,)).astype(np.float32)
    l64 = ref.forward(params, x, torch.float64)
    l32 = ref.forward(params, x, torch.float32)
    gap = float(np.abs(l32 - l64).max())
    pgap = float(np.abs(ref.softmax(l32.astype(np.float64)) - ref.softmax(l64)).max())
    print("float32 vs float64 at %s x %d: max |logit| %.2f, logit gap %.2e, probability gap %.2e" % (shape, cin, np.abs(l64).max(), gap, pgap))
    assert l64.shape == (1,) + shape + (2,)
    assert gap < 5e-5


def test_extents_must_be_multiples_of_16():
    torch = pytest.importorskip("torch")
    from point_unet_amd import saliency as sal
    with pytest.raises(AssertionError):
        ref.forward(sal.init_params(1, 2, 0), np.zeros((1, 16, 24, 32, 1), np.float32), torch.float32)


# ---- the window rule ---------------------------------------------------------------------------------------------------------------------------

def _literal_origins(n, crop, step):
    """The loop np.arange(0, max(1, n - crop + step), step) stands for."""
    out, o = [], 0
    while o < max(1, n - crop + step):
        out.append(o)
        o += step
    return out


@pytest.mark.parametrize("n, crop, step", [(10, 16, 12), (16, 16, 12), (17, 16, 12), (23, 16, 12), (50, 32, 24), (64, 64, 48), (65, 64, 48),
                                           (230, 160, 118), (160, 160, 118), (100, 160, 118)])
def test_window_origins(n, crop, step):
    from point_unet_amd import saliency as sal
    want = _literal_origins(n, crop, step)
    assert ref.window_origins(n, crop, step).tolist() == want == sal.window_origins(n, crop, step)
    count = np.zeros(n, int)
    for o in want:
        count[o:o + crop] += 1
    assert count.min() >= 1
    if n <= crop:
        assert want == [0]
    if n == crop + 1:
        assert want == [0, step]


def test_overlapping_inference_counts_and_average():
    """A model that returns its window's first channel as the probability of class 1: the average gives the volume back wherever a
    window covers it, whatever the count."""
    rng = np.random.default_rng(0)
    vol = rng.random((1, 23, 40, 50))

    def probs_of(window):
        assert window.shape == (1, 16, 32, 32, 1)
        return np.concatenate([1.0 - window, window], -1)

    mean, count = ref.overlapping_inference(vol, probs_of, (16, 32, 32), (12, 24, 24), 2)
    assert mean.shape == (23, 40, 50, 2) and count.min() >= 1 and count.max() == 8
    assert np.allclose(mean[..., 1], vol[0], rtol=0, atol=1e-15) and np.allclose(mean.sum(-1), 1.0, rtol=0, atol=1e-15)
    # smaller than the patch: one zero-filled window
    mean, count = ref.overlapping_inference(vol[:, :10, :20, :30], probs_of, (16, 32, 32), (12, 24, 24), 2)
    assert mean.shape == (10, 20, 30, 2) and (count == 1).all()


# ---- the C surface: fails before the feature exists -----------------------------------------------------------------------------------------------

def _declared(hname):
    src = open(os.path.join(ROOT, "include", hname)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return set(re.findall(r"\b(ps_[a-z0-9_]+)\s*\(", src))


NAMES = {"ps_conv3d", "ps_instance_norm_relu", "ps_saliency_weight_count", "ps_saliency_forward", "ps_saliency_accumulate", "ps_saliency_finish"}


def test_header_matches_its_prototype_table():
    from point_unet_amd import _lib
    assert _declared("pointseg_saliency.h") == set(_lib.SALIENCY_PROTOTYPES) == NAMES
    others = set(_lib.PROTOTYPES) | set(_lib.PREPARE_PROTOTYPES) | set(_lib.POSTPROCESS_PROTOTYPES)
    assert not NAMES & others
    assert not NAMES & (_declared("pointseg.h") | _declared("pointseg_prepare.h") | _declared("pointseg_train_ops.h") | _declared("pointseg_postprocess.h"))
    # PROTOTYPES still is the two old headers
    assert set(_lib.PROTOTYPES) == _declared("pointseg.h") | _declared("pointseg_train_ops.h")


def test_library_exports_the_symbols(lib):
    from point_unet_amd import _lib
    for name, (_, args) in _lib.SALIENCY_PROTOTYPES.items():
        assert len(getattr(lib, name).argtypes) == len(args)


def _conv(lib, **kw):
    a = dict(ctx=None, x=None, x2=None, B=1, Ds=4, Hs=4, Ws=4, C1=4, C2=0, up=1, w=None, bias=None, kd=3, kh=3, kw=3, C_out=8, stride=1, dilation=1, y=None)
    a.update(kw)
    return lib.ps_conv3d(*a.values())


def test_bad_arguments_are_found_before_any_hip_call(lib):
    err = lib.ps_last_error
    assert _conv(lib) == 1 and b"ps_conv3d" in err() and b"NULL" in err()
    for kw, word in ((dict(kd=5), b"kernel"), (dict(kw=2), b"kernel"), (dict(stride=3), b"stride"), (dict(dilation=2), b"dilation"), (dict(up=0), b"up"),
                     (dict(C1=385), b"C1"), (dict(C1=300, C2=100), b"C1"), (dict(C_out=257), b"C_out"), (dict(C_out=0), b"C_out"), (dict(Ds=0), b"input"),
                     (dict(Ds=1 << 12, Hs=1 << 12, Ws=1 << 12), b"input"), (dict(B=0), b"B")):
        assert _conv(lib, **kw) == 1 and word in err(), kw
    need = ctypes.c_int64(-1)
    # instance norm: the size call needs no context, bad shapes are found in it
    assert lib.ps_instance_norm_relu(None, None, 2, 5000, 3, None, None, 1e-5, None, None, ctypes.byref(need)) == 0
    assert need.value >= 2 * 2 * 3 * 2 * 8 and need.value % 256 == 0
    assert lib.ps_instance_norm_relu(None, None, 2, 0, 3, None, None, 1e-5, None, None, ctypes.byref(need)) == 1 and b"V" in err()
    assert lib.ps_instance_norm_relu(None, None, 2, 10, 3, None, None, 0.0, None, None, ctypes.byref(need)) == 1 and b"eps" in err()
    assert lib.ps_instance_norm_relu(None, None, 2, 10, 3, None, None, 1e-5, None, None, None) == 1 and b"NULL" in err()
    # the network
    n = lib.ps_saliency_weight_count(1, 2)
    fwd = lambda D, H, W, cin=1, k=2, count=n: lib.ps_saliency_forward(None, None, 1, D, H, W, cin, k, None, count, None, None, None, None, ctypes.byref(need))
    assert fwd(64, 160, 160) == 0 and need.value > 64 * 160 * 160 * 4 * 300 and need.value % 256 == 0
    assert fwd(16, 24, 32) == 1 and b"multiple of 16" in err()
    assert fwd(0, 16, 16) == 1 and b"multiple of 16" in err()
    assert fwd(16, 16, 16, count=n - 1) == 1 and b"weight_count" in err()
    assert fwd(16, 16, 16, k=1) == 1 and b"num_classes" in err()
    assert fwd(16, 16, 16, cin=0) == 1 and b"C_in" in err()
    assert lib.ps_saliency_weight_count(0, 2) == -1 and lib.ps_saliency_weight_count(1, 1) == -1
    # the window average
    assert lib.ps_saliency_accumulate(None, None, 16, 32, 32, 2, 0, 0, 0, 23, 40, 50, None, None) == 1 and b"NULL" in err()
    assert lib.ps_saliency_accumulate(None, None, 16, 32, 32, 2, 23, 0, 0, 23, 40, 50, None, None) == 1 and b"origin" in err()
    assert lib.ps_saliency_accumulate(None, None, 16, 32, 32, 0, 0, 0, 0, 23, 40, 50, None, None) == 1 and b"C =" in err()
    assert lib.ps_saliency_finish(None, None, None, 23, 40, 50, 2, None) == 1 and b"NULL" in err()
    assert lib.ps_saliency_finish(None, None, None, 0, 40, 50, 2, None) == 1 and b"volume" in err()


# ---- parameters --------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cin, classes", [(1, 2), (4, 2), (4, 4)])
def test_parameter_count_and_round_trip(lib, cin, classes):
    from point_unet_amd import saliency as sal
    params = sal.init_params(cin, classes, seed=1)
    total = sum(v.size for v in params.values())
    assert total == ref.param_count(cin, classes) == lib.ps_saliency_weight_count(cin, classes)
    assert all(v.dtype == np.float32 for v in params.values()) and all(k.startswith("unet3d_attention/") for k in params)
    flat = sal.flatten_params(params, cin, classes)
    assert flat.dtype == np.float32 and flat.shape == (total,)
    back = sal.unflatten_params(flat, cin, classes)
    assert list(back) == list(params) and all(np.array_equal(back[k], params[k]) for k in params)
    # the buffer starts with init_conv's kernel and ends with final's bias
    k0 = params["unet3d_attention/init_conv/kernel"]
    assert k0.shape == (3, 3, 3, cin, 16) and np.array_equal(flat[:k0.size], k0.reshape(-1))
    assert np.array_equal(flat[-classes:], params["unet3d_attention/final/bias"])
    # the four convolutions of every CFE3D carry no bias (model.py:139-174)
    assert not [k for k in params if "_cfe" in k and "_up" not in k and k.endswith("/bias")]
    with pytest.raises(ValueError):
        sal.flatten_params({k: v for k, v in params.items() if not k.endswith("final/bias")}, cin, classes)
    with pytest.raises(ValueError):
        sal.flatten_params(dict(params, extra=np.zeros(1, np.float32)), cin, classes)


def test_python_surface_rejects_cpu_tensors():
    torch = pytest.importorskip("torch")
    from point_unet_amd import saliency as sal
    x = torch.zeros((1, 4, 4, 4, 2))
    with pytest.raises(ValueError):
        sal.conv3d(x, torch.zeros((3, 3, 3, 2, 4)))
    with pytest.raises(ValueError):
        sal.instance_norm_relu(x, torch.ones(2), torch.zeros(2))
