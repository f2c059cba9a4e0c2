"""ps_saliency_map (include/pointseg_saliency_map.h) on the device: the defaults against the old window loop written out, the views against
permuted copies made in torch, the flip and the fusion against their float32 compositions, the batch against batch = 1, the restatement
(saliency_map_ref.py) fed with the device's own window probabilities, the edges, the argument checks, a C++ host, and the evaluation.
Everything but the restatement is byte equality.  Base case: volume (23, 40, 50), patch (16, 32, 32), steps (12, 24, 24): 8 axial, 8 sagittal
and 6 coronal windows, three distinct extents, none a multiple of the patch or the step."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

import saliency_map_ref as mref

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE, PATCH, STEPS = (23, 40, 50), (16, 32, 32), (12, 24, 24)
VIEWS = ("axial", "sagittal", "coronal")
PERM = {"axial": (0, 1, 2), "sagittal": (2, 0, 1), "coronal": (1, 0, 2)}   # volume -> view
BACK = {"axial": (0, 1, 2, 3), "sagittal": (1, 2, 0, 3), "coronal": (1, 0, 2, 3)}  # view map -> volume


def _sal():
    from point_unet_amd import saliency
    return saliency


@functools.lru_cache(maxsize=None)
def _nets(precision="fp32", C=1):
    sal = _sal()
    return {v: sal.SaliencyNet(sal.init_params(C, 2, seed=41 + i), C, 2, precision=precision) for i, v in enumerate(VIEWS)}


@functools.lru_cache(maxsize=None)
def _vol(C=1, shape=SHAPE):
    return torch.from_numpy(np.random.default_rng(22).standard_normal((C,) + shape).astype(np.float32)).cuda()


@functools.lru_cache(maxsize=None)
def _single(view, flip=False):
    """The map of one view with its own net: the reference every composition below shares.  Never written to."""
    return _sal().saliency_map(_vol(), _nets()[view], PATCH, STEPS, direction=view, flip=flip)


def _old_loop(vol, net, patch, steps):
    """saliency_map as it was before ps_saliency_map: crop, net.probs, ps_saliency_accumulate, ps_saliency_finish."""
    from point_unet_amd import _lib, runtime
    sal = _sal()
    C, D, H, W = vol.shape
    K = net.num_classes
    v = vol.permute(1, 2, 3, 0).contiguous()
    total = torch.zeros((D, H, W, K), dtype=torch.float32, device=vol.device)
    count = torch.zeros((D, H, W), dtype=torch.int32, device=vol.device)
    crop = torch.empty((1,) + tuple(patch) + (C,), dtype=torch.float32, device=vol.device)
    ctx = runtime.default_context(vol.device.index)
    ctx.use_torch_stream()
    lib = _lib.lib()
    for o0 in sal.window_origins(D, patch[0], steps[0]):
        for o1 in sal.window_origins(H, patch[1], steps[1]):
            for o2 in sal.window_origins(W, patch[2], steps[2]):
                part = v[o0:o0 + patch[0], o1:o1 + patch[1], o2:o2 + patch[2]]
                crop.zero_()
                crop[0, :part.shape[0], :part.shape[1], :part.shape[2]] = part
                p = net.probs(crop)
                _lib.check(lib.ps_saliency_accumulate(ctx.handle, runtime.ptr(p), patch[0], patch[1], patch[2], K, o0, o1, o2, D, H, W, runtime.ptr(total),
                                                      runtime.ptr(count)))
    _lib.check(lib.ps_saliency_finish(ctx.handle, runtime.ptr(total), runtime.ptr(count), D, H, W, K, runtime.ptr(total)))
    return total


def _by_permuted_copy(vol, net, view, patch, steps):
    """The composition the call replaces: permute the volume in torch, the AXIAL map of the copy, permute the map back."""
    p = PERM[view]
    turned = vol.permute(0, 1 + p[0], 1 + p[1], 1 + p[2]).contiguous()
    return _sal().saliency_map(turned, net, patch, steps).permute(*BACK[view]).contiguous()


# ---- 1. defaults ------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["fp32", "bf16x3", "bf16"])
def test_defaults_give_the_old_loop_bytes(precision):
    net = _nets(precision)["axial"]
    got = _sal().saliency_map(_vol(), net, PATCH, STEPS)
    want = _old_loop(_vol(), net, PATCH, STEPS)
    assert got.shape == SHAPE + (2,) and got.dtype == torch.float32 and torch.equal(got, want)
    assert torch.equal(_sal().saliency_map(_vol()[0], net, PATCH, STEPS), want)  # [D, H, W]
    if precision == "fp32":
        assert torch.equal(_single("axial"), want)


# ---- 2. views ---------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("view", ["sagittal", "coronal"])
def test_view_equals_the_permuted_copy(view):
    net = _nets()[view]
    want = _by_permuted_copy(_vol(), net, view, PATCH, STEPS)
    assert want.shape == SHAPE + (2,)
    assert torch.equal(_single(view), want)
    assert not torch.equal(_single(view), _sal().saliency_map(_vol(), net, PATCH, STEPS))  # (the view is seen at all)
    channels_last = _vol().permute(1, 2, 3, 0).contiguous()
    assert torch.equal(_sal().saliency_map(channels_last, net, PATCH, STEPS, direction=view, layout="DHWC"), want)
    assert torch.equal(_sal().saliency_map(channels_last[..., 0], net, PATCH, STEPS, direction=view, layout="DHWC"), want)


@pytest.mark.parametrize("view", VIEWS)
def test_two_channels_interleave_in_both_layouts(view):
    vol, net = _vol(2), _nets("fp32", 2)[view]
    patch, steps = (16, 16, 16), (12, 20, 27)
    want = _by_permuted_copy(vol, net, view, patch, steps)
    assert torch.equal(_sal().saliency_map(vol, net, patch, steps, direction=view), want)
    assert torch.equal(_sal().saliency_map(vol.permute(1, 2, 3, 0).contiguous(), net, patch, steps, direction=view, layout="DHWC"), want)
    swapped = _by_permuted_copy(vol.flip(0), net, view, patch, steps)
    assert not torch.equal(swapped, want)  # (the channels matter)


# ---- 3. flip ----------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("view", ["axial", "sagittal"])
def test_flip_is_the_average_with_the_mirrored_volumes_map(view):
    net = _nets()[view]
    mirrored = _sal().saliency_map(_vol().flip(-1).contiguous(), net, PATCH, STEPS, direction=view).flip(2)
    want = (_single(view) + mirrored) * 0.5
    assert torch.equal(_single(view, True), want)
    assert not torch.equal(mirrored, _single(view))


# ---- 4. fusion --------------------------------------------------------------------------------------------------------------------------------------

def _third(x):
    """x / 3 in float32, correctly rounded (numpy's division; torch's division by a Python scalar may multiply by a rounded reciprocal)."""
    return torch.from_numpy(x.cpu().numpy() / np.float32(3.0)).to(x.device)


@pytest.mark.parametrize("flip", [False, True])
def test_three_views_fuse_in_float32_in_the_dicts_order(flip):
    got = _sal().saliency_map(_vol(), _nets(), PATCH, STEPS, flip=flip)
    want = _third((_single("axial") + _single("sagittal")) + _single("coronal"))
    if flip:  # the fusion of the mirrored volume's three maps, mirrored back, then the average
        mirrored = {v: _sal().saliency_map(_vol().flip(-1).contiguous(), _nets()[v], PATCH, STEPS, direction=v) for v in VIEWS}
        want = (want + _third((mirrored["axial"] + mirrored["sagittal"]) + mirrored["coronal"]).flip(2)) * 0.5
    assert torch.equal(got, want)
    assert np.abs(got.cpu().numpy().sum(-1) - 1.0).max() <= 1e-6


def test_two_views_and_another_order():
    nets = _nets()
    got = _sal().saliency_map(_vol(), {"coronal": nets["coronal"], "axial": nets["axial"]}, PATCH, STEPS)
    want = torch.from_numpy((_single("coronal") + _single("axial")).cpu().numpy() / np.float32(2.0)).cuda()
    assert torch.equal(got, want)
    # three views in another order: another float32 sum
    other = _sal().saliency_map(_vol(), {"coronal": nets["coronal"], "sagittal": nets["sagittal"], "axial": nets["axial"]}, PATCH, STEPS)
    assert torch.equal(other, _third((_single("coronal") + _single("sagittal")) + _single("axial")))


# ---- 5. batch ---------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("view", VIEWS)
def test_batch_does_not_change_a_byte(view):
    net = _nets()[view]
    for batch in (3, 8):  # 8 (6) windows: a tail of 2 (0), and everything in one call
        assert torch.equal(_sal().saliency_map(_vol(), net, PATCH, STEPS, direction=view, batch=batch), _single(view))
    assert torch.equal(_sal().saliency_map(_vol(), net, PATCH, STEPS, direction=view), _single(view))  # two runs


def test_batch_with_views_and_flip():
    want = _sal().saliency_map(_vol(), _nets(), PATCH, STEPS, flip=True)
    assert torch.equal(_sal().saliency_map(_vol(), _nets(), PATCH, STEPS, flip=True, batch=3), want)


# ---- 6. the restatement, fed with the device's own window probabilities -------------------------------------------------------------------------------

@pytest.mark.parametrize("views, flip", [(("sagittal",), False), (("coronal",), True), (VIEWS, True)])
def test_restatement_on_the_devices_own_probabilities(views, flip):
    nets = _nets()
    fns = [lambda w, n=nets[v]: n.probs(torch.from_numpy(w).cuda()).cpu().numpy() for v in views]
    vol = _vol().cpu().numpy()
    want = mref.saliency_map(vol, fns, PATCH, STEPS, 2, views, flip)
    net = nets[views[0]] if len(views) == 1 else {v: nets[v] for v in views}
    got = _sal().saliency_map(_vol(), net, PATCH, STEPS, direction=views[0] if len(views) == 1 else "axial", flip=flip).cpu().numpy()
    err = float(np.abs(got - want).max())
    err32 = float(np.abs(got - mref.saliency_map(vol, fns, PATCH, STEPS, 2, views, flip, f32=True)).max())
    print("saliency_map %s flip %d: %.3e from the float64 restatement on the device's own window probabilities, %.3e from its float32 fusion" % (
        "+".join(views), flip, err, err32))
    assert err <= 1e-6
    assert np.abs(got.sum(-1) - 1.0).max() <= 1e-6


# ---- 7. edges ---------------------------------------------------------------------------------------------------------------------------------------

def test_volume_smaller_than_the_patch_in_the_sagittal_view():
    net = _nets()["sagittal"]
    small = _vol()[:, :10, :20, :30].contiguous()
    got = _sal().saliency_map(small, net, PATCH, STEPS, direction="sagittal")  # the view's extents (30, 10, 20) against (16, 32, 32)
    assert got.shape == (10, 20, 30, 2) and torch.equal(got, _by_permuted_copy(small, net, "sagittal", PATCH, STEPS))
    window = torch.zeros((1,) + PATCH + (1,), device="cuda")
    window[0, :16, :10, :20, 0] = small[0].permute(2, 0, 1)[:16]
    assert torch.equal(got[:, :, :12], net.probs(window)[0, :12, :10, :20].permute(1, 2, 0, 3))  # the first 12 columns: one window, count 1


@pytest.mark.parametrize("view", VIEWS)
def test_an_extent_of_one_along_w(view):
    net = _nets()[view]
    thin = _vol()[:, :, :, 7:8].contiguous()
    got = _sal().saliency_map(thin, net, PATCH, STEPS, direction=view, flip=True)
    assert got.shape == (23, 40, 1, 2)
    assert torch.equal(got, _sal().saliency_map(thin, net, PATCH, STEPS, direction=view))  # a mirror of one column: (m + m) * 0.5
    assert torch.equal(got, _by_permuted_copy(thin, net, view, PATCH, STEPS))


@pytest.mark.parametrize("view", VIEWS)
def test_a_step_larger_than_the_patch_leaves_exact_zeros(view):
    net = _nets()[view]
    patch, steps = (16, 16, 16), (20, 17, 33)
    got = _sal().saliency_map(_vol(), net, patch, steps, direction=view, flip=True, batch=2)
    n = [SHAPE[a] for a in PERM[view]]
    cover = [np.zeros(n[a], bool) for a in range(3)]
    for a in range(3):
        for o in _sal().window_origins(n[a], patch[a], steps[a]):
            cover[a][o:o + patch[a]] = True
    covered = np.transpose(cover[0][:, None, None] & cover[1][None, :, None] & cover[2][None, None, :], BACK[view][:3])
    covered = covered & covered[:, :, ::-1]  # the flip pass covers the mirror image
    either = np.transpose(cover[0][:, None, None] & cover[1][None, :, None] & cover[2][None, None, :], BACK[view][:3])
    either = either | either[:, :, ::-1]
    g = got.cpu().numpy()
    assert covered.shape == SHAPE and 0 < covered.sum() and either.sum() < either.size
    assert (g[~either] == 0).all()
    assert np.abs(g[covered].sum(-1) - 1.0).max() <= 1e-6


# ---- 8. errors --------------------------------------------------------------------------------------------------------------------------------------

def test_argument_errors_write_nothing():
    from point_unet_amd import _lib, runtime
    lib = _lib.lib()
    net = _nets()["axial"]
    vol = _vol()
    ctx = runtime.default_context(0)
    ctx.use_torch_stream()
    out = torch.full(SHAPE + (2,), -7.0, device="cuda")
    good = dict(layout=0, C_in=1, D=23, H=40, W=50, K=2, n_views=1, views=(0,), weight_count=net.weights.numel(), patch=PATCH, step=STEPS, flip=0, batch=1, precision=0)
    arr = lambda t, v: None if v is None else (t * len(v))(*v)

    def call(scratch, need, **over):
        a = dict(good, **over)
        weights = (ctypes.c_void_p * 3)(*([runtime.ptr(net.weights)] * 3)) if a.get("weights", 1) else None
        return lib.ps_saliency_map(ctx.handle, runtime.ptr(vol), a["layout"], a["C_in"], a["D"], a["H"], a["W"], a["K"], a["n_views"], arr(ctypes.c_int32, a["views"]),
                                   weights, a["weight_count"], arr(ctypes.c_int64, a["patch"]), arr(ctypes.c_int64, a["step"]), a["flip"], a["batch"], a["precision"],
                                   runtime.ptr(out) if a.get("out", 1) else None, scratch, need)

    need = ctypes.c_int64(0)
    assert call(None, ctypes.byref(need)) == 0 and need.value > 0
    scratch = torch.empty(need.value, dtype=torch.uint8, device="cuda")
    bad = [dict(layout=2), dict(n_views=0), dict(n_views=4, views=(0, 1, 2, 0)), dict(views=(3,)), dict(n_views=2, views=(2, 2)), dict(flip=2), dict(batch=0),
           dict(batch=9), dict(precision=3), dict(patch=(16, 24, 32)), dict(step=(12, 0, 24)), dict(C_in=2), dict(K=3), dict(weight_count=7), dict(views=None),
           dict(patch=None), dict(step=None), dict(D=1 << 11, H=1 << 10, W=1 << 10), dict(patch=(256, 256, 256)), dict(weights=0), dict(out=0)]
    for over in bad:
        sized = ctypes.c_int64(-7)
        if "weights" not in over and "out" not in over:  # (those two may be NULL in the sizing call)
            assert call(None, ctypes.byref(sized), **over) == 1 and sized.value == -7, over
        n = ctypes.c_int64(need.value)
        assert call(runtime.ptr(scratch), ctypes.byref(n), **over) == 1, over
        assert lib.ps_last_error()
    n = ctypes.c_int64(need.value - 1)
    assert call(runtime.ptr(scratch), ctypes.byref(n)) == 1 and b"scratch" in lib.ps_last_error()
    n = ctypes.c_int64(need.value)
    assert call(ctypes.c_void_p(scratch.data_ptr() + 16), ctypes.byref(n)) == 1 and b"aligned" in lib.ps_last_error()
    assert call(runtime.ptr(scratch), None) == 1
    torch.cuda.synchronize()
    assert (out == -7.0).all()
    n = ctypes.c_int64(need.value)
    assert call(runtime.ptr(scratch), ctypes.byref(n)) == 0
    assert torch.equal(out, _single("axial"))


# ---- 9. a C++ host ----------------------------------------------------------------------------------------------------------------------------------

def test_cxx_host_gives_the_python_calls_bytes(tmp_path):
    exe = tmp_path / "saliency_map_host"
    lib_dir = os.path.join(ROOT, "point-unet_amd")
    subprocess.run(["hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cxx", "saliency_map_host.cpp"), "-L" + lib_dir, "-lpointseg_hip", "-Wl,-rpath," + lib_dir, "-o", str(exe)],
                   check=True, timeout=300)
    nets = _nets()
    nw = nets["axial"].weights.numel()
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.array([1, *SHAPE, 2, nw, *PATCH, *STEPS, 3, 0, 0, 0], np.int64).tobytes())
        f.write(_vol().cpu().numpy().tobytes())
        for v in VIEWS:
            f.write(nets[v].weights.cpu().numpy().tobytes())
    p = subprocess.run([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    assert p.stdout.startswith("scratch_bytes ")
    got = np.fromfile(tmp_path / "out.bin", np.float32).reshape(SHAPE + (2,))
    want = _sal().saliency_map(_vol(), nets, PATCH, STEPS, flip=True).cpu().numpy()
    assert np.array_equal(got, want)


# ---- 10. evaluation -----------------------------------------------------------------------------------------------------------------------------------

def test_evaluate_saliency_takes_the_views():
    from point_unet_amd import metrics, saliency_data
    bank = saliency_data.PatchBank(1)
    label = np.zeros(SHAPE, np.uint8)
    label[6:17, 10:30, 12:38] = 1
    image = _vol().permute(1, 2, 3, 0).contiguous()
    c = bank.add_prepared(image, label, np.ones(SHAPE, np.uint8))
    dice, = saliency_data.evaluate_saliency(bank, _nets(), [c], PATCH, STEPS)
    fused = _sal().saliency_map(_vol(), _nets(), PATCH, STEPS)
    cm = metrics.confusion(fused, torch.from_numpy(label).cuda(), 2).cpu().numpy()
    want = (2.0 * cm[1, 1] + 1e-10) / (cm[:, 1].sum() + cm[1, :].sum() + 1e-10)
    assert isinstance(dice, float) and dice == want and cm[1, 1] > 0
    one, = saliency_data.evaluate_saliency(bank, _nets()["sagittal"], [c], PATCH, STEPS, direction="sagittal", flip=True, batch=4)
    cm = metrics.confusion(_single("sagittal", True), torch.from_numpy(label).cuda(), 2).cpu().numpy()
    assert one == (2.0 * cm[1, 1] + 1e-10) / (cm[:, 1].sum() + cm[1, :].sum() + 1e-10)
