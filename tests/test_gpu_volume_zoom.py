"""ps_volume_zoom (csrc/resample.hip) and prepare.zoom_volume / resample_pancreas_ct on the GPU against the numpy restatement of the rule
(zoom_ref.py) and, for cases 0 - 8, against scipy's recorded results (golden/volume_zoom.npz), with the bounds of zoom_ref.check_*:
order 0 equal voxel for voxel; int16 order 3 equal except on rounding ties (at most 1 % of a case with a resampled axis shorter than 16,
none otherwise); float32 order 3 within 1e-9 * max|input| or one float32 ulp.  The flip of every axis against np.flip in front of the
zoom, the clamp against np.clip behind it, the Pancreas chains of the reference's two scripts against scipy's recorded volumes, the
hand-over into prepare_pancreas_volume, argument errors, and the scratch bound.

The shapes are the smallest that reach each way to go wrong (zoom_ref.CASES); three more reach paths of the kernels those do not: a first
filter along the contiguous axis (the float64 copy of the input), a first axis too short to filter, and lines longer than the start sum."""
import ctypes
import os

import numpy as np
import pytest

import zoom_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PS_EINVAL = 1
I16, F32, U8 = 1, 2, 3


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "volume_zoom.npz"))


@pytest.fixture(scope="module")
def expected():
    """The restatement's results, computed once per (case, dtype) and shared."""
    cache = {}

    def get(k, kind):
        if (k, kind) not in cache:
            ct, f32, seg = ref.case_inputs(k)
            z = ref.CASES[k][1]
            cache[(k, kind)] = {"i16": lambda: ref.zoom(ct, z, 3), "f32": lambda: ref.zoom(f32, z, 3), "u8": lambda: ref.zoom(seg, z, 0),
                                "i16_o0": lambda: ref.zoom(ct, z, 0)}[kind]()
        return cache[(k, kind)]
    return get


def _zoom(x, z, **kw):
    from point_unet_amd import prepare
    out = prepare.zoom_volume(x, z, **kw)
    assert out.is_cuda and tuple(out.shape) == ref.out_shape(x.shape, z)
    return out.cpu().numpy()


@pytest.mark.parametrize("k", range(len(ref.CASES)))
def test_cases_equal_the_restatement_and_scipy(k, golden, expected):
    ct, f32, seg = ref.case_inputs(k)
    z = ref.CASES[k][1]
    got_i16, got_f32, got_u8, got_o0 = _zoom(ct, z), _zoom(f32, z), _zoom(seg, z, order=0), _zoom(ct, z, order=0)
    assert got_u8.dtype == np.uint8 and np.array_equal(got_u8, expected(k, "u8"))
    assert np.array_equal(got_o0, expected(k, "i16_o0"))
    ref.check_i16(got_i16, expected(k, "i16"), ct, k)
    ref.check_f32(got_f32, expected(k, "f32"), f32, k)
    if k < ref.GOLDEN_CASES:
        assert np.array_equal(got_u8, golden["u8_o0_%d" % k])
        ref.check_i16(got_i16, golden["i16_o3_%d" % k], ct, "%d (scipy)" % k)
        ref.check_f32(got_f32, golden["f32_o3_%d" % k], f32, "%d (scipy)" % k)


def test_overshoot_plane_is_zero():
    """Case 2: the 30-long axis maps j = 14 to 29.000000000000004 and scipy zeroes the plane -- so does the device, in every dtype."""
    ct, f32, seg = ref.case_inputs(2)
    for x, order in ((ct, 3), (f32, 3), (seg, 0), (ct + 5000, 0)):
        out = _zoom(x, 0.5, order=order)
        assert (out[:, 14, :] == 0).all() and out[:, 14, :].size == 224 and (out[:, :14, :] != 0).any()


EXTRA = [
    ((6, 9, 70), (1, 1, 0.5), "i16"),    # integers: the contiguous axis is the only one filtered, so the input is first copied to float64
    ((1, 5, 4), (1, 1, 1), "f32"),       # float32 keeps every axis: the first one is too short to filter
    ((3, 5, 150), (1, 1, 0.5), "f32"),   # contiguous lines of five LDS tiles, longer than the start sum
    ((150, 3, 5), (0.5, 1, 1), "i16"),   # strided lines longer than the start sum
    ((5, 4, 3), (1, 1, 1), "i16"),       # integers at an unchanged shape: a copy
]


@pytest.mark.parametrize("shape,z,kind", EXTRA)
def test_paths_the_cases_do_not_reach(shape, z, kind):
    x = np.random.default_rng(5).integers(-1024, 3072, shape).astype(np.int16)
    if kind == "f32":
        x = (x * 0.37).astype(np.float32)
        ref.check_f32(_zoom(x, z), ref.zoom(x, z), x, shape)
    else:
        ref.check_i16(_zoom(x, z), ref.zoom(x, z), x, shape)
    for a in range(3):  # (each of these paths reads the caller's volume in its own way: through the flip as well)
        got, want = _zoom(x, z, flip=(a,)), ref.zoom(np.flip(x, a), z)
        if kind == "f32":
            ref.check_f32(got, want, x, shape)
        else:
            ref.check_i16(got, want, np.flip(x, a), shape)


@pytest.mark.parametrize("k", (0, 8))
def test_flip_of_each_axis(k):
    """np.flip(x, a) followed by the zoom; case 0 starts along axis 0 in every dtype, case 8 along axis 1 for the integers."""
    ct, f32, seg = ref.case_inputs(k)
    z = ref.CASES[k][1]
    for axes in ((0,), (1,), (2,), (0, 1, 2)):
        ref.check_i16(_zoom(ct, z, flip=axes), ref.zoom(np.flip(ct, axes), z), np.flip(ct, axes), "%d flip %s" % (k, axes))
        assert np.array_equal(_zoom(seg, z, order=0, flip=axes), ref.zoom(np.flip(seg, axes), z, 0))
    ref.check_f32(_zoom(f32, z, flip=1), ref.zoom(np.flip(f32, 1), z), f32, "%d flip 1" % k)


def test_clamp_equals_clip_of_the_unclamped_result():
    ct, f32, seg = ref.case_inputs(0)
    for x, order, lo, hi in ((ct, 3, -100, 240), (f32, 3, -37.5, 88.25), (seg, 0, 1, 1), (ct, 0, -100, 240), (ct, 3, -32768, 32767)):
        free = _zoom(x, 0.5, order=order)
        got = _zoom(x, 0.5, order=order, clip=(lo, hi))
        assert got.dtype == x.dtype and np.array_equal(got, np.clip(free, lo, hi))
        assert (free < lo).any() or (free > hi).any() or (lo, hi) == (-32768, 32767)


def _chain_inputs(golden):
    lo, hi = (int(v) for v in golden["chain_clip"])
    kw = dict(spacing_z=float(golden["chain_spacing_z"]), down_scale=float(golden["chain_down_scale"]), lower=lo, upper=hi)
    return golden["chain_ct"], golden["chain_seg"], kw


def test_pancreas_chains_equal_the_scripts(golden):
    """Both script forms against scipy's recorded volumes.  make_zoom_golden.py asserts that no voxel of either chain sits on a rounding
    tie, so equality is the bar -- also behind the intermediate int16 rounding."""
    import torch
    from point_unet_amd import prepare
    ct, seg, kw = _chain_inputs(golden)
    out = prepare.resample_pancreas_ct(ct, seg, **kw)
    assert out["ct"].dtype == torch.int16 and out["seg"].dtype == torch.uint8 and out["ct"].is_cuda
    assert np.array_equal(out["ct"].cpu().numpy(), golden["down_ct"]) and np.array_equal(out["seg"].cpu().numpy(), golden["down_seg"])
    assert out["spacing_scale"] == (2, 2, 2.0)
    crop = [tuple(r) for r in golden["chain_crop"].tolist()]
    out = prepare.resample_pancreas_ct(torch.from_numpy(ct).cuda(), torch.from_numpy(seg).cuda(), flip_y=True, crop=crop, **kw)
    assert np.array_equal(out["ct"].cpu().numpy(), golden["crop_ct"]) and np.array_equal(out["seg"].cpu().numpy(), golden["crop_seg"])
    # without a label, and with nothing to resample: the flip and the clip alone
    assert prepare.resample_pancreas_ct(ct, **kw)["seg"] is None
    out = prepare.resample_pancreas_ct(ct, seg, spacing_z=1, down_scale=1, flip_y=True)
    assert np.array_equal(out["ct"].cpu().numpy(), np.clip(np.flip(ct, 1), -100, 240)) and np.array_equal(out["seg"].cpu().numpy(), seg)


def test_chain_feeds_prepare_pancreas_volume(golden):
    """The docstring's hand-over: [z, y, x] -> [x, y, z] on the device, then the sampling; its statistics are the expected volume's."""
    from point_unet_amd import prepare
    ct, seg, kw = _chain_inputs(golden)
    out = prepare.resample_pancreas_ct(ct, seg, **kw)
    d = prepare.prepare_pancreas_volume(out["ct"].permute(2, 1, 0).contiguous(), label=out["seg"].permute(2, 1, 0).contiguous(), n_point=64, loops=2)
    want = golden["down_ct"].transpose(2, 1, 0).astype(np.float64)
    stats = d["stats"].cpu().numpy()
    assert stats[0] == want.mean() and abs(stats[1] - want.std()) <= 1e-12 * want.std()
    P = int((golden["down_seg"] > 0).sum())
    assert int(d["positives"].item()) == P and tuple(d["xyz"].shape) == (2, 64, 3)
    origin = d["xyz_origin"].cpu().numpy()
    labels = d["labels"].cpu().numpy()
    assert np.array_equal(labels, golden["down_seg"].transpose(2, 1, 0)[origin[..., 0], origin[..., 1], origin[..., 2]]) and (labels[:, :P] > 0).all()


def _raw(lib, ctx, x, out, m, dtype=None, order=3, flip=0, clamp=0, lo=0.0, hi=0.0, scratch=None, size=None, n=None):
    from point_unet_amd import runtime
    need = ctypes.c_int64(0 if size is None else size)
    n = n or x.shape
    rc = lib.ps_volume_zoom(ctx.handle, runtime.ptr(x), I16 if dtype is None else dtype, *n, order, *m, flip, clamp, lo, hi, runtime.ptr(out),
                            None if scratch is None else runtime.ptr(scratch), ctypes.byref(need))
    return rc, int(need.value)


def test_argument_errors_and_the_scratch_bound(lib):
    import torch
    from point_unet_amd import runtime
    ctx = runtime.default_context(0)
    ctx.use_torch_stream()
    x = torch.zeros((8, 10, 12), dtype=torch.int16, device="cuda")
    sentinel = 1234
    out = torch.full((4, 5, 6), sentinel, dtype=torch.int16, device="cuda")
    m = (4, 5, 6)
    rc, need = _raw(lib, ctx, x, out, m)
    assert rc == 0 and 0 < need <= 2 * 8 * x.numel() + 48 * sum(m) + 5 * 256
    rc, need0 = _raw(lib, ctx, x, out, m, order=0)
    assert rc == 0 and need0 <= 48 * sum(m) + 5 * 256  # order 0 holds no float64 volume
    sized = ctypes.c_int64(0)  # the sizing call looks at neither volume: a host may size the scratch before it allocates them
    assert lib.ps_volume_zoom(ctx.handle, None, I16, *x.shape, 3, *m, 0, 0, 0.0, 0.0, None, None, ctypes.byref(sized)) == 0 and sized.value == need
    scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
    for vols in ((None, runtime.ptr(out)), (runtime.ptr(x), None)):
        sized = ctypes.c_int64(need)
        rc = lib.ps_volume_zoom(ctx.handle, vols[0], I16, *x.shape, 3, *m, 0, 0, 0.0, 0.0, vols[1], runtime.ptr(scratch), ctypes.byref(sized))
        assert rc == PS_EINVAL and b"NULL" in lib.ps_last_error()
    bad = [dict(dtype=0), dict(dtype=4), dict(order=1), dict(order=2), dict(flip=8), dict(m=(0, 5, 6)), dict(n=(8, 0, 12)), dict(n=(1 << 20, 1 << 10, 2)), dict(n=((1 << 30) + 1, 1, 1)), dict(m=((1 << 30) + 1, 1, 1)),
           dict(m=(1 << 11, 1 << 10, 1 << 10)), dict(clamp=1, lo=5.0, hi=4.0), dict(clamp=1, lo=float("nan"), hi=1.0), dict(clamp=1, lo=-0.5, hi=3.0),
           dict(clamp=1, lo=-40000.0, hi=3.0), dict(dtype=U8, clamp=1, lo=-1.0, hi=3.0), dict(size=need - 1)]
    for kw in bad:
        kw = dict(kw)
        mm = kw.pop("m", m)
        size = kw.pop("size", need)
        rc, _ = _raw(lib, ctx, x, out, mm, scratch=scratch, size=size, **kw)
        assert rc == PS_EINVAL and b"ps_volume_zoom" in lib.ps_last_error(), kw
    rc, _ = _raw(lib, ctx, x, out, m, scratch=scratch[1:], size=need)  # not 256-byte aligned
    assert rc == PS_EINVAL and b"aligned" in lib.ps_last_error()
    ctx.synchronize()
    assert (out == sentinel).all()  # nothing was enqueued
    rc, _ = _raw(lib, ctx, x, out, m, scratch=scratch, size=need)
    ctx.synchronize()
    assert rc == 0 and (out == 0).all()
