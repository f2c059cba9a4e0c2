"""ps_volume_sample (csrc/volume_sample.hip) and prepare.pancreas_mask / prepare_pancreas_volume on the GPU: idx, origin, labels, xyz, mask and
P equal, bit for bit, to the numpy restatement of the rule (volume_sample_ref.py) from 1 x 1 x 1 to 512 x 512 x 240; statistics and values
against numpy's float64 (1e-12 relative; 2e-7 of the largest value -- the bar test_gpu_grid_ops.py applies to the BraTS z-scores: one
float64 expression rounded once, statistics that may differ from numpy's pairwise sums in the last bits); argument errors found before any
launch; P > N reported as PS_ESTATE, from the call or from the next ps_synchronize, with nothing written outside the buffers; determinism;
the scratch bound; and the chain volume -> clouds -> pyramid -> forward -> point2prod -> labels -> Dice."""
import ctypes

import numpy as np
import pytest

import volume_sample_ref as ref

pytestmark = pytest.mark.gpu

PS_EINVAL, PS_ESTATE = 1, 4
I16, F32 = 1, 2


def _ct(shape, seed=0, dtype=np.int16):
    """Hounsfield-like values with a negative mean."""
    v = np.clip(np.random.default_rng(seed).normal(-200, 400, shape), -1024, 3000)
    return v.astype(dtype)


def _blob(shape, frac=0.25, centre=None):
    g = np.stack(np.meshgrid(*[np.arange(s) for s in shape], indexing="ij"), -1).astype(np.float64)
    c = np.array(shape) / 2.0 if centre is None else np.asarray(centre, np.float64)
    r = np.maximum(np.array(shape) * frac, 0.6)
    return ((((g - c) / r) ** 2).sum(-1) < 1.0).astype(np.uint8)


class Call:
    """One ps_volume_sample call on uploaded arrays; outputs sentinel-filled with `pad` guard elements behind each."""

    def __init__(self, volume, mask=None, probs=None, N=0, loops=1, seed=0, dilate=0, truth=None, label_src=None, threshold=0.9, channel=1,
                 pad=0, fill=-7, ctx=None, shape=None, scratch_bytes=None, overrides=None, dtype=None):
        import torch
        from point_unet_amd import _lib, runtime
        self.lib, self.ctx = _lib.lib(), ctx or runtime.default_context(0)
        up = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()  # noqa: E731
        self.keep = [up(volume), up(mask), up(probs), up(truth), up(label_src)]
        X, Y, Z = shape or volume.shape
        self.L, self.N, self.pad, self.fill = loops, N, pad, fill
        a = self.a = _lib.PsVolumeSampleArgs()
        a.volume = runtime.ptr(self.keep[0])
        a.volume_dtype = dtype if dtype is not None else (I16 if volume is not None and volume.dtype == np.int16 else F32)
        a.X, a.Y, a.Z = X, Y, Z
        a.mask, a.probs = runtime.ptr(self.keep[1]), runtime.ptr(self.keep[2])
        if probs is not None:
            a.probs_C, a.probs_channel = probs.shape[-1], channel
        a.threshold, a.dilate, a.loops, a.N, a.seed = threshold, dilate, loops, N, seed & 0xFFFFFFFF
        a.truth, a.label_src = runtime.ptr(self.keep[3]), runtime.ptr(self.keep[4])
        mk = lambda cnt, dt: torch.full((max(cnt, 0) + pad,), fill % 256 if dt == torch.uint8 else fill, dtype=dt, device="cuda")  # noqa: E731
        T = max(loops, 0) * max(N, 0) if N <= (1 << 24) else 0
        nvox = int(np.prod(volume.shape))  # (the real arrays' size, also where a case passes a wrong shape)
        self.out = dict(mask=mk(nvox, torch.uint8), stats=mk(2, torch.float64), positives=mk(1, torch.int64), xyz=mk(3 * T, torch.float32),
                        features=mk(4 * T, torch.float32), labels=mk(T, torch.int32), origin=mk(3 * T, torch.int32), idx=mk(T, torch.int32))
        self.sizes = dict(mask=nvox, stats=2, positives=1, xyz=3 * T, features=4 * T, labels=T, origin=3 * T, idx=T)
        for k, t in self.out.items():
            setattr(a, "out_" + k, runtime.ptr(t))
        for k, v in (overrides or {}).items():
            setattr(a, k, v)
        self.rc = self.lib.ps_volume_sample(self.ctx.handle, ctypes.byref(a))
        if self.rc != 0:
            return
        self.need = int(a.scratch_bytes)
        self.scratch = torch.empty(self.need if scratch_bytes is None else max(scratch_bytes, 256), dtype=torch.uint8, device="cuda")
        a.scratch = runtime.ptr(self.scratch)
        if scratch_bytes is not None:
            a.scratch_bytes = scratch_bytes
        self.rc = self.lib.ps_volume_sample(self.ctx.handle, ctypes.byref(a))

    def host(self):
        import torch
        torch.cuda.synchronize()
        L, N = self.L, self.N
        shp = dict(mask=(-1,), stats=(2,), positives=(1,), xyz=(L, N, 3), features=(L, N, 4), labels=(L, N), origin=(L, N, 3), idx=(L, N))
        return {k: t[:self.sizes[k]].cpu().numpy().reshape(shp[k]) for k, t in self.out.items()}

    def untouched(self, whole=False):
        import torch
        torch.cuda.synchronize()
        for k, t in self.out.items():
            part = t if whole else t[self.sizes[k]:]
            if not bool((part == self.fill % 256 if t.dtype == torch.uint8 else part == self.fill).all()):
                return False
        return True


def _expect(volume, mask, N, loops, seed, label_src=None, values=True, **kw):
    c = Call(volume, mask=mask, N=N, loops=loops, seed=seed, label_src=label_src, pad=64, **kw)
    assert c.rc == 0, c.lib.ps_last_error()
    got = c.host()
    want = ref.sample(volume, mask, N, loops, seed, label_src)
    for k in ("idx", "origin", "labels", "xyz"):
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (k, volume.shape, N, loops, seed)
    assert np.array_equal(got["mask"].reshape(volume.shape), (np.asarray(mask) != 0).astype(np.uint8))
    assert int(got["positives"][0]) == want["positives"]
    if values:
        d = volume.astype(np.float64)
        assert abs(got["stats"][0] - d.mean()) <= 1e-12 * max(abs(d.mean()), d.std()) and abs(got["stats"][1] - d.std()) <= 1e-12 * d.std()
        assert np.array_equal(got["features"][..., :3], want["xyz"])
        if N:
            wv = ((d - d.mean()) / d.std()).reshape(-1)[want["idx"]]
            assert np.abs(got["features"][..., 3] - wv).max() <= 2e-7 * np.abs(wv).max()
    assert c.untouched()
    return got


def test_edge_sizes_exact():
    one = np.array([[[5]]], np.int16)
    _expect(one, np.ones((1, 1, 1), np.uint8), 1, 1, 3, values=False)       # 1 x 1 x 1, P = N = n
    _expect(one, np.zeros((1, 1, 1), np.uint8), 1, 16, 3, values=False)     # no positive, loops 16
    line = _ct((1, 1, 1000), 1)
    m = np.zeros((1, 1, 1000), np.uint8)
    m[0, 0, 100:200] = 1
    _expect(line, m, 400, 2, 4)                                             # 1 x 1 x n
    vol = _ct((23, 19, 37), 2)                                              # Z not a multiple of 16, n not a multiple of 16
    blob = _blob(vol.shape)
    P = int(blob.sum())
    _expect(vol, blob, P + 500, 3, 5)
    _expect(vol, np.zeros_like(blob), 700, 1, 6)                            # P = 0
    _expect(vol, blob, P, 2, 7)                                             # P = N
    _expect(vol, blob, vol.size, 2, 8)                                      # N = n: every voxel, positives first
    _expect(vol, blob, P + 100, 16, 9)                                      # loops 16
    lab = blob * np.random.default_rng(3).integers(1, 4, vol.shape).astype(np.uint8)
    _expect(vol, lab, P + 300, 2, 10, label_src=lab)                        # the training form: the label is mask and label source
    got = Call(vol, mask=blob, N=0, loops=0, pad=8)                         # N = 0: mask / statistics only
    assert got.rc == 0 and int(got.host()["positives"][0]) == P and got.untouched()


def test_threshold_ties_share_the_hash_byte_prefix():
    """N around the closest pair of neighbouring selection hashes of a 300 000-voxel volume: the threshold falls between two hashes that share
    their three leading bytes."""
    from cloud_sample_ref import keys, slot_seeds
    shape, seed = (60, 50, 100), 41
    nvox = 300000
    k = np.sort(keys(nvox, slot_seeds(seed, 0)[0]) >> np.uint64(32)).astype(np.int64)
    N = int(np.argmin(np.diff(k)[1000:-1000])) + 1001
    assert k[N] - k[N - 1] <= 4
    vol = _ct(shape, 5)
    for m in (N - 1, N, N + 1):
        _expect(vol, np.zeros(shape, np.uint8), m, 1, seed)
    mask = np.zeros(nvox, np.uint8)
    mask[keys(nvox, slot_seeds(seed, 0)[0]).argsort()[-500:]] = 1  # positives among the largest keys: the background below is unchanged
    _expect(vol, mask.reshape(shape), N + 500, 1, seed)


def test_full_ct_size_and_the_scratch_bound():
    shape, L, N = (512, 512, 240), 8, 180000
    rng = np.random.default_rng(11)
    vol = rng.integers(-1024, 1500, shape, dtype=np.int16)
    blob = _blob(shape, frac=0.0545)
    assert 30000 <= blob.sum() <= 50000
    c = Call(vol, mask=blob, N=N, loops=L, seed=77, pad=64)
    assert c.rc == 0, c.lib.ps_last_error()
    n = vol.size
    assert c.need <= n + 128 * L * N + (1 << 20)
    got = c.host()
    m = blob.reshape(-1)
    assert int(got["positives"][0]) == int(m.sum()) and np.array_equal(got["mask"], m)
    for l in (0, 5):  # (each loop of the restatement hashes all 63 M voxels)
        idx = ref.sample_indices(m, N, 77, l)
        assert np.array_equal(got["idx"][l], idx.astype(np.int32))
        origin, xyz = ref.rows(shape, idx)
        assert np.array_equal(got["origin"][l], origin) and np.array_equal(got["xyz"][l], xyz)
        assert np.array_equal(got["labels"][l], m[idx].astype(np.int32))
    P = int(m.sum())
    assert (got["idx"][:, :P] == got["idx"][0, :P]).all()
    mean, std = ref.statistics(vol)
    assert abs(got["stats"][0] - mean) <= 1e-12 * std and abs(got["stats"][1] - std) <= 1e-12 * std
    assert c.untouched()
    again = Call(vol, mask=blob, N=N, loops=L, seed=77).host()
    assert all(np.array_equal(got[k], again[k]) for k in got)  # int16: statistics and values bit-identical between runs


def test_float32_volume_against_the_float64_expression():
    vol = (np.random.default_rng(12).normal(2.0, 1.0, (31, 33, 29))).astype(np.float32)  # |mean| <= 3 std
    blob = _blob(vol.shape)
    a = _expect(vol, blob, int(blob.sum()) + 2000, 2, 13)
    b = Call(vol, mask=blob, N=int(blob.sum()) + 2000, loops=2, seed=13).host()
    assert all(np.array_equal(a[k], b[k]) for k in b)


def test_mask_from_threshold_dilation_and_truth():
    shape = (21, 18, 35)
    rng = np.random.default_rng(14)
    t = np.float32(0.9)
    p1 = rng.random(shape).astype(np.float32) * np.float32(0.95)
    ties = rng.integers(0, 3, shape)
    edge = rng.random(shape) < 0.05
    p1[edge] = np.array([np.nextafter(t, np.float32(0)), t, np.nextafter(t, np.float32(1))], np.float32)[ties[edge]]
    p1[0, 0, 0] = p1[-1, -1, -1] = p1[10, 0, 34] = 1.0  # faces and corners
    probs = np.stack([1 - p1, p1], -1)
    truth = _blob(shape, 0.15, centre=(4, 4, 4))
    vol = _ct(shape, 15)
    for rounds in (0, 1, 3):
        for tr in (None, truth):
            want = ref.positive_mask(probs=probs, dilate_rounds=rounds, truth=tr)
            c = Call(vol, probs=probs, dilate=rounds, truth=tr, pad=32)
            assert c.rc == 0, c.lib.ps_last_error()
            got = c.host()
            assert np.array_equal(got["mask"].reshape(shape), want), (rounds, tr is None)
            assert int(got["positives"][0]) == int(want.sum()) and c.untouched()
    for shp in ((9, 7, 32), (5, 3, 16), (4, 6, 48), (2, 2, 17)):  # rows of whole 16-voxel runs (the word path of the dilation) and not
        seed_mask = (np.random.default_rng(sum(shp)).random(shp) < 0.04).astype(np.uint8)
        seed_mask[0, 0, 0] = seed_mask[-1, -1, -1] = 1
        for rounds in (1, 2, 5):
            got = Call(_ct(shp, 1), mask=seed_mask, dilate=rounds).host()["mask"].reshape(shp)
            assert np.array_equal(got, ref.dilate(seed_mask, rounds).astype(np.uint8)), (shp, rounds)
    # the inference form: probs -> mask with one dilation gives the same rows as feeding the resulting mask back
    want = ref.positive_mask(probs=probs, dilate_rounds=1)
    N = int(want.sum()) + 1500
    a = Call(vol, probs=probs, dilate=1, N=N, loops=3, seed=16).host()
    b = Call(vol, mask=a["mask"].reshape(shape), N=N, loops=3, seed=16).host()
    assert all(np.array_equal(a[k], b[k]) for k in a)
    w = ref.sample(vol, want, N, 3, 16)
    assert np.array_equal(a["idx"], w["idx"]) and np.array_equal(a["labels"], w["labels"])


def test_argument_errors_leave_the_outputs_untouched():
    vol = _ct((10, 12, 14), 17)
    blob = _blob(vol.shape)
    probs = np.zeros(vol.shape + (2,), np.float32)
    cases = [
        dict(N=vol.size + 1),                                   # N > n
        dict(N=100, loops=0), dict(N=100, loops=17),            # loops
        dict(N=-1),
        dict(N=100, dilate=-1),
        dict(N=100, shape=(0, 12, 14)), dict(N=100, shape=(65536, 1, 1)), dict(N=100, shape=(65535, 65535, 2)),
        dict(N=100, dtype=3),                                   # volume_dtype
        dict(N=100, overrides=dict(mask=None)),                 # no positive source
        dict(N=100, overrides=dict(probs=ctypes.c_void_p(256))),  # two sources
        dict(N=100, overrides=dict(volume=None)),               # features asked for without a volume
        dict(N=100, overrides=dict(reserved=1)),
    ]
    for k, cs in enumerate(cases):
        c = Call(vol, mask=blob, pad=4, **({"loops": 1} | cs))
        assert c.rc == PS_EINVAL, (k, c.rc)
        assert c.lib.ps_last_error().startswith(b"ps_volume_sample"), (k, c.lib.ps_last_error())
        assert c.untouched(whole=True), k
    for cs in (dict(channel=2), dict(channel=-1), dict(threshold=float("nan")), dict(overrides=dict(probs_C=65536))):
        c = Call(vol, probs=probs, N=100, loops=1, **cs)
        assert c.rc == PS_EINVAL and c.untouched(whole=True)
    c = Call(vol, mask=blob, N=500, loops=2, scratch_bytes=4096)  # too little scratch
    assert c.rc == PS_EINVAL and b"scratch" in c.lib.ps_last_error() and c.untouched(whole=True)


def test_more_positives_than_rows_is_reported_and_stays_inside_the_buffers():
    from point_unet_amd import runtime
    vol = _ct((20, 20, 20), 18)
    blob = _blob(vol.shape, 0.4)
    P = int(blob.sum())
    for deferred in (False, True):
        ctx = runtime.Context(0)
        ctx.use_torch_stream()
        if deferred:
            ctx.set_deferred_checks(True)
        for N in (P - 1, P // 3, 1):
            c = Call(vol, mask=blob, N=N, loops=3, seed=19, pad=4096, ctx=ctx)
            if deferred:
                assert c.rc == 0, c.lib.ps_last_error()
                assert c.lib.ps_synchronize(ctx.handle) == PS_ESTATE
            else:
                assert c.rc == PS_ESTATE
            assert b"positive" in c.lib.ps_last_error()
            assert c.untouched()
            assert int(c.host()["positives"][0]) == P
        assert c.lib.ps_synchronize(ctx.handle) == 0  # reported once
        ok = Call(vol, mask=blob, N=P + 10, loops=1, seed=19, ctx=ctx)
        assert ok.rc == 0 and c.lib.ps_synchronize(ctx.handle) == 0
        ctx.close()


def test_deterministic_across_calls_contexts_and_streams():
    import torch
    from point_unet_amd import runtime
    vol = _ct((40, 36, 28), 20)
    blob = _blob(vol.shape)
    N = int(blob.sum()) + 3000
    first = _expect(vol, blob, N, 4, 77)
    for _ in range(2):
        again = Call(vol, mask=blob, N=N, loops=4, seed=77).host()
        assert all(np.array_equal(first[k], again[k]) for k in first)
    ctx = runtime.Context(0)
    s = torch.cuda.Stream()
    ctx.set_stream(s)
    with torch.cuda.stream(s):
        other = Call(vol, mask=blob, N=N, loops=4, seed=77, ctx=ctx).host()
    assert all(np.array_equal(first[k], other[k]) for k in first)
    ctx.close()
    diff = Call(vol, mask=blob, N=N, loops=4, seed=78).host()
    assert not np.array_equal(first["idx"], diff["idx"])


def test_python_surface_and_the_chain_to_dice():
    import torch
    import netcase
    from point_unet_amd import metrics, weights
    from point_unet_amd.postprocess import point2prod
    from point_unet_amd.prepare import pancreas_mask, prepare_pancreas_volume
    from point_unet_amd.pyramid import build_pyramid
    from point_unet_amd.RandLANet import Network
    from point_unet_amd.train import Trainer
    shape = (40, 36, 30)  # (X, Y, Z)
    X, Y, Z = shape
    vol = _ct(shape, 21)
    label = _blob(shape, 0.2)
    L, N = 8, 6000
    d = prepare_pancreas_volume(vol, label=label, n_point=N, loops=L, seed=5)
    w = ref.sample(vol, label, N, L, 5, label_src=label)
    for k, wk in (("idx", "idx"), ("xyz_origin", "origin"), ("labels", "labels"), ("xyz", "xyz")):
        assert d[k].is_cuda and np.array_equal(d[k].cpu().numpy(), w[wk]), k
    assert int(d["positives"][0]) == int(label.sum()) and d["value"].shape == (L, N, 1)
    dt = prepare_pancreas_volume(torch.from_numpy(vol).cuda(), label=torch.from_numpy(label).cuda(), n_point=N, loops=L, seed=5)
    assert all(torch.equal(d[k], dt[k]) for k in d)
    df = prepare_pancreas_volume(vol.astype(np.float32), mask=label, n_point=N, loops=L, seed=5)
    assert torch.equal(df["idx"], d["idx"]) and float((df["features"] - d["features"]).abs().max()) <= 1e-6
    probs = np.stack([1 - label, label], -1).astype(np.float32)
    m = pancreas_mask(probs=probs, threshold=0.9, dilate=1)
    assert np.array_equal(m.cpu().numpy(), ref.positive_mask(probs=probs, dilate_rounds=1))
    di = prepare_pancreas_volume(vol, probs=probs, dilate=1, n_point=N, loops=2, seed=6)
    dm = prepare_pancreas_volume(vol, mask=m, n_point=N, loops=2, seed=6)
    assert all(torch.equal(di[k], dm[k]) for k in di)

    cfg = netcase.make_cfg(5, (16, 32, 64, 32, 16), (4, 4, 4, 4, 2), 16, 2, 4)  # ConfigPancreas' shape at small widths
    params = weights.init_params(cfg, seed=3, randomize_bn=True)
    net = Network(cfg, params=params)
    l = 2
    pyr = build_pyramid(d["xyz"][l:l + 1].contiguous(), cfg)
    logits = net.inference({"pyramid": pyr, "features": d["features"][l:l + 1].contiguous()})
    volp = point2prod(logits[0], None, d["xyz_origin"][l].contiguous(), volume_shape=(Z, X, Y))
    v = volp.cpu().numpy()  # [Z, Y, X, C]
    written = v.sum(-1) > 0
    o = w["origin"][l]
    want = np.zeros((Z, Y, X), bool)
    want[o[:, 2], o[:, 1], o[:, 0]] = True
    assert np.array_equal(written, want)  # exactly the sampled voxels of that loop
    pred = metrics.probs_to_labels(volp, label_values=(0, 1))
    truth = torch.from_numpy(np.ascontiguousarray(label.transpose(2, 1, 0))).cuda()
    s = metrics.segmentation_metrics(pred, truth, metrics.PANCREAS_REGIONS)
    assert 0.0 <= s["pancreas"]["dice"] <= 1.0 and s["pancreas"]["n_truth"] == int(label.sum())

    cw = np.array([1.0, 2.0], np.float32)
    # host-made arrays, values included: for int16 the statistics are exact integers rounded once, on both sides
    host = [torch.from_numpy(w[k]).cuda() for k in ("xyz", "features", "labels")]
    assert torch.equal(host[1], d["features"])
    res = []
    for bx, bf, bl in ((d["xyz"], d["features"], d["labels"]), host):
        with Trainer(cfg, params=params, learning_rate=1e-3, class_weights=cw, keep_prob=1.0) as tr:
            loss = tr.train_step(build_pyramid(bx.contiguous(), cfg), bf.contiguous(), bl.contiguous())
            torch.cuda.synchronize()
            res.append(loss.clone())
    assert bool(torch.isfinite(res[0]).all()) and torch.equal(res[0], res[1])


def test_against_the_reference_functions():
    """tests/golden/pancreas_prepare.npz holds what the reference's own itensity_normalize_one_volume + sampling_convert_pc2ply
    (dataPreparePancreas.py:34-46, 132-169), genSegmentation (genBinaryMap.py:67-80) and dilation_over_truth (over_sampling.py:58-65) gave
    on a 40 x 36 x 28 int16 volume (make_pancreas_golden.py; the full draw holds every voxel, rows matched by origin): mask from threshold +
    dilation + truth exact; per-voxel xyz, origin, labels exact; values within 2e-7 of the largest; statistics within 1e-12 relative."""
    import os
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pancreas_prepare.npz"))
    vol, label = g["volume"], g["label"]
    n = vol.size
    c = Call(vol, mask=label, N=n, loops=2, seed=3, label_src=label, pad=16)
    assert c.rc == 0, c.lib.ps_last_error()
    got = c.host()
    for l in range(2):
        order = np.argsort(got["idx"][l])
        assert np.array_equal(got["idx"][l][order], np.arange(n))
        assert np.array_equal(got["xyz"][l][order], g["xyz"].T)
        assert np.array_equal(got["labels"][l][order], g["labels"].astype(np.int32))
        o = got["origin"][l][order]
        assert np.array_equal((o[:, 0] * vol.shape[1] + o[:, 1]) * vol.shape[2] + o[:, 2], np.arange(n))
        v = got["features"][l][order][:, 3]
        assert np.abs(v - g["value"]).max() <= 2e-7 * np.abs(g["value"]).max()
    assert vol.mean() < 0
    assert abs(got["stats"][0] - vol.mean()) <= 1e-12 * abs(vol.mean()) and abs(got["stats"][1] - vol.std()) <= 1e-12 * vol.std()
    # the reference's smaller draw: its positives come first and ascending, as the rule's
    P = int(label.sum())
    small = g["small_flat"]
    assert np.array_equal(small[:P], np.flatnonzero(label.reshape(-1)))
    mine = Call(vol, mask=label, N=int(g["small_n_point"]), loops=1, seed=4).host()["idx"][0]
    assert np.array_equal(mine[:P], small[:P]) and not label.reshape(-1)[mine[P:]].any() and len(np.unique(mine)) == len(mine)
    # attention map -> binary map -> dilation OR truth
    p1 = g["probs1"]
    probs = np.stack([1 - p1, p1], -1).astype(np.float32)
    a = Call(vol, probs=probs, threshold=0.9).host()["mask"].reshape(vol.shape)
    assert np.array_equal(a, g["binary"])
    b = Call(vol, probs=probs, threshold=0.9, dilate=1, truth=label).host()["mask"].reshape(vol.shape)
    assert np.array_equal(b, g["dilated_truth"])


def test_unaligned_pointers_and_other_channel_counts():
    """Every input and output at an odd element offset inside its allocation (the 16-byte paths fall back to element accesses), and
    probabilities with 1, 3 and 5 channels, aligned or not: the same rows and masks as from aligned tensors."""
    import torch
    from point_unet_amd import _lib, runtime
    shape = (19, 23, 21)
    n = int(np.prod(shape))
    rng = np.random.default_rng(30)
    blob = _blob(shape)
    truth = _blob(shape, 0.15, centre=(3, 3, 3))
    L, N = 2, int(blob.sum()) + 900
    h = runtime.default_context(0).handle
    lib = _lib.lib()

    def off(arr, k=1):  # the array at element offset k of a larger allocation
        t = torch.zeros(arr.size + k + 8, dtype=torch.from_numpy(arr.reshape(-1)[:1]).dtype, device="cuda")
        t[k:k + arr.size] = torch.from_numpy(np.ascontiguousarray(arr).reshape(-1)).cuda()
        return t, t[k:]

    for vol in (_ct(shape, 31), _ct(shape, 32).astype(np.float32)):
        want = Call(vol, mask=blob, N=N, loops=L, seed=9, label_src=blob).host()
        keep = [off(vol), off(blob), off(blob, 3)]
        outs = {k: torch.full((cnt + 9,), -7, dtype=dt, device="cuda") for k, cnt, dt in (
            ("xyz", 3 * L * N, torch.float32), ("features", 4 * L * N, torch.float32), ("labels", L * N, torch.int32), ("origin", 3 * L * N, torch.int32),
            ("idx", L * N, torch.int32))}
        omask = torch.full((n + 9,), 249, dtype=torch.uint8, device="cuda")
        a = _lib.PsVolumeSampleArgs()
        a.volume, a.volume_dtype = runtime.ptr(keep[0][1]), I16 if vol.dtype == np.int16 else F32
        a.X, a.Y, a.Z = shape
        a.mask, a.label_src = runtime.ptr(keep[1][1]), runtime.ptr(keep[2][1])
        a.loops, a.N, a.seed = L, N, 9
        for k, t in outs.items():
            setattr(a, "out_" + k, runtime.ptr(t[1:]))
        a.out_mask = runtime.ptr(omask[1:])
        assert lib.ps_volume_sample(h, ctypes.byref(a)) == 0
        scratch = torch.empty(int(a.scratch_bytes), dtype=torch.uint8, device="cuda")
        a.scratch = runtime.ptr(scratch)
        assert lib.ps_volume_sample(h, ctypes.byref(a)) == 0, lib.ps_last_error()
        torch.cuda.synchronize()
        for k, t in outs.items():
            cnt = want[k].size
            assert np.array_equal(t[1:1 + cnt].cpu().numpy(), want[k].reshape(-1)), k
            assert float(t[0]) == -7 and bool((t[1 + cnt:] == -7).all()), k
        assert np.array_equal(omask[1:1 + n].cpu().numpy(), blob.reshape(-1)) and int(omask[0]) == 249 and bool((omask[1 + n:] == 249).all())
        # a scratch pointer that is not 256-byte aligned is refused
        a.scratch = ctypes.c_void_p(scratch.data_ptr() + 16)
        assert lib.ps_volume_sample(h, ctypes.byref(a)) == PS_EINVAL
    vol = _ct(shape, 33)
    for C in (1, 2, 3, 5):
        for ch in {0, C - 1}:
            probs = rng.random(shape + (C,)).astype(np.float32)
            want = ref.positive_mask(probs=probs, channel=ch, threshold=0.8, dilate_rounds=1, truth=truth)
            got = Call(vol, probs=probs, channel=ch, threshold=0.8, dilate=1, truth=truth).host()["mask"]
            assert np.array_equal(got.reshape(shape), want), (C, ch)
            # the probabilities at an odd float offset, the truth and the mask output at odd byte offsets
            pk, tk = off(probs), off(truth)
            omask = torch.full((n + 9,), 249, dtype=torch.uint8, device="cuda")
            a = _lib.PsVolumeSampleArgs()
            a.X, a.Y, a.Z = shape
            a.probs, a.probs_C, a.probs_channel, a.threshold, a.dilate = runtime.ptr(pk[1]), C, ch, 0.8, 1
            a.truth, a.out_mask = runtime.ptr(tk[1]), runtime.ptr(omask[1:])
            assert lib.ps_volume_sample(h, ctypes.byref(a)) == 0
            scratch = torch.empty(int(a.scratch_bytes), dtype=torch.uint8, device="cuda")
            a.scratch = runtime.ptr(scratch)
            assert lib.ps_volume_sample(h, ctypes.byref(a)) == 0, lib.ps_last_error()
            torch.cuda.synchronize()
            assert np.array_equal(omask[1:1 + n].cpu().numpy(), want.reshape(-1)), (C, ch)
            assert int(omask[0]) == 249 and bool((omask[1 + n:] == 249).all())
