"""ps_cloud_sample / ps_cloud_positive_counts (csrc/cloud_sample.hip) and dataset.CloudBank on the GPU: every output equal, bit for bit, to
the numpy restatement of the rule (cloud_sample_ref.py) on the edge cases, banks of mixed cloud sizes, B up to PS_CLOUD_SAMPLE_MAX_B, the
threshold's neighbourhood and BraTS-sized clouds; argument errors found before any launch; a stale positive count reported as
PS_ESTATE, from the call or from the next ps_synchronize, with nothing written outside [B, N]; determinism across calls, contexts and
streams; and a bank batch as the drop-in input of build_pyramid + Trainer.train_step, Network.inference + point2prod and metrics.validate."""
import ctypes

import numpy as np
import pytest

import cloud_sample_ref as ref

pytestmark = pytest.mark.gpu

MAX_B = 64  # PS_CLOUD_SAMPLE_MAX_B
PS_EINVAL, PS_ESTATE = 1, 4


def _bank(sizes, C=4, pos_frac=0.1, seed=0, labelled=True, max_pos=None):
    """Host bank: xyz f32 [total, 3], modalities f32 [total, C], labels i32 [total] (or None), offsets int64 [n_clouds + 1]."""
    rng = np.random.default_rng(seed)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    total = int(off[-1])
    xyz = rng.random((total, 3), dtype=np.float32)
    mods = rng.standard_normal((total, C)).astype(np.float32)
    labels = None
    if labelled:
        labels = np.zeros(total, np.int32)
        for c, n in enumerate(sizes):
            k = int(n * pos_frac) if max_pos is None else min(int(n * pos_frac), max_pos)
            labels[off[c] + rng.choice(n, k, replace=False)] = rng.integers(1, 4, k)
    return xyz, mods, labels, off


def _positives(labels, off):
    if labels is None:
        return np.zeros(len(off) - 1, np.int64)
    return np.array([(labels[off[c]:off[c + 1]] > 0).sum() for c in range(len(off) - 1)], np.int64)


class Dev:
    """A host bank uploaded once."""

    def __init__(self, xyz, mods, labels, off):
        import torch
        self.xyz, self.mods, self.labels, self.off = xyz, mods, labels, off
        self.d_xyz = torch.from_numpy(xyz).cuda()
        self.d_mods = torch.from_numpy(mods).cuda()
        self.d_lab = torch.from_numpy(labels).cuda() if labels is not None else None
        self.pos = _positives(labels, off)
        self.C = mods.shape[1]


def _outputs(B, N, C, fill=0, pad=0):
    import torch
    mk = lambda n, dt: torch.full((n + pad,), fill, dtype=dt, device="cuda")  # noqa: E731
    return mk(B * N * 3, torch.float32), mk(B * N * (3 + C), torch.float32), mk(B * N, torch.int32), mk(B * N, torch.int32)


def _call(dev, ids, N, seed, outs=None, ctx=None, pos=None, labels="bank", C=None, off=None, n_clouds=None, B=None):
    from point_unet_amd import _lib, runtime
    C = dev.C if C is None else C
    ids = np.asarray(ids, np.int32)
    B = len(ids) if B is None else B
    outs = outs if outs is not None else _outputs(len(ids), N, dev.C)
    off = dev.off if off is None else off
    pos = dev.pos if pos is None else pos
    lab = dev.d_lab if labels == "bank" else labels
    ctx = ctx or runtime.default_context(0)
    o = (ctypes.c_int64 * len(off))(*[int(v) for v in off])
    p = (ctypes.c_int64 * len(pos))(*[int(v) for v in pos])
    cid = (ctypes.c_int32 * max(len(ids), 1))(*ids.tolist())
    rc = _lib.lib().ps_cloud_sample(ctx.handle, runtime.ptr(dev.d_xyz), runtime.ptr(dev.d_mods), C, runtime.ptr(lab), o,
                                    len(off) - 1 if n_clouds is None else n_clouds, p, cid, B, N, seed & 0xFFFFFFFF, *[runtime.ptr(t) for t in outs])
    return rc, outs


def _host(outs, B, N, C):
    x, f, lab, idx = [t.cpu().numpy() for t in outs]
    return x[:B * N * 3].reshape(B, N, 3), f[:B * N * (3 + C)].reshape(B, N, 3 + C), lab[:B * N].reshape(B, N), idx[:B * N].reshape(B, N)


def _expect_equal(dev, ids, N, seed, labels="bank", ctx=None):
    import torch
    from point_unet_amd import _lib
    rc, outs = _call(dev, ids, N, seed, labels=labels, ctx=ctx)
    assert rc == 0, _lib.lib().ps_last_error()
    torch.cuda.synchronize()
    got = _host(outs, len(ids), N, dev.C)
    want = ref.sample(dev.xyz, dev.mods, dev.labels if labels == "bank" else None, dev.off, dev.pos, list(ids), N, seed)
    for name, g, w in zip(("xyz", "features", "labels", "idx"), got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w), (name, ids, N, seed)
    return got


def test_edge_sizes_exact():
    """n = N (a pure permutation), n = N + 1, N = 1; all-positive with |P| = N; no positives; labels = NULL."""
    dev = Dev(*_bank([5000, 5001, 3000], pos_frac=0.05, seed=1))
    _expect_equal(dev, [0], 5000, 11)              # n = N
    _expect_equal(dev, [1], 5000, 12)              # n = N + 1
    _expect_equal(dev, [2], 150, 13)               # N = |P| of cloud 2 (150 positives): no background at all
    nopos = Dev(*_bank([4000, 2500], pos_frac=0.0, seed=2))
    _expect_equal(nopos, [1, 0], 1, 14)             # N = 1, no positives
    _expect_equal(nopos, [0, 1], 2500, 15)
    allpos = Dev(*_bank([3000, 777], pos_frac=1.0, seed=3))
    _expect_equal(allpos, [1], 777, 16)             # every point positive, |P| = N = n
    unl = Dev(*_bank([6000, 4321], seed=4, labelled=False))
    _expect_equal(unl, [1, 0, 1], 4321, 17, labels=None)  # labels NULL: a uniform N-subset, labels written as zeros
    # the same rows with labels passed as NULL: the all-background rule on a labelled bank
    lab = Dev(*_bank([6000], seed=5))
    rc, outs = _call(lab, [0], 2000, 18, labels=None, pos=np.zeros(1, np.int64))
    assert rc == 0
    got = _host(outs, 1, 2000, 4)
    want = ref.sample(lab.xyz, lab.mods, None, lab.off, None, [0], 2000, 18)
    assert all(np.array_equal(g, w) for g, w in zip(got, want))


def test_mixed_bank_out_of_order_and_batch_sizes():
    """Clouds from 1 000 to 300 000 points, sampled out of order with one cloud in two slots; B = 1, 8 and the maximum B."""
    sizes = [1000, 5000, 77777, 300000, 12345, 2048]
    dev = Dev(*_bank(sizes, pos_frac=0.2, seed=6, max_pos=600))
    got = _expect_equal(dev, [3, 1, 3, 0, 4, 2], 1000, 21)
    assert not np.array_equal(got[3][0], got[3][2])  # the same cloud in two slots: two samples
    _expect_equal(dev, [3], 1000, 22)                                  # B = 1
    _expect_equal(dev, [5, 4, 3, 2, 1, 0, 2, 3], 1000, 23)             # B = 8
    ids = np.random.default_rng(0).integers(0, len(sizes), MAX_B)
    _expect_equal(dev, ids, 900, 24)                                   # B = PS_CLOUD_SAMPLE_MAX_B


def test_threshold_neighbourhood_and_the_index_half():
    """The selection hash hash32(i * 2654435761 ^ s) is a bijection of i (odd multiplier, xor, invertible mixer), so within a cloud no two
    keys share their hash half and the threshold never straddles a tie: checked over 2^22 indices for several slot seeds.  The kernels
    are then checked around the closest pair of neighbouring hashes of a 300 000-point cloud (N - 1, N, N + 1 with the pair at the
    threshold), unlabelled and with positives above them."""
    for seed in range(4):
        h = ref.hashes(1 << 22, ref.slot_seeds(seed, seed)[0])
        assert len(np.unique(h)) == len(h)
    n, seed = 300000, 41
    s_sel = ref.slot_seeds(seed, 0)[0]
    k = np.sort(ref.keys(n, s_sel) >> np.uint64(32)).astype(np.int64)
    N = int(np.argmin(np.diff(k)[1000:-1000])) + 1001  # k[N - 1], k[N]: the closest pair of neighbouring hashes
    assert k[N] - k[N - 1] <= 4
    dev = Dev(*_bank([n], seed=7, labelled=False))
    for m in (N - 1, N, N + 1):
        _expect_equal(dev, [0], m, seed, labels=None)
    lab = np.zeros(n, np.int32)
    lab[ref.keys(n, s_sel).argsort()[-500:]] = 2  # 500 positives among the largest selection keys: the background below them is unchanged
    dev2 = Dev(dev.xyz, dev.mods, lab, dev.off)
    _expect_equal(dev2, [0], N + 500, seed)


def test_brats_sized_batches():
    """8 clouds of 1.5 M points with ~90 k positives each at N = 180 000 and ConfigBraTS.num_points = 365 000."""
    dev = Dev(*_bank([1500000] * 8, pos_frac=0.06, seed=8))
    assert 85000 <= dev.pos.min() and dev.pos.max() <= 95000
    for N in (180000, 365000):
        _expect_equal(dev, list(range(8)), N, 31 + N)


def test_argument_errors_leave_the_outputs_untouched():
    import torch
    from point_unet_amd import _lib, runtime
    dev = Dev(*_bank([3000, 2000], pos_frac=0.1, seed=9))
    L = _lib.lib()
    cases = [
        dict(ids=[0], N=3001),                              # N > n
        dict(ids=[0], N=299),                               # positives (300) > N
        dict(ids=[2], N=100),                               # cloud id outside the bank
        dict(ids=[-1], N=100),
        dict(ids=[0], N=100, C=0),                          # C
        dict(ids=[0], N=100, C=17),
        dict(ids=[0], N=0),                                 # N
        dict(ids=[0] * (MAX_B + 1), N=100),                 # B above the stated maximum
        dict(ids=[0], N=100, B=0),
        dict(ids=[0], N=100, n_clouds=0),
        dict(ids=[0], N=100, pos=None),                     # NULL positives with labels
    ]
    for k, cs in enumerate(cases):
        B = max(len(cs["ids"]), 1)
        outs = _outputs(B, max(cs["N"], 1), 4, fill=-7)
        kw = {kk: v for kk, v in cs.items() if kk not in ("ids", "N", "pos")}
        if "pos" in cs:
            from point_unet_amd import _lib as lb
            o = (ctypes.c_int64 * 3)(*dev.off.tolist())
            cid = (ctypes.c_int32 * 1)(0)
            rc = lb.lib().ps_cloud_sample(runtime.default_context(0).handle, runtime.ptr(dev.d_xyz), runtime.ptr(dev.d_mods), 4,
                                          runtime.ptr(dev.d_lab), o, 2, None, cid, 1, cs["N"], 1, *[runtime.ptr(t) for t in outs])
        else:
            rc, _ = _call(dev, cs["ids"], cs["N"], 1, outs=outs, **kw)
        assert rc == PS_EINVAL, (k, rc)
        assert L.ps_last_error().startswith(b"ps_cloud_sample"), (k, L.ps_last_error())
        torch.cuda.synchronize()
        for t in outs:
            assert bool((t == -7).all()), k
    # NULL data pointers
    o = (ctypes.c_int64 * 3)(*dev.off.tolist())
    p = (ctypes.c_int64 * 2)(*dev.pos.tolist())
    cid = (ctypes.c_int32 * 1)(0)
    outs = _outputs(1, 100, 4, fill=-7)
    ptrs = [runtime.ptr(t) for t in outs]
    h = runtime.default_context(0).handle
    assert L.ps_cloud_sample(h, None, runtime.ptr(dev.d_mods), 4, runtime.ptr(dev.d_lab), o, 2, p, cid, 1, 100, 1, *ptrs) == PS_EINVAL
    assert b"NULL" in L.ps_last_error()
    assert L.ps_cloud_sample(h, runtime.ptr(dev.d_xyz), runtime.ptr(dev.d_mods), 4, runtime.ptr(dev.d_lab), o, 2, p, cid, 1, 100, 1, ptrs[0], None,
                             ptrs[2], ptrs[3]) == PS_EINVAL
    torch.cuda.synchronize()
    assert all(bool((t == -7).all()) for t in outs)


def test_stale_positive_count_is_reported_and_stays_inside_the_batch():
    import torch
    from point_unet_amd import _lib, runtime
    L = _lib.lib()
    dev = Dev(*_bank([3000, 2000], pos_frac=0.1, seed=10))  # 300 / 200 positives
    B, N, PAD = 2, 400, 4096
    for deferred in (False, True):
        ctx = runtime.Context(0)
        ctx.use_torch_stream()
        if deferred:
            ctx.set_deferred_checks(True)
        for stale in ([299, 200], [0, 200], [300, 201]):
            outs = _outputs(B, N, 4, fill=-7, pad=PAD)
            rc, _ = _call(dev, [0, 1], N, 3, outs=outs, ctx=ctx, pos=np.array(stale, np.int64))
            if deferred:
                assert rc == 0, L.ps_last_error()
                assert L.ps_synchronize(ctx.handle) == PS_ESTATE
            else:
                assert rc == PS_ESTATE
            assert b"positive" in L.ps_last_error() and b"stale" in L.ps_last_error()
            torch.cuda.synchronize()
            for t in outs:
                assert bool((t[-PAD:] == -7).all())  # nothing past [B, N]
            # the batch was drawn with the device's counts: it is the rule's
            got = _host(outs, B, N, 4)
            want = ref.sample(dev.xyz, dev.mods, dev.labels, dev.off, None, [0, 1], N, 3)
            assert all(np.array_equal(g, w) for g, w in zip(got, want))
        # more positives on the device than N (the host said 0): the first N rows only, never past them
        many = Dev(*_bank([3000], pos_frac=0.5, seed=11))
        outs = _outputs(1, N, 4, fill=-7, pad=PAD)
        rc, _ = _call(many, [0], N, 4, outs=outs, ctx=ctx, pos=np.zeros(1, np.int64))
        if deferred:
            assert rc == 0 and L.ps_synchronize(ctx.handle) == PS_ESTATE
        else:
            assert rc == PS_ESTATE
        torch.cuda.synchronize()
        for t in outs:
            assert bool((t[-PAD:] == -7).all())
        idx = outs[3][:N].cpu().numpy()
        assert len(np.unique(idx)) == N and (many.labels[idx] > 0).all()
        assert L.ps_synchronize(ctx.handle) == 0  # reported once
        ctx.close()


def test_positive_counts_entry():
    from point_unet_amd import _lib, runtime
    sizes = [0, 5000, 1, 70000, 0, 333]
    xyz, mods, labels, off = _bank(sizes, pos_frac=0.3, seed=12)
    labels[off[2]] = 1  # the one-point cloud
    dev = Dev(xyz, mods, labels, off)
    o = (ctypes.c_int64 * len(off))(*off.tolist())
    out = (ctypes.c_int64 * len(sizes))()
    h = runtime.default_context(0).handle
    assert _lib.lib().ps_cloud_positive_counts(h, runtime.ptr(dev.d_lab), o, len(sizes), out) == 0
    assert list(out) == _positives(labels, off).tolist()
    assert _lib.lib().ps_cloud_positive_counts(h, None, o, len(sizes), out) == 0 and list(out) == [0] * len(sizes)
    bad = (ctypes.c_int64 * 3)(0, 10, 5)
    assert _lib.lib().ps_cloud_positive_counts(h, runtime.ptr(dev.d_lab), bad, 2, out) == PS_EINVAL


def test_deterministic_across_calls_contexts_and_streams():
    import torch
    from point_unet_amd import runtime
    dev = Dev(*_bank([40000, 25000, 9000], pos_frac=0.1, seed=13))
    ids, N = [1, 0, 2, 1], 8000
    first = _expect_equal(dev, ids, N, 77)
    for _ in range(3):
        again = _expect_equal(dev, ids, N, 77)
        assert all(np.array_equal(a, b) for a, b in zip(first, again))
    ctx = runtime.Context(0)
    s = torch.cuda.Stream()
    ctx.set_stream(s)
    with torch.cuda.stream(s):
        other = _expect_equal(dev, ids, N, 77, ctx=ctx)
    assert all(np.array_equal(a, b) for a, b in zip(first, other))
    ctx.close()
    diff = _expect_equal(dev, ids, N, 78)
    assert not np.array_equal(first[3], diff[3])


# ---- CloudBank and the consumers of its batches ---------------------------------------------------------------------------------------

def _origins(n, shape, seed):
    """n distinct voxels (x, y, z) of a volume of shape (Z, X, Y), as int32 [n, 3]."""
    Z, X, Y = shape
    flat = np.random.default_rng(seed).choice(X * Y * Z, n, replace=False)
    x, y, z = flat % X, (flat // X) % Y, flat // (X * Y)
    return np.stack([x, y, z], 1).astype(np.int32)


def _host_batch(bank_arrays, ids, N, seed):
    import torch
    xyz, mods, labels, off = bank_arrays
    out = ref.sample(xyz, mods, labels, off, None, list(ids), N, seed)
    return [torch.from_numpy(a).cuda() for a in out]


def test_cloud_bank_matches_the_rule_and_epoch_order():
    import torch
    from point_unet_amd.dataset import CloudBank, batch_seed
    arrays = _bank([7000, 9000, 6000, 8000, 6500], pos_frac=0.1, seed=14)
    xyz, mods, labels, off = arrays
    bank = CloudBank(channels=4)
    for c in range(5):
        r = slice(off[c], off[c + 1])
        src = (xyz[r], mods[r], labels[r]) if c % 2 else (torch.from_numpy(xyz[r]).cuda(), torch.from_numpy(mods[r]).cuda(),
                                                          torch.from_numpy(labels[r]).cuda())
        assert bank.add(*src) == c
    assert len(bank) == 5 and [bank.positives(c) for c in range(5)] == _positives(labels, off).tolist()
    b = bank.sample([3, 1, 3], 5000, seed=9)
    want = _host_batch(arrays, [3, 1, 3], 5000, 9)
    for g, w in zip(b[:4], want):
        assert torch.equal(g, w)
    got = list(bank.epoch_batches(2, 5000, epoch=4, seed=1, rank=1, world=2))
    assert [g.cloud_ids for g in got] == [[2, 3]]  # batches 0 ([0, 1]) and 1 ([2, 3]) of floor(5 / 2) = 2; rank 1 takes batch 1
    assert got[0].seed == batch_seed(1, 4, 1, 1) == ref.batch_seed(1, 4, 1, 1)
    for g, w in zip(got[0][:4], _host_batch(arrays, [2, 3], 5000, got[0].seed)):
        assert torch.equal(g, w)
    got0 = list(bank.epoch_batches(2, 5000, epoch=4, seed=1))
    assert [g.cloud_ids for g in got0] == [[0, 1], [2, 3]]
    bank.synchronize()


def test_bank_batch_trains_infers_and_validates_like_the_host_batch():
    import torch
    import netcase
    from point_unet_amd import metrics, weights
    from point_unet_amd.dataset import CloudBank
    from point_unet_amd.postprocess import point2prod
    from point_unet_amd.pyramid import build_pyramid
    from point_unet_amd.RandLANet import Network
    from point_unet_amd.train import Trainer
    cfg, _, _ = netcase.small_deep(12000, seed=8, B=2)
    cfg.d_out = [16, 32, 64, 32, 16]
    sizes = [20000, 16000, 18000]
    vol = (30, 40, 40)  # (Z, X, Y)
    xyz, mods, labels, off = _bank(sizes, pos_frac=0.15, seed=15)
    labels[labels > 0] = np.minimum(labels[labels > 0], cfg.num_classes - 1)
    origins = [_origins(n, vol, 20 + c) for c, n in enumerate(sizes)]
    for c in range(len(sizes)):  # xyz of the voxel lattice, as volume_to_cloud writes them
        xyz[off[c]:off[c + 1]] = origins[c] / np.array([40, 40, 30], np.float32)
    bank = CloudBank(channels=4)
    for c in range(len(sizes)):
        r = slice(off[c], off[c + 1])
        bank.add(xyz[r], mods[r], labels[r], xyz_origin=origins[c])
    ids, N, seed = [2, 0], 12000, 33
    b = bank.sample(ids, N, seed)
    hx, hf, hl, hi = _host_batch((xyz, mods, labels, off), ids, N, seed)
    assert torch.equal(b.xyz, hx) and torch.equal(b.features, hf) and torch.equal(b.labels, hl) and torch.equal(b.idx, hi)

    params = weights.init_params(cfg, seed=3, randomize_bn=True)
    cw = np.linspace(1.0, 2.0, cfg.num_classes).astype(np.float32)
    res = []
    for bx, bf, bl in ((b.xyz, b.features, b.labels), (hx, hf, hl)):
        with Trainer(cfg, params=params, learning_rate=1e-3, class_weights=cw, keep_prob=1.0) as tr:
            pyr = build_pyramid(bx, cfg)
            loss = tr.train_step(pyr, bf, bl)
            torch.cuda.synchronize()
            res.append((loss.clone(), tr.grad.clone(), tr.flat.clone()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]) and torch.equal(res[0][2], res[1][2])

    net = Network(cfg, params=params)
    outs = []
    for bx, bf, bl, bi in ((b.xyz, b.features, b.labels, b.idx), (hx, hf, hl, hi)):
        pyr = build_pyramid(bx, cfg)
        logits = net.inference({"pyramid": pyr, "features": bf})
        vols = [point2prod(logits[k], bi[k], bank.origin(ids[k]), volume_shape=vol) for k in range(len(ids))]
        scores = metrics.validate(net, [(pyr, bf, bl)])
        torch.cuda.synchronize()
        outs.append((logits.clone(), vols, scores["confusion"].clone()))
    assert torch.equal(outs[0][0], outs[1][0])
    assert all(torch.equal(a, c) for a, c in zip(outs[0][1], outs[1][1]))
    assert torch.equal(outs[0][2], outs[1][2]) and int(outs[0][2].sum()) == len(ids) * N
    # the volume holds the softmax of the sampled points at their voxels: every sampled voxel is non-zero
    k = 0
    o = origins[ids[k]][b.idx[k].cpu().numpy()]
    v = outs[0][1][k].cpu().numpy()
    assert np.allclose(v[o[:, 2], o[:, 1], o[:, 0]].sum(-1), 1.0, atol=1e-5)
    bank.synchronize()


def test_prepared_volume_on_device_feeds_the_bank():
    import os
    import torch
    from point_unet_amd.dataset import CloudBank
    from point_unet_amd.prepare import prepare_brats_volume
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "volume_to_cloud.npz"))
    host = prepare_brats_volume(g["raw"], g["seg"], sub_grid_size=float(g["sub_grid_size"]))
    dev = prepare_brats_volume(g["raw"], g["seg"], sub_grid_size=float(g["sub_grid_size"]), on_device=True)
    for k, v in host.items():
        t = dev[k]
        assert isinstance(t, torch.Tensor) and t.is_cuda, k
        assert np.array_equal(t.cpu().numpy(), v.astype(t.cpu().numpy().dtype)), k
    bank = CloudBank()
    a, b = bank.add_prepared(host), bank.add_prepared(dev)
    N = min(len(host["xyz"]), max(int((host["labels"] > 0).sum()) + 10, len(host["xyz"]) // 2))
    x, y = bank.sample([a], N, 5), bank.sample([b], N, 5)
    assert all(torch.equal(p, q) for p, q in zip(x[:4], y[:4]))
    assert torch.equal(bank.origin(b), torch.from_numpy(host["xyz_origin"]).cuda())
    bank.synchronize()
