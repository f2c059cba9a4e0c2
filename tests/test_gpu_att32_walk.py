"""The wave-major tile walk of the d >= 64 attention kernels (csrc/att32_tile_walk.h) and att32b_kernel's raw-buffer gathers and batched
weight staging (csrc/attpool32b.hip), through ps_debug_att_stage form 1 on one-level networks with random weights (d = 64: the width of
encoder level 1, d = 128: level 2; K = 16).

A launch is at most 256 workgroups of WAVES waves (16 / 12 at d = 64 stage 1 / 2, 8 at d = 128), a tile is two points: a wave only takes a
second tile past 256 x WAVES tiles, so the smallest levels that reach the changed deal are 8 209 points (d = 64, stage 1: 4 105 tiles > 4 096),
6 161 (stage 2: 3 081 > 3 072) and 4 111 (d = 128: 2 056 > 2 048) -- odd, so the last tile is partial.  Each runs as one cloud and as two
clouds of half the size, rounded up (4 105 / 3 081 points are odd: a tile straddles the two clouds), in storage order and in a random
per-cloud order.  The bar is form 1's own float64 bar of tests/test_gpu_forward_stages.py (_att_bar).  The existing tests assert no bit
equality between forms 1 and 2 (only errs[1] <= 2 errs[2] + 2e-6, _att_check's rule, applied here too), so none is asserted here.
"""
import ctypes

import numpy as np
import pytest

from test_gpu_forward_stages import _att_bar, _att_case, _net, bind

pytestmark = pytest.mark.gpu

GUARD = 3  # NaN rows in front of and behind agg

# (d, stage) -> the smallest level whose launch gives some waves a second tile
SECOND_TILE = {(64, 1): 8209, (64, 2): 6161, (128, 1): 4111, (128, 2): 4111}
CASES = sorted(SECOND_TILE)


def _orders(B, n_cloud, seed):
    import torch
    rng = np.random.default_rng(seed + 1)
    return (None, torch.from_numpy(np.concatenate([rng.permutation(n_cloud) for _ in range(B)]).astype(np.int32)).cuda())


def _run_guarded(dbg, lib, net, d, stage, form, dev, n_total, n_cloud, order):
    """agg with GUARD NaN rows on both sides: the stage must leave them NaN and fill every row between."""
    import torch
    d_xyz, d_idx, d_fg = dev
    buf = torch.full((n_total + 2 * GUARD, d), float("nan"), dtype=torch.float32, device="cuda")
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731
    torch.cuda.synchronize()
    rc = dbg.ps_debug_att_stage(net._h, 0, stage, form, p(d_xyz), p(d_idx), p(order), p(d_fg), n_total, n_cloud, ctypes.c_void_p(buf[GUARD:].data_ptr()))
    assert rc == 0, (rc, lib.ps_last_error())
    torch.cuda.synchronize()
    h = buf.cpu().numpy()
    assert np.isnan(h[:GUARD]).all(), "form %d wrote in front of the first point" % form
    assert np.isnan(h[GUARD + n_total:]).all(), "form %d wrote behind the last point" % form
    assert np.isfinite(h[GUARD:GUARD + n_total]).all()
    return h[GUARD:GUARD + n_total]


def _against_float64(dbg, lib, d, stage, B, n_cloud, seed, forms=(1,)):
    """Every form inside its own bar, in storage order and in a random per-cloud order; with forms 1 and 2 also the rule the existing tests
    hold the pair to (_att_check): errs[1] <= 2 errs[2] + 2e-6.  One float64 reference per case."""
    import torch
    net, params = _net(d, 16)
    xyz, idx, fg, want = _att_case(params, d, 16, stage, B, n_cloud, seed)
    dev = tuple(torch.from_numpy(v).cuda() for v in (xyz, idx, fg))
    mag = float(np.abs(want).max())
    errs = {}
    for order in _orders(B, n_cloud, seed):
        for form in forms:
            got = _run_guarded(dbg, lib, net, d, stage, form, dev, B * n_cloud, n_cloud, order)
            err = float(np.abs(got.astype(np.float64) - want).max()) / mag
            print("ATT32WALK form %d d %d stage %d n %d x %d order %d: %.3e (bar %.3e)" % (form, d, stage, B, n_cloud, order is not None, err, _att_bar(form, d)))
            assert err <= _att_bar(form, d), (form, d, stage, B, n_cloud, err)
            errs[form] = max(errs.get(form, 0.0), err)
    if 1 in errs and 2 in errs:
        assert errs[1] <= 2 * errs[2] + 2e-6, errs


@pytest.mark.parametrize("d,stage", CASES)
def test_second_tile_of_the_wave_major_walk_one_cloud(lib, dbg, d, stage):
    """Form 1 and, on the same level, the fp32 kernel (form 2), which shares the walk."""
    bind(dbg)
    _against_float64(dbg, lib, d, stage, 1, SECOND_TILE[(d, stage)], seed=900 + d + stage, forms=(1, 2))


@pytest.mark.parametrize("d,stage", CASES)
def test_second_tile_of_the_wave_major_walk_two_clouds(lib, dbg, d, stage):
    bind(dbg)
    _against_float64(dbg, lib, d, stage, 2, (SECOND_TILE[(d, stage)] + 1) // 2, seed=950 + d + stage)


@pytest.mark.parametrize("d,stage", CASES)
def test_a_cloud_alone_and_as_both_halves_of_a_batch_is_bit_equal(lib, dbg, d, stage):
    """The batch of two reaches the second tile per wave, the cloud alone does not, and in the batch the rows of the second copy land on other
    waves and other XCDs than those of the first: all three sets of rows must be the same bits."""
    import torch
    bind(dbg)
    n = (SECOND_TILE[(d, stage)] + 1) // 2
    net, params = _net(d, 16)
    xyz, idx, fg, _ = _att_case(params, d, 16, stage, 1, n, seed=970 + d + stage)
    one = tuple(torch.from_numpy(v).cuda() for v in (xyz, idx, fg))
    two = tuple(torch.from_numpy(np.concatenate([v, v])).cuda() for v in (xyz, idx, fg))
    for o1, o2 in zip(_orders(1, n, 5), (None, torch.cat([_orders(1, n, 5)[1]] * 2))):
        alone = _run_guarded(dbg, lib, net, d, stage, 1, one, n, n, o1).view(np.uint32)
        both = _run_guarded(dbg, lib, net, d, stage, 1, two, 2 * n, n, o2).view(np.uint32)
        for half in (both[:n], both[n:]):
            assert np.array_equal(alone, half), "d %d stage %d order %d: %d elements differ" % (d, stage, o1 is not None, int((alone != half).sum()))


@pytest.mark.parametrize("d", [64, 128])
def test_degenerate_grids(lib, dbg, d):
    """1, 2 and 67 points: XCDs without a tile, one partial tile, fewer tiles than waves in a workgroup."""
    bind(dbg)
    for stage in (1, 2):
        for n in (1, 2, 67):
            _against_float64(dbg, lib, d, stage, 1, n, seed=800 + 10 * stage + n)


def test_device_split_equals_the_host_pieces_bit_for_bit(lib, dbg):
    """b3_split8 on the device (ps_debug_pack_b3_device: the training step's packing kernel, accumulator K order) against b3_piece_of on the
    host (ps_debug_pack_b3, the same K order): the three bfloat16 planes of every element, over the magnitudes a weight or an activation
    takes -- zeros, powers of two, values whose second or third piece is zero, both signs."""
    import torch
    from point_unet_amd import runtime
    dbg.ps_debug_pack_b3_device.restype = ctypes.c_int
    dbg.ps_debug_pack_b3_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    cin, cout = 64, 96
    rng = np.random.default_rng(11)
    W = (rng.standard_normal((cin, cout)) * np.exp2(rng.integers(-40, 40, (cin, cout)))).astype(np.float32)
    W[0, :7] = [0.0, -0.0, 1.0, -1.0, 2.0 ** -126, 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -16]
    W[1, :4] = [3.0e38, -3.0e38, 1.0 + 2.0 ** -23, 0.2]
    nq, ncb = cin // 16, cout // 32
    host = np.zeros(ncb * nq * 3 * 64 * 8, np.uint16)
    assert dbg.ps_debug_pack_b3(W.ctypes.data, cin, cout, host.ctypes.data) == 0
    d_w = torch.from_numpy(W).cuda()
    d_out = torch.zeros(nq * ncb * 3 * 64 * 8, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    assert dbg.ps_debug_pack_b3_device(runtime.default_context(0).handle, d_w.data_ptr(), cin, cout, d_out.data_ptr()) == 0, lib.ps_last_error()
    torch.cuda.synchronize()
    dev = d_out.cpu().numpy().view(np.uint16).reshape(nq, ncb, 3, 64, 8).transpose(1, 0, 2, 3, 4)
    host = host.reshape(ncb, nq, 3, 64, 8)
    assert np.array_equal(dev, host), "%d pieces differ" % int((dev != host).sum())
    # the pieces are what they claim: three bfloat16 that add up to the weight exactly
    parts = (host.astype(np.uint32) << 16).view(np.float32).astype(np.float64).sum(axis=2)
    assert np.array_equal(np.sort(parts.reshape(-1)), np.sort(W.astype(np.float64).reshape(-1)))
