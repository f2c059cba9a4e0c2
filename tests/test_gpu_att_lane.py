"""Level-0 attention on the vector ALU (csrc/attpool_lane.hip: att_lane_kernel, one lane per neighbour row) against the kernel it replaces.

att_lane_kernel runs att_direct_kernel's arithmetic in the same order (k-ordered fma chains for the three products, the softmax's four
in-order partial sums combined as (0 + 1) + (2 + 3)), so form 4 of ps_debug_att_stage must equal form 3 BIT FOR BIT at d = 16, K = 16; the
float64 bar is form 3's own, _att_bar(3, 16) of tests/test_gpu_forward_stages.py.  Outputs cannot show which kernel ran: ps_debug_att_form
tells which form att_pool_stage takes.
"""
import contextlib
import ctypes

import numpy as np
import pytest

import netcase
from test_gpu_forward_stages import PS_EINVAL, _att_bar, _att_case, _att_run, _net, bind

pytestmark = pytest.mark.gpu

# level sizes: 1 .. 5 trailing groups of every length (a wave iteration takes four points); 7, 8, 9 XCDs with no point or one point (the
# walk gives each of the 8 XCDs a contiguous share rounded up to whole groups); 31, 33, 64, 65, 67 several groups, whole and partial;
# 3 x 37: cloud bases, and groups of four that straddle a cloud boundary in the walk
SIZES = [(1, n) for n in (1, 2, 3, 4, 5, 7, 8, 9, 31, 33, 64, 65, 67)] + [(3, 37)]


def _bind(dbg):
    bind(dbg)
    dbg.ps_debug_att_form.restype = ctypes.c_int
    dbg.ps_debug_att_form.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int64]
    dbg.ps_debug_att_lane_pass_points.restype = ctypes.c_int
    dbg.ps_debug_att_lane_pass_points.argtypes = []
    dbg.ps_debug_set_att_lane.restype = ctypes.c_int
    dbg.ps_debug_set_att_lane.argtypes = [ctypes.c_void_p, ctypes.c_int]
    return dbg


@contextlib.contextmanager
def _lane_context(dbg, on):
    """A fresh runtime.Context on torch's current device and stream with the att_lane switch set through ps_debug_set_att_lane; closed on
    exit.  The session's shared context keeps the shipped value."""
    import torch
    from point_unet_amd import runtime
    ctx = runtime.Context(torch.cuda.current_device())
    try:
        ctx.use_torch_stream()
        assert dbg.ps_debug_set_att_lane(ctx.handle, int(on)) == 0
        yield ctx
    finally:
        torch.cuda.synchronize()
        ctx.close()


def _orders(B, n_cloud, seed):
    import torch
    rng = np.random.default_rng(seed + 1)
    return (None, torch.from_numpy(np.concatenate([rng.permutation(n_cloud) for _ in range(B)]).astype(np.int32)).cuda())


def _lane_against_direct_and_float64(dbg, lib, stage, B, n_cloud, seed):
    """Form 4 equals form 3 bit for bit and holds form 3's float64 bar, with order = NULL and with a random per-cloud permutation; the NaN row
    behind n_total stays NaN (_att_run).  _att_case's tables hold repeated indices (every fourth row) and, being random within the cloud,
    the point itself (always at n_cloud = 1, in most rows of the small levels, in a dozen rows of the largest): zero distance."""
    import torch
    net, params = _net(16, 16)
    xyz, idx, fg, want = _att_case(params, 16, 16, stage, B, n_cloud, seed)
    dev = tuple(torch.from_numpy(v).cuda() for v in (xyz, idx, fg))
    n_total = B * n_cloud
    for order in _orders(B, n_cloud, seed):
        lane = _att_run(dbg, lib, net, 16, stage, 4, dev, n_total, n_cloud, order)
        direct = _att_run(dbg, lib, net, 16, stage, 3, dev, n_total, n_cloud, order)
        assert np.array_equal(lane.view(np.uint32), direct.view(np.uint32)), "stage %d, %d x %d: %d elements differ, max |d| %.3e" % (
            stage, B, n_cloud, int((lane.view(np.uint32) != direct.view(np.uint32)).sum()), float(np.abs(lane - direct).max()))
        err = float(np.abs(lane.astype(np.float64) - want).max()) / float(np.abs(want).max())
        print("ATTLANE stage %d n %d x %d order %d: %.3e" % (stage, B, n_cloud, order is not None, err))
        assert err <= _att_bar(3, 16), (stage, B, n_cloud, err)


@pytest.mark.parametrize("stage", [1, 2])
def test_lane_kernel_equals_the_direct_kernel_bit_for_bit_on_small_levels(lib, dbg, stage):
    _bind(dbg)
    for B, n_cloud in SIZES:
        _lane_against_direct_and_float64(dbg, lib, stage, B, n_cloud, seed=300 * stage + n_cloud)


@pytest.mark.parametrize("stage", [1, 2])
def test_lane_kernel_second_group_per_wave(lib, dbg, stage):
    """One pass of the largest grid covers ps_debug_att_lane_pass_points points (workgroups x waves x 4); 37 more make some waves walk to a
    second group, the last of them partial."""
    _bind(dbg)
    n = dbg.ps_debug_att_lane_pass_points() + 37
    assert 30000 < n < 40000, n
    _lane_against_direct_and_float64(dbg, lib, stage, 1, n, seed=500 + stage)


@pytest.mark.parametrize("stage", [1, 2])
def test_lane_kernel_leaves_rows_it_does_not_own_alone(lib, dbg, stage):
    """5 and 9 points with eight NaN rows behind them in agg: the partial last group stores nothing for the points it does not have."""
    import torch
    _bind(dbg)
    net, params = _net(16, 16)
    for n in (5, 9):
        xyz, idx, fg, _ = _att_case(params, 16, 16, stage, 1, n, seed=40 + n)
        dev = tuple(torch.from_numpy(v).cuda() for v in (xyz, idx, fg))
        agg = torch.full((n + 8, 16), float("nan"), dtype=torch.float32, device="cuda")
        p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
        torch.cuda.synchronize()
        assert dbg.ps_debug_att_stage(net._h, 0, stage, 4, p(dev[0]), p(dev[1]), None, p(dev[2]), n, n, p(agg)) == 0, lib.ps_last_error()
        torch.cuda.synchronize()
        h = agg.cpu().numpy()
        assert np.isfinite(h[:n]).all() and np.isnan(h[n:]).all()


def test_routing_of_the_lane_kernel(lib, dbg):
    """att_pool_stage takes the lane kernel (form 4) for level 0 of the shipped widths at K = 16 with the context's att_lane switch on, and the direct
    kernel (form 3) with the switch off, at K = 32 and at d_out[0] = 32; called directly the lane kernel refuses d = 32 and K = 32."""
    import torch
    from point_unet_amd import weights
    from point_unet_amd.RandLANet import Network
    _bind(dbg)
    cfg, _, _ = netcase.small_deep(4000)
    params = weights.init_params(cfg, seed=2, randomize_bn=True)
    net = Network(cfg, params=params)
    for stage in (1, 2):
        assert dbg.ps_debug_att_form(net._h, 0, stage, 16, 45056) == 4
        assert dbg.ps_debug_att_form(net._h, 0, stage, 32, 45056) == 3
    with _lane_context(dbg, 0) as ctx:
        off = Network(cfg, params=params, ctx=ctx)
        for stage in (1, 2):
            assert dbg.ps_debug_att_form(off._h, 0, stage, 16, 45056) == 3
        del off
    for d, k_n in ((32, 16), (16, 32)):
        other, oparams = _net(d, k_n)
        xyz, idx, fg, _ = _att_case(oparams, d, k_n, 1, 1, 9, seed=1)
        dev = tuple(torch.from_numpy(v).cuda() for v in (xyz, idx, fg))
        for stage in (1, 2):
            assert dbg.ps_debug_att_form(other._h, 0, stage, k_n, 9) == 3
            _att_run(dbg, lib, other, d, stage, 4, dev, 9, 9, None, expect=PS_EINVAL)


def test_whole_forward_is_bit_identical_with_the_switch_on_and_off(dbg):
    """Five levels, 4 000 points: the logits with level 0 on the lane kernel equal the logits with it on att_direct_kernel, bit for bit."""
    import torch
    from point_unet_amd import weights
    from point_unet_amd.RandLANet import Network
    from point_unet_amd.pyramid import build_pyramid
    cfg, xyz, feats = netcase.small_deep(4000)
    params = weights.init_params(cfg, seed=2, randomize_bn=True)
    _bind(dbg)
    out = []
    for on in (1, 0):
        with _lane_context(dbg, on) as ctx:
            net = Network(cfg, params=params, ctx=ctx)
            pyr = build_pyramid(torch.from_numpy(xyz).cuda(), cfg, ctx=ctx)
            out.append(net.inference({"pyramid": pyr, "features": torch.from_numpy(feats).cuda()}).cpu().numpy())
            del net, pyr
    assert np.isfinite(out[0]).all()
    assert np.array_equal(out[0].view(np.uint32), out[1].view(np.uint32)), float(np.abs(out[0] - out[1]).max())
