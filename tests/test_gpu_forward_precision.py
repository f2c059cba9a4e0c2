"""The point network's forward at PS_PREC_BF16 (include/pointseg_forward_precision.h) on the GPU, against tests/forward_precision_ref.py.

Tight checks are per product or per fused stage, on inputs the test controls: a dense product or a chain layer against the float64 product
of the test's own rounded operands at the project's fp32 dot bar (flip-free: the test rounds the very float32 the kernel reads); a fused
attention stage against model64 at 0.1 dist, dist = max |exact64 - model64| (tests/test_forward_precision_rule.py holds the model's own
float32 noise to 0.025 dist on the same cases and seeds, ref.att_cases; the second-tile walks repeat a small geometry pattern under random
features for that, ref.att_case).  The whole network only gets a bfloat16-class bound, 3 dist: a rounding that flips in a deep level fans out to
every point.
"""
import ctypes

import numpy as np
import pytest

import forward_precision_ref as ref
import netcase
from test_gpu_forward_stages import DOT_BAR, Chain, ChainDesc, _att_run, _net, bind, shape_desc

pytestmark = pytest.mark.gpu

PS_EINVAL = 1
_DOORS = {}


def _doors(dbg):
    """The doors of this module on a handle of their own (prototypes are per handle)."""
    if "h" not in _DOORS:
        c_vp, c_int, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
        h = bind(ctypes.CDLL(dbg._name))
        for name, args in {
            "ps_debug_gemm32": [c_vp, c_int, c_vp, c_int, c_int, c_vp, c_vp, c_int, c_int, c_vp, c_int, c_int, c_vp, c_vp, i64, c_int, c_int, c_vp, c_int],
            "ps_debug_gemm32_plan": [c_vp, c_int, i64, c_int, c_int, ctypes.POINTER(c_int * 4)],
            "ps_debug_chain_plan_prec": [ctypes.POINTER(ChainDesc), c_int, ctypes.POINTER(c_int * 4)],
            "ps_debug_att_form": [c_vp, c_int, c_int, c_int, i64],
            "ps_debug_dense_form": [c_vp, c_int, c_int, i64],
        }.items():
            fn = getattr(h, name)
            fn.restype = c_int
            fn.argtypes = args
        _DOORS["h"] = h
    return _DOORS["h"]


def _lrelu(z):
    return np.where(z >= 0, z, 0.2 * z)


# ---- 1. dense products ----------------------------------------------------------------------------------------------------------------
def _gemm_plan(h, R, cin, cout, split=2):
    from point_unet_amd import runtime
    out = (ctypes.c_int * 4)()
    assert h.ps_debug_gemm32_plan(runtime.default_context(0).handle, split, R, cin, cout, ctypes.byref(out)) == 0
    return tuple(out)  # (rw, cw, sk, pd)


def _dense_check(h, lib, c1, c2, cout, R, seed):
    """Y = lrelu([X1 | X2[g]] . W + b) through the one-plane gemm32b kernels against the float64 product of the rounded operands."""
    import torch
    from point_unet_amd import runtime
    rng = np.random.default_rng(seed)
    cin = c1 + c2
    x1 = (rng.standard_normal((R, c1)) * rng.uniform(0.05, 3.0, (1, c1))).astype(np.float32)
    a = x1
    d_x2 = d_g2 = None
    n2 = 0
    if c2:
        n2 = R // 3 + 2
        x2 = (rng.standard_normal((n2, c2)) * rng.uniform(0.05, 3.0, (1, c2))).astype(np.float32)
        g2 = rng.integers(0, n2, R).astype(np.int32)
        a = np.concatenate([x1, x2[g2]], 1)
        d_x2, d_g2 = torch.from_numpy(x2).cuda(), torch.from_numpy(g2).cuda()
    W = (rng.standard_normal((cin, cout)) / np.sqrt(cin)).astype(np.float32)
    b = rng.standard_normal(cout).astype(np.float32)
    d_x1 = torch.from_numpy(x1).cuda()
    y = torch.full((R + 1, cout + 4), float("nan"), dtype=torch.float32, device="cuda")
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    torch.cuda.synchronize()
    rc = h.ps_debug_gemm32(runtime.default_context(0).handle, 2, p(d_x1), c1, c1, None, p(d_x2), max(c2, 1), c2, p(d_g2), 0, 0, W.ctypes.data,
                           b.ctypes.data, R, cout, 1, p(y), cout + 4)
    assert rc == 0, lib.ps_last_error()
    torch.cuda.synchronize()
    got = y.cpu().numpy()
    assert np.isnan(got[R]).all() and np.isnan(got[:, cout:]).all(), "wrote outside its rows"
    got = got[:R, :cout].astype(np.float64)
    ar, Wr, b64 = ref.rb(a).astype(np.float64), ref.rb(W).astype(np.float64), b.astype(np.float64)
    want = _lrelu(ar @ Wr + b64)
    bar = DOT_BAR * (np.abs(ar) @ np.abs(Wr) + np.abs(b64))
    ratio = float((np.abs(got - want) / bar).max())
    exact = _lrelu(a.astype(np.float64) @ W.astype(np.float64) + b64)
    rel = float(np.abs(got - exact).max() / np.abs(exact).max())
    print("DENSE %d+%d -> %d R %d plan %s: error / bar %.3f, vs the unrounded product %.2e" % (c1, c2, cout, R, _gemm_plan(h, R, cin, cout), ratio, rel))
    assert ratio <= 1.0, (c1, c2, cout, R, ratio)
    assert 1e-5 < rel < 3e-2, "it IS a bfloat16 product: %.3e" % rel


@pytest.mark.parametrize("shape", [(32, 0, 32), (64, 0, 128), (32, 128, 32), (1536, 0, 512), (80, 0, 64)])
def test_dense_products_on_one_plane(lib, dbg, shape):
    """(cin, cout) = (32, 32), (64, 128), (160, 32) from two sources with a gather, (1536, 512), and (80, 64) -- a K axis of five chunks, a
    tail of the ring of four: R = 1, 33 and the smallest R of every further launch form (tile shape, K split) the plan door reports."""
    h = _doors(dbg)
    c1, c2, cout = shape
    sizes, seen = [1, 33], {_gemm_plan(h, 1, c1 + c2, cout), _gemm_plan(h, 33, c1 + c2, cout)}
    for R in (257, 1025, 1600, 3100, 8200, 32768):
        pl = _gemm_plan(h, R, c1 + c2, cout)
        if pl not in seen:
            seen.add(pl)
            sizes.append(R)
    assert len({pl[2] for pl in seen}) >= (2 if c1 + c2 >= 1024 else 1), seen  # split-K and not, where the plan has both
    assert all(pl[3] == 4 for pl in seen)  # the one-plane ring
    for R in sizes:
        _dense_check(h, lib, c1, c2, cout, R, seed=R + cout)


def _chain_input(ch):
    a = ch.x1[:, :ch.c1]
    if ch.c2:
        a = np.concatenate([a, ch.x2[:, :ch.c2]], 1)
    return a.astype(np.float64)


def _teacher_forced(ch, got, what):
    """Layer l of a run with every layer stored against rb(stored a_{l-1}) . rb(W_l) + b_l in float64 where the rule rounds the layer, and
    against the unrounded operands where it does not; returns the worst error / bar."""
    worst = 0.0
    prev = _chain_input(ch)
    for i, (cin, cout, leaky) in enumerate(ch.layers):
        a = prev
        if i in ch.ex:
            a = np.concatenate([a, ch.ex[i].astype(np.float64)], 1)
        W, b = ch.W[i].astype(np.float64), ch.b[i].astype(np.float64)
        if ref.dense_rounded(cin):
            a, W = ref.rb(a), ref.rb(W)
        want = a @ W + b
        if leaky:
            want = _lrelu(want)
        bar = DOT_BAR * (np.abs(a) @ np.abs(W) + np.abs(b))
        ratio = float((np.abs(got[i].astype(np.float64) - want) / bar).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, "%s layer %d (rounded %d): error is %.3g of the bar" % (what, i, ref.dense_rounded(cin), ratio)
        if ref.dense_rounded(cin) and a.shape[0] > 8:  # ... and it IS the rounded product
            exact = prev if i not in ch.ex else np.concatenate([prev, ch.ex[i].astype(np.float64)], 1)
            exact = exact @ ch.W[i].astype(np.float64) + b
            exact = _lrelu(exact) if leaky else exact
            assert np.abs(got[i] - exact).max() > 1e-5 * np.abs(exact).max()
        prev = got[i].astype(np.float64)
    return worst


def test_dense_fallback_kernels_round_on_load(lib, dbg):
    """Shapes the 32x32 tiles do not take (cout % 32 != 0), layer by layer through rowgemm at PS_PREC_BF16 (ps_debug_chain form 7): the
    direct-load kernel on aligned rows, the generic LDS kernel on a row stride of 65 floats; and rowchain_kernel (form 6) on the same."""
    h = _doors(dbg)
    for ld1 in (None, 65):
        for R in (1, 77):
            ch = Chain([(64, 48, 1), (48, 24, 0)], 64, R=R, seed=R, ld1=ld1)
            for form in (7, 6, 4):
                w = _teacher_forced(ch, ch.run(h, lib, form), "form %d" % form)
                print("FALLBACK ld1 %s R %d form %d: worst error / bar = %.3f" % (ld1, R, form, w))


# ---- 2. chains ------------------------------------------------------------------------------------------------------------------------
_CHAINS = {
    "RcPair1": ([(32, 32, 1), (32, 64, 0)], 32, 0, None),
    "RcPair1b": ([(64, 32, 1), (32, 64, 0)], 64, 0, None),
    "RcEnc1": ([(64, 64, 1), (96, 128, 1)], 64, 0, {1: 32}),
    "RcPair2": ([(128, 64, 1), (64, 128, 0)], 128, 0, None),
    "RcHead-4": ([(64, 32, 1), (32, 64, 1), (64, 32, 1), (32, 4, 0)], 32, 32, None),
}


def _plan_prec(h, d, prec=2):
    out = (ctypes.c_int * 4)()
    assert h.ps_debug_chain_plan_prec(ctypes.byref(d), prec, ctypes.byref(out)) == 0
    return tuple(out)


@pytest.mark.parametrize("name", list(_CHAINS))
def test_compiled_chains_on_one_plane(lib, dbg, name):
    """The level-1 chains, level 2's pair and the head on regchain's one-plane policy (form 5), every layer stored and teacher-forced; a
    second run that keeps the middles in registers gives the same last layer; the dispatch (form 4) takes the same kernel.  R = 1 and just
    past one tile per wave of the largest launch (eight waves of 16 rows per workgroup)."""
    h = _doors(dbg)
    layers, c1, c2, extras = _CHAINS[name]
    cap = _plan_prec(h, shape_desc([(a, b) for a, b, _ in layers], c1, c2, R=1 << 22, extras=extras))
    assert cap[0] == 3, cap
    assert _plan_prec(h, shape_desc([(a, b) for a, b, _ in layers], c1, c2, R=1 << 22, extras=extras), 1)[0] == 1
    big = cap[1] * 128 + 5
    assert big <= 66000
    last = len(layers) - 1
    for R in (1, big):
        ch = Chain(layers, c1, c2, R=R, extras=extras, seed=R)
        full = ch.run(h, lib, 5)
        w = _teacher_forced(ch, full, name)
        lean = ch.run(h, lib, 5, store=[last])
        assert np.array_equal(lean[last], full[last]), "the stored middles changed the last layer"
        disp = ch.run(h, lib, 4, store=[last])
        assert np.array_equal(disp[last], full[last]), "rowchain() at PS_PREC_BF16 did not take the one-plane chain kernel"
        d = ChainDesc.from_buffer_copy(ch.desc)
        p = _plan_prec(h, d)
        assert p[0] == 3 and (R == 1 or p[1] * 128 < R), p
        print("CHAIN %s R %d: worst error / bar = %.3f, %d workgroups, %d bytes of LDS" % (name, R, w, p[1], p[2]))


def test_a_chain_that_mixes_rounded_and_unrounded_layers(lib, dbg):
    """K = 16 then K = 32: the rule rounds the second layer only; regchain refuses the chain (form 5), the dispatch takes rowchain_kernel."""
    h = _doors(dbg)
    for R in (1, 333):
        ch = Chain([(16, 32, 1), (32, 64, 0)], 16, R=R, seed=R)
        for form in (4, 6, 7):
            _teacher_forced(ch, ch.run(h, lib, form), "mixed, form %d" % form)
        ch.run(h, lib, 5, expect=PS_EINVAL)
        assert _plan_prec(h, ChainDesc.from_buffer_copy(ch.desc))[0] == 2


# ---- 3. attention stages, form 5 --------------------------------------------------------------------------------------------------------
RATIOS = {}


_SEEDS = {c[:5]: c[5:] for c in ref.att_cases()}


def _att_check5(h, lib, d, K, stage, B, n_cloud, seed=None, orders=(False,), net=None, params=None):
    import torch
    period = 0
    if net is None:
        net, params = _net(d, K)
        seed, period = _SEEDS[(d, K, stage, B, n_cloud)]  # the case as the CPU test checked it
    xyz, idx, fg, exact64, model64, model32 = ref.att_case(params, d, K, stage, B, n_cloud, seed, period)
    dev = tuple(torch.from_numpy(v).cuda() for v in (xyz, idx, fg))
    n_total = B * n_cloud
    dist = float(np.abs(exact64 - model64).max())
    flip = float(np.abs(model32.astype(np.float64) - model64).max())
    one = n_total == 1 and stage == 1
    assert flip <= 0.025 * dist or one, "the reference's own noise %.3e is above 0.025 dist = %.3e" % (flip, 0.025 * dist)
    # (stage 1 of ONE point: K equal rows, a uniform softmax, dist = 0 exactly -- what is left is the fp32 error of the unrounded arithmetic)
    bar = 0.1 * dist if not one else ref.FP32_FLOOR * float(np.abs(exact64).max())
    for with_order in orders:
        order = None
        if with_order:
            rng = np.random.default_rng(seed + 1)
            order = torch.from_numpy(np.concatenate([rng.permutation(n_cloud) for _ in range(B)]).astype(np.int32)).cuda()
        got = _att_run(h, lib, net, d, stage, 5, dev, n_total, n_cloud, order)  # (checks the NaN guard row and that the output is finite)
        err = float(np.abs(got.astype(np.float64) - model64).max())
        ratio = err / bar
        RATIOS[(d, K, stage)] = max(RATIOS.get((d, K, stage), 0.0), ratio)
        print("ATT5 d %d K %d stage %d n %d x %d order %d: |agg - model64| %.3e = %.3f dist, dist %.3e, flip %.3e, error / bar %.3f"
              % (d, K, stage, B, n_cloud, with_order, err, err / max(dist, 1e-30), dist, flip, ratio))
        if not one:  # ... and the stage IS rounded: an unrounded one misses model64 by dist
            assert float(np.abs(got.astype(np.float64) - exact64).max()) >= 0.5 * dist
        assert err <= bar, "d %d K %d stage %d n %d x %d: %.3e above the bar %.3e (dist %.3e)" % (d, K, stage, B, n_cloud, err, bar, dist)


@pytest.mark.parametrize("k_n", [16, 32])
@pytest.mark.parametrize("d", [64, 128, 256, 512])
def test_attention_stage_on_one_plane_small_levels(lib, dbg, d, k_n):
    h = _doors(dbg)
    for stage in (1, 2):
        for B, n_cloud in ref.SMALL_LEVELS:
            _att_check5(h, lib, d, k_n, stage, B, n_cloud, orders=(False, True))
        print("ATT5 RATIO d %d K %d stage %d: largest error / bar = %.3f" % (d, k_n, stage, RATIOS[(d, k_n, stage)]))


@pytest.mark.parametrize("d", [64, 128, 256, 512])
def test_attention_on_one_plane_second_tile_k32(lib, dbg, d):
    h = _doors(dbg)
    for stage in (1, 2):
        _att_check5(h, lib, d, 32, stage, 1, 4133)


@pytest.mark.parametrize("d", [64, 256])
def test_attention_on_one_plane_second_tile_k16(lib, dbg, d):
    h = _doors(dbg)
    for stage in (1, 2):
        _att_check5(h, lib, d, 16, stage, 1, 8267, orders=(True,))


def test_attention_with_one_live_mlp2_column(lib, dbg):
    """LFA mlp2 zero except one output column, stage 2: every other column of f_xyz2 is lrelu(bias); the stage still meets its bar and
    writes nothing outside its block (the guard row and the finite check of _att_run)."""
    from point_unet_amd import weights
    from point_unet_amd.RandLANet import Network
    h = _doors(dbg)
    for d, K in ((64, 16), (256, 32)):
        cfg = ref.OneLevel(d, K)
        params = dict(weights.init_params(cfg, seed=d + K, randomize_bn=True))
        w = np.zeros_like(params["Encoder_layer_0LFAmlp2/weights"])
        w[:, 5] = params["Encoder_layer_0LFAmlp2/weights"][:, 5]
        params["Encoder_layer_0LFAmlp2/weights"] = w
        net = Network(cfg, params=params)
        _att_check5(h, lib, d, K, 2, 3, 37, seed=5, orders=(False, True), net=net, params=params)
        net.close()


def test_form_5_refuses_a_narrow_level(lib, dbg):
    import torch
    h = _doors(dbg)
    net, params = _net(16, 16)
    rng = np.random.default_rng(1)
    dev = (torch.from_numpy(rng.random((9, 3), dtype=np.float32)).cuda(), torch.from_numpy(rng.integers(0, 9, (9, 16)).astype(np.int32)).cuda(),
           torch.from_numpy(rng.standard_normal((9, 8)).astype(np.float32)).cuda())
    _att_run(h, lib, net, 16, 1, 5, dev, 9, 9, None, expect=PS_EINVAL)


# ---- 4. dispatch ------------------------------------------------------------------------------------------------------------------------
def test_dispatch_at_bf16_on_the_brats_widths(lib, dbg):
    from point_unet_amd import weights
    from point_unet_amd.RandLANet import Network
    h = _doors(dbg)
    cfg = netcase.make_cfg(5, (16, 64, 128, 256, 512), (4, 4, 4, 4, 2), 16, 4, 7)
    params = weights.init_params(cfg, seed=1)
    net = Network(cfg, params=params, precision="bf16")
    n = [18000, 4500, 1125, 281, 70]
    for level in range(5):
        for stage in (1, 2):
            assert h.ps_debug_att_form(net._h, level, stage, 16, n[level]) == (5 if level else 4), (level, stage)
    # the network's own dense layers through rowgemm's dispatch: the one-plane gemm32b (5) wherever the 32x32 tiles take the layer
    dense = [(w, lv, n[lv]) for lv in (2, 3, 4) for w in (0, 1, 2)] + [(3, 0, 35)] + [(4, j, n[4 - j]) for j in range(4)]
    assert [h.ps_debug_dense_form(net._h, w, lv, R) for w, lv, R in dense] == [5] * len(dense)
    assert h.ps_debug_dense_form(net._h, 2, 0, n[0]) == 3  # level 0's [mlp2 ; shortcut] (K = 24, not rounded): the 16x16 kernels
    net.set_precision("bf16x3")
    assert [h.ps_debug_att_form(net._h, level, 1, 16, n[level]) for level in range(5)] == [4, 1, 1, 1, 1]
    assert all(h.ps_debug_dense_form(net._h, w, lv, R) in (1, 2) for w, lv, R in dense)
    net.close()
    # the chains: level 0's stay on the fp32 / split policies (form 1), level 1's and the head go to the one-plane policy (form 3)
    for layers, c1, c2, extras, form in (([(7, 8), (8, 8)], 7, 0, None, 1), ([(16, 16), (24, 32)], 16, 0, {1: 8}, 1), ([(16, 8)], 16, 0, None, 1),
                                         ([(32, 32), (32, 64)], 32, 0, None, 3), ([(64, 32), (32, 64)], 64, 0, None, 3),
                                         ([(64, 64), (96, 128)], 64, 0, {1: 32}, 3), ([(128, 64), (64, 128)], 128, 0, None, 3),
                                         ([(64, 32), (32, 64), (64, 32), (32, 4)], 32, 32, None, 3)):
        assert _plan_prec(h, shape_desc(layers, c1, c2, R=18000, extras=extras))[0] == form, layers
    # the dense layers of the deep levels and the decoder: the plan of the split form with the one-plane ring
    for R, cin, cout in ((1125, 256, 256), (281, 512, 512), (70, 1024, 1024), (140, 1536, 512), (1125, 384, 128)):
        p1, p3 = _gemm_plan(h, R, cin, cout, 2), _gemm_plan(h, R, cin, cout, 1)
        assert p1[:3] == p3[:3] and p1[3] == 4, (p1, p3)


# ---- 5. the whole network ---------------------------------------------------------------------------------------------------------------
_CASES = {}


def _case(oracle, which):
    """Inputs, the oracle's index pyramid, exact64 and dist of one whole-network case; computed once."""
    from oracle import randla_oracle as ro
    from point_unet_amd import weights
    if which not in _CASES:
        if which == "two":
            cfg, n0 = netcase.make_cfg(2, (16, 64), (4, 4), 16, 4, 7), 2400
        else:
            cfg, n0 = netcase.make_cfg(5, (16, 64, 128, 256, 512), (4, 4, 4, 4, 2), 16, 4, 7), 18000
        clouds = []
        for b in range(2):
            rng = np.random.default_rng(11 + b)
            xyz = rng.random((1, n0, 3), dtype=np.float32)
            feats = np.concatenate([xyz, rng.standard_normal((1, n0, 4)).astype(np.float32)], -1)
            pyr = ro.build_pyramid(lambda s, q, k: oracle.knn_batch(s, q, k), xyz, cfg.k_n, cfg.sub_sampling_ratio)
            clouds.append((xyz, feats, pyr))
        params = weights.init_params(cfg, seed=6, randomize_bn=True)
        xyz, feats, (pts, nbr, pool, up) = clouds[0]
        exact64 = ro.inference(params, cfg.num_layers, pts, nbr, pool, up, feats, np.float64)
        model64 = ref.inference(cfg, params, pts, nbr, pool, up, feats, np.float64)
        _CASES[which] = dict(cfg=cfg, params=params, clouds=clouds, exact64=exact64, dist=float(np.abs(exact64 - model64).max()))
    return _CASES[which]


def _forward(net, clouds):
    """The network on the oracle's own index lists (one cloud, or a batch of them)."""
    import torch
    cat = lambda k, i: torch.from_numpy(np.ascontiguousarray(np.concatenate([c[2][k][i] for c in clouds], 0))).cuda()  # noqa: E731
    L = len(clouds[0][2][0])
    inputs = {"xyz": [cat(0, i).float() for i in range(L)], "neigh_idx": [cat(1, i) for i in range(L)], "sub_idx": [cat(2, i) for i in range(L)],
              "interp_idx": [cat(3, i) for i in range(L)], "features": torch.from_numpy(np.concatenate([c[1] for c in clouds], 0)).cuda()}
    return net.inference(inputs)


@pytest.mark.parametrize("which", ["two", "five"])
def test_whole_network_at_bf16(oracle, lib, which):
    import torch
    from point_unet_amd.RandLANet import Network
    c = _case(oracle, which)
    net = Network(c["cfg"], params=c["params"], precision="bf16")
    plain = Network(c["cfg"], params=c["params"])
    assert net.precision == "bf16" and plain.precision == "bf16x3"
    one = c["clouds"][:1]
    a = _forward(net, one)
    b = _forward(net, one)
    assert torch.equal(a, b), "two forwards differ"
    err = float(np.abs(a.cpu().numpy().astype(np.float64) - c["exact64"]).max())
    mag = float(np.abs(c["exact64"]).max())
    print("NET %s: |logits - exact64| %.3e, dist %.3e (%.2f %% of the largest logit), error / dist %.3f" % (which, err, c["dist"], 100 * c["dist"] / mag, err / c["dist"]))
    assert err <= 3 * c["dist"], (err, c["dist"])
    assert err > 1e-5 * mag  # it IS the bfloat16 forward
    want = _forward(plain, one)
    agree = float((a.argmax(-1) == want.argmax(-1)).float().mean())
    print("NET %s: argmax agreement with the default precision %.4f" % (which, agree))
    both = _forward(net, c["clouds"])  # B = 2 is two B = 1 forwards (at these sizes no layer's K split changes with the doubled row count)
    assert torch.equal(both[0], a[0]) and torch.equal(both[1], _forward(net, c["clouds"][1:])[0])
    net.set_precision("bf16x3")
    assert net.precision == "bf16x3"
    assert torch.equal(_forward(net, one), want), "back at the default precision the bytes are not the default's"
    net.close()
    plain.close()


# ---- 6. the surface -------------------------------------------------------------------------------------------------------------------
def test_precision_surface(oracle, lib):
    import torch
    from oracle import randla_oracle as ro
    from point_unet_amd import _lib, weights
    from point_unet_amd.RandLANet import Network
    from point_unet_amd.pipeline import ForwardPipeline
    from point_unet_amd.pyramid import build_pyramid
    c = _case(oracle, "two")
    cfg = c["cfg"]
    with pytest.raises(ValueError):
        Network(cfg, params=c["params"], precision="fp32")
    net = Network(cfg, params=c["params"])
    with pytest.raises(ValueError):
        net.set_precision("bf16x2")
    with pytest.raises(ValueError):
        ForwardPipeline(cfg, params=c["params"], lanes=1, precision="fp16")
    for bad in (_lib.PS_PREC_FP32, 7):
        assert lib.ps_randla_set_precision(net._h, bad) == PS_EINVAL
        assert b"ps_set_att_bf16x3" in lib.ps_last_error()
        assert net.precision == "bf16x3"
    v = ctypes.c_int32(0)
    for name, val in (("bf16", _lib.PS_PREC_BF16), ("bf16x3", _lib.PS_PREC_BF16X3), ("bf16", _lib.PS_PREC_BF16)):
        net.set_precision(name)
        assert lib.ps_randla_get_precision(net._h, ctypes.byref(v)) == 0 and v.value == val and net.precision == name
    # new weights after set_precision("bf16"): the one-plane images are packed again, from the new blob
    one = c["clouds"][:1]
    first = _forward(net, one)
    params2 = weights.init_params(cfg, seed=9, randomize_bn=True)
    net.set_params(params2)
    assert net.precision == "bf16"
    xyz, feats, (pts, nbr, pool, up) = one[0]
    exact2 = ro.inference(params2, cfg.num_layers, pts, nbr, pool, up, feats, np.float64)
    dist2 = float(np.abs(exact2 - ref.inference(cfg, params2, pts, nbr, pool, up, feats, np.float64)).max())
    got2 = _forward(net, one)
    assert not torch.equal(got2, first)
    assert float(np.abs(got2.cpu().numpy() - exact2).max()) <= 3 * dist2
    # every lane of a pipeline runs at the pipeline's precision
    net.set_params(c["params"])
    x, f = torch.from_numpy(xyz).cuda(), torch.from_numpy(feats).cuda()
    want = net.inference({"pyramid": build_pyramid(x, cfg), "features": f})
    pipe = ForwardPipeline(cfg, params=c["params"], lanes=2, precision="bf16")
    assert all(ln.net.precision == "bf16" for ln in pipe.lanes)
    got = [pipe.submit(x, f) for _ in range(3)]
    pipe.synchronize()
    assert all(torch.equal(g, want) for g in got)
    pipe.close()
    net.set_precision("bf16x3")
    assert not torch.equal(net.inference({"pyramid": build_pyramid(x, cfg), "features": f}), want)
    net.close()
