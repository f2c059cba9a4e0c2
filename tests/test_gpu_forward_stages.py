"""The inference forward's layer chains and fused attention stages, each form on its own against float64 NumPy.

Chains (csrc/regchain.hip, rowchain_kernel and the 16x16x4 rowgemm kernels of csrc/rowgemm.hip) run through the test-only door
ps_debug_chain, which packs weights as ps_randla_set_weights does; ps_debug_chain_plan tells which kernel rowchain() takes and how many
workgroups it launches, so the tests assert the path they mean and size R just past "one tile per wave" from the launch itself.  The bar
per output element is the forward-error recurrence  E_0 = 0,  E_l = E_{l-1} . |W_l| + 2e-6 (|a_{l-1}| . |W_l| + |b_l|)  over the float64
activations a: 2e-6 is the fp32-MFMA dot-product bar of tests/test_gpu_shapes.py, LeakyReLU (slope <= 1) does not enlarge it.

Attention stages (csrc/attpool.hip, attpool32.hip, attpool32b.hip) run through ps_debug_att_stage on one-level networks, i.e. on the
product's own packed images, against relative_pos_encoding -> conv2d [-> conv2d] -> gather -> concat -> dense -> softmax -> weighted sum
of oracle/randla_oracle.py in float64.  Forms: 0 = att_pool_stage (the product's dispatch), 1 = split-bf16 32x32, 2 = fp32 32x32,
3 = the 16x16x4 kernels (att_direct_kernel at d <= 32, att_kernel above).

Measured on an MI355X, max |agg - ref| / max |ref| over every attention case of this module (both K, both stages, all sizes):

    form                         d = 16     32        64        128       256       512
    0  att_pool_stage            2.00e-7   3.25e-7   2.43e-7   2.43e-7   2.08e-7   2.22e-7
    1  split-bf16 32x32             -         -      2.43e-7   3.00e-7   2.09e-7   2.22e-7
    2  fp32 32x32                   -         -      2.43e-7   2.27e-7   2.12e-7   2.12e-7
    3  16x16x4                   2.00e-7   3.25e-7   2.86e-7   4.77e-7   9.10e-7   1.06e-6

(form 3 is att_direct_kernel at d <= 32 -- the kernel form 0 dispatches to there -- and att_kernel from d = 64, whose softmax is __expf on
unscaled scores and whose K axis runs in 16x16x4 steps; at d = 256 the wave-split launch measured 8.5e-7 at 500 points and 8.2e-7 at
4 133 (a second point per workgroup), the general one 9.1e-7 at 16 387.)  MEASURED_ATT_ERR holds these figures; each form's bar is 4 x its figure (_att_bar), all below 4 x 2e-6, the bar of the
fused fp32 training attention (tests/test_gpu_train.py).
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PS_EINVAL = 1
DOT_BAR = 2e-6  # fp32-MFMA dot product against float64, relative to |x| . |w| + |b| (tests/test_gpu_shapes.py)

# max |agg - ref| / max |ref| per (form, d), the largest figure over all attention cases of this module (both K, both stages, all sizes)
MEASURED_ATT_ERR = {
    (0, 16): 2.00e-7, (3, 16): 2.00e-7,
    (0, 32): 3.25e-7, (3, 32): 3.25e-7,
    (0, 64): 2.43e-7, (1, 64): 2.43e-7, (2, 64): 2.43e-7, (3, 64): 2.86e-7,
    (0, 128): 2.43e-7, (1, 128): 3.00e-7, (2, 128): 2.27e-7, (3, 128): 4.77e-7,
    (0, 256): 2.08e-7, (1, 256): 2.09e-7, (2, 256): 2.12e-7, (3, 256): 9.10e-7,
    (0, 512): 2.22e-7, (1, 512): 2.22e-7, (2, 512): 2.12e-7, (3, 512): 1.06e-6,
}


def _att_bar(form, d):
    return 4.0 * MEASURED_ATT_ERR[(form, d)]


# ---- the doors (csrc/debug_hooks.h) ------------------------------------------------------------------------------------------------
class ChainLayer(ctypes.Structure):
    _fields_ = [("W", ctypes.c_void_p), ("bias", ctypes.c_void_p), ("cin", ctypes.c_int), ("cout", ctypes.c_int), ("leaky", ctypes.c_int),
                ("y", ctypes.c_void_p), ("ldy", ctypes.c_int), ("extra", ctypes.c_void_p), ("ld_extra", ctypes.c_int), ("c_extra", ctypes.c_int),
                ("extra_gather", ctypes.c_void_p)]


class ChainDesc(ctypes.Structure):
    _fields_ = [("n_layers", ctypes.c_int), ("layer", ChainLayer * 4),
                ("x1", ctypes.c_void_p), ("g1", ctypes.c_void_p), ("ld1", ctypes.c_int), ("c1", ctypes.c_int), ("g1m", ctypes.c_int), ("g1n", ctypes.c_int),
                ("x2", ctypes.c_void_p), ("g2", ctypes.c_void_p), ("ld2", ctypes.c_int), ("c2", ctypes.c_int), ("g2m", ctypes.c_int), ("g2n", ctypes.c_int),
                ("R", ctypes.c_int64)]


def bind(dbg):
    """ctypes prototypes of the doors this module (and tests/test_chain_plan.py) uses."""
    c_vp, c_int, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    for name, args in {
        "ps_debug_chain": [c_vp, ctypes.POINTER(ChainDesc), c_int],
        "ps_debug_chain_plan": [ctypes.POINTER(ChainDesc), ctypes.POINTER(c_int * 4)],
        "ps_debug_att_stage": [c_vp, c_int, c_int, c_int, c_vp, c_vp, c_vp, c_vp, i64, i64, c_vp],
    }.items():
        fn = getattr(dbg, name)
        fn.restype = c_int
        fn.argtypes = args
    return dbg


def shape_desc(layers, c1, c2=0, R=1, ld1=None, ld2=None, extras=None):
    """A description carrying channel counts only (what the plan door reads).  layers: [(cin, cout)], extras: {layer: channels}."""
    d = ChainDesc()
    d.n_layers = len(layers)
    for i, (cin, cout) in enumerate(layers):
        d.layer[i].cin, d.layer[i].cout = cin, cout
        if extras and i in extras:
            d.layer[i].extra, d.layer[i].ld_extra, d.layer[i].c_extra = 16, extras[i], extras[i]  # (an aligned, never-read address)
    d.x1, d.ld1, d.c1 = 16, ld1 or c1, c1
    if c2:
        d.x2, d.ld2, d.c2 = 16, ld2 or c2, c2
    d.R = R
    return d


def plan(dbg, d):
    out = (ctypes.c_int * 4)()
    assert dbg.ps_debug_chain_plan(ctypes.byref(d), ctypes.byref(out)) == 0
    return tuple(out)  # (form, workgroups, lds bytes, fast_in)


# ---- chains ------------------------------------------------------------------------------------------------------------------------
def _lrelu(z):
    return np.where(z >= 0, z, 0.2 * z)


class Chain:
    """One chain with its random inputs, the float64 activations and the error bar of every layer.
    layers: [(cin, cout, leaky)]; extras: {layer: channels}; gather: {1 or 2: (n_src, gm, gn)} (gm == 0: one index table over n_src rows)."""

    def __init__(self, layers, c1, c2=0, R=1, extras=None, gather=None, seed=0, ld1=None, ld2=None, offset1=0):
        import torch
        rng = np.random.default_rng(seed)
        self.layers, self.c1, self.c2, self.R = layers, c1, c2, R
        self.extras, self.gather = extras or {}, gather or {}
        self.ld1, self.ld2, self.offset1 = ld1 or c1, ld2 or max(c2, 1), offset1

        def rows(n, c):
            return (rng.standard_normal((n, c)) * rng.uniform(0.05, 3.0, (1, c))).astype(np.float32)

        def source(which, c, ld):
            g = None
            n = R
            if which in self.gather:
                n_src, gm, gn = self.gather[which]
                if gm:  # batched: row r reads (r // gm) * gn + g[r]
                    g = rng.integers(0, gn, R).astype(np.int32)
                    n = -(-R // gm) * gn
                    take = (np.arange(R) // gm) * gn + g
                else:
                    g = rng.integers(0, n_src, R).astype(np.int32)
                    n, take = n_src, g
            else:
                take = np.arange(R)
            x = np.full((n, ld), np.nan, np.float32)  # (the padding columns of a row are never read)
            x[:, :c] = rows(n, c)
            return x, g, x[take, :c].astype(np.float64)

        self.x1, self.g1, a1 = source(1, c1, self.ld1)
        a = a1
        if c2:
            self.x2, self.g2, a2 = source(2, c2, self.ld2)
            a = np.concatenate([a1, a2], 1)
        else:
            self.x2 = self.g2 = None
        self.W, self.b, self.ex, self.want, self.bar = [], [], {}, [], []
        E = np.zeros_like(a)
        for i, (cin, cout, leaky) in enumerate(layers):
            if i in self.extras:
                ex = rows(R, self.extras[i])
                self.ex[i] = ex
                a = np.concatenate([a, ex.astype(np.float64)], 1)
                E = np.concatenate([E, np.zeros(ex.shape)], 1)
            W = (rng.standard_normal((cin, cout)) / np.sqrt(cin)).astype(np.float32)
            b = rng.standard_normal(cout).astype(np.float32)
            self.W.append(W)
            self.b.append(b)
            if a.shape[1] == cin:  # (a mismatched chain has no reference: the refusal tests)
                aW = np.abs(W.astype(np.float64))
                E = E @ aW + DOT_BAR * (np.abs(a) @ aW + np.abs(b.astype(np.float64)))
                a = a @ W.astype(np.float64) + b.astype(np.float64)
                if leaky:
                    a = _lrelu(a)
            self.want.append(a)
            self.bar.append(E)
        # device copies, made once
        dev = lambda v: None if v is None else torch.from_numpy(v).cuda()  # noqa: E731
        if offset1:  # the same rows behind a base pointer moved by `offset1` floats
            flat = torch.empty(self.x1.size + offset1, dtype=torch.float32, device="cuda")
            flat[offset1:] = torch.from_numpy(self.x1).cuda().reshape(-1)
            self.d_x1 = flat[offset1:]
        else:
            self.d_x1 = dev(self.x1)
        self.d_x2, self.d_g1, self.d_g2 = dev(self.x2), dev(self.g1), dev(self.g2)
        self.d_ex = {i: dev(v) for i, v in self.ex.items()}

    def run(self, dbg, lib, form, store=None, pad=4, gather_extra=False, expect=0):
        """Runs the chain; `store`: the layers whose rows are stored (default: all).  Returns {layer: rows} after checking that the
        padding columns and the extra row of every output buffer are still NaN.  A refused run (expect != 0) must leave the buffers all NaN."""
        import torch
        from point_unet_amd import runtime
        store = range(len(self.layers)) if store is None else store
        p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        d = ChainDesc()
        d.n_layers = len(self.layers)
        outs = {}
        keep = []
        for i, (cin, cout, leaky) in enumerate(self.layers):
            y = d.layer[i]
            y.W, y.bias = self.W[i].ctypes.data, self.b[i].ctypes.data
            y.cin, y.cout, y.leaky = cin, cout, leaky
            if i in store:
                outs[i] = torch.full((self.R + 1, cout + pad), float("nan"), dtype=torch.float32, device="cuda")
                y.y, y.ldy = outs[i].data_ptr(), cout + pad
            if i in self.d_ex:
                y.extra, y.ld_extra, y.c_extra = self.d_ex[i].data_ptr(), self.extras[i], self.extras[i]
                if gather_extra:
                    keep.append(torch.zeros(self.R, dtype=torch.int32, device="cuda"))
                    y.extra_gather = keep[-1].data_ptr()
        d.x1, d.g1, d.ld1, d.c1 = p(self.d_x1), p(self.d_g1), self.ld1, self.c1
        if 1 in self.gather:
            d.g1m, d.g1n = self.gather[1][1], self.gather[1][2]
        if self.c2:
            d.x2, d.g2, d.ld2, d.c2 = p(self.d_x2), p(self.d_g2), self.ld2, self.c2
            if 2 in self.gather:
                d.g2m, d.g2n = self.gather[2][1], self.gather[2][2]
        d.R = self.R
        self.desc = d
        torch.cuda.synchronize()
        rc = dbg.ps_debug_chain(runtime.default_context(0).handle, ctypes.byref(d), form)
        assert rc == expect, (rc, lib.ps_last_error())
        torch.cuda.synchronize()
        if expect:
            assert len(lib.ps_last_error()) > 0
            assert all(bool(torch.isnan(t).all()) for t in outs.values()), "a refused chain wrote rows"
            return None
        got = {}
        for i, t in outs.items():
            h = t.cpu().numpy()
            cout = self.layers[i][1]
            assert np.isnan(h[:, cout:]).all() and np.isnan(h[self.R]).all(), "form %d layer %d wrote outside its rows" % (form, i)
            got[i] = h[:self.R, :cout]
        return got

    def check(self, got, form):
        worst = 0.0
        for i, h in got.items():
            assert np.isfinite(h).all(), (form, i)
            ratio = float((np.abs(h.astype(np.float64) - self.want[i]) / self.bar[i]).max())
            worst = max(worst, ratio)
            assert ratio <= 1.0, "form %d layer %d: error is %.3g of the bar" % (form, i, ratio)
        return worst

    def plan(self, dbg, R=None):
        """The launch of rowchain() for this chain (needs a run() first: the description with its pointers)."""
        d = ChainDesc.from_buffer_copy(self.desc)
        if R:
            d.R = R
        return plan(dbg, d)


# the network's channel counts per compiled chain shape (csrc/regchain.hip): (layers, c1, c2, extras)
_RC_SHAPES = {
    "RcFc0-in4": ([(4, 8, 1), (8, 8, 1)], 4, 0, None),
    "RcFc0-in7": ([(7, 8, 1), (8, 8, 1)], 7, 0, None),
    "RcOne0": ([(16, 8, 1)], 16, 0, None),
    "RcEnc0": ([(16, 16, 1), (24, 32, 1)], 16, 0, {1: 8}),
    "RcPair1": ([(32, 32, 1), (32, 64, 0)], 32, 0, None),
    "RcPair1b": ([(64, 32, 1), (32, 64, 0)], 64, 0, None),
    "RcEnc1": ([(64, 64, 1), (96, 128, 1)], 64, 0, {1: 32}),
    "RcPair2": ([(128, 64, 1), (64, 128, 0)], 128, 0, None),
    "RcHead-2": ([(64, 32, 1), (32, 64, 1), (64, 32, 1), (32, 2, 0)], 32, 32, None),
    "RcHead-4": ([(64, 32, 1), (32, 64, 1), (64, 32, 1), (32, 4, 0)], 32, 32, None),
    "RcHead-13": ([(64, 32, 1), (32, 64, 1), (64, 32, 1), (32, 13, 0)], 32, 32, None),
}


def _within_lds_form(layers):
    return all(cin <= 96 and cout <= 96 for cin, cout, _ in layers)


@pytest.mark.parametrize("name", list(_RC_SHAPES))
def test_compiled_chain_shapes_in_every_form(lib, dbg, name):
    """Each RcShape at the network's channel counts: rowchain() as the network calls it (cached image), regchain re-ordering the image in
    the kernel (bit-identical: the same kernel), the LDS-staged kernel where the channels allow it and the per-layer kernels, all inside
    the bar; R around one tile, a few tiles, and just past one tile per wave of the largest launch (the next-tile prefetch loop)."""
    bind(dbg)
    layers, c1, c2, extras = _RC_SHAPES[name]
    cap = plan(dbg, shape_desc([(a, b) for a, b, _ in layers], c1, c2, R=1 << 22, extras=extras))
    assert cap[0] == 1, cap
    sizes = [1, 15, 16, 17, 4 * 16 * 3 + 5, cap[1] * 64 + 5]
    assert sizes[-1] <= 66000
    for R in sizes:
        ch = Chain(layers, c1, c2, R=R, extras=extras, seed=R)
        big = R == sizes[-1]
        got = {}
        for form in (0, 1) if big else (0, 1, 2, 3):
            if form == 2 and not _within_lds_form(layers):
                ch.run(dbg, lib, 2, expect=PS_EINVAL)
                continue
            got[form] = ch.run(dbg, lib, form)
            worst = ch.check(got[form], form)
            print("%s R %d form %d: worst error / bar = %.3f" % (name, R, form, worst))
        p = ch.plan(dbg)
        assert p[0] == 1 and (not big or p[1] * 64 < R), p
        for i in got[0]:
            assert np.array_equal(got[0][i], got[1][i]), "layer %d: the cached image and the in-kernel re-ordering differ" % i


@pytest.mark.parametrize("store_middle", [True, False])
def test_head_chain_with_the_decoder_sources(lib, dbg, store_middle):
    """RcHead as the network feeds it: [skip | up[interp]] with the batched gather over B = 3 clouds of an odd size; the middle layers'
    rows stored (the tap mode) or kept in registers."""
    bind(dbg)
    n0, n1 = 333, 83
    layers = _RC_SHAPES["RcHead-4"][0]
    ch = Chain(layers, 32, 32, R=3 * n0, gather={2: (0, n0, n1)}, seed=5)
    ref = None
    for form in (0, 1, 2, 3):
        got = ch.run(dbg, lib, form, store=None if store_middle else [3])
        ch.check(got, form)
        assert sorted(got) == ([0, 1, 2, 3] if store_middle else [3])
        if form == 0:
            ref = got
        if form == 1:
            assert all(np.array_equal(ref[i], got[i]) for i in got)
    assert ch.plan(dbg)[0] == 1


_LDS_CASES = {
    # name: (layers, c1, c2, extras, gather, ld1, offset1, expected fast_in)
    "d_out0=32 ladder": ([(32, 32, 1), (40, 64, 1)], 32, 0, {1: 8}, None, None, 0, 3),
    "20 inputs: scalar staging": ([(20, 16, 1), (16, 8, 0)], 20, 0, None, None, None, 0, 0),
    "32 inputs, aligned: float4 staging": ([(32, 24, 1), (24, 16, 0)], 32, 0, None, None, None, 0, 3),
    "32 inputs, base off by one float": ([(32, 24, 1), (24, 16, 0)], 32, 0, None, None, None, 1, 0),
    "32 inputs, row stride 33": ([(32, 24, 1), (24, 16, 0)], 32, 0, None, None, 33, 0, 0),
    "cout 6: zero padding of the K axis": ([(8, 6, 1), (6, 16, 1), (16, 7, 0)], 8, 0, None, None, None, 0, 1),
    "gathered first source": ([(20, 16, 1), (16, 8, 0)], 20, 0, None, {1: (57, 0, 0)}, None, 0, 0),
    "two sources, batched gathers": ([(48, 32, 1), (32, 12, 0)], 32, 16, None, {1: (0, 67, 23), 2: (0, 67, 9)}, None, 0, 0),
}


@pytest.mark.parametrize("name", list(_LDS_CASES))
def test_chains_outside_the_compiled_shapes_take_the_lds_kernel(lib, dbg, name):
    """Chains that are not one of regchain's shapes: rowchain() must take rowchain_kernel (asserted through the plan door, with the input
    staging it chooses), and agree with float64 and with the per-layer kernels; R from one row to past the kernel's own workgroup cap."""
    bind(dbg)
    layers, c1, c2, extras, gather, ld1, offset1, fast_in = _LDS_CASES[name]
    cap = plan(dbg, shape_desc([(a, b) for a, b, _ in layers], c1, c2, R=1 << 22, extras=extras))
    assert cap[0] == 2, cap
    for R in (1, 17, 4 * 16 * 3 + 5, cap[1] * 64 + 5):
        g = gather
        if gather and R > 67 * 3:  # (the batched tables keep B = 3 clouds)
            g = {k: ((v[0], 0, 0) if not v[1] else (0, -(-R // 3), v[2])) for k, v in gather.items()}
        ch = Chain(layers, c1, c2, R=R, extras=extras, gather=g, seed=R, ld1=ld1, offset1=offset1)
        for form in (0, 2, 3):
            worst = ch.check(ch.run(dbg, lib, form), form)
            print("%s R %d form %d: worst error / bar = %.3f" % (name, R, form, worst))
        ch.run(dbg, lib, 1, expect=PS_EINVAL)
        p = ch.plan(dbg)
        assert p[0] == 2 and p[3] == fast_in, p
        if R > 1000:
            assert p[1] * 64 < R, p


@pytest.mark.parametrize("aligned", [True, False])
def test_single_decoder_layer_with_two_sources_and_a_batched_gather(lib, dbg, aligned):
    """[skip | up[g]] -> 32 at widths too small for gemm32, through rowgemm: 16-byte aligned rows take the direct-load kernel, a row stride of
    33 floats the generic LDS kernel (rowgemm's `direct` predicate; the door packs no 32x32 image, so gemm32 never takes the layer); the same
    layer as a one-step chain takes rowchain_kernel."""
    bind(dbg)
    n0, n1 = 301, 75
    ch = Chain([(64, 32, 1)], 32, 32, R=3 * n0, gather={2: (0, n0, n1)}, seed=9, ld1=32 if aligned else 33, ld2=32 if aligned else 35)
    for form in (3, 0, 2):
        ch.check(ch.run(dbg, lib, form), form)
    assert ch.plan(dbg)[0] == 2


def test_chain_refusals(lib, dbg):
    """A chain no form can run returns PS_EINVAL with a message and writes nothing."""
    bind(dbg)
    wide = Chain([(100, 16, 1), (16, 8, 0)], 100, R=40)  # above kChainMaxC = 96
    for form in (0, 1, 2):
        wide.run(dbg, lib, form, expect=PS_EINVAL)
    assert wide.plan(dbg)[0] == 0
    ex = Chain([(16, 16, 1), (24, 32, 1)], 16, R=40, extras={1: 8})
    for form in (0, 1, 2, 3):
        ex.run(dbg, lib, form, gather_extra=True, expect=PS_EINVAL)
    ex.check(ex.run(dbg, lib, 0), 0)  # (the same chain with plain extra rows runs)
    mismatch = Chain([(16, 16, 1), (20, 32, 1)], 16, R=40)  # the second layer expects 20 channels, the first gives 16
    for form in (0, 1, 2, 3):
        mismatch.run(dbg, lib, form, expect=PS_EINVAL)


# ---- attention stages ----------------------------------------------------------------------------------------------------------------
class _OneLevel:
    num_layers, num_classes, in_channels = 1, 4, 7
    sub_sampling_ratio = [4]

    def __init__(self, d, k_n):
        self.d_out, self.k_n = (d,), k_n


_NETS = {}


def _net(d, k_n):
    """One-level network (and its parameters) per (d, K), shared by the tests of this module."""
    from point_unet_amd import weights
    from point_unet_amd.RandLANet import Network
    if (d, k_n) not in _NETS:
        cfg = _OneLevel(d, k_n)
        params = weights.init_params(cfg, seed=d + k_n, randomize_bn=True)
        _NETS[(d, k_n)] = (Network(cfg, params=params), params)
    return _NETS[(d, k_n)]


def _att_case(params, d, K, stage, B, n_cloud, seed):
    """Inputs of one stage and its float64 result: xyz, idx (random within the cloud, every fourth row with repeated entries), f, and for
    d >= 64 G = f . Wfc[:h] rounded to fp32 -- the reference takes the rounded values."""
    from oracle import randla_oracle as ro
    rng = np.random.default_rng(seed)
    h = d // 2
    xyz = rng.random((B, n_cloud, 3), dtype=np.float32)
    idx = rng.integers(0, n_cloud, (B, n_cloud, K)).astype(np.int32)
    idx[:, ::4, K // 2:] = idx[:, ::4, :K // 2]
    f = rng.standard_normal((B, n_cloud, h)).astype(np.float32)
    name = "Encoder_layer_0LFA"
    Wfc = params[name + "att_pooling_%dfc/kernel" % stage].astype(np.float64)
    dt = np.dtype(np.float64)
    fx = ro.conv2d(ro.relative_pos_encoding(xyz.astype(np.float64), idx), params, name + "mlp1", dt)
    if stage == 2:
        fx = ro.conv2d(fx, params, name + "mlp2", dt)
    fset = np.concatenate([ro.gather_neighbour(f.astype(np.float64), idx), fx], -1)
    if d >= 64:
        G = (f.astype(np.float64) @ Wfc[:h]).astype(np.float32)
        fg = np.concatenate([f, G], -1)
        act = ro.gather_neighbour(G.astype(np.float64), idx) + fx @ Wfc[h:]
    else:
        fg = f
        act = fset @ Wfc
    act = act - act.max(axis=2, keepdims=True)
    e = np.exp(act)
    want = np.sum(fset * (e / e.sum(axis=2, keepdims=True)), axis=2)
    return xyz.reshape(-1, 3), idx.reshape(-1, K), fg.reshape(B * n_cloud, -1), want.reshape(B * n_cloud, d)


def _att_run(dbg, lib, net, d, stage, form, dev, n_total, n_cloud, order, expect=0):
    import torch
    d_xyz, d_idx, d_fg = dev
    agg = torch.full((n_total + 1, d), float("nan"), dtype=torch.float32, device="cuda")
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731
    torch.cuda.synchronize()
    rc = dbg.ps_debug_att_stage(net._h, 0, stage, form, p(d_xyz), p(d_idx), p(order), p(d_fg), n_total, n_cloud, p(agg))
    assert rc == expect, (rc, lib.ps_last_error())
    torch.cuda.synchronize()
    if expect:
        assert len(lib.ps_last_error()) > 0 and bool(torch.isnan(agg).all())
        return None
    h = agg.cpu().numpy()
    assert np.isnan(h[n_total]).all(), "form %d wrote behind the last point" % form
    assert np.isfinite(h[:n_total]).all()
    return h[:n_total]


def _att_check(dbg, lib, d, K, stage, forms, B, n_cloud, seed, orders=(False,)):
    """Runs the forms on one case; returns {form: relative error} after asserting every bar, and the split-bf16 rule of
    test_split_bf16_attention_is_as_accurate_as_the_fp32_mfma when forms 1 and 2 both ran."""
    import torch
    net, params = _net(d, K)
    xyz, idx, fg, want = _att_case(params, d, K, stage, B, n_cloud, seed)
    dev = tuple(torch.from_numpy(v).cuda() for v in (xyz, idx, fg))
    n_total = B * n_cloud
    mag = float(np.abs(want).max())
    errs = {}
    for with_order in orders:
        order = None
        if with_order:
            rng = np.random.default_rng(seed + 1)
            order = torch.from_numpy(np.concatenate([rng.permutation(n_cloud) for _ in range(B)]).astype(np.int32)).cuda()
        for form in forms:
            got = _att_run(dbg, lib, net, d, stage, form, dev, n_total, n_cloud, order)
            err = float(np.abs(got.astype(np.float64) - want).max()) / mag
            print("ATTERR form %d d %d K %d stage %d n %d x %d order %d: %.3e" % (form, d, K, stage, B, n_cloud, with_order, err))
            errs[form] = max(errs.get(form, 0.0), err)
    for form, err in errs.items():
        assert err <= _att_bar(form, d), "form %d d %d K %d stage %d n %d x %d: %.3e above the bar %.3e" % (form, d, K, stage, B, n_cloud, err, _att_bar(form, d))
    if 1 in errs and 2 in errs:
        assert errs[1] <= 2 * errs[2] + 2e-6, errs
    return errs


def _forms(d):
    return (0, 1, 2, 3) if d >= 64 else (0, 3)


@pytest.mark.parametrize("k_n", [16, 32])
@pytest.mark.parametrize("d", [16, 32, 64, 128, 256, 512])
def test_attention_stage_forms_on_small_levels(lib, dbg, d, k_n):
    """Every form, both stages: levels of 1 .. 33 points (a partial last tile, XCDs without points) and B = 3 clouds of 37 points (at K = 16
    a tile of two points straddles two clouds), walked in storage order (order = NULL) and in a random per-cloud permutation."""
    bind(dbg)
    for stage in (1, 2):
        for B, n_cloud in ((1, 1), (1, 3), (1, 9), (1, 33), (3, 37)):
            _att_check(dbg, lib, d, k_n, stage, _forms(d), B, n_cloud, seed=100 * stage + n_cloud, orders=(False, True))


@pytest.mark.parametrize("d", [64, 128, 256, 512])
def test_attention_second_tile_per_wave_k32(lib, dbg, d):
    """K = 32 at 4 133 points: 4 096 workgroups (or waves) of one tile each is the largest launch of the 32x32 kernels, so the last 37
    points are a wave's second tile -- the walk to the next tile with its geometry prefetched (att32_tile_walk.h)."""
    bind(dbg)
    for stage in (1, 2):
        _att_check(dbg, lib, d, 32, stage, (1, 2), 1, 4133, seed=7 + stage)


@pytest.mark.parametrize("d", [64, 256])
def test_attention_second_tile_per_wave_k16(lib, dbg, d):
    """K = 16 (two points per tile) at 8 267 points: 4 134 tiles, the same walk; with a per-cloud order."""
    bind(dbg)
    for stage in (1, 2):
        _att_check(dbg, lib, d, 16, stage, (1, 2), 1, 8267, seed=17 + stage, orders=(True,))


@pytest.mark.parametrize("n_total", [500, 4133, 16387])
def test_pre_product_kernel_both_launch_forms_at_d256(lib, dbg, n_total):
    """att_kernel (attpool.hip), the kernel a level past the 32x32 forms' limits runs: one point per workgroup with the four waves
    splitting the column blocks below 16 384 points (4 096 workgroups at most: at 4 133 points a workgroup walks to a second point), one point
    per wave from there on."""
    bind(dbg)
    for stage in (1, 2):
        _att_check(dbg, lib, 256, 16, stage, (3,), 1, n_total, seed=27 + stage)


def test_attention_forms_refuse_a_level_they_do_not_fit(lib, dbg):
    """The 32x32 forms need d >= 64: asked for a d = 16 level they return PS_EINVAL and leave agg alone."""
    import torch
    bind(dbg)
    net, params = _net(16, 16)
    xyz, idx, fg, _ = _att_case(params, 16, 16, 1, 1, 9, seed=1)
    dev = tuple(torch.from_numpy(v).cuda() for v in (xyz, idx, fg))
    for form in (1, 2):
        _att_run(dbg, lib, net, 16, 1, form, dev, 9, 9, None, expect=PS_EINVAL)
