"""The register-resident layer chains on the split-bf16 matrix pipe (csrc/regchain.hip, policy RcB3: v_mfma_f32_16x16x32_bf16 over exact
three-way bfloat16 splits of weights and activations, six piece products, fp32 accumulate).

The chains run through ps_debug_chain as in tests/test_gpu_forward_stages.py, whose Chain / bars / shape table this module imports; the
policy is a switch of the context (on by default), set through the test door ps_debug_set_regchain_b3 and put back on the way out of
every `with policy(...)` block, passing or failing, because the context is the session's shared one.  The bar stays DOT_BAR = 2e-6 of |x| . |w| + |b| per layer, propagated through the
layers: the split is exact and the three dropped piece products are below 2^-23 of |x| |w|.

ROUTED names the compiled shapes that take the policy (regchain.hip: kRcSplit) at the network's channel counts.  "Policy off" has no run
of an older library to compare with, so it is held to what can be observed: the result is inside the bar, differs from the policy-on
result (another kernel ran), and after the switch is put back the policy-on result is bit for bit what it was before the door was
touched (the switch leaks nothing)."""
import ctypes
import os
import re

import numpy as np
import pytest

from test_gpu_forward_stages import DOT_BAR, Chain, _RC_SHAPES, _lrelu, bind, plan, shape_desc

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the shapes of _RC_SHAPES that regchain.hip routes to the split-bf16 policy
ROUTED = ["RcHead-2", "RcHead-4", "RcHead-13", "RcEnc1", "RcPair1", "RcPair1b"]


class policy:
    """`with policy(dbg, on):` sets the context's operand policy and puts the shipped value (on) back."""

    def __init__(self, dbg, on):
        from point_unet_amd import runtime
        self.dbg, self.on, self.ctx = dbg, on, runtime.default_context(0).handle
        dbg.ps_debug_set_regchain_b3.restype = ctypes.c_int
        dbg.ps_debug_set_regchain_b3.argtypes = [ctypes.c_void_p, ctypes.c_int]

    def __enter__(self):
        assert self.dbg.ps_debug_set_regchain_b3(self.ctx, int(self.on)) == 0
        return self

    def __exit__(self, *exc):
        assert self.dbg.ps_debug_set_regchain_b3(self.ctx, 1) == 0


def _same(a, b):
    return sorted(a) == sorted(b) and all(np.array_equal(a[i], b[i]) for i in a)


@gpu
@pytest.mark.parametrize("name", ROUTED)
def test_routed_shapes_on_the_split_policy(lib, dbg, name):
    """R around one tile, a few tiles, and just past one tile per wave of the fp32 launch (the split launch has no more waves: the second
    tile per wave and the next-tile prefetch).  The cached, host-side image and the in-kernel re-ordering give the same bits, both inside
    the bar; the per-layer fp32 kernels (form 3) are the cross-check at the small sizes; and the fp32 chain kernel gives other bits."""
    bind(dbg)
    layers, c1, c2, extras = _RC_SHAPES[name]
    cap = plan(dbg, shape_desc([(a, b) for a, b, _ in layers], c1, c2, R=1 << 22, extras=extras))
    assert cap[0] == 1, cap
    sizes = [1, 15, 16, 17, 197, cap[1] * 64 + 5]
    assert sizes[-1] <= 66000
    for R in sizes:
        ch = Chain(layers, c1, c2, R=R, extras=extras, seed=R + 1)
        big = R == sizes[-1]
        with policy(dbg, True):
            got = {form: ch.run(dbg, lib, form) for form in ((0, 1) if big else (0, 1, 3))}
        for form, g in got.items():
            print("%s R %d form %d: worst error / bar = %.3f" % (name, R, form, ch.check(g, form)))
        assert _same(got[0], got[1]), "the cached image and the in-kernel re-ordering differ"
        assert ch.plan(dbg)[0] == 1  # (the plan door is context-free: form 1 whatever the policy)
        if R == 197:
            with policy(dbg, False):
                off = ch.run(dbg, lib, 0)
            ch.check(off, 0)
            assert not _same(off, got[0]), "policy on and off gave the same bits: the split kernel did not run"


@gpu
@pytest.mark.parametrize("store_middle", [True, False])
def test_head_with_the_decoder_sources_on_the_split_policy(lib, dbg, store_middle):
    """RcHead as the network feeds it: [skip | up[interp]] with the batched gather over B = 3 clouds of an odd size; the middle layers'
    rows stored (the tap mode) or kept in registers."""
    bind(dbg)
    n0, n1 = 333, 83
    ch = Chain(_RC_SHAPES["RcHead-4"][0], 32, 32, R=3 * n0, gather={2: (0, n0, n1)}, seed=6)
    store = None if store_middle else [3]
    with policy(dbg, True):
        got = {form: ch.run(dbg, lib, form, store=store) for form in (0, 1, 3)}
    for form, g in got.items():
        assert sorted(g) == ([0, 1, 2, 3] if store_middle else [3])
        ch.check(g, form)
    assert _same(got[0], got[1])


@gpu
@pytest.mark.parametrize("name", ["RcHead-4", "RcEnc1"])
def test_policy_off_runs_the_fp32_kernel_and_leaks_nothing(lib, dbg, name):
    bind(dbg)
    layers, c1, c2, extras = _RC_SHAPES[name]
    ch = Chain(layers, c1, c2, R=197, extras=extras, seed=3)
    before = {form: ch.run(dbg, lib, form) for form in (0, 1)}  # the door not touched yet: the shipped policy
    with policy(dbg, False):
        off = {form: ch.run(dbg, lib, form) for form in (0, 1)}
        again = ch.run(dbg, lib, 0)
    after = {form: ch.run(dbg, lib, form) for form in (0, 1)}
    for form in (0, 1):
        ch.check(off[form], form)
        ch.check(before[form], form)
        assert _same(before[form], after[form]), "the switch leaked into later calls"
    assert _same(off[0], off[1]) and _same(off[0], again)
    assert not _same(off[0], before[0]), "the fp32 kernel and the split kernel gave the same bits"


@gpu
def test_a_shape_with_an_odd_input_tile_count_stays_on_fp32(lib, dbg):
    """RcEnc0: 16 -> 16, [16 | 8] -> 32 has one and three input tiles: no pairs of tiles to make a K = 32 step from."""
    bind(dbg)
    layers, c1, c2, extras = _RC_SHAPES["RcEnc0"]
    for R in (17, 197):
        ch = Chain(layers, c1, c2, R=R, extras=extras, seed=R)
        with policy(dbg, True):
            on = {form: ch.run(dbg, lib, form) for form in (0, 1)}
        with policy(dbg, False):
            off = {form: ch.run(dbg, lib, form) for form in (0, 1)}
        for form in (0, 1):
            ch.check(on[form], form)
            assert _same(on[form], off[form])


@gpu
def test_operand_range_of_the_split(lib, dbg):
    """One RcEnc1 chain at R = 197 whose input rows (and appended shortcut rows) mix magnitudes from 2^-20 to 2^20 with exact zeros, and
    whose weights include values with all 24 significand bits set: a wrong third plane or a truncated split shows here."""
    import torch
    bind(dbg)
    layers, c1, c2, extras = _RC_SHAPES["RcEnc1"]
    R = 197
    ch = Chain(layers, c1, c2, R=R, extras=extras, seed=11)
    rng = np.random.default_rng(12)

    def wide(shape):
        x = (rng.standard_normal(shape) * np.exp2(rng.integers(-20, 21, shape))).astype(np.float32)
        x[rng.random(shape) < 0.1] = 0.0
        return x

    ch.x1 = wide(ch.x1.shape)
    ch.d_x1 = torch.from_numpy(ch.x1).cuda()
    for i in ch.ex:
        ch.ex[i] = wide(ch.ex[i].shape)
        ch.d_ex[i] = torch.from_numpy(ch.ex[i]).cuda()
    for i, W in enumerate(ch.W):
        full = rng.random(W.shape) < 0.3
        W.view(np.uint32)[full] |= np.uint32(0x007fffff)  # all 24 significand bits set
        assert (W.view(np.uint32)[full] & 0x7fffff == 0x7fffff).all() and full.any()
    # the float64 activations and the bar, by the recurrence of Chain.__init__
    a = ch.x1[:, :c1].astype(np.float64)
    E = np.zeros_like(a)
    ch.want, ch.bar = [], []
    for i, (cin, cout, leaky) in enumerate(layers):
        if i in ch.ex:
            a = np.concatenate([a, ch.ex[i].astype(np.float64)], 1)
            E = np.concatenate([E, np.zeros(ch.ex[i].shape)], 1)
        aW, b = np.abs(ch.W[i].astype(np.float64)), ch.b[i].astype(np.float64)
        E = E @ aW + DOT_BAR * (np.abs(a) @ aW + np.abs(b))
        a = a @ ch.W[i].astype(np.float64) + b
        if leaky:
            a = _lrelu(a)
        ch.want.append(a)
        ch.bar.append(E)
    with policy(dbg, True):
        got = {form: ch.run(dbg, lib, form) for form in (0, 1)}
    for form, g in got.items():
        print("operand range, form %d: worst error / bar = %.3f" % (form, ch.check(g, form)))
    assert _same(got[0], got[1])


def test_the_policy_switch_reads_the_environment_only_in_the_tuning_build():
    """The switch is a constant of the default build: its variable, named like the knobs of struct Tuning, is read inside
    #ifdef PS_TUNING_ENV only (tests/test_host_logic.py holds every getenv of csrc/ to that), and the shipped library does not hold the name."""
    csrc = os.path.join(ROOT, "point-unet_amd", "csrc")
    src = open(os.path.join(csrc, "context.hip")).read()
    m = re.search(r"#ifdef PS_TUNING_ENV\n([^#]*getenv\(\"(PS_[A-Z0-9_]+)\"\)[^#]*regchain_b3[^#]*)#endif", src)
    assert m and m.group(2) == "PS_REGCHAIN_B3"
    assert re.search(r"bool regchain_b3 = true;", open(os.path.join(csrc, "common.h")).read())
    assert b"PS_REGCHAIN_B3" not in open(os.path.join(os.path.dirname(csrc), "libpointseg_hip.so"), "rb").read()
