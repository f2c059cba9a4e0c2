"""What include/pointseg_forward_precision.h's PS_PREC_BF16 computes, restated on the CPU (NumPy; no GPU here): the rule that says which
products of the point network's forward take both operands rounded once to bfloat16, the rounding itself, one fused attention stage in the
shape of tests/test_gpu_forward_stages.py's _att_case, and the whole network on oracle/randla_oracle.py's pieces.

The weight that is rounded is the float32 the library's packer holds, computed here from `params` with NumPy alone (folded): W * gamma /
sqrt(var + eps) in float64 then float32 for a convolution, the kernel itself for Wfc[:h], and float32(float64(Wfc[h:]) * log2 e) for the
half of the score product the attention kernels compute (their softmax is exp2).

Two numbers a test compares against, both from this file:  exact64 = the float64 oracle (no rounding anywhere);  model64 = the same graph in
float64 with the contract's roundings;  dist = max |exact64 - model64| is the size of the bfloat16 effect itself.  model32 (the model in
float32) shows the model's own noise: an operand within fp32 noise of a bfloat16 boundary may round the other way ("flip").
"""
import numpy as np

from oracle import randla_oracle as ro
from point_unet_amd import weights

LOG2E = 1.4426950408889634
# The bar of stage 1 of a level of ONE point, relative to max |reference|: K equal rows give a uniform softmax whatever the scores are, so dist
# = 0 exactly and a share of dist is no bar.  What is left is the fp32-level error of everything the contract does not round (LocSE, exp2, the
# weighted sum): the bar the split-bf16 form of the same stage is held to (4 x 3.0e-7, the largest form-1 figure of
# tests/test_gpu_forward_stages.py).  No other case uses it.
FP32_FLOOR = 1.2e-6


def rb(x):
    """x rounded to bfloat16, round to nearest even, as a value of x's own dtype (a float64 goes through float32 first: the device rounds
    the float32 it holds)."""
    x = np.asarray(x)
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).reshape(x.shape).astype(x.dtype)


def truncate(x):
    """x with the low 16 bits of its float32 cleared: what rb is NOT."""
    x = np.asarray(x)
    u = np.ascontiguousarray(x, np.float32).view(np.uint32) & np.uint32(0xFFFF0000)
    return u.view(np.float32).reshape(x.shape).astype(x.dtype)


# ---- the rule ------------------------------------------------------------------------------------------------------------------------
def dense_rounded(cin):
    """A dense layer / 1x1 convolution outside the attention kernels: K a multiple of 16 and at least 32."""
    return cin % 16 == 0 and cin >= 32


def att_rounded(d, k_n):
    """An attention stage (LFA mlp2, both halves of the score product): the levels the 32x32 kernels serve."""
    return d in (64, 128, 256, 512) and k_n in (16, 32)


def rule_table(cfg):
    """[(scope, K axis, rounded)] for every layer of weights.layer_dims(cfg), in its order.  mlp2 and shortcut are one product over the
    concatenated K axis d + d_in; the attention fc entries stand for both halves of F . Wfc; LFAmlp1 is the LocSE convolution."""
    out = []
    d_in = 8
    level = {}
    for i in range(cfg.num_layers):
        level["Encoder_layer_%d" % i] = (cfg.d_out[i], d_in)
        d_in = 2 * cfg.d_out[i]
    for scope, kind, cin, cout in weights.layer_dims(cfg):
        if scope == "fc0":
            out.append((scope, cin, False))
        elif scope.startswith("Encoder_layer_"):
            d, din = level[scope[:len("Encoder_layer_0")]]
            tail = scope[len("Encoder_layer_0"):]
            if tail == "LFAmlp1":
                out.append((scope, cin, False))
            elif tail in ("LFAmlp2", "LFAatt_pooling_1fc", "LFAatt_pooling_2fc"):
                out.append((scope, cin, att_rounded(d, cfg.k_n)))
            elif tail in ("mlp2", "shortcut"):
                out.append((scope, d + din, dense_rounded(d + din)))
            else:
                out.append((scope, cin, dense_rounded(cin)))
        else:
            out.append((scope, cin, dense_rounded(cin)))
    return out


# ---- the float32 weights the packer holds ------------------------------------------------------------------------------------------------
def folded(cfg, p):
    """{scope: (W [cin, cout] float32, b [cout] float32)}: BatchNorm folded in float64, then float32 (the blob of ps_randla_set_weights)."""
    out = {}
    for scope, kind, cin, cout in weights.layer_dims(cfg):
        if kind == "dense_nobias":
            out[scope] = (p[scope + "/kernel"].astype(np.float32), np.zeros(cout, np.float32))
            continue
        w = (p[scope + "/kernel"] if kind == "dense" else p[scope + "/weights"]).astype(np.float64)
        b = (p[scope + "/bias"] if kind == "dense" else p[scope + "/biases"]).astype(np.float64)
        if kind == "deconv":
            w = w.T
        bn = "batch_normalization" if kind == "dense" else (None if kind == "conv_nobn" else scope + "/batch_normalization")
        if bn:
            s = p[bn + "/gamma"].astype(np.float64) / np.sqrt(p[bn + "/moving_variance"].astype(np.float64) + ro.BN_EPS)
            w = w * s[None, :]
            b = (b - p[bn + "/moving_mean"].astype(np.float64)) * s + p[bn + "/beta"].astype(np.float64)
        out[scope] = (w.astype(np.float32), b.astype(np.float32))
    return out


def _dense(x, Wb, rounded, dt, act=True):
    W, b = Wb
    if rounded:
        x, W = rb(x), rb(W)
    y = x @ W.astype(dt) + b.astype(dt)
    return ro.leaky_relu(y) if act else y


def pre_product(f, Wfc, rounded):
    """G = f . Wfc[:h] as the layer in front of a stage stores it: float32; rounded operands where the stage is rounded."""
    h = f.shape[-1]
    top = Wfc[:h].astype(np.float32)
    a = f.astype(np.float32)
    if rounded:
        a, top = rb(a), rb(top)
    return (a.astype(np.float64) @ top.astype(np.float64)).astype(np.float32)


def att_pool(f, G, fx, Wfc, idx, rounded, dt):
    """One attentive pooling over [f[nbr] | fx] in the pre-product form the d >= 64 kernels compute: scores' = G[nbr] log2 e + fx . (Wfc[h:]
    log2 e), softmax in base 2 over the K rows, weighted sum of the UNROUNDED values.  rounded: fx and the scaled float32 weight are rounded."""
    h = f.shape[-1]
    bot = (Wfc[h:].astype(np.float64) * LOG2E).astype(np.float32)
    a = fx
    if rounded:
        a, bot = rb(fx), rb(bot)
    s = ro.gather_neighbour(G.astype(dt), idx) * np.asarray(LOG2E, dt) + a @ bot.astype(dt)
    s = s - s.max(axis=2, keepdims=True)
    e = np.exp2(s)
    fset = np.concatenate([ro.gather_neighbour(f.astype(dt), idx), fx], -1)
    return np.sum(fset * (e / e.sum(axis=2, keepdims=True)), axis=2)


# ---- one fused stage, in the shape of test_gpu_forward_stages._att_case ------------------------------------------------------------------
class OneLevel:
    num_layers, num_classes, in_channels = 1, 4, 7
    sub_sampling_ratio = [4]

    def __init__(self, d, k_n):
        self.d_out, self.k_n = (d,), k_n


PERIOD = 9  # points of the geometry pattern a walk case repeats


def att_case(params, d, K, stage, B, n_cloud, seed, period=0):
    """Inputs of one stage of a one-level network at PS_PREC_BF16 and its three references.  Returns (xyz, idx, fg, exact64, model64,
    model32): fg = [f | G] with G = float32(rb(f) . rb(Wfc[:h])), the value the contract supplies to the kernel; exact64 takes the same G
    and no other rounding.
    period > 0 (the second-tile walks, thousands of points): the GEOMETRY is a pattern of `period` points repeated -- point i sits where
    point i % period sits and its neighbours are the pattern's, inside its own repetition (the last, partial repetition points into the one
    before) -- while f and G stay random per point.  The only operand the kernel rounds is f_xyz, a function of the geometry alone: the
    walk then has period x K distinct rows of it where a random cloud has n x K, so the reference meets a bfloat16 boundary as rarely as on
    a level of `period` points and its noise can be kept under the bar by the seed; every point still has its own neighbour rows, features,
    scores and result, so a walk that reads another tile's rows is seen."""
    rng = np.random.default_rng(seed)
    h = d // 2
    if period:
        assert B == 1 and n_cloud > 2 * period
        xyz_p = rng.random((period, 3), dtype=np.float32)
        idx_p = rng.integers(0, period, (period, K)).astype(np.int32)
        idx_p[::4, K // 2:] = idx_p[::4, :K // 2]
        i = np.arange(n_cloud)
        rep = np.minimum(i // period, (n_cloud // period) - 1)
        xyz = xyz_p[i % period][None]
        idx = (rep[:, None] * period + idx_p[i % period]).astype(np.int32)[None]
    else:
        xyz = rng.random((B, n_cloud, 3), dtype=np.float32)
        idx = rng.integers(0, n_cloud, (B, n_cloud, K)).astype(np.int32)
        idx[:, ::4, K // 2:] = idx[:, ::4, :K // 2]
    f = rng.standard_normal((B, n_cloud, h)).astype(np.float32)
    F = folded(OneLevel(d, K), params)
    name = "Encoder_layer_0LFA"
    Wfc = F[name + "att_pooling_%dfc" % stage][0]
    G = pre_product(f, Wfc, True)

    def run(dt, rounded):
        fx = _dense(ro.relative_pos_encoding(xyz.astype(dt), idx), F[name + "mlp1"], False, dt)  # LocSE: never rounded
        if stage == 2:
            fx = _dense(fx, F[name + "mlp2"], rounded, dt)
        return att_pool(f, G, fx, Wfc, idx, rounded, dt).reshape(B * n_cloud, d)

    fg = np.concatenate([f, G], -1).reshape(B * n_cloud, -1)
    return (xyz.reshape(-1, 3), idx.reshape(-1, K), fg, run(np.dtype(np.float64), False), run(np.dtype(np.float64), True),
            run(np.dtype(np.float32), True))


# the attention cases of tests/test_gpu_forward_precision.py: (d, K, stage, B, n_cloud, seed); the CPU test checks every one of them
SMALL_LEVELS = ((1, 1), (1, 3), (1, 9), (1, 33), (3, 37))


# (d, K, stage, B, n) -> seed, where the default seed's reference noise is above 0.025 dist (found on the CPU, see att_cases)
SEEDS = {(64, 32, 2, 1, 33): 1233, (256, 16, 2, 1, 33): 1233, (256, 16, 2, 3, 37): 1237, (256, 32, 1, 1, 4133): 1008, (256, 32, 1, 3, 37):
         1137, (256, 32, 2, 1, 33): 1233, (256, 32, 2, 3, 37): 2237, (512, 16, 2, 3, 37): 8237, (512, 32, 2, 3, 37): 2237}


def att_cases():
    """(d, K, stage, B, n, seed, period) of every attention case.  The default seeds are test_gpu_forward_stages.py's; a case whose
    max |model32 - model64| exceeds 0.025 dist at its default seed takes the first seed default + 1000 j at which it is at most 0.02 dist."""
    out = []
    for d in (64, 128, 256, 512):
        for K in (16, 32):
            for stage in (1, 2):
                for B, n in SMALL_LEVELS:
                    out.append((d, K, stage, B, n, 100 * stage + n, 0))
    for d in (64, 128, 256, 512):
        for stage in (1, 2):
            out.append((d, 32, stage, 1, 4133, 7 + stage, PERIOD))
    for d in (64, 256):
        for stage in (1, 2):
            out.append((d, 16, stage, 1, 8267, 17 + stage, PERIOD))
    return [(d, K, st, B, n, SEEDS.get((d, K, st, B, n), seed), per) for d, K, st, B, n, seed, per in out]

# ---- the whole network ---------------------------------------------------------------------------------------------------------------
def inference(cfg, p, xyz, neigh_idx, sub_idx, interp_idx, features, dtype=np.float64, rounded=True):
    """oracle/randla_oracle.py's inference on the folded weights; rounded: with the roundings of PS_PREC_BF16 (False: no rounding -- the
    oracle's own result up to the folding, a check of this restatement)."""
    dt = np.dtype(dtype)
    F = folded(cfg, p)
    K = cfg.k_n

    def R(cin):
        return rounded and dense_rounded(cin)

    f = _dense(features.astype(dt), F["fc0"], False, dt)
    enc = []
    d_in = 8
    for i in range(cfg.num_layers):
        d = cfg.d_out[i]
        n = "Encoder_layer_%d" % i
        att = rounded and att_rounded(d, K)
        idx = neigh_idx[i]
        f_pc = _dense(f, F[n + "mlp1"], R(d_in), dt)
        fx = _dense(ro.relative_pos_encoding(xyz[i].astype(dt), idx), F[n + "LFAmlp1"], False, dt)
        for stage in (1, 2):
            Wfc = F[n + "LFAatt_pooling_%dfc" % stage][0]
            if stage == 2:
                fx = _dense(fx, F[n + "LFAmlp2"], att, dt)
            if d >= 64:
                agg = att_pool(f_pc, pre_product(f_pc, Wfc, att), fx, Wfc, idx, att, dt)
            else:  # the direct formulation of the narrow levels: exactly the oracle's
                fset = np.concatenate([ro.gather_neighbour(f_pc, idx), fx], -1)
                act = fset @ Wfc.astype(dt)
                act = act - act.max(axis=2, keepdims=True)
                e = np.exp(act)
                agg = np.sum(fset * (e / e.sum(axis=2, keepdims=True)), axis=2)
            f_pc = _dense(agg, F[n + "LFAatt_pooling_%dmlp" % stage], R(d), dt)
        Wm, bm = F[n + "mlp2"]
        Ws, bs = F[n + "shortcut"]
        f_enc = _dense(np.concatenate([f_pc, f], -1), (np.concatenate([Wm, Ws], 0), bm + bs), R(d + d_in), dt)
        f = ro.random_sample(f_enc, sub_idx[i])
        if i == 0:
            enc.append(f_enc)
        enc.append(f)
        d_in = 2 * d
    f = _dense(enc[-1], F["decoder_0"], R(d_in), dt)
    for j in range(cfg.num_layers):
        x = np.concatenate([enc[-j - 2], ro.nearest_interpolation(f, interp_idx[-j - 1])], -1)
        f = _dense(x, F["Decoder_layer_%d" % j], R(x.shape[-1]), dt)
    f = _dense(f, F["fc1"], R(f.shape[-1]), dt)
    f = _dense(f, F["fc2"], R(64), dt)
    return _dense(f, F["fc"], R(32), dt, act=False)
