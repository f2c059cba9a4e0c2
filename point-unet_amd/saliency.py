"""The saliency attention map in front of prepare.pancreas_mask: the reference's SaliencyAttention network (`unet3d_attention`,
SaliencyAttention/model.py:176-314 with attention.py:79-174) run patch by patch over a volume (`overlapping_inference`,
SaliencyAttention/eval.py:103-193), on the device -- include/pointseg_saliency.h, csrc/conv3d.hip, csrc/saliency.hip.  SaliencyNet runs it for inference behind one call, its convolutions in fp32 or on the
bf16 matrix pipe (precision="fp32" | "bf16x3" | "bf16": include/pointseg_saliency_precision.h, csrc/conv3d_bf16.hip); the gradients of its
ops (include/pointseg_saliency_train.h, include/pointseg_saliency_attention.h) stand behind it, op by op, and TrainableSaliencyNet composes the graph from them;
SaliencyTrainer runs the whole training step behind one call (include/pointseg_saliency_step.h, csrc/saliency_step.hip).

Parameters are a dict of TensorFlow-named arrays in TensorFlow layout under the `unet3d_attention/` scope: `<layer>/kernel`
[kd, kh, kw, in, out] (dense layers: [in, out]), `<layer>/bias`, `<layer>/ins_norm/gamma`, `<layer>/ins_norm/beta`, with <layer> the
reference's `name=` arguments.  No checkpoint of the reference exists here, so these names are UNPINNED (as weights.from_tf_variables'
are): they follow the source, not a saved graph."""
import ctypes

import numpy as np
import torch

from . import _lib, runtime

SCOPE = "unet3d_attention/"
EPS = 1e-5  # InstanceNorm5d's epsilon (custom_ops.py:29)
_CA = "C345_ChannelWiseAttention_withcpfe"


def layer_table(in_channels, num_classes=2):
    """The layers in the order of the flat weight buffer (include/pointseg_saliency.h): (name, kernel shape, has bias, has norm)."""
    t = [("init_conv", (3, 3, 3, in_channels, 16), True, True)]
    for d in range(5):
        w = 16 << d
        t += [("down%d_conv_0" % d, (3, 3, 3, w, w), True, True), ("down%d_conv_1" % d, (3, 3, 3, w, w), True, True)]
        if d < 4:
            t.append(("stride2conv%d" % d, (3, 3, 3, w, 2 * w), True, True))
    t += [("C1_conv", (3, 3, 3, 16, 64), True, True), ("C2_conv", (3, 3, 3, 32, 64), True, True)]
    for p, cin in (("C3_cfe", 64), ("C4_cfe", 128), ("C5_cfe", 256)):
        t.append((p + "_cfe0", (1, 1, 1, cin, 32), False, True))
        t += [("%s_cfe%d_dilation" % (p, r), (3, 3, 3, cin, 32), False, True) for r in (1, 2, 3)]
    t += [("up_conv1_C5_cfe_up4", (3, 3, 3, 128, 128), True, True), ("up_conv1_C4_cfe_up2", (3, 3, 3, 128, 128), True, True)]
    t += [(_CA + "_dense_1", (384, 96), True, False), (_CA + "_dense_2", (96, 384), True, False)]
    t += [("C345_conv", (1, 1, 1, 384, 64), True, True), ("up_conv1_C345_up4", (3, 3, 3, 64, 64), True, True)]
    for i, (a, b) in enumerate((((1, 9, 9), (9, 1, 1)), ((9, 1, 9), (1, 9, 1)), ((9, 9, 1), (1, 1, 9))), 1):
        t += [("spatial_attention_%d_conv1" % i, a + (64, 32), True, True), ("spatial_attention_%d_conv2" % i, b + (32, 1), True, True)]
    t += [("up_conv1_C2_up2", (3, 3, 3, 64, 64), True, True), ("C12_conv", (3, 3, 3, 128, 64), True, True)]
    t.append(("final", (3, 3, 3, 128, num_classes), True, False))
    return t


def param_shapes(in_channels, num_classes=2):
    """name -> shape of every parameter, in flat-buffer order."""
    out = {}
    for name, shape, bias, norm in layer_table(in_channels, num_classes):
        out[SCOPE + name + "/kernel"] = shape
        if bias:
            out[SCOPE + name + "/bias"] = (shape[-1],)
        if norm:
            out[SCOPE + name + "/ins_norm/gamma"] = (shape[-1],)
            out[SCOPE + name + "/ins_norm/beta"] = (shape[-1],)
    return out


def init_params(in_channels, num_classes=2, seed=0):
    """The initialisation the tests' error bars were sized on: kernels N(0, sqrt(2 / fan_in)), biases N(0, 0.1), gamma U(0.5, 1.5),
    beta N(0, 0.2).  float32 numpy arrays."""
    rng = np.random.default_rng(seed)
    p = {}
    for name, shape in param_shapes(in_channels, num_classes).items():
        if name.endswith("/kernel"):
            fan_in = int(np.prod(shape[:-1]))
            a = rng.standard_normal(shape) * np.sqrt(2.0 / fan_in)
        elif name.endswith("/bias"):
            a = rng.standard_normal(shape) * 0.1
        elif name.endswith("/gamma"):
            a = rng.uniform(0.5, 1.5, shape)
        else:
            a = rng.standard_normal(shape) * 0.2
        p[name] = a.astype(np.float32)
    return p


def flatten_params(params, in_channels, num_classes=2):
    """The TF-named dict -> the flat float32 buffer ps_saliency_forward reads.  Every name must be there with its shape, and no other."""
    shapes = param_shapes(in_channels, num_classes)
    extra = set(params) - set(shapes)
    if extra:
        raise ValueError("flatten_params: unknown parameters %s" % sorted(extra)[:4])
    parts = []
    for name, shape in shapes.items():
        if name not in params:
            raise ValueError("flatten_params: parameter %s is missing" % name)
        a = np.asarray(params[name], dtype=np.float32)
        if tuple(a.shape) != tuple(shape):
            raise ValueError("flatten_params: %s has shape %s, expected %s" % (name, tuple(a.shape), tuple(shape)))
        parts.append(a.reshape(-1))
    return np.concatenate(parts)


def unflatten_params(flat, in_channels, num_classes=2):
    """The inverse of flatten_params."""
    flat = np.asarray(flat)
    out, off = {}, 0
    for name, shape in param_shapes(in_channels, num_classes).items():
        n = int(np.prod(shape))
        out[name] = flat[off:off + n].reshape(shape)
        off += n
    if off != flat.size:
        raise ValueError("unflatten_params: the buffer has %d values, the network %d" % (flat.size, off))
    return out


# ---- op wrappers (the tests' doors to the kernels) ---------------------------------------------------------------------------------------------

_scratch = {}  # (entry point, device index) -> uint8 tensor, grown to the largest call so far


def _f32(t, who, name, dims=None):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ValueError("%s: %s must be a CUDA tensor" % (who, name))
    if t.dtype != torch.float32:
        raise ValueError("%s: %s must be float32, got %s" % (who, name, t.dtype))
    if dims is not None and t.dim() != dims:
        raise ValueError("%s: %s must have %d dimensions, got shape %s" % (who, name, dims, tuple(t.shape)))
    return t.contiguous()


def _scratch_for(key, need, dev):
    buf = _scratch.get(key)
    if buf is None or buf.numel() < need:
        buf = _scratch[key] = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
    return buf


def _ctx_for(t):
    ctx = runtime.default_context(t.device.index)
    ctx.use_torch_stream()
    return ctx


def _two_call(name, dev, call):
    """The two-call scratch protocol: call(None, byref(need)) sizes (it looks at the shapes alone), then the same call runs on the
    cached buffer.  Returns the size."""
    need = ctypes.c_int64(0)
    _lib.check(call(None, ctypes.byref(need)))
    buf = _scratch_for((name, dev.index), need.value, dev)
    _lib.check(call(runtime.ptr(buf), ctypes.byref(need)))
    return need.value


def _same_out(n, stride):
    return -(-n // stride)


def _conv_args(who, x, w, x2, up, stride):
    """What conv3d and conv3d_backward check alike: (x, w, x2, the geometry's (B, Ds, Hs, Ws, C1, C2), the output's shape)."""
    x = _f32(x, who, "x", 5)
    w = _f32(w, who, "w", 5)
    B, Ds, Hs, Ws, C1 = x.shape
    C2 = 0
    if x2 is not None:
        x2 = _f32(x2, who, "x2", 5)
        if x2.shape[:4] != x.shape[:4]:
            raise ValueError("%s: x2 must have x's batch and extents" % who)
        C2 = x2.shape[4]
    if w.shape[3] != C1 + C2:
        raise ValueError("%s: w has %d input channels, the input %d" % (who, w.shape[3], C1 + C2))
    return x, w, x2, (B, Ds, Hs, Ws, C1, C2), (B, _same_out(Ds * up, stride), _same_out(Hs * up, stride), _same_out(Ws * up, stride), w.shape[4])


def _precision(who, precision, roles=3):
    """"fp32" | "bf16x3" | "bf16", or a triple (forward, data_grad, weight_grad) of those names, -> the three PS_PREC_* values of
    include/pointseg_saliency_precision.h, one per role of a convolution in training; a single name means that name three times.
    roles=1 (inference: one role): a single name alone -> its one value."""
    names = _lib.SALIENCY_PRECISIONS
    try:
        if roles == 3 and isinstance(precision, (tuple, list)):
            if len(precision) != 3:
                raise KeyError(precision)
            return tuple(names[p] for p in precision)
        return names[precision] if roles == 1 else (names[precision],) * 3
    except (KeyError, TypeError):
        what = "one of %s" % ", ".join(map(repr, names))
        if roles == 3:
            what += ", or a triple (forward, data_grad, weight_grad) of them"
        raise ValueError("%s: precision must be %s, got %r" % (who, what, precision)) from None


def conv3d(x, w, bias=None, stride=1, dilation=1, x2=None, up=1, precision="fp32"):
    """tf.layers.conv3d(x, padding="SAME") without activation: x [B, D, H, W, C1] (and x2 [B, D, H, W, C2], concatenated behind it on the
    channel axis; both up-sampled `up` times by repetition first), w [kd, kh, kw, C1 + C2, C_out], bias [C_out] or None.  CUDA float32.
    precision: "fp32" (ps_conv3d), or "bf16x3" / "bf16" on the bf16 matrix pipe (ps_conv3d_prec, include/pointseg_saliency_precision.h)."""
    who = "conv3d"
    prec = _precision(who, precision, roles=1)
    x, w, x2, dims, out_shape = _conv_args(who, x, w, x2, up, stride)
    if bias is not None:
        bias = _f32(bias, who, "bias", 1)
        if bias.shape[0] != w.shape[4]:
            raise ValueError("conv3d: bias must have C_out values")
    y = torch.empty(out_shape, dtype=torch.float32, device=x.device)
    args = (_ctx_for(x).handle, runtime.ptr(x), runtime.ptr(x2), *dims, up, runtime.ptr(w), runtime.ptr(bias), w.shape[0], w.shape[1], w.shape[2], w.shape[4],
            stride, dilation, runtime.ptr(y))
    _lib.check(_lib.lib().ps_conv3d_prec(*args, prec) if prec else _lib.lib().ps_conv3d(*args))
    return y


def instance_norm_relu(x, gamma, beta, eps=EPS):
    """BN_Relu with INSTANCE_NORM (model.py:366-372): x [B, ..., C] CUDA float32, normalised per sample and channel over everything between."""
    who = "instance_norm_relu"
    x = _f32(x, who, "x")
    if x.dim() < 2:
        raise ValueError("instance_norm_relu: x must be [B, ..., C]")
    gamma, beta = _f32(gamma, who, "gamma", 1), _f32(beta, who, "beta", 1)
    B, C = x.shape[0], x.shape[-1]
    V = x.numel() // (B * C)
    if gamma.shape[0] != C or beta.shape[0] != C:
        raise ValueError("instance_norm_relu: gamma and beta must have C values")
    y = torch.empty_like(x)
    ctx = _ctx_for(x)
    fn = _lib.lib().ps_instance_norm_relu
    _two_call("ps_instance_norm_relu", x.device, lambda scratch, n: fn(ctx.handle, runtime.ptr(x), B, V, C, runtime.ptr(gamma), runtime.ptr(beta), eps,
                                                                       runtime.ptr(y), scratch, n))
    return y


# ---- the network ---------------------------------------------------------------------------------------------------------------------------------

class SaliencyNet:
    """unet3d_attention for inference.  params: the TF-named dict (see the module's docstring); the weights live on `device` as one flat
    buffer.  A patch is [B, D, H, W, C_in] (or [D, H, W, C_in]) CUDA float32 with D, H, W multiples of 16.  precision: the arithmetic of
    every convolution -- "fp32", "bf16x3" (fp32-level results from split bfloat16 operands) or "bf16" (operands rounded to bfloat16):
    include/pointseg_saliency_precision.h; forward, probs and forward_taps use it, and so does saliency_map through the net it is given."""

    def __init__(self, params, in_channels, num_classes=2, device=0, precision="fp32"):
        self.precision = precision
        self._prec = _precision("SaliencyNet", precision, roles=1)
        self.in_channels, self.num_classes = int(in_channels), int(num_classes)
        flat = flatten_params(params, self.in_channels, self.num_classes)
        want = _lib.lib().ps_saliency_weight_count(self.in_channels, self.num_classes)
        if want != flat.size:
            raise _lib.PointSegError("SaliencyNet: the library's network has %d weights, this package's layer table %d" % (want, flat.size))
        self.device = torch.device("cuda", device)
        self.weights = torch.from_numpy(flat).to(self.device)

    def _run(self, patch, want_logits, want_probs, taps=False):
        who = "SaliencyNet"
        x = _f32(patch, who, "patch")
        if x.dim() == 4:
            x = x[None]
        if x.dim() != 5 or x.shape[4] != self.in_channels:
            raise ValueError("SaliencyNet: patch must be [B, D, H, W, %d], got %s" % (self.in_channels, tuple(patch.shape)))
        B, D, H, W, _ = x.shape
        if D % 16 or H % 16 or W % 16 or min(D, H, W) < 16:
            raise ValueError("SaliencyNet: the patch extents %s must be multiples of 16" % ((D, H, W),))
        K = self.num_classes
        logits = torch.empty((B, D, H, W, K), dtype=torch.float32, device=x.device) if want_logits else None
        probs = torch.empty((B, D, H, W, K), dtype=torch.float32, device=x.device) if want_probs else None
        out = {"logits": logits, "probs": probs}
        tp = None
        if taps:
            out["down4"] = torch.empty((B, D // 16, H // 16, W // 16, 256), dtype=torch.float32, device=x.device)
            out["c345"] = torch.empty((B, D, H, W, 64), dtype=torch.float32, device=x.device)
            out["sa"] = torch.empty((B, D, H, W), dtype=torch.float32, device=x.device)
            out["c12"] = torch.empty((B, D, H, W, 64), dtype=torch.float32, device=x.device)
            tp = _lib.PsSaliencyTaps(*(runtime.ptr(out[k]) for k in ("down4", "c345", "sa", "c12")))
        ctx = _ctx_for(x)
        fn = _lib.lib().ps_saliency_forward_prec if self._prec else _lib.lib().ps_saliency_forward
        tail = (self._prec,) if self._prec else ()
        self.scratch_bytes = _two_call("ps_saliency_forward", x.device, lambda scratch, n: fn(
            ctx.handle, runtime.ptr(x), B, D, H, W, self.in_channels, K, runtime.ptr(self.weights), self.weights.numel(), runtime.ptr(logits), runtime.ptr(probs),
            ctypes.byref(tp) if tp is not None else None, scratch, n, *tail))
        return out

    def forward(self, patch):
        """The logits [B, D, H, W, num_classes]."""
        return self._run(patch, True, False)["logits"]

    def probs(self, patch):
        """softmax(logits) (train.py:116)."""
        return self._run(patch, False, True)["probs"]

    def forward_taps(self, patch):
        """logits, probs and the four activations of ps_saliency_taps, as a dict."""
        return self._run(patch, True, True, taps=True)


def window_origins(n, crop, step):
    """eval.py:142-144: np.arange(0, max(1, n - crop + step), step)."""
    return list(range(0, max(1, n - crop + step), step))


def saliency_map(volume, net, patch=(64, 160, 160), steps=(48, 118, 118), direction="axial", flip=False, batch=1, layout=None):
    """segment_one_image / overlapping_inference (eval.py:103-193, 355-411) on the device, one ps_saliency_map call
    (include/pointseg_saliency_map.h states the rule): volume [C_in, D, H, W] or [D, H, W], or with layout="DHWC" a PatchBank image
    [D, H, W, C_in] (CUDA float32) -> the window-averaged softmax probabilities [D, H, W, num_classes], in the volume's orientation.
    net: a SaliencyNet, whose view is `direction` ("axial", "sagittal", "coronal": config.DIRECTION, utils.py:80-104), or a dict that maps
    view names to the SaliencyNet trained for each (config.MULTI_VIEW, eval.py:254): the maps are fused in the dict's order, and
    `direction` must be left at its default.  patch and steps are in the view's axes.  flip: config.TEST_FLIP, the average with the map of
    the left-right mirrored volume (utils.py:15-28, eval.py:461-463).  batch: windows per forward call, 1 .. 8; the result does not depend
    on it.  A window that overhangs the volume is zero-filled and its prediction cut back to the part inside.  The reference feeds
    BATCH_SIZE copies of the window and keeps pred[0]; with instance norm the samples of a batch do not see each other, so one copy gives
    the same result.  The window loop, the views and the flip run inside the library; no permuted copy is made, nothing is read back."""
    who = "saliency_map"
    if isinstance(net, dict):
        if direction != "axial":
            raise ValueError("saliency_map: with a dict of nets the views are the dict's keys; leave direction at its default")
        names, nets = list(net.keys()), list(net.values())
    else:
        names, nets = [direction], [net]
    if not 1 <= len(nets) <= 3 or any(n not in _lib.SALIENCY_VIEWS for n in names):
        raise ValueError("saliency_map: the views must be one to three of %s, got %r" % (", ".join(map(repr, _lib.SALIENCY_VIEWS)), names))
    first = nets[0]
    if any((n.in_channels, n.num_classes, n._prec) != (first.in_channels, first.num_classes, first._prec) for n in nets):
        raise ValueError("saliency_map: the nets of a multi-view call must share in_channels, num_classes and precision")
    if layout not in (None, "CDHW", "DHWC"):
        raise ValueError("saliency_map: layout must be None, 'CDHW' or 'DHWC', got %r" % (layout,))
    v = _f32(volume, who, "volume")
    if v.dim() == 3:
        v = v[None] if layout != "DHWC" else v[..., None]
    C, K = first.in_channels, first.num_classes
    if layout == "DHWC":
        ok, (D, H, W) = v.dim() == 4 and v.shape[3] == C, tuple(v.shape[:3])
    else:
        ok, (D, H, W) = v.dim() == 4 and v.shape[0] == C, tuple(v.shape[1:])
    if not ok:
        raise ValueError("saliency_map: volume must be [%d, D, H, W] or [D, H, W] (layout='DHWC': [D, H, W, %d]), got %s" % (C, C, tuple(volume.shape)))
    if len(patch) != 3 or len(steps) != 3 or min(steps) < 1 or any(p % 16 or p < 16 for p in patch):
        raise ValueError("saliency_map: patch %s (multiples of 16) / steps %s (>= 1)" % (tuple(patch), tuple(steps)))
    if any(n.weights.device != v.device for n in nets):
        raise ValueError("saliency_map: the volume and the nets must be on one device")
    out = torch.empty((D, H, W, K), dtype=torch.float32, device=v.device)
    views = (ctypes.c_int32 * len(nets))(*(_lib.SALIENCY_VIEWS[n] for n in names))
    weights = (ctypes.c_void_p * len(nets))(*(runtime.ptr(n.weights) for n in nets))
    patch_c, step_c = (ctypes.c_int64 * 3)(*map(int, patch)), (ctypes.c_int64 * 3)(*map(int, steps))
    ctx = _ctx_for(v)
    fn = _lib.lib().ps_saliency_map
    _two_call("ps_saliency_map", v.device, lambda scratch, n: fn(
        ctx.handle, runtime.ptr(v), _lib.PS_VOLUME_DHWC if layout == "DHWC" else _lib.PS_VOLUME_CDHW, C, D, H, W, K, len(nets), views, weights,
        first.weights.numel(), patch_c, step_c, int(bool(flip)), int(batch), first._prec, runtime.ptr(out), scratch, n))
    return out


# ---- the gradients of the two op wrappers (include/pointseg_saliency_train.h, csrc/conv3d_train.hip, csrc/saliency_train.hip) ---------------------------------------------

def conv3d_backward(dy, x, w, stride=1, dilation=1, x2=None, up=1, need=("x", "x2", "w", "bias"), precision="fp32"):
    """The gradients of conv3d(x, w, bias, stride, dilation, x2, up) for the output gradient dy: a dict with the entries of `need` --
    "x" [like x], "x2" [like x2; only with x2], "w" [like w], "bias" [C_out].  Arguments are checked as conv3d checks them.
    precision: "fp32" (ps_conv3d_bwd_data, ps_conv3d_bwd_weight), or "bf16x3" / "bf16" on the bf16 matrix pipe (their _prec entries,
    include/pointseg_saliency_train_precision.h); a triple (forward, data_grad, weight_grad) gives the data gradient (x, x2) its second
    name and the weight gradient (w, bias) its third."""
    who = "conv3d_backward"
    _, prec_data, prec_weight = _precision(who, precision)
    x, w, x2, dims, want = _conv_args(who, x, w, x2, up, stride)
    dy = _f32(dy, who, "dy", 5)
    if tuple(dy.shape) != want:
        raise ValueError("conv3d_backward: dy has shape %s, the convolution's output %s" % (tuple(dy.shape), want))
    need = set(need)
    if not need or need - {"x", "x2", "w", "bias"}:
        raise ValueError("conv3d_backward: need must name some of x, x2, w, bias")
    if x2 is None:
        need.discard("x2")
        if not need:
            raise ValueError("conv3d_backward: the gradient of x2 was asked for and there is no x2")
    out = {}
    ctx = _ctx_for(x)
    geometry = dims + (up, w.shape[0], w.shape[1], w.shape[2], w.shape[4], stride, dilation)
    if need & {"x", "x2"}:
        dx = torch.empty_like(x) if "x" in need else None
        dx2 = torch.empty_like(x2) if "x2" in need else None
        fn = _lib.lib().ps_conv3d_bwd_data_prec if prec_data else _lib.lib().ps_conv3d_bwd_data
        tail = (prec_data,) if prec_data else ()
        _two_call("ps_conv3d_bwd_data", x.device, lambda scratch, n: fn(ctx.handle, runtime.ptr(dy), runtime.ptr(w), *geometry, runtime.ptr(dx),
                                                                        runtime.ptr(dx2), scratch, n, *tail))
        if dx is not None:
            out["x"] = dx
        if dx2 is not None:
            out["x2"] = dx2
    if need & {"w", "bias"}:
        dw = torch.empty_like(w) if "w" in need else None
        db = torch.empty((w.shape[4],), dtype=torch.float32, device=x.device) if "bias" in need else None
        fn = _lib.lib().ps_conv3d_bwd_weight_prec if prec_weight else _lib.lib().ps_conv3d_bwd_weight
        tail = (prec_weight,) if prec_weight else ()
        _two_call("ps_conv3d_bwd_weight", x.device, lambda scratch, n: fn(ctx.handle, runtime.ptr(x), runtime.ptr(x2), runtime.ptr(dy), *geometry,
                                                                          runtime.ptr(dw), runtime.ptr(db), scratch, n, *tail))
        if dw is not None:
            out["w"] = dw
        if db is not None:
            out["bias"] = db
    return out


def _norm_backward(dy, x, y, gamma, eps, need):
    who = "instance_norm_relu_backward"
    x, y, dy = _f32(x, who, "x"), _f32(y, who, "y"), _f32(dy, who, "dy")
    gamma = _f32(gamma, who, "gamma", 1)
    if x.dim() < 2 or y.shape != x.shape or dy.shape != x.shape:
        raise ValueError("instance_norm_relu_backward: x, y and dy must be [B, ..., C] of one shape")
    B, C = x.shape[0], x.shape[-1]
    V = x.numel() // (B * C)
    if gamma.shape[0] != C:
        raise ValueError("instance_norm_relu_backward: gamma must have C values")
    if not any(need):
        raise ValueError("instance_norm_relu_backward: no gradient asked for")
    dx = torch.empty_like(x) if need[0] else None
    dgamma = torch.empty_like(gamma) if need[1] else None
    dbeta = torch.empty_like(gamma) if need[2] else None
    ctx = _ctx_for(x)
    fn = _lib.lib().ps_instance_norm_relu_bwd
    _two_call("ps_instance_norm_relu_bwd", x.device, lambda scratch, n: fn(ctx.handle, runtime.ptr(x), runtime.ptr(y), runtime.ptr(dy), B, V, C,
                                                                           runtime.ptr(gamma), eps, runtime.ptr(dx), runtime.ptr(dgamma), runtime.ptr(dbeta),
                                                                           scratch, n))
    return dx, dgamma, dbeta


def instance_norm_relu_backward(dy, x, y, gamma, eps=EPS):
    """The gradients of y = instance_norm_relu(x, gamma, beta, eps) for the output gradient dy: (dx, dgamma, dbeta).  y is only the ReLU's
    mask (y > 0)."""
    return _norm_backward(dy, x, y, gamma, eps, (True, True, True))


class Conv3dFunction(torch.autograd.Function):
    """conv3d with its gradients: forward ps_conv3d, backward ps_conv3d_bwd_data and ps_conv3d_bwd_weight, all three at `precision`, or
    each at its own name of a triple (forward, data_grad, weight_grad).  Saves x, x2 and w."""

    @staticmethod
    def forward(ctx, x, w, bias, stride, dilation, x2, up, precision="fp32"):
        ctx.save_for_backward(x, x2, w)
        ctx.geometry = (stride, dilation, up)
        ctx.precision = precision
        return conv3d(x, w, bias, stride, dilation, x2, up, precision[0] if isinstance(precision, (tuple, list)) else precision)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, x2, w = ctx.saved_tensors
        stride, dilation, up = ctx.geometry
        wanted = ctx.needs_input_grad
        need = [name for name, i in (("x", 0), ("w", 1), ("bias", 2), ("x2", 5)) if wanted[i] and (name != "x2" or x2 is not None)]
        g = conv3d_backward(dy, x, w, stride, dilation, x2, up, need, ctx.precision) if need else {}
        return g.get("x"), g.get("w"), g.get("bias"), None, None, g.get("x2"), None, None


class InstanceNormReluFunction(torch.autograd.Function):
    """instance_norm_relu with its gradients: forward ps_instance_norm_relu, backward ps_instance_norm_relu_bwd.  Saves x, y and gamma."""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps):
        y = instance_norm_relu(x, gamma, beta, eps)
        ctx.save_for_backward(x, y, gamma)
        ctx.eps = eps
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, y, gamma = ctx.saved_tensors
        need = tuple(ctx.needs_input_grad[:3])
        if not any(need):
            return None, None, None, None
        dx, dgamma, dbeta = _norm_backward(dy, x, y, gamma, ctx.eps, need)
        return dx, dgamma, dbeta, None


def differentiable_conv3d(x, w, bias=None, stride=1, dilation=1, x2=None, up=1, precision="fp32"):
    """conv3d, recorded by torch.autograd: the forward and both gradients run at `precision`, or -- a triple (forward, data_grad,
    weight_grad) -- each at its own."""
    _precision("differentiable_conv3d", precision)
    return Conv3dFunction.apply(x, w, bias, stride, dilation, x2, up, precision)


def differentiable_instance_norm_relu(x, gamma, beta, eps=EPS):
    """instance_norm_relu, recorded by torch.autograd."""
    return InstanceNormReluFunction.apply(x, gamma, beta, eps)


# ---- the channel attention, the spatial gate and softmax + Dice (include/pointseg_saliency_attention.h, csrc/saliency_train.hip) ------------------

def _rows(x, who, name):
    """x [B, ..., C] -> (contiguous x, B, V, C)."""
    x = _f32(x, who, name)
    if x.dim() < 2:
        raise ValueError("%s: %s must be [B, ..., C]" % (who, name))
    B, C = x.shape[0], x.shape[-1]
    return x, B, x.numel() // max(B * C, 1), C


def channel_attention(x, w1, b1, w2, b2, want_y=True):
    """ChannelWiseAttention3D (attention.py:166-174): x [B, ..., C], w1 [C, Ch], b1 [Ch], w2 [Ch, C], b2 [C] -> (y, mean, hidden, scale) with
    y = x * scale (None without want_y), mean [B, C], hidden [B, Ch], scale [B, C]: what channel_attention_backward takes."""
    who = "channel_attention"
    x, B, V, C = _rows(x, who, "x")
    w1, b1, w2, b2 = _f32(w1, who, "w1", 2), _f32(b1, who, "b1", 1), _f32(w2, who, "w2", 2), _f32(b2, who, "b2", 1)
    Ch = w1.shape[1]
    if w1.shape[0] != C or tuple(w2.shape) != (Ch, C) or b1.shape[0] != Ch or b2.shape[0] != C:
        raise ValueError("channel_attention: w1 %s, b1 %s, w2 %s, b2 %s do not fit C = %d" % (tuple(w1.shape), tuple(b1.shape), tuple(w2.shape), tuple(b2.shape), C))
    mean, scale = (torch.empty((B, C), dtype=torch.float32, device=x.device) for _ in range(2))
    hidden = torch.empty((B, Ch), dtype=torch.float32, device=x.device)
    y = torch.empty_like(x) if want_y else None
    ctx = _ctx_for(x)
    fn = _lib.lib().ps_channel_attention
    _two_call("ps_channel_attention", x.device, lambda scratch, n: fn(ctx.handle, runtime.ptr(x), B, V, C, Ch, runtime.ptr(w1), runtime.ptr(b1), runtime.ptr(w2),
                                                                      runtime.ptr(b2), runtime.ptr(mean), runtime.ptr(hidden), runtime.ptr(scale), runtime.ptr(y),
                                                                      scratch, n))
    return y, mean, hidden, scale


def channel_attention_backward(dy, x, mean, hidden, scale, w1, w2, need=("x", "w1", "b1", "w2", "b2")):
    """The gradients of channel_attention for the output gradient dy: a dict with the entries of `need`."""
    who = "channel_attention_backward"
    x, B, V, C = _rows(x, who, "x")
    dy = _f32(dy, who, "dy")
    w1, w2 = _f32(w1, who, "w1", 2), _f32(w2, who, "w2", 2)
    mean, hidden, scale = _f32(mean, who, "mean", 2), _f32(hidden, who, "hidden", 2), _f32(scale, who, "scale", 2)
    Ch = w1.shape[1]
    if dy.shape != x.shape or w1.shape[0] != C or tuple(w2.shape) != (Ch, C) or tuple(mean.shape) != (B, C) or tuple(scale.shape) != (B, C) \
            or tuple(hidden.shape) != (B, Ch):
        raise ValueError("channel_attention_backward: the shapes do not fit x %s" % (tuple(x.shape),))
    need = set(need)
    if not need or need - {"x", "w1", "b1", "w2", "b2"}:
        raise ValueError("channel_attention_backward: need must name some of x, w1, b1, w2, b2")
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=x.device)
    out = {"x": torch.empty_like(x) if "x" in need else None, "w1": new(C, Ch) if "w1" in need else None, "b1": new(Ch) if "b1" in need else None,
           "w2": new(Ch, C) if "w2" in need else None, "b2": new(C) if "b2" in need else None}
    ctx = _ctx_for(x)
    fn = _lib.lib().ps_channel_attention_bwd
    _two_call("ps_channel_attention_bwd", x.device, lambda scratch, n: fn(ctx.handle, runtime.ptr(x), runtime.ptr(dy), runtime.ptr(mean), runtime.ptr(hidden),
                                                                          runtime.ptr(scale), runtime.ptr(w1), runtime.ptr(w2), B, V, C, Ch,
                                                                          *(runtime.ptr(out[k]) for k in ("x", "w1", "b1", "w2", "b2")), scratch, n))
    return {k: v for k, v in out.items() if v is not None}


def spatial_gate(a1, a2, a3, f):
    """attention.py:148-152 and model.py:295: a1, a2, a3 [B, ...] (or [B, ..., 1]), f [B, ..., C] -> (y = f * sa, sa = sigmoid(a1 + a2 + a3))."""
    who = "spatial_gate"
    f, B, V, C = _rows(f, who, "f")
    a1, a2, a3 = _f32(a1, who, "a1"), _f32(a2, who, "a2"), _f32(a3, who, "a3")
    if not a1.numel() == a2.numel() == a3.numel() == B * V:
        raise ValueError("spatial_gate: a1, a2 and a3 must have one value per voxel of f %s" % (tuple(f.shape),))
    sa = torch.empty(f.shape[:-1], dtype=torch.float32, device=f.device)
    y = torch.empty_like(f)
    _lib.check(_lib.lib().ps_spatial_gate(_ctx_for(f).handle, runtime.ptr(a1), runtime.ptr(a2), runtime.ptr(a3), runtime.ptr(f), B, V, C, runtime.ptr(sa),
                                          runtime.ptr(y)))
    return y, sa


def spatial_gate_backward(dy, f, sa, need=("f", "a")):
    """The gradients of spatial_gate: {"f": dy * sa, "a": the gradient of each of a1, a2, a3 (one tensor, sa's shape)}; f is the value before the gate."""
    who = "spatial_gate_backward"
    f, B, V, C = _rows(f, who, "f")
    dy, sa = _f32(dy, who, "dy"), _f32(sa, who, "sa")
    if dy.shape != f.shape or sa.numel() != B * V:
        raise ValueError("spatial_gate_backward: dy %s and sa %s do not fit f %s" % (tuple(dy.shape), tuple(sa.shape), tuple(f.shape)))
    need = set(need)
    if not need or need - {"f", "a"}:
        raise ValueError("spatial_gate_backward: need must name some of f, a")
    df = torch.empty_like(f) if "f" in need else None
    da = torch.empty_like(sa) if "a" in need else None
    _lib.check(_lib.lib().ps_spatial_gate_bwd(_ctx_for(f).handle, runtime.ptr(dy), runtime.ptr(f), runtime.ptr(sa), B, V, C, runtime.ptr(df), runtime.ptr(da)))
    return {k: v for k, v in (("f", df), ("a", da)) if v is not None}


def _is_soft(labels):
    """Soft labels (include/pointseg_saliency_mixup.h): a float32 row of C values per voxel, where hard labels are one int32."""
    return labels.dtype == torch.float32


def _loss_args(who, logits, labels, weight):
    logits, B, V, C = _rows(logits, who, "logits")
    if not isinstance(labels, torch.Tensor) or labels.device != logits.device or labels.dtype not in (torch.int32, torch.float32):
        raise ValueError("%s: labels must be an int32 tensor, or a float32 tensor of soft labels, on the logits' device" % who)
    if labels.numel() != (B * V * C if _is_soft(labels) else B * V):
        raise ValueError("%s: labels must have one value per voxel of logits %s (soft labels: one per logit)" % (who, tuple(logits.shape)))
    if weight is not None:
        weight = _f32(weight, who, "weight")
        if weight.numel() != B * V:
            raise ValueError("%s: weight must have one value per voxel of logits %s" % (who, tuple(logits.shape)))
    return logits, labels.contiguous(), weight, B, V, C


def softmax_dice_loss(logits, labels, weight=None):
    """Loss / dice of model.py:491-548, 592-618 (weight_map branch): logits [B, ..., C], labels [B, ...] int32, weight [B, ...] or None
    (ones) -> (loss, a 0-dim device tensor; sums [B, C, 3] float64, what softmax_dice_loss_backward takes).  float32 labels [B, ..., C] are
    soft labels (mixup's): dice_mixup, model.py:550-590, 602-612."""
    who = "softmax_dice_loss"
    logits, labels, weight, B, V, C = _loss_args(who, logits, labels, weight)
    loss = torch.empty((), dtype=torch.float32, device=logits.device)
    sums = torch.empty((B, C, 3), dtype=torch.float64, device=logits.device)
    ctx = _ctx_for(logits)
    name = "ps_softmax_dice_soft_loss" if _is_soft(labels) else "ps_softmax_dice_loss"
    fn = getattr(_lib.lib(), name)
    _two_call(name, logits.device, lambda scratch, n: fn(ctx.handle, runtime.ptr(logits), runtime.ptr(labels), runtime.ptr(weight), B, V, C,
                                                                           runtime.ptr(loss), runtime.ptr(sums), scratch, n))
    return loss, sums


def softmax_dice_loss_backward(logits, labels, weight, sums, dloss=None):
    """d loss / d logits times dloss (a device tensor of one float32, handed over as a pointer; None: 1).  labels as softmax_dice_loss
    takes them, hard or soft."""
    who = "softmax_dice_loss_backward"
    logits, labels, weight, B, V, C = _loss_args(who, logits, labels, weight)
    if not isinstance(sums, torch.Tensor) or sums.device != logits.device or sums.dtype != torch.float64 or tuple(sums.shape) != (B, C, 3):
        raise ValueError("softmax_dice_loss_backward: sums must be the forward's [B, C, 3] float64 tensor")
    if dloss is not None:
        dloss = _f32(dloss, who, "dloss")
        if dloss.numel() != 1:
            raise ValueError("softmax_dice_loss_backward: dloss must hold one value")
    dlogits = torch.empty_like(logits)
    fn = _lib.lib().ps_softmax_dice_soft_loss_bwd if _is_soft(labels) else _lib.lib().ps_softmax_dice_loss_bwd
    _lib.check(fn(_ctx_for(logits).handle, runtime.ptr(logits), runtime.ptr(labels), runtime.ptr(weight), runtime.ptr(sums.contiguous()), runtime.ptr(dloss),
                  B, V, C, runtime.ptr(dlogits)))
    return dlogits


class ChannelAttentionFunction(torch.autograd.Function):
    """channel_attention with its gradients.  Saves x, the two kernels and the forward's mean, hidden and scale."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2):
        y, mean, hidden, scale = channel_attention(x, w1, b1, w2, b2)
        ctx.save_for_backward(x, w1, w2, mean, hidden, scale)
        ctx.mark_non_differentiable(hidden)
        return y, hidden

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy, _dhidden):
        x, w1, w2, mean, hidden, scale = ctx.saved_tensors
        need = [n for n, wanted in zip(("x", "w1", "b1", "w2", "b2"), ctx.needs_input_grad) if wanted]
        g = channel_attention_backward(dy, x, mean, hidden, scale, w1, w2, need) if need else {}
        return tuple(g.get(n) for n in ("x", "w1", "b1", "w2", "b2"))


class SpatialGateFunction(torch.autograd.Function):
    """spatial_gate with its gradients.  Saves f (before the gate) and sa."""

    @staticmethod
    def forward(ctx, a1, a2, a3, f):
        y, sa = spatial_gate(a1, a2, a3, f)
        ctx.save_for_backward(f, sa)
        ctx.shapes = (a1.shape, a2.shape, a3.shape)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        f, sa = ctx.saved_tensors
        wanted = ctx.needs_input_grad
        need = (["a"] if any(wanted[:3]) else []) + (["f"] if wanted[3] else [])
        g = spatial_gate_backward(dy, f, sa, need) if need else {}
        da = g.get("a")
        return tuple(da.reshape(s) if da is not None and w else None for s, w in zip(ctx.shapes, wanted[:3])) + (g.get("f"),)


class SoftmaxDiceLossFunction(torch.autograd.Function):
    """softmax_dice_loss with its gradient.  Saves the logits, the labels, the weight and the forward's sums; the upstream gradient stays on
    the device."""

    @staticmethod
    def forward(ctx, logits, labels, weight):
        loss, sums = softmax_dice_loss(logits, labels, weight)
        ctx.save_for_backward(logits, labels, weight, sums)
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dloss):
        logits, labels, weight, sums = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None, None
        return softmax_dice_loss_backward(logits, labels, weight, sums, dloss.to(torch.float32)), None, None


def differentiable_channel_attention(x, w1, b1, w2, b2, with_hidden=False):
    """channel_attention's y, recorded by torch.autograd (with_hidden: (y, hidden), hidden detached -- the dense ReLU's mask)."""
    y, hidden = ChannelAttentionFunction.apply(x, w1, b1, w2, b2)
    return (y, hidden) if with_hidden else y


def differentiable_spatial_gate(a1, a2, a3, f):
    """spatial_gate's y, recorded by torch.autograd."""
    return SpatialGateFunction.apply(a1, a2, a3, f)


def differentiable_softmax_dice_loss(logits, labels, weight=None):
    """softmax_dice_loss's loss (0-dim, on the device), recorded by torch.autograd.  The labels, hard or soft, receive no gradient."""
    return SoftmaxDiceLossFunction.apply(logits, labels, weight)


class TrainableSaliencyNet(torch.nn.Module):
    """unet3d_attention (model.py:176-314) composed from the differentiable ops above: one torch.nn.Parameter per entry of param_shapes,
    under the same name, so torch.autograd and a torch optimiser train it on this package's kernels.  params: the TF-named dict.
    precision: the arithmetic of every convolution and of its two gradients -- "fp32", "bf16x3" or "bf16"
    (include/pointseg_saliency_train_precision.h), or a triple (forward, data_grad, weight_grad) of those names, one per role;
    everything between the convolutions stays fp32, as in SaliencyNet.  One difference from
    SaliencyNet: here the channel attention scales the ACTIVATION in front of C345_conv, where inference folds the scale into that layer's
    kernel; under "bf16" this graph therefore rounds the scaled activation (and the plain kernel), inference the activation and the scaled
    kernel."""

    def __init__(self, params, in_channels, num_classes=2, device=0, precision="fp32"):
        super().__init__()
        _precision("TrainableSaliencyNet", precision)
        self.precision = precision
        self.in_channels, self.num_classes = int(in_channels), int(num_classes)
        self.device = torch.device("cuda", device)
        flat = flatten_params(params, self.in_channels, self.num_classes)  # (checks the names and the shapes)
        for name, a in unflatten_params(flat, self.in_channels, self.num_classes).items():
            self.register_parameter(name, torch.nn.Parameter(torch.from_numpy(np.ascontiguousarray(a)).to(self.device)))

    def logits(self, x, masks=None):
        """The logits [B, D, H, W, num_classes] of a patch [B, D, H, W, C_in] (extents multiples of 16).  masks: a dict that receives, per
        layer name, the ReLU's mask of this forward (y > 0; the channel attention's hidden layer under its dense_1 name)."""
        x = _f32(x, "TrainableSaliencyNet", "x", 5)
        if x.shape[4] != self.in_channels or any(n % 16 or n < 16 for n in x.shape[1:4]):
            raise ValueError("TrainableSaliencyNet: x must be [B, D, H, W, %d] with extents that are multiples of 16, got %s" % (self.in_channels, tuple(x.shape)))
        P = dict(self.named_parameters())

        def conv(name, t, stride=1, dilation=1, norm=True, x2=None, up=1):
            n = SCOPE + name
            y = differentiable_conv3d(t, P[n + "/kernel"], P.get(n + "/bias"), stride, dilation, x2, up, self.precision)
            if not norm:
                return y
            y = differentiable_instance_norm_relu(y, P[n + "/ins_norm/gamma"], P[n + "/ins_norm/beta"])
            if masks is not None:
                masks[name] = y.detach() > 0
            return y

        def cfe(prefix, t):  # CFE3D, model.py:154-174: the four branches meet in a torch.cat (reduced resolution)
            return torch.cat([conv(prefix + "_cfe0", t)] + [conv("%s_cfe%d_dilation" % (prefix, r), t, dilation=d) for r, d in ((1, 3), (2, 5), (3, 7))], -1)

        layer = conv("init_conv", x)
        down = []
        for d in range(5):
            l_in = layer
            for i in range(2):
                layer = conv("down%d_conv_%d" % (d, i), layer)
            layer = l_in + layer
            down.append(layer)
            if d != 4:
                layer = conv("stride2conv%d" % d, layer, stride=2)
        C1 = conv("C1_conv", down[0])
        C2 = conv("C2_conv", down[1])
        C3 = cfe("C3_cfe", down[2])
        C4 = conv("up_conv1_C4_cfe_up2", cfe("C4_cfe", down[3]), up=2)
        C5 = conv("up_conv1_C5_cfe_up4", cfe("C5_cfe", down[4]), up=4)
        ca = SCOPE + _CA
        C345, hidden = differentiable_channel_attention(torch.cat([C3, C4, C5], -1), P[ca + "_dense_1/kernel"], P[ca + "_dense_1/bias"],
                                                        P[ca + "_dense_2/kernel"], P[ca + "_dense_2/bias"], with_hidden=True)
        if masks is not None:
            masks[_CA + "_dense_1"] = hidden > 0
        C345 = conv("up_conv1_C345_up4", conv("C345_conv", C345), up=4)
        a = [conv("spatial_attention_%d_conv2" % i, conv("spatial_attention_%d_conv1" % i, C345)) for i in (1, 2, 3)]
        C12 = conv("C12_conv", C1, x2=conv("up_conv1_C2_up2", C2, up=2))
        C12 = differentiable_spatial_gate(a[0], a[1], a[2], C12)
        return conv("final", C12, norm=False, x2=C345)

    def loss(self, x, labels, weight=None, masks=None):
        """The reference's training loss (train.py:83-110 without the regulariser, which reference_optimizer carries as weight decay).
        labels: [B, D, H, W] int32, or soft labels float32 [B, D, H, W, num_classes] (PatchBank.sample(mixup=...))."""
        return differentiable_softmax_dice_loss(self.logits(x, masks), labels, weight)

    def export(self, precision=None):
        """The parameters as the TF-named dict of float32 numpy arrays that SaliencyNet takes; with precision ("fp32" | "bf16x3" | "bf16":
        one name, inference has one role), the SaliencyNet of them at that precision, on this net's device; with precision="forward", at
        the precision this net's forward runs at (the first name of a triple)."""
        params = {name: p.detach().cpu().numpy() for name, p in self.named_parameters()}
        if precision is None:
            return params
        if precision == "forward":
            precision = self.precision[0] if isinstance(self.precision, (tuple, list)) else self.precision
        return SaliencyNet(params, self.in_channels, self.num_classes, self.device.index, precision)


def reference_optimizer(net, lr=0.01):
    """train.py:50-56, 102-107: tf.train.MomentumOptimizer(lr, 0.9) on the loss plus tensorpack's l2_regularizer(1e-5) of every `kernel`
    variable (the two dense kernels included).  The regulariser is tf.nn.l2_loss, whose gradient is 1e-5 * w: torch's weight_decay; and
    TensorFlow's accum = 0.9 * accum + g, var -= lr * accum is torch.optim.SGD's momentum rule.  Biases, gammas and betas do not decay."""
    named = list(net.named_parameters())
    decay = [p for n, p in named if n.endswith("/kernel")]
    rest = [p for n, p in named if not n.endswith("/kernel")]
    return torch.optim.SGD([{"params": decay, "weight_decay": 1e-5}, {"params": rest, "weight_decay": 0.0}], lr=lr, momentum=0.9)


# ---- the training step behind one call (include/pointseg_saliency_step.h, csrc/saliency_step.hip) ----------------------------------------------------

class SaliencyTrainer:
    """unet3d_attention trained without torch.autograd: the flat parameters `flat`, this rank's gradients `grad`, the momentum `accum` and
    the cached scratch are device tensors, and one call of ps_saliency_train_step is a step of train.py:83-110 (forward, softmax + Dice, the
    whole backward, the optional gradient all-reduce, the momentum update with the regulariser).  params: the TF-named dict.
    precision: the arithmetic of the step's convolutions -- "fp32", "bf16x3" or "bf16", or a triple (forward, data_grad, weight_grad) of
    those names, one per role (include/pointseg_saliency_step_precision.h); backward and step run ps_saliency_backward_prec and
    ps_saliency_train_step_prec with it, and "fp32" gives the bytes of the entries without a precision."""

    def __init__(self, params, in_channels, num_classes=2, device=0, momentum=0.9, l2=1e-5, precision="fp32"):
        self._prec = _precision("SaliencyTrainer", precision)
        self.precision = precision
        self.in_channels, self.num_classes = int(in_channels), int(num_classes)
        self.momentum, self.l2 = float(momentum), float(l2)
        flat = flatten_params(params, self.in_channels, self.num_classes)
        want = _lib.lib().ps_saliency_weight_count(self.in_channels, self.num_classes)
        if want != flat.size:
            raise _lib.PointSegError("SaliencyTrainer: the library's network has %d weights, this package's layer table %d" % (want, flat.size))
        self.device = torch.device("cuda", device)
        self.flat = torch.from_numpy(flat).to(self.device)
        self.grad = torch.zeros_like(self.flat)
        self.accum = torch.zeros_like(self.flat)
        self.loss = torch.zeros((), dtype=torch.float32, device=self.device)
        self.scratch = None
        self.scratch_bytes = 0
        self._coll = None

    def _args(self, x, labels, weight):
        who = "SaliencyTrainer"
        x = _f32(x, who, "x", 5)
        if x.shape[4] != self.in_channels or any(n % 16 or n < 16 for n in x.shape[1:4]):
            raise ValueError("SaliencyTrainer: x must be [B, D, H, W, %d] with extents that are multiples of 16, got %s" % (self.in_channels, tuple(x.shape)))
        logits = torch.empty(tuple(x.shape[:4]) + (self.num_classes,), dtype=torch.float32, device=x.device)
        _, labels, weight, _, _, _ = _loss_args(who, logits, labels, weight)
        return x, labels, weight, logits

    def _call(self, fn, x, head, tail, soft):
        """fn(ctx, *head, B, D, H, W, C_in, num_classes, *tail, scratch, &bytes, soft, *the three precisions) under the two-call protocol, on
        this trainer's own scratch."""
        ctx = _ctx_for(x)
        shape = tuple(x.shape[:4]) + (self.in_channels, self.num_classes)
        modes = (soft,) + self._prec
        need = ctypes.c_int64(0)
        _lib.check(fn(None, *head, *shape, *tail, None, ctypes.byref(need), *modes))
        if self.scratch is None or self.scratch.numel() < need.value:
            self.scratch = torch.empty(max(need.value, 1), dtype=torch.uint8, device=x.device)
        self.scratch_bytes = need.value
        _lib.check(fn(ctx.handle, *head, *shape, *tail, runtime.ptr(self.scratch), ctypes.byref(need), *modes))

    def backward(self, x, labels, weight=None, want_logits=False):
        """The loss (0-dim, on the device; overwritten by the next call) of a patch x [B, D, H, W, C_in] with labels [B, D, H, W] int32 (or
        soft labels float32 [B, D, H, W, num_classes]: soft_labels = 1) and weight [B, D, H, W] or None, its gradients left in `grad`; no
        parameter changes.  want_logits: (loss, logits)."""
        x, labels, weight, logits = self._args(x, labels, weight)
        p = runtime.ptr
        self._call(_lib.lib().ps_saliency_backward_prec, x, (p(x), p(labels), p(weight)),
                   (p(self.flat), self.flat.numel(), p(self.grad), p(self.loss), p(logits) if want_logits else None), int(_is_soft(labels)))
        return (self.loss, logits) if want_logits else self.loss

    def _collective(self, dist):
        """torch.distributed's all-reduce as the C callback, exactly as train.Trainer._collective wraps it: the raw device pointer, on the
        context's stream (= torch's current stream), becomes a tensor without a copy through __cuda_array_interface__."""
        if self._coll is not None and self._coll[1] is dist:
            return self._coll[0]
        device = self.device

        class _Raw:
            def __init__(self, ptr, count, f64):
                self.__cuda_array_interface__ = {"shape": (int(count),), "typestr": "<f8" if f64 else "<f4", "data": (int(ptr), False), "version": 2}

        def cb(user, buf, count, dtype, stream):
            try:
                t = torch.as_tensor(_Raw(buf, count, dtype == 1), device=device)
                dist.all_reduce(t)
                return 0
            except Exception as e:  # never let an exception cross the C boundary
                import sys
                print("all-reduce callback failed: %r" % (e,), file=sys.stderr)
                return 1

        fn = _lib.PS_ALLREDUCE_FN(cb)
        self._coll = (fn, dist)
        return fn

    def step(self, x, labels, weight, lr, dist=None, allreduce=None, world_size=None):
        """One training step at learning rate lr (labels hard or soft, as backward takes them); returns the loss before it.  dist: a torch.distributed-like module (all_reduce,
        get_world_size) whose sum the gradients go through when the world has more than one rank.  allreduce / world_size: a ready
        PS_ALLREDUCE_FN and its world instead (a host that brings its own collective)."""
        x, labels, weight, _ = self._args(x, labels, weight)
        if dist is not None:
            allreduce, world_size = self._collective(dist), dist.get_world_size()
        opt = _lib.PsSaliencyStepOptions(allreduce if allreduce is not None else _lib.PS_ALLREDUCE_FN(), None, int(world_size or 1), self.momentum, self.l2)
        p = runtime.ptr
        self._call(_lib.lib().ps_saliency_train_step_prec, x, (p(x), p(labels), p(weight)),
                   (p(self.flat), self.flat.numel(), p(self.grad), p(self.accum), float(lr), ctypes.byref(opt), p(self.loss), None), int(_is_soft(labels)))
        return self.loss

    def update(self, lr, grad_scale=1.0):
        """ps_saliency_sgd_update on flat / grad / accum."""
        p = runtime.ptr
        ctx = runtime.default_context(self.device.index)
        ctx.use_torch_stream()
        _lib.check(_lib.lib().ps_saliency_sgd_update(ctx.handle, p(self.flat), p(self.grad), p(self.accum), self.in_channels, self.num_classes, self.flat.numel(),
                                                     float(lr), self.momentum, self.l2, float(grad_scale)))

    def _named(self, flat):
        out, off = {}, 0
        for name, shape in param_shapes(self.in_channels, self.num_classes).items():
            n = int(np.prod(shape))
            out[name] = flat[off:off + n].view(shape)
            off += n
        return out

    def named_gradients(self):
        """name -> a view of `grad`, by TensorFlow name."""
        return self._named(self.grad)

    def named_parameters(self):
        """name -> a view of `flat`, by TensorFlow name."""
        return self._named(self.flat)

    def export(self):
        """The parameters as the TF-named dict of float32 numpy arrays that SaliencyNet takes."""
        return unflatten_params(self.flat.cpu().numpy(), self.in_channels, self.num_classes)
