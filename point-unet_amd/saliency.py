"""The saliency attention map in front of prepare.pancreas_mask: the reference's SaliencyAttention network (`unet3d_attention`,
SaliencyAttention/model.py:176-314 with attention.py:79-174) run patch by patch over a volume (`overlapping_inference`,
SaliencyAttention/eval.py:103-193), on the device -- include/pointseg_saliency.h, csrc/conv3d.hip, csrc/saliency.hip.  The network runs for inference only; the gradients of its convolution and
of its instance norm + ReLU (include/pointseg_saliency_train.h, csrc/conv3d_train.hip) stand at the end of this module, op by op.

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


def _same_out(n, stride):
    return -(-n // stride)


def conv3d(x, w, bias=None, stride=1, dilation=1, x2=None, up=1):
    """tf.layers.conv3d(x, padding="SAME") without activation: x [B, D, H, W, C1] (and x2 [B, D, H, W, C2], concatenated behind it on the
    channel axis; both up-sampled `up` times by repetition first), w [kd, kh, kw, C1 + C2, C_out], bias [C_out] or None.  CUDA float32."""
    who = "conv3d"
    x = _f32(x, who, "x", 5)
    w = _f32(w, who, "w", 5)
    B, Ds, Hs, Ws, C1 = x.shape
    C2 = 0
    if x2 is not None:
        x2 = _f32(x2, who, "x2", 5)
        if x2.shape[:4] != x.shape[:4]:
            raise ValueError("conv3d: x2 must have x's batch and extents")
        C2 = x2.shape[4]
    if w.shape[3] != C1 + C2:
        raise ValueError("conv3d: w has %d input channels, the input %d" % (w.shape[3], C1 + C2))
    if bias is not None:
        bias = _f32(bias, who, "bias", 1)
        if bias.shape[0] != w.shape[4]:
            raise ValueError("conv3d: bias must have C_out values")
    y = torch.empty((B, _same_out(Ds * up, stride), _same_out(Hs * up, stride), _same_out(Ws * up, stride), w.shape[4]), dtype=torch.float32,
                    device=x.device)
    ctx = runtime.default_context(x.device.index)
    ctx.use_torch_stream()
    _lib.check(_lib.lib().ps_conv3d(ctx.handle, runtime.ptr(x), runtime.ptr(x2), B, Ds, Hs, Ws, C1, C2, up, runtime.ptr(w), runtime.ptr(bias), w.shape[0],
                                    w.shape[1], w.shape[2], w.shape[4], stride, dilation, runtime.ptr(y)))
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
    ctx = runtime.default_context(x.device.index)
    ctx.use_torch_stream()
    fn = _lib.lib().ps_instance_norm_relu
    need = ctypes.c_int64(0)
    _lib.check(fn(ctx.handle, None, B, V, C, None, None, eps, None, None, ctypes.byref(need)))
    buf = _scratch_for(("ps_instance_norm_relu", x.device.index), need.value, x.device)
    _lib.check(fn(ctx.handle, runtime.ptr(x), B, V, C, runtime.ptr(gamma), runtime.ptr(beta), eps, runtime.ptr(y), runtime.ptr(buf), ctypes.byref(need)))
    return y


# ---- the network ---------------------------------------------------------------------------------------------------------------------------------

class SaliencyNet:
    """unet3d_attention for inference.  params: the TF-named dict (see the module's docstring); the weights live on `device` as one flat
    buffer.  A patch is [B, D, H, W, C_in] (or [D, H, W, C_in]) CUDA float32 with D, H, W multiples of 16."""

    def __init__(self, params, in_channels, num_classes=2, device=0):
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
        ctx = runtime.default_context(x.device.index)
        ctx.use_torch_stream()
        fn = _lib.lib().ps_saliency_forward
        need = ctypes.c_int64(0)
        n = self.weights.numel()
        _lib.check(fn(ctx.handle, None, B, D, H, W, self.in_channels, K, None, n, None, None, None, None, ctypes.byref(need)))
        buf = _scratch_for(("ps_saliency_forward", x.device.index), need.value, x.device)
        self.scratch_bytes = need.value
        _lib.check(fn(ctx.handle, runtime.ptr(x), B, D, H, W, self.in_channels, K, runtime.ptr(self.weights), n, runtime.ptr(logits), runtime.ptr(probs),
                      ctypes.byref(tp) if tp is not None else None, runtime.ptr(buf), ctypes.byref(need)))
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


def saliency_map(volume, net, patch=(64, 160, 160), steps=(48, 118, 118)):
    """overlapping_inference (eval.py:103-193) on the device: volume [C_in, D, H, W] or [D, H, W] (CUDA float32) -> the window-averaged
    softmax probabilities [D, H, W, num_classes].  A window that overhangs the volume is zero-filled and its prediction cut back to the
    part inside.  The reference feeds BATCH_SIZE copies of the window and keeps pred[0]; with instance norm the samples of a batch do not
    see each other, so one copy gives the same result.  The window loop runs on the host; nothing is read back."""
    who = "saliency_map"
    v = _f32(volume, who, "volume")
    if v.dim() == 3:
        v = v[None]
    if v.dim() != 4 or v.shape[0] != net.in_channels:
        raise ValueError("saliency_map: volume must be [%d, D, H, W] or [D, H, W], got %s" % (net.in_channels, tuple(volume.shape)))
    if len(patch) != 3 or len(steps) != 3 or min(steps) < 1 or any(p % 16 or p < 16 for p in patch):
        raise ValueError("saliency_map: patch %s (multiples of 16) / steps %s (>= 1)" % (tuple(patch), tuple(steps)))
    C, D, H, W = v.shape
    K = net.num_classes
    vol = v.permute(1, 2, 3, 0).contiguous()  # [D, H, W, C]: np.rollaxis(image, 0, 4)
    total = torch.zeros((D, H, W, K), dtype=torch.float32, device=v.device)
    count = torch.zeros((D, H, W), dtype=torch.int32, device=v.device)
    crop = torch.empty((1,) + tuple(patch) + (C,), dtype=torch.float32, device=v.device)
    ctx = runtime.default_context(v.device.index)
    lib = _lib.lib()
    for o0 in window_origins(D, patch[0], steps[0]):
        for o1 in window_origins(H, patch[1], steps[1]):
            for o2 in window_origins(W, patch[2], steps[2]):
                part = vol[o0:o0 + patch[0], o1:o1 + patch[1], o2:o2 + patch[2]]
                if tuple(part.shape[:3]) != tuple(patch):
                    crop.zero_()
                crop[0, :part.shape[0], :part.shape[1], :part.shape[2]] = part
                p = net.probs(crop)
                _lib.check(lib.ps_saliency_accumulate(ctx.handle, runtime.ptr(p), patch[0], patch[1], patch[2], K, o0, o1, o2, D, H, W,
                                                      runtime.ptr(total), runtime.ptr(count)))
    _lib.check(lib.ps_saliency_finish(ctx.handle, runtime.ptr(total), runtime.ptr(count), D, H, W, K, runtime.ptr(total)))
    return total


# ---- the gradients of the two op wrappers (include/pointseg_saliency_train.h, csrc/conv3d_train.hip) ---------------------------------------------

def _two_call(name, dev, call):
    """The two-call scratch protocol: call(None, byref(need)) sizes (it looks at the shapes alone), then the same call runs on the
    cached buffer."""
    need = ctypes.c_int64(0)
    _lib.check(call(None, ctypes.byref(need)))
    buf = _scratch_for((name, dev.index), need.value, dev)
    _lib.check(call(runtime.ptr(buf), ctypes.byref(need)))


def conv3d_backward(dy, x, w, stride=1, dilation=1, x2=None, up=1, need=("x", "x2", "w", "bias")):
    """The gradients of conv3d(x, w, bias, stride, dilation, x2, up) for the output gradient dy: a dict with the entries of `need` --
    "x" [like x], "x2" [like x2; only with x2], "w" [like w], "bias" [C_out].  Arguments are checked as conv3d checks them."""
    who = "conv3d_backward"
    x = _f32(x, who, "x", 5)
    w = _f32(w, who, "w", 5)
    dy = _f32(dy, who, "dy", 5)
    B, Ds, Hs, Ws, C1 = x.shape
    C2 = 0
    if x2 is not None:
        x2 = _f32(x2, who, "x2", 5)
        if x2.shape[:4] != x.shape[:4]:
            raise ValueError("conv3d_backward: x2 must have x's batch and extents")
        C2 = x2.shape[4]
    if w.shape[3] != C1 + C2:
        raise ValueError("conv3d_backward: w has %d input channels, the input %d" % (w.shape[3], C1 + C2))
    want = (B, _same_out(Ds * up, stride), _same_out(Hs * up, stride), _same_out(Ws * up, stride), w.shape[4])
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
    ctx = runtime.default_context(x.device.index)
    ctx.use_torch_stream()
    geometry = (B, Ds, Hs, Ws, C1, C2, up, w.shape[0], w.shape[1], w.shape[2], w.shape[4], stride, dilation)
    if need & {"x", "x2"}:
        dx = torch.empty_like(x) if "x" in need else None
        dx2 = torch.empty_like(x2) if "x2" in need else None
        fn = _lib.lib().ps_conv3d_bwd_data
        _two_call("ps_conv3d_bwd_data", x.device, lambda scratch, n: fn(ctx.handle, runtime.ptr(dy), runtime.ptr(w), *geometry, runtime.ptr(dx),
                                                                        runtime.ptr(dx2), scratch, n))
        if dx is not None:
            out["x"] = dx
        if dx2 is not None:
            out["x2"] = dx2
    if need & {"w", "bias"}:
        dw = torch.empty_like(w) if "w" in need else None
        db = torch.empty((w.shape[4],), dtype=torch.float32, device=x.device) if "bias" in need else None
        fn = _lib.lib().ps_conv3d_bwd_weight
        _two_call("ps_conv3d_bwd_weight", x.device, lambda scratch, n: fn(ctx.handle, runtime.ptr(x), runtime.ptr(x2), runtime.ptr(dy), *geometry,
                                                                          runtime.ptr(dw), runtime.ptr(db), scratch, n))
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
    ctx = runtime.default_context(x.device.index)
    ctx.use_torch_stream()
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
    """conv3d with its gradients: forward ps_conv3d, backward ps_conv3d_bwd_data and ps_conv3d_bwd_weight.  Saves x, x2 and w."""

    @staticmethod
    def forward(ctx, x, w, bias, stride, dilation, x2, up):
        ctx.save_for_backward(x, x2, w)
        ctx.geometry = (stride, dilation, up)
        return conv3d(x, w, bias, stride, dilation, x2, up)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, x2, w = ctx.saved_tensors
        stride, dilation, up = ctx.geometry
        wanted = ctx.needs_input_grad
        need = [name for name, i in (("x", 0), ("w", 1), ("bias", 2), ("x2", 5)) if wanted[i] and (name != "x2" or x2 is not None)]
        g = conv3d_backward(dy, x, w, stride, dilation, x2, up, need) if need else {}
        return g.get("x"), g.get("w"), g.get("bias"), None, None, g.get("x2"), None


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


def differentiable_conv3d(x, w, bias=None, stride=1, dilation=1, x2=None, up=1):
    """conv3d, recorded by torch.autograd."""
    return Conv3dFunction.apply(x, w, bias, stride, dilation, x2, up)


def differentiable_instance_norm_relu(x, gamma, beta, eps=EPS):
    """instance_norm_relu, recorded by torch.autograd."""
    return InstanceNormReluFunction.apply(x, gamma, beta, eps)
