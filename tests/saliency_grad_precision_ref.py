"""What include/pointseg_saliency_train_precision.h's PS_PREC_BF16 mode computes for the convolution's gradients, restated on the CPU next
to saliency_precision_ref.py (no GPU here): torch.autograd.grad through saliency_ref.conv3d_same / upsample / torch.cat in `dtype`, on
operands rounded to bfloat16 the way the kernels round them.

Which elements a gradient rounds: the data gradient dy (as the gather fetches it) and the kernel w; the weight gradient the convolution's
input as ps_conv3d fetches it -- the concat and the up-sampling copy values, so rounding the sources is the same thing; a padding tap is 0
either way -- and dy; the bias gradient is the weight gradient's row of ones, the sum of the ROUNDED dy.  A gradient is linear in dy and in
the other operand, so it is the exact gradient evaluated at the rounded operands.  With `rounded=False` each function gives the
exact-operand gradient (what PS_PREC_BF16X3 is held to)."""
import torch

import saliency_precision_ref as pref
import saliency_ref as ref


def _operand(t, dtype, rounded):
    return (pref.round_bf16(t) if rounded else t).to(dtype)


def data_grad_rounded(dy, w, in_shape, stride=1, dilation=1, up=1, c1=None, dtype=torch.float64, rounded=True):
    """The gradient of conv3d_same(upsample(cat(x, x2), up), w, stride, dilation) for x (and x2) at round_bf16(dy), round_bf16(w).
    dy, w: float32 tensors; in_shape: (B, Ds, Hs, Ws) of the source; the sources have w.shape[3] channels, the first c1 of them x's.
    Returns (dx, dx2), dx2 None without c1."""
    cin = w.shape[3]
    c1 = cin if c1 is None else c1
    x = torch.zeros(tuple(in_shape) + (c1,), dtype=dtype, requires_grad=True)
    x2 = torch.zeros(tuple(in_shape) + (cin - c1,), dtype=dtype, requires_grad=True) if c1 < cin else None
    inp = x if x2 is None else torch.cat([x, x2], -1)
    y = ref.conv3d_same(ref.upsample(inp, up) if up > 1 else inp, _operand(w, dtype, rounded), None, stride, dilation)
    g = torch.autograd.grad(y, [x] if x2 is None else [x, x2], _operand(dy, dtype, rounded))
    return g[0], (g[1] if x2 is not None else None)


def weight_grad_rounded(x, x2, up, dy, kernel, stride=1, dilation=1, dtype=torch.float64, rounded=True):
    """The gradient of the same convolution for its kernel (extents `kernel` = (kd, kh, kw)) at the rounded materialised input and the
    rounded dy.  x, x2 (or None), dy: float32 tensors."""
    inp = x if x2 is None else torch.cat([x, x2], -1)
    full = _operand(ref.upsample(inp, up) if up > 1 else inp, dtype, rounded)
    w = torch.zeros(tuple(kernel) + (inp.shape[-1], dy.shape[-1]), dtype=dtype, requires_grad=True)
    y = ref.conv3d_same(full, w, None, stride, dilation)
    return torch.autograd.grad(y, w, _operand(dy, dtype, rounded))[0]


def bias_grad_rounded(dy, dtype=torch.float64, rounded=True):
    """The sum of round_bf16(dy) over everything but the channel."""
    return _operand(dy, dtype, rounded).reshape(-1, dy.shape[-1]).sum(0)
