"""What include/pointseg_saliency_precision.h's two reduced modes compute, restated on the CPU next to saliency_ref.py (no GPU here):
the bfloat16 rounding and the exact three-way truncating split of an operand element, a convolution on rounded operands, and the whole
network in float64 with every convolution's operands rounded the way PS_PREC_BF16 rounds them.

Which elements a convolution rounds: its activation as fetched (the concat and the up-sampling copy values, so rounding the materialised
input is the same thing; a padding tap is 0 either way) and its kernel as the convolution receives it.  C345_conv receives the per-sample
kernel fl32(scale[b, ci] * w[ci, co]) -- the channel attention's scale folded in, formed in float32 -- so forward_rounded rounds C345's
activation and that float32 product, not the scaled activation."""
import numpy as np
import torch

import saliency_ref as ref

SCOPE = ref.SCOPE


def round_bf16(t):
    """Each element to the nearest bfloat16, ties to even, back in t's dtype (float32 or float64 tensors)."""
    return t.to(torch.float32).to(torch.bfloat16).to(t.dtype)


def split3(x):
    """The truncating split of float32 numpy values: p1 = x with its low 16 bits cleared, p2 = (x - p1) likewise, p3 = x - p1 - p2.  Every
    subtraction is exact, each piece is a bfloat16, and p1 + p2 + p3 == x."""
    x = np.asarray(x, np.float32)

    def trunc(v):
        return (v.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)

    p1 = trunc(x)
    r = x - p1
    p2 = trunc(r)
    return p1, p2, r - p2


def conv3d_rounded(x, w, bias=None, stride=1, dilation=1, dtype=torch.float64):
    """saliency_ref.conv3d_same in `dtype` on operands rounded to bfloat16 (x, w float32 tensors); the bias is not rounded."""
    return ref.conv3d_same(round_bf16(x).to(dtype), round_bf16(w).to(dtype), None if bias is None else bias.to(dtype), stride, dilation)


def forward_rounded(params, x):
    """saliency_ref.forward in float64 with the operands of every convolution rounded as PS_PREC_BF16 rounds them.  Everything between the
    convolutions (norms, dense layers, gate) stays float64."""
    dtype = torch.float64
    P = {k: torch.from_numpy(np.asarray(v)).to(dtype) for k, v in params.items()}
    x = torch.from_numpy(np.asarray(x)).to(dtype)
    assert x.dim() == 5 and all(n % 16 == 0 and n >= 16 for n in x.shape[1:4])

    def conv(name, t, stride=1, dilation=1, norm=True):
        n = SCOPE + name
        y = ref.conv3d_same(round_bf16(t), round_bf16(P[n + "/kernel"]), P.get(n + "/bias"), stride, dilation)
        return ref.instance_norm_relu(y, P[n + "/ins_norm/gamma"], P[n + "/ins_norm/beta"]) if norm else y

    def up_conv(prefix, t, scale):
        return conv("up_conv1_" + prefix, ref.upsample(t, scale))

    def cfe(prefix, t):
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
    C4 = up_conv("C4_cfe_up2", cfe("C4_cfe", down[3]), 2)
    C5 = up_conv("C5_cfe_up4", cfe("C5_cfe", down[4]), 4)
    C345 = torch.cat([C3, C4, C5], -1)
    ca = SCOPE + "C345_ChannelWiseAttention_withcpfe"
    a = C345.mean((1, 2, 3))
    a = torch.relu(a @ P[ca + "_dense_1/kernel"] + P[ca + "_dense_1/bias"])
    a = torch.sigmoid(a @ P[ca + "_dense_2/kernel"] + P[ca + "_dense_2/bias"])
    # C345_conv on the per-sample folded kernel: the float32 product of the float32 scale and the float32 kernel, then rounded
    n = SCOPE + "C345_conv"
    wk = P[n + "/kernel"].to(torch.float32)[0, 0, 0]  # [384, 64]
    folded = (a.to(torch.float32)[:, :, None] * wk[None]).to(dtype)  # [B, 384, 64]
    y = torch.einsum("bdhwc,bco->bdhwo", round_bf16(C345), round_bf16(folded)) + P[n + "/bias"]
    C345 = ref.instance_norm_relu(y, P[n + "/ins_norm/gamma"], P[n + "/ins_norm/beta"])
    C345 = up_conv("C345_up4", C345, 4)
    SA = torch.sigmoid(sum(conv("spatial_attention_%d_conv2" % i, conv("spatial_attention_%d_conv1" % i, C345)) for i in (1, 2, 3)))
    C2 = up_conv("C2_up2", C2, 2)
    C12 = conv("C12_conv", torch.cat([C1, C2], -1)) * SA
    return conv("final", torch.cat([C12, C345], -1), norm=False).numpy()
