"""torch-CPU restatement of the reference's saliency attention network for inference -- `unet3d_attention`
(SaliencyAttention/model.py:176-314, attention.py:79-174, custom_ops.py:29-82; config.DEPTH = 5, FILTER_GROW, RESIDUAL, INSTANCE_NORM,
CA_attention and SA_attention on) -- and a numpy restatement of the rule of `overlapping_inference` (SaliencyAttention/eval.py:103-193).
The yardstick of include/pointseg_saliency.h: float64 is what the kernels are compared with, float32 sizes the bars.

PARITY UNPINNED.  TensorFlow, tensorpack and keras are not installed here, so nothing below was ever compared with the reference running:
it is written from the reference's call sites and TensorFlow's documented rules (padding="SAME", tf.nn.moments' biased variance,
UpSampling3D's repetition), like rows A4-A13 of DESIGN.md.

Layout: activations [B, D, H, W, C] (channels last), kernels [kd, kh, kw, C_in, C_out], parameters by the names of
point_unet_amd.saliency.param_shapes.  The spatial extents must be multiples of 16: four stride-2 convolutions halve them (SAME: ceil), and
the results are up-sampled back by 2 and 4 and concatenated with the unhalved ones, which only fits when every halving was exact."""
import numpy as np
import torch
import torch.nn.functional as F

SCOPE = "unet3d_attention/"
EPS = 1e-5


def same_padding(n, k, stride=1, dilation=1):
    """tf.layers.conv3d(padding="SAME") on one axis: (out, pad_before, pad_after)."""
    out = -(-n // stride)
    total = max((out - 1) * stride + (k - 1) * dilation + 1 - n, 0)
    return out, total // 2, total - total // 2


def conv3d_same(x, w, bias=None, stride=1, dilation=1):
    """x [B, D, H, W, C], w [kd, kh, kw, C, O] (torch tensors of one dtype) -> [B, D', H', W', O].  The padding is explicit (F.pad): torch's
    own `padding=` is symmetric, TensorFlow's puts the odd voxel behind."""
    pads = [same_padding(x.shape[1 + a], w.shape[a], stride, dilation) for a in range(3)]
    xc = x.permute(0, 4, 1, 2, 3)
    xc = F.pad(xc, (pads[2][1], pads[2][2], pads[1][1], pads[1][2], pads[0][1], pads[0][2]))
    y = F.conv3d(xc, w.permute(4, 3, 0, 1, 2), bias, stride=stride, dilation=dilation)
    assert tuple(y.shape[2:]) == tuple(p[0] for p in pads)
    return y.permute(0, 2, 3, 4, 1).contiguous()


def instance_norm_relu(x, gamma, beta, eps=EPS):
    """BN_Relu with INSTANCE_NORM (model.py:366-372): InstanceNorm5d -- per sample and channel over D, H, W, tf.nn.moments' mean and BIASED
    variance, (x - mean) * rsqrt(var + eps) * gamma + beta -- then ReLU.  x [B, ..., C]."""
    axes = tuple(range(1, x.dim() - 1))
    mean = x.mean(axes, keepdim=True)
    var = ((x - mean) ** 2).mean(axes, keepdim=True)
    return torch.relu((x - mean) * torch.rsqrt(var + eps) * gamma + beta)


def upsample(x, s):
    """tf.keras.layers.UpSampling3D(size=(s, s, s)): every voxel repeated s times per axis."""
    return x.repeat_interleave(s, 1).repeat_interleave(s, 2).repeat_interleave(s, 3)


def forward(params, x, dtype=torch.float64, taps=None):
    """The logits [B, D, H, W, num_classes] of unet3d_attention(x) in `dtype`.  params: name -> numpy array; x: numpy [B, D, H, W, C_in].
    taps: a dict that receives down4, c345, sa (one channel) and c12 as numpy arrays."""
    P = {k: torch.from_numpy(np.asarray(v)).to(dtype) for k, v in params.items()}
    x = torch.from_numpy(np.asarray(x)).to(dtype)
    assert x.dim() == 5 and all(n % 16 == 0 and n >= 16 for n in x.shape[1:4]), "the spatial extents must be multiples of 16"

    def conv(name, t, stride=1, dilation=1, norm=True):
        n = SCOPE + name
        y = conv3d_same(t, P[n + "/kernel"], P.get(n + "/bias"), stride, dilation)
        return instance_norm_relu(y, P[n + "/ins_norm/gamma"], P[n + "/ins_norm/beta"]) if norm else y

    def up_conv(prefix, t, scale):  # UnetUpsample, model.py:340-364
        return conv("up_conv1_" + prefix, upsample(t, scale))

    def cfe(prefix, t):  # CFE3D, model.py:154-174
        return torch.cat([conv(prefix + "_cfe0", t)] + [conv("%s_cfe%d_dilation" % (prefix, r), t, dilation=d) for r, d in ((1, 3), (2, 5), (3, 7))], -1)

    layer = conv("init_conv", x)
    down = []
    for d in range(5):
        l_in = layer
        for i in range(2):  # Unet3dBlock, model.py:374-388
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
    ca = SCOPE + "C345_ChannelWiseAttention_withcpfe"  # ChannelWiseAttention3D, attention.py:166-174
    a = C345.mean((1, 2, 3))
    a = torch.relu(a @ P[ca + "_dense_1/kernel"] + P[ca + "_dense_1/bias"])
    a = torch.sigmoid(a @ P[ca + "_dense_2/kernel"] + P[ca + "_dense_2/bias"])
    C345 = C345 * a[:, None, None, None, :]
    C345 = up_conv("C345_up4", conv("C345_conv", C345), 4)
    # SpatialAttention3D, attention.py:79-154 (one channel here; the reference tiles it over the 64)
    SA = torch.sigmoid(sum(conv("spatial_attention_%d_conv2" % i, conv("spatial_attention_%d_conv1" % i, C345)) for i in (1, 2, 3)))
    C2 = up_conv("C2_up2", C2, 2)
    C12 = conv("C12_conv", torch.cat([C1, C2], -1)) * SA
    logits = conv("final", torch.cat([C12, C345], -1), norm=False)
    if taps is not None:
        taps.update(down4=down[4].numpy(), c345=C345.numpy(), sa=SA[..., 0].numpy(), c12=C12.numpy())
    return logits.numpy()


def softmax(logits):
    """final_probs = tf.nn.softmax(logits) (train.py:116), numpy, in the logits' dtype."""
    e = np.exp(logits - logits.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def param_count(in_channels, num_classes=2):
    """The number of trainable values of the graph above, counted from its own layer list (not from the package's table)."""
    n = 0

    def conv(k, cin, cout, bias=True, norm=True):
        return k * cin * cout + (cout if bias else 0) + (2 * cout if norm else 0)

    n += conv(27, in_channels, 16)
    for d in range(5):
        w = 16 << d
        n += 2 * conv(27, w, w) + (conv(27, w, 2 * w) if d != 4 else 0)
    n += conv(27, 16, 64) + conv(27, 32, 64)
    for cin in (64, 128, 256):
        n += conv(1, cin, 32, bias=False) + 3 * conv(27, cin, 32, bias=False)
    n += 2 * conv(27, 128, 128)
    n += (384 * 96 + 96) + (96 * 384 + 384)
    n += conv(1, 384, 64) + conv(27, 64, 64)
    n += 3 * (conv(81, 64, 32) + conv(9, 32, 1))
    n += conv(27, 64, 64) + conv(27, 128, 64)
    n += conv(27, 128, num_classes, norm=False)
    return n


# ---- the window average (eval.py:103-193) ----------------------------------------------------------------------------------------------------

def window_origins(n, crop, step):
    """The window origins on an axis of n voxels: np.arange(0, max(1, n - crop + step), step) (eval.py:142-144)."""
    return np.arange(0, max(1, n - crop + step), step)


def overlapping_inference(volume, probs_of, crop, steps, num_classes):
    """The rule of eval.py:103-193, with the crop, the steps and the class count as arguments.  volume: [C, D, H, W]; probs_of: a
    zero-filled window [1, d, h, w, C] -> its softmax probabilities [1, d, h, w, num_classes].  Every window is cut from the volume, what
    overhangs stays zero; the part of its prediction inside the volume is added to a float64 sum and 1 to the voxel's count; the result is
    sum / count.  The reference feeds BATCH_SIZE copies of the window and keeps the first prediction: with instance norm the samples of a
    batch are independent, so one copy gives the same.  Returns (mean [D, H, W, num_classes] float64, count [D, H, W])."""
    vol = np.moveaxis(np.asarray(volume), 0, -1)
    shape = vol.shape[:3]
    total = np.zeros(shape + (num_classes,), np.float64)
    count = np.zeros(shape, np.float64)
    for o0 in window_origins(shape[0], crop[0], steps[0]):
        for o1 in window_origins(shape[1], crop[1], steps[1]):
            for o2 in window_origins(shape[2], crop[2], steps[2]):
                inside = vol[o0:o0 + crop[0], o1:o1 + crop[1], o2:o2 + crop[2]]
                n0, n1, n2 = inside.shape[:3]
                window = np.zeros((1,) + tuple(crop) + (vol.shape[3],), vol.dtype)
                window[0, :n0, :n1, :n2] = inside
                pred = probs_of(window)
                total[o0:o0 + n0, o1:o1 + n1, o2:o2 + n2] += pred[0, :n0, :n1, :n2]
                count[o0:o0 + n0, o1:o1 + n1, o2:o2 + n2] += 1
    return total / count[..., None], count
