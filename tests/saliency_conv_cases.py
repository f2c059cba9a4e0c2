"""The case list of the 3-D convolution's joint-geometry tests (test_saliency_conv_geometry_rule.py on the CPU,
test_gpu_saliency_conv_geometry.py on the GPU), built from code so that the CPU test can state what it covers, with each case's operands
and CPU references -- computed once per case (functools.lru_cache) and left unchanged -- and the geometry facts that hold exactly.

A case is (shape, kernel, C1, C2, C_out, stride, dilation, up, B): `shape` the SOURCE extents (Ds, Hs, Ws), the convolution's input being
upsample(cat(x [.., C1], x2 [.., C2]), up).  include/pointseg_saliency.h is the contract for every one of them:
    out = ceil(in / stride);  pad_total = max((out - 1) * stride + (k - 1) * dilation + 1 - in, 0), the smaller half in front;
    y[o] = bias + sum over taps of in[o * stride - pad_before + t * dilation] . w[t].
TensorFlow itself refuses stride > 1 together with dilation > 1; those cases are held to the header's formula, not to TensorFlow.

The groups
  JOINT       the full product kernel extents {1, 3, 9}^3 x stride {1, 2} x dilation {1, 3, 5, 7} = 216 geometries, each on (5, 8, 7); the
              stride-2 ones a second time on the opposite parities (6, 7, 10).  The fetch forms alternate: C1 = 8 takes the 16-byte
              activation fetch (conv3d_b_vec), 6 the scalar one; C_out = 12 the 16-byte fetch of dy in the data gradient (the only form
              the split-bf16 data gradient has), 10 the scalar one.  The two bits come from different digits of the geometry's index, and
              the second run of a stride-2 geometry flips both.
  DEGENERATE  extents of 1 and 2, where the dilated footprint exceeds the input and most taps never leave the padding.
  KWALK       conv3d_b_kernel's division-free k walk where one chunk of 32 k carries across several taps and tap rows: C1 in {1, 2, 3, 5}
              (and 4: the 16-byte fetch) under 81 and 729 taps; C1 = 36, just above one chunk.
  FUSED       the concat and the up-sampling together with stride 2, dilation 3 and non-cubic kernels.  (16 + 48 -> 36 is the one form of
              this list that "bf16x3" routes to the split weight-gradient kernel: conv3d_bwd_weight_split_pays.)
  BATCH       three joint geometries at B = 3, each with the precision at which the batch is compared with its single-sample runs.
  FORMS       one case per kernel instantiation, sitting on the launchers' thresholds (csrc/conv3d_kit.h's form rule;
              test_saliency_conv_geometry_rule.py restates it and shows that all 52 instantiations are reached), B = 1.  Rows of the forward
              and the data gradient: 2048 voxels (16 x 16 x 8) against 2047 (23 x 89 x 1), each with 16, 17, 32, 33 and 36 channels in and
              out -- the fp32 column classes 16 | 17 and 32 | 33, the bf16 pipe's 32 | 33, and the 16-byte fetch (16, 32, 36) against the
              4-byte one (17, 33) of the activation and of dy alike.  Rows of the weight gradient: Ktot + 1 = 64 | 65 under a 1 x 1 x 1
              kernel with 63 and 64 input channels on a few hundred voxels, with 16, 17, 32 and 33 output channels; 64 -> 32 and 64 -> 33
              are what "bf16x3" routes to the split weight gradient.  FORMS_PARTIAL: the calls with one result NULL that land in another
              form than the full call -- 16 + 17 channels, whose data gradient narrows from 33 columns to 16 (x alone) and 17 (x2 alone),
              and 64 -> 32, whose weight gradient has 64 rows without the bias and one row with the bias alone.
Every tensor of every case stays below about 10^5 elements."""
import functools
import itertools
import zlib

import numpy as np
import torch

import saliency_grad_precision_ref as gref
import saliency_precision_ref as pref
import saliency_ref as ref

F64, F32 = torch.float64, torch.float32
PRECISIONS = ("fp32", "bf16x3", "bf16")

EXTENTS = (1, 3, 9)
STRIDES = (1, 2)
DILATIONS = (1, 3, 5, 7)
KERNELS = tuple(itertools.product(EXTENTS, repeat=3))
GEOMETRIES = tuple(itertools.product(KERNELS, STRIDES, DILATIONS))  # 216
SHAPE_A, SHAPE_B = (5, 8, 7), (6, 7, 10)  # opposite parities on every axis
VEC_C1, SCALAR_C1 = 8, 6
VEC_COUT, SCALAR_COUT = 12, 10


def is_vec(c1, c2=0):
    """conv3d_b_vec (csrc/conv3d_bf16.hip) for dense, 16-byte aligned tensors: the 16-byte fetch of 4 consecutive channels."""
    return c1 % 4 == 0 and c2 % 4 == 0


def _joint():
    cases = []
    for ki, k in enumerate(KERNELS):
        for si, stride in enumerate(STRIDES):
            for di, dilation in enumerate(DILATIONS):
                vec_in, vec_out = (ki + si + di) % 2 == 0, (ki + di // 2) % 2 == 0
                cases.append((SHAPE_A, k, VEC_C1 if vec_in else SCALAR_C1, 0, VEC_COUT if vec_out else SCALAR_COUT, stride, dilation, 1, 2))
                if stride == 2:
                    cases.append((SHAPE_B, k, SCALAR_C1 if vec_in else VEC_C1, 0, SCALAR_COUT if vec_out else VEC_COUT, stride, dilation, 1, 2))
    return cases


def _degenerate():
    cases = []
    product = itertools.product([(1, 1, 1), (1, 2, 5), (2, 1, 3), (3, 2, 1)], [(3, 3, 3), (9, 9, 1), (1, 9, 9), (9, 9, 9)], (1, 2), (1, 7))
    for i, (shape, k, stride, dilation) in enumerate(product):
        cases.append((shape, k, (VEC_C1, SCALAR_C1)[i % 2], 0, (VEC_COUT, SCALAR_COUT)[i // 2 % 2], stride, dilation, 1, 2))
    return cases


KWALK_KERNELS = ((1, 9, 9), (9, 9, 1), (9, 1, 9), (9, 9, 9))
KWALK_C1 = (1, 2, 3, 5, 4, 36)


def _kwalk():
    cases = []
    for c1, k, dilation in itertools.product(KWALK_C1, KWALK_KERNELS, (1, 3)):
        taps = k[0] * k[1] * k[2]
        cout = VEC_COUT if taps * c1 * VEC_COUT <= 100000 else 3  # 729 taps x 36 channels: the kernel stays below 10^5 values
        cases.append((SHAPE_A, k, c1, 0, cout, 1, dilation, 1, 2))
    return cases


FUSED_SOURCE = (3, 4, 5)
FUSED_INPUTS = ((2, 8, 24), (2, 5, 30), (3, 6, 0), (1, 16, 48))  # (up, C1, C2)
FUSED_KERNELS = ((3, 3, 3), (1, 9, 9), (9, 1, 1))


def _fused():
    cases = []
    for (up, c1, c2), stride, dilation, k in itertools.product(FUSED_INPUTS, (1, 2), (1, 3), FUSED_KERNELS):
        cin, taps = c1 + c2, k[0] * k[1] * k[2]
        cout = 24 if cin < 64 else (36 if taps * cin * 36 <= 100000 else 16)  # (81 taps x 64 channels: the kernel stays below 10^5 values)
        cases.append((FUSED_SOURCE, k, c1, c2, cout, stride, dilation, up, 2))
    return cases


FORMS_WIDE, FORMS_NARROW = (16, 16, 8), (23, 89, 1)  # 2048 voxels: the 128-row forms of the forward and the data gradient; 2047: the 64-row ones
FORMS_CHANNELS = (16, 17, 32, 33, 36)
FORMS_SMALL = (5, 8, 7)
FORMS_NARROWING = (FORMS_SMALL, (3, 3, 3), 16, 17, 12, 1, 1, 1, 1)
FORMS_SPLIT = (FORMS_SMALL, (1, 1, 1), 64, 0, 32, 1, 1, 1, 1)


def _forms():
    cases = [(shape, (3, 3, 3), ch, 0, ch, 1, 1, 1, 1) for shape in (FORMS_WIDE, FORMS_NARROW) for ch in FORMS_CHANNELS]
    cases += [(FORMS_SMALL, (1, 1, 1), 63, 0, cout, 1, 1, 1, 1) for cout in (16, 17, 32, 33)]
    cases += [FORMS_SPLIT, (FORMS_SMALL, (1, 1, 1), 64, 0, 33, 1, 1, 1, 1), FORMS_NARROWING]
    return cases


def at(cases, shape, k, stride, dilation):
    return next(c for c in cases if (c[0], c[1], c[5], c[6]) == (shape, k, stride, dilation))


JOINT = _joint()
DEGENERATE = _degenerate()
KWALK = _kwalk()
FUSED = _fused()
# (case, the precision of the batch comparison): B = 3 on three joint geometries
BATCH = [(at(JOINT, SHAPE_A, (3, 9, 1), 2, 3)[:8] + (3,), "fp32"), (at(JOINT, SHAPE_B, (9, 3, 3), 2, 3)[:8] + (3,), "bf16x3"),
         (at(JOINT, SHAPE_A, (1, 3, 9), 1, 5)[:8] + (3,), "bf16")]
FORMS = _forms()
FORMS_PARTIAL = {FORMS_NARROWING: (("x",), ("x2",)), FORMS_SPLIT: (("w",), ("bias",))}  # case: the `need`s that reach another form
GROUPS = {"joint": JOINT, "degenerate": DEGENERATE, "kwalk": KWALK, "fused": FUSED, "batch": [c for c, _ in BATCH], "forms": FORMS}
ALL = [c for group in GROUPS.values() for c in group]


def case_id(c):
    shape, k, c1, c2, cout, stride, dilation, up, B = c
    return "%s-k%s-%d+%dto%d-s%d-d%d-up%d-B%d" % ("x".join(map(str, shape)), "".join(map(str, k)), c1, c2, cout, stride, dilation, up, B)


def virtual_shape(c):
    """The extents of the convolution's (up-sampled) input."""
    return tuple(n * c[7] for n in c[0])


def out_shape(c):
    return tuple(-(-n // c[5]) for n in virtual_shape(c))


# ---- the geometry facts that hold exactly, whatever the arithmetic ----------------------------------------------------------------------------

def axis_positions(n, k, stride, dilation):
    """[out, k]: the input position o * stride - pad_before + t * dilation that tap t of output o reads on one axis."""
    out, before, _ = ref.same_padding(n, k, stride, dilation)
    return np.arange(out)[:, None] * stride - before + np.arange(k)[None, :] * dilation


def _axes(c):
    return [axis_positions(n, k, c[5], c[6]) for n, k in zip(virtual_shape(c), c[1])], virtual_shape(c)


def _outer_and(a, b, c):
    return a[:, None, None] & b[None, :, None] & c[None, None, :]


def live_taps(c):
    """bool [kd, kh, kw]: the taps that reach the input from at least one output voxel; the weight gradient of the others is exactly 0."""
    pos, n = _axes(c)
    return _outer_and(*[((p >= 0) & (p < m)).any(0) for p, m in zip(pos, n)])


def fed_outputs(c):
    """bool [Do, Ho, Wo]: the output voxels with at least one tap inside the input; the others are exactly the bias.  (SAME padding always
    leaves the centre tap inside, so every output is fed: the rule test shows it on the whole list.)"""
    pos, n = _axes(c)
    return _outer_and(*[((p >= 0) & (p < m)).any(1) for p, m in zip(pos, n)])


def reached_voxels(c):
    """bool [Ds, Hs, Ws]: the source voxels with at least one of their up^3 virtual voxels read by some output; the data gradient of the
    others is exactly 0 (stride 2 under a 1-tap axis reads every other voxel)."""
    pos, n = _axes(c)
    axes = []
    for p, m in zip(pos, n):
        hit = np.zeros(m, bool)
        hit[p[(p >= 0) & (p < m)]] = True
        axes.append(hit)
    up = c[7]
    virtual = _outer_and(*axes)
    return virtual.reshape(c[0][0], up, c[0][1], up, c[0][2], up).any((1, 3, 5))


# ---- operands and references ---------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def operands(c):
    """CPU float32 tensors (x, x2 or None, w, bias, dy): test_gpu_saliency_grad_precision.py's recipe, seeded by the case."""
    shape, k, c1, c2, cout, stride, dilation, up, B = c
    rng = np.random.default_rng(zlib.crc32(case_id(c).encode()))
    cin = c1 + c2
    x = torch.from_numpy(rng.standard_normal((B,) + shape + (c1,)).astype(np.float32))
    x2 = torch.from_numpy(rng.standard_normal((B,) + shape + (c2,)).astype(np.float32)) if c2 else None
    w = torch.from_numpy((rng.standard_normal(k + (cin, cout)) * np.sqrt(2.0 / (k[0] * k[1] * k[2] * cin))).astype(np.float32))
    bias = torch.from_numpy((rng.standard_normal(cout) * 0.1).astype(np.float32))
    dy = torch.from_numpy(rng.standard_normal((B,) + out_shape(c) + (cout,)).astype(np.float32))
    return x, x2, w, bias, dy


def materialised(x, x2, up):
    """upsample(cat(x, x2), up) as a dense tensor: copies, no arithmetic (rounding commutes with them)."""
    full = x if x2 is None else torch.cat([x, x2], -1)
    return (ref.upsample(full, up) if up > 1 else full).contiguous()


ROLES = ("y", "x", "x2", "w", "bias")  # the forward's result and the four gradients


@functools.lru_cache(maxsize=None)
def references(c):
    """{rounded: {role: (float64 result as numpy, max |torch-CPU float32 - float64| on the same operands)}}: rounded False = the exact
    operands ("fp32" and "bf16x3" are held to it), True = the bfloat16-rounded operands ("bf16").  The float32 result is kept only as
    its distance from float64 -- all the op bar takes from it."""
    shape, k, c1, c2, cout, stride, dilation, up, B = c
    x, x2, w, bias, dy = operands(c)
    full = materialised(x, x2, up)
    out = {}
    for rounded in (False, True):
        by_dtype = []
        for dt in (F64, F32):
            r = {"y": pref.conv3d_rounded(full, w, bias, stride, dilation, dt) if rounded
                 else ref.conv3d_same(full.to(dt), w.to(dt), bias.to(dt), stride, dilation)}
            r["x"], dx2 = gref.data_grad_rounded(dy, w, (B,) + shape, stride, dilation, up, c1, dt, rounded)
            if c2:
                r["x2"] = dx2
            r["w"] = gref.weight_grad_rounded(x, x2, up, dy, k, stride, dilation, dt, rounded)
            r["bias"] = gref.bias_grad_rounded(dy, dt, rounded)
            by_dtype.append({n: t.detach().numpy() for n, t in r.items()})
        r64, r32 = by_dtype
        out[rounded] = {n: (r64[n], float(np.abs(r32[n].astype(np.float64) - r64[n]).max())) for n in r64}
    return out


def op_bar(want64, cpu_error):
    """The project's op bar (test_gpu_saliency.py, test_gpu_saliency_precision.py's _bar): 4 x (torch-CPU float32 vs float64 on the same
    operands) + 1e-6 x max |expected|."""
    return 4.0 * cpu_error + 1e-6 * float(np.abs(want64).max())
