"""The 3-D convolution and its two gradients across JOINT geometry on the GPU: saliency.conv3d and saliency.conv3d_backward (ps_conv3d[_prec],
ps_conv3d_bwd_data[_prec], ps_conv3d_bwd_weight[_prec]; csrc/conv3d.hip, conv3d_bf16.hip, conv3d_train.hip, conv3d_train_bf16.hip) on every
case of saliency_conv_cases.py -- all 216 (kernel, stride, dilation) geometries on both parities and both fetch forms, the degenerate
extents, the k walk's carries, the fused concat and up-sampling under stride 2, dilation 3 and non-cubic kernels, one case per kernel instantiation on the launchers'
thresholds -- in all three roles and all three precisions.  test_saliency_conv_geometry_rule.py holds the list and the references to account on the CPU.

The contract is include/pointseg_saliency.h's formula for every combination the entries accept.  TensorFlow itself refuses stride > 1
together with dilation > 1: those cases are held to the header, not to TensorFlow.

Bars.  The project's op bar, unchanged: 4 x |torch-CPU float32 - float64 on the SAME operands| + 1e-6 x max |expected|
(saliency_conv_cases.op_bar mirrors _bar of test_gpu_saliency_precision.py).  "fp32" and "bf16x3" are held to it against the float64
result of the exact operands, "bf16" against the float64 result of the bfloat16-rounded operands (saliency_precision_ref.conv3d_rounded,
saliency_grad_precision_ref.*_rounded).  Every figure is printed (kernel error, CPU-float32 error, bar); a test goes through all its cases
and fails at the end with the list of those that missed.  DESIGN.md 4.16 records the worst error / bar per role and precision.

Exact in every precision: the weight gradient of a tap that never leaves the padding is 0.0, the data gradient of an input voxel no
output reads is 0.0, an output voxel whose every tap lies in the padding is the bias (SAME padding leaves none: the check is kept for the
day that changes); the fused concat / up-sampling gives the bytes of the materialised input, forward, dw and dbias; a batch gives the bytes
of its single-sample runs, forward and data gradient (dw and dbias are sums over the batch); a partial `need` gives the bytes of the full
call; two runs give the same bytes.

The wrappers allocate their results themselves (torch.empty), so this file allocates no result buffer and has none to start as NaN.  A
stale result in a reused block cannot pass for a fresh one: a case's results of all three precisions stay alive until the case is done, and
the two sides of every torch.equal are alive together, so they are different blocks."""
import numpy as np
import pytest

import saliency_conv_cases as cc

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def _sal():
    from point_unet_amd import saliency
    return saliency


def _cuda(c):
    return tuple(None if t is None else t.cuda() for t in cc.operands(c))


def _forward(c, ops, precision):
    x, x2, w, bias, dy = ops
    return _sal().conv3d(x, w, bias, c[5], c[6], x2, c[7], precision=precision)


def _backward(c, ops, precision, need=("x", "x2", "w", "bias")):
    x, x2, w, bias, dy = ops
    return _sal().conv3d_backward(dy, x, w, c[5], c[6], x2, c[7], need=need, precision=precision)


def _hold(failures, got, want, what):
    """One result against its bar; prints the figures, notes a miss."""
    want64, cpu = want
    got = got.cpu().numpy()
    assert got.shape == want64.shape, what
    err, bar = float(np.abs(got.astype(np.float64) - want64).max()), cc.op_bar(want64, cpu)
    print("%s: kernel %.3e, torch-CPU float32 %.3e, bar %.3e, ratio %.3f (max |expected| %.2f)" % (what, err, cpu, bar, err / bar if bar else 0.0, np.abs(want64).max()))
    if not err <= bar:  # (also a NaN)
        failures.append("%s: %.3e > %.3e" % (what, err, bar))
    return got


def _check(c, failures):
    """Every role of the case in every precision: the bars and the exact facts.  Returns {precision: (y, gradients)} on the device."""
    refs = cc.references(c)
    live, reached, fed = cc.live_taps(c), cc.reached_voxels(c), cc.fed_outputs(c)
    ops = _cuda(c)
    bias = cc.operands(c)[3].numpy()
    out = {}
    for precision in cc.PRECISIONS:
        want = refs[precision == "bf16"]
        what = "%s %s" % (precision, cc.case_id(c))
        y = _forward(c, ops, precision)
        grads = _backward(c, ops, precision)
        assert set(grads) == set(want) - {"y"}, what
        yh = _hold(failures, y, want["y"], what + " forward y")
        got = {n: _hold(failures, g, want[n], "%s %s gradient d%s" % (what, "weight" if n in ("w", "bias") else "data", n)) for n, g in grads.items()}
        if not (np.moveaxis(yh, 0, 3)[~fed] == bias).all():
            failures.append(what + ": an output voxel whose every tap lies in the padding is not exactly the bias")
        if got["w"][~live].any():
            failures.append(what + ": dw of a tap that never leaves the padding is not exactly 0")
        for n in ("x", "x2"):
            if n in got and np.moveaxis(got[n], 0, 3)[~reached].any():
                failures.append("%s: d%s of an input voxel that no output reads is not exactly 0" % (what, n))
        out[precision] = (y, grads)
    return out


def _run_group(cases):
    failures = []
    for c in cases:
        _check(c, failures)
    assert not failures, "%d results missed:\n%s" % (len(failures), "\n".join(failures))


@pytest.mark.parametrize("kernel", cc.KERNELS, ids=lambda k: "k%d%d%d" % k)
def test_joint_geometry(kernel):
    """Stride {1, 2} x dilation {1, 3, 5, 7} under one kernel: 4 cases at stride 1, 8 at stride 2 (both parities of every axis)."""
    cases = [c for c in cc.JOINT if c[1] == kernel]
    assert len(cases) == 12
    _run_group(cases)


def test_degenerate_extents():
    _run_group(cc.DEGENERATE)


def test_k_walk():
    _run_group(cc.KWALK)


def test_every_kernel_form():
    """saliency_conv_cases.FORMS: one case per kernel instantiation on the launchers' thresholds (test_saliency_conv_geometry_rule.py shows
    that they reach all 52), every role in every precision under the bars; and the calls with one result NULL that land in another form
    than the full call (FORMS_PARTIAL) -- the bar again, and the bytes of the full call: a narrower column range or fewer rows regroup no sum."""
    failures = []
    for c in cc.FORMS:
        got = _check(c, failures)
        for need in cc.FORMS_PARTIAL.get(c, ()):
            ops = _cuda(c)
            for precision in cc.PRECISIONS:
                part = _backward(c, ops, precision, need=need)
                assert set(part) == set(need)
                n, what = need[0], "%s %s need=%s" % (precision, cc.case_id(c), need[0])
                _hold(failures, part[n], cc.references(c)[precision == "bf16"][n], what + " gradient d" + n)
                if not torch.equal(part[n], got[precision][1][n]):
                    failures.append(what + ": not the bytes of the full call")
    assert not failures, "%d results missed:\n%s" % (len(failures), "\n".join(failures))


def test_fused_input_jointly():
    """The bars, and the fused forms against the materialised input: the same operand values in the same order, whichever fetch form each
    takes -- test_conv3d_fused_concat_and_upsampling's claim, now with dilation, stride 2 and non-cubic kernels."""
    sal = _sal()
    failures = []
    for c in cc.FUSED:
        got = _check(c, failures)
        x, x2, w, bias, dy = _cuda(c)
        full = cc.materialised(*cc.operands(c)[:2], c[7]).cuda()
        for precision in cc.PRECISIONS:
            y, grads = got[precision]
            plain = sal.conv3d(full, w, bias, c[5], c[6], precision=precision)
            plain_g = sal.conv3d_backward(dy, full, w, c[5], c[6], need=("w", "bias"), precision=precision)
            for name, a, b in (("y", y, plain), ("dw", grads["w"], plain_g["w"]), ("dbias", grads["bias"], plain_g["bias"])):
                if not torch.equal(a, b):
                    failures.append("%s %s: the fused %s is not the materialised input's" % (precision, cc.case_id(c), name))
    assert not failures, "%d results missed:\n%s" % (len(failures), "\n".join(failures))


def test_batch_equals_the_single_runs():
    """B = 3: the bars in every precision; at the case's precision the forward and the data gradient of the batch are the bytes of the
    three single-sample runs (dw and dbias are sums over the batch and have no single-sample counterpart)."""
    failures = []
    for c, precision in cc.BATCH:
        y, grads = _check(c, failures)[precision]
        x, x2, w, bias, dy = _cuda(c)
        for b in range(c[8]):
            one = (x[b:b + 1].contiguous(), None, w, bias, dy[b:b + 1].contiguous())
            if not torch.equal(_forward(c, one, precision), y[b:b + 1]):
                failures.append("%s %s: y of sample %d differs from its single run" % (precision, cc.case_id(c), b))
            if not torch.equal(_backward(c, one, precision, need=("x",))["x"], grads["x"][b:b + 1]):
                failures.append("%s %s: dx of sample %d differs from its single run" % (precision, cc.case_id(c), b))
    assert not failures, "\n".join(failures)


# fused, stride 2, dilation 3: 5 + 30 behind up = 2 (the scalar fetch; the data gradient goes through scratch) and 16 + 48 (the 16-byte fetch;
# dx2 alone is c0 = C1 in place; "bf16x3" runs the split weight gradient)
PARTIAL_CASES = [c for c in cc.FUSED if c[5] == 2 and c[6] == 3 and (c[1], c[7], c[2]) in (((1, 9, 9), 2, 5), ((3, 3, 3), 1, 16))]


@pytest.mark.parametrize("precision", cc.PRECISIONS)
def test_partial_outputs(precision):
    """need = x2 alone, x alone, bias alone, w alone: each gives the bytes of the full call."""
    assert len(PARTIAL_CASES) == 2
    for c in PARTIAL_CASES:
        ops = _cuda(c)
        every = _backward(c, ops, precision)
        assert set(every) == {"x", "x2", "w", "bias"}
        for need in (("x2",), ("x",), ("bias",), ("w",)):
            part = _backward(c, ops, precision, need=need)
            assert set(part) == set(need) and torch.equal(part[need[0]], every[need[0]]), (cc.case_id(c), need)


DETERMINISM_CASE = cc.at(cc.JOINT, cc.SHAPE_B, (9, 3, 9), 2, 3)


@pytest.mark.parametrize("precision", cc.PRECISIONS)
def test_two_runs_give_the_same_bytes(precision):
    c = DETERMINISM_CASE
    ops = _cuda(c)
    one, two = (_forward(c, ops, precision), _backward(c, ops, precision)), (_forward(c, ops, precision), _backward(c, ops, precision))
    assert torch.equal(one[0], two[0]) and set(one[1]) == {"x", "w", "bias"} and all(torch.equal(one[1][n], two[1][n]) for n in one[1])
    assert all(bool(torch.isfinite(t).all()) for t in (one[0],) + tuple(one[1].values()))
