"""The case list of saliency_conv_cases.py and its yardstick, held to account without a GPU, before test_gpu_saliency_conv_geometry.py runs
the kernels on them.

Coverage: computed from the list with saliency_ref.same_padding -- all 216 geometries; on every axis an odd pad_total, a negative one that
is clamped, a footprint larger than the extent, and extent 1; stride 2 with every dilation at both parities of every axis; every kernel,
stride and dilation with both fetch forms; the k walk's regime; every kernel instantiation -- the launchers' selection rules are restated
here and the FORMS group is shown to reach all 52.  A failed condition names what to add.
The yardstick agrees with itself: the float64 gradients of saliency_grad_precision_ref equal float64 autograd through
conv3d_same(upsample(cat(x, x2))) on real operands, and on the degenerate extents a plain loop written straight from
include/pointseg_saliency.h's formula equals conv3d_same -- the header is the contract, also where TensorFlow refuses stride > 1 with
dilation > 1.
The cases discriminate: three deliberately wrong restatements of the header -- pad_before as the larger half, pad_total not clamped, the
data gradient's parity test dropped -- each move a named case of the list by more than 100 of that case's op bars, which is the evidence
that the GPU test would fail on such a kernel."""
import time

import numpy as np
import pytest

import saliency_conv_cases as cc
import saliency_ref as ref

torch = pytest.importorskip("torch")


def _axes_of(c):
    """[(axis, extent of the convolution's input, kernel extent)]"""
    return [(a, n, c[1][a]) for a, n in enumerate(cc.virtual_shape(c))]


def _raw_pad_total(n, k, stride, dilation):
    return (-(-n // stride) - 1) * stride + (k - 1) * dilation + 1 - n


# ---- coverage -----------------------------------------------------------------------------------------------------------------------------------

def test_the_groups_are_what_the_docstring_says():
    assert (len(cc.JOINT), len(cc.DEGENERATE), len(cc.KWALK), len(cc.FUSED), len(cc.BATCH), len(cc.FORMS)) == (108 + 216, 64, 48, 48, 3, 17)
    assert len(set(cc.ALL)) == len(cc.ALL) and len(set(map(cc.case_id, cc.ALL))) == len(cc.ALL)
    for c in cc.ALL:
        shape, k, c1, c2, cout, stride, dilation, up, B = c
        assert all(e in cc.EXTENTS for e in k) and stride in cc.STRIDES and dilation in cc.DILATIONS and 1 <= up <= 8, cc.case_id(c)
        sizes = [B * int(np.prod(shape)) * max(c1, c2), B * int(np.prod(cc.virtual_shape(c))) * (c1 + c2), int(np.prod(k)) * (c1 + c2) * cout,
                 B * int(np.prod(cc.out_shape(c))) * cout]
        assert max(sizes) < 100000, "%s: a tensor of %d elements" % (cc.case_id(c), max(sizes))
    assert all(c[8] == 2 for c in cc.JOINT + cc.DEGENERATE + cc.KWALK + cc.FUSED) and all(c[8] == 1 for c in cc.FORMS)
    assert sorted(p for _, p in cc.BATCH) == sorted(cc.PRECISIONS) and all(c[8] == 3 and c[:8] + (2,) in cc.JOINT for c, _ in cc.BATCH)
    assert any(c[5] == 2 and c[6] == 3 for c, _ in cc.BATCH), "add a B = 3 case with stride 2 and dilation 3"


def test_every_geometry_is_present():
    have = {(c[1], c[5], c[6]) for c in cc.JOINT}
    missing = [g for g in cc.GEOMETRIES if g not in have]
    assert len(cc.GEOMETRIES) == 216 and not missing, "add joint cases for (kernel, stride, dilation) %s" % missing[:5]
    # the stride-2 geometries run on both shapes, whose extents have opposite parities axis by axis
    assert all((a + b) % 2 == 1 for a, b in zip(cc.SHAPE_A, cc.SHAPE_B)) and len({n % 2 for n in cc.SHAPE_A}) == 2
    for g in cc.GEOMETRIES:
        shapes = {c[0] for c in cc.JOINT if (c[1], c[5], c[6]) == g}
        assert shapes == ({cc.SHAPE_A, cc.SHAPE_B} if g[1] == 2 else {cc.SHAPE_A}), g


def test_every_axis_meets_every_padding_regime():
    seen = set()
    for c in cc.ALL:
        for a, n, k in _axes_of(c):
            raw = _raw_pad_total(n, k, c[5], c[6])
            out, before, after = ref.same_padding(n, k, c[5], c[6])
            assert before + after == max(raw, 0) and before == max(raw, 0) // 2
            seen.update([(a, "odd pad_total")] if (before + after) % 2 else [])
            seen.update([(a, "a clamped negative pad_total")] if raw < 0 else [])
            seen.update([(a, "a footprint larger than the extent")] if (k - 1) * c[6] + 1 > n else [])
            seen.update([(a, "extent 1")] if n == 1 else [])
            seen.update([(a, "extent 1 at stride 2")] if n == 1 and c[5] == 2 else [])
    want = {(a, what) for a in range(3) for what in ("odd pad_total", "a clamped negative pad_total", "a footprint larger than the extent", "extent 1",
                                                      "extent 1 at stride 2")}
    assert not want - seen, "add a case with, on (axis, what): %s" % sorted(want - seen)


def test_stride_2_meets_every_dilation_at_both_parities_of_every_axis():
    seen = {(a, c[6], n % 2, k) for c in cc.JOINT if c[5] == 2 for a, n, k in _axes_of(c)}
    want = {(a, d, parity, k) for a in range(3) for d in cc.DILATIONS for parity in (0, 1) for k in cc.EXTENTS}
    assert not want - seen, "add stride-2 cases with (axis, dilation, extent parity, kernel extent) %s" % sorted(want - seen)[:5]


def test_both_fetch_forms_meet_every_kernel_stride_and_dilation():
    """conv3d_b_vec restated (saliency_conv_cases.is_vec): C1 % 4 == 0 and C2 % 4 == 0.  The forward and the weight gradient fetch the
    activation, the data gradient fetches dy, whose "C1" is C_out."""
    for what, form in (("activation", lambda c: cc.is_vec(c[2], c[3])), ("dy", lambda c: cc.is_vec(c[4]))):
        for name, key in (("kernel", lambda c: c[1]), ("stride", lambda c: c[5]), ("dilation", lambda c: c[6]), ("geometry at stride 2", lambda c: c[5] == 2 and (c[1], c[6])),
                          ("extent on axis 0", lambda c: c[1][0]), ("extent on axis 1", lambda c: c[1][1]), ("extent on axis 2", lambda c: c[1][2])):
            forms = {}
            for c in cc.JOINT:
                forms.setdefault(key(c), set()).add(form(c))
            forms.pop(False, None)
            one = sorted(str(k) for k, f in forms.items() if f != {True, False})
            assert not one, "the %s fetch meets %s %s in one form only" % (what, name, one)
    # the two bits are independent: all four combinations occur under every kernel
    for k in cc.KERNELS:
        assert len({(cc.is_vec(c[2]), cc.is_vec(c[4])) for c in cc.JOINT if c[1] == k}) == 4, k
    # the fused list: every kernel, stride and dilation with both forms; a concat and an up-sampling on either
    assert {cc.is_vec(c[2], c[3]) for c in cc.FUSED if c[3] and c[7] > 1} == {True, False}
    for key in (lambda c: c[1], lambda c: c[5], lambda c: c[6]):
        forms = {}
        for c in cc.FUSED:
            forms.setdefault(key(c), set()).add(cc.is_vec(c[2], c[3]))
        assert all(f == {True, False} for f in forms.values()), forms
    assert any(c[2] + c[3] >= 64 and c[4] >= 32 and c[5] == 2 and c[6] == 3 for c in cc.FUSED), "add a fused stride-2, dilation-3 case that bf16x3 routes to the split weight gradient"


def test_the_k_walk_cases_carry_across_taps():
    """One chunk is 32 k; with C1 < 32 and more than 32 taps a chunk step carries through several taps, with 81 = 9 x 9 taps and C1 <= 3
    through more than one tap row, with 729 through the tap plane as well."""
    assert all(c[5] == 1 and c[7] == 1 and np.prod(c[1]) > 32 for c in cc.KWALK)
    small = [c for c in cc.KWALK if c[2] < 32]
    for c1 in (1, 2, 3, 5, 4):
        for k in cc.KWALK_KERNELS:
            assert {c[6] for c in small if c[2] == c1 and c[1] == k} == {1, 3}, "add k-walk cases C1 = %d, kernel %s at dilation 1 and 3" % (c1, k)
    assert {cc.is_vec(c[2]) for c in small} == {True, False}
    assert {c[1] for c in cc.KWALK if c[2] == 36} == set(cc.KWALK_KERNELS), "add C1 = 36 (just above one chunk) with every k-walk kernel"
    assert any(32 // c[2] > c[1][2] for c in small) and any(32 // c[2] > c[1][1] * c[1][2] for c in small)  # a tap row, a tap plane per step


# ---- the launchers' selection rules, restated (csrc/conv3d_kit.h: conv_form, conv_form_b; conv3d_train.hip's routing) -------------------------------

def _tiles(precision, tall, cols):
    """(RT, NT): 128 rows per workgroup where `tall`; fp32 column tiles are 16 wide (1, 2 or 4 of them), the bf16 pipe's 32 wide (1 or 2)."""
    if precision == "fp32":
        return (2 if tall else 1, 1 if cols <= 16 else 2 if cols <= 32 else 4)
    return (2 if tall else 1, 1 if cols <= 32 else 2)


def _planes(precision):
    return {"bf16x3": 3, "bf16": 1}[precision]


def forward_form(c, precision):
    """ps_conv3d[_prec]: the rows are the output voxels, the columns C_out."""
    rt, nt = _tiles(precision, int(np.prod(cc.out_shape(c))) >= 2048, c[4])
    if precision == "fp32":
        return ("conv3d_kernel", rt, nt, False)
    return ("conv3d_b_kernel", _planes(precision), rt, nt, cc.is_vec(c[2], c[3]), False)


def data_grad_form(c, precision, need):
    """ps_conv3d_bwd_data[_prec]: the rows are the voxels of the virtual (up-sampled) input, the columns its channels that are asked for;
    the fetch is dy's, whose channel count is C_out; "bf16x3" keeps the fp32 kernel where dy does not take the 16-byte fetch."""
    c1, c2, cout = c[2], c[3], c[4]
    c0 = 0 if "x" in need else c1
    cols = (c1 + c2 if "x2" in need and c2 else c1) - c0
    vec = cc.is_vec(cout)
    if precision == "bf16x3" and not vec:
        precision = "fp32"
    rt, nt = _tiles(precision, int(np.prod(cc.virtual_shape(c))) >= 2048, cols)
    if precision == "fp32":
        return ("conv3d_kernel", rt, nt, True)
    return ("conv3d_b_kernel", _planes(precision), rt, nt, vec, True)


def weight_grad_form(c, precision, need):
    """ps_conv3d_bwd_weight[_prec]: the rows are the Ktot kernel rows (with dw) and the row of ones (with dbias), the columns C_out;
    "bf16x3" runs the split kernel from 64 input and 32 output channels on (conv3d_bwd_weight_split_pays), which has the 128-row forms only."""
    ktot, cout = int(np.prod(c[1])) * (c[2] + c[3]), c[4]
    rows = (ktot if "w" in need else 0) + (1 if "bias" in need else 0)
    if precision == "bf16x3" and not (cout >= 32 and c[2] + c[3] >= 64):
        precision = "fp32"
    rt, nt = _tiles(precision, rows > 64 or precision == "bf16x3", cout)
    if precision == "fp32":
        return ("conv3d_bwd_weight_kernel", rt, nt)
    return ("conv3d_bwd_weight_b_kernel", _planes(precision), rt, nt)


def forms_reached(c, precision, need=("x", "x2", "w", "bias")):
    """The kernel instantiations that conv3d and conv3d_backward(need=need) launch for the case."""
    out = {forward_form(c, precision)}
    if set(need) & ({"x", "x2"} if c[3] else {"x"}):
        out.add(data_grad_form(c, precision, need))
    if set(need) & {"w", "bias"}:
        out.add(weight_grad_form(c, precision, need))
    return out


INSTANTIATIONS = (
    [("conv3d_kernel", rt, nt, grad) for rt in (1, 2) for nt in (1, 2, 4) for grad in (False, True)]
    + [("conv3d_bwd_weight_kernel", rt, nt) for rt in (1, 2) for nt in (1, 2, 4)]
    # (the split data gradient exists with the 16-byte fetch alone)
    + [("conv3d_b_kernel", p, rt, nt, vec, grad) for p in (1, 3) for rt in (1, 2) for nt in (1, 2) for vec in (False, True) for grad in (False, True)
       if not (p == 3 and grad and not vec)]
    + [("conv3d_bwd_weight_b_kernel", 1, rt, nt) for rt in (1, 2) for nt in (1, 2)] + [("conv3d_bwd_weight_b_kernel", 3, 2, nt) for nt in (1, 2)])


def test_the_form_cases_reach_every_kernel_instantiation():
    assert len(INSTANTIATIONS) == len(set(INSTANTIATIONS)) == 52
    assert [sum(1 for i in INSTANTIATIONS if i[0] in names) for names in (("conv3d_kernel", "conv3d_bwd_weight_kernel"), ("conv3d_b_kernel",),
                                                                          ("conv3d_bwd_weight_b_kernel",))] == [18, 28, 6]
    reached = {}
    for c in cc.FORMS:
        for precision in cc.PRECISIONS:
            for form in forms_reached(c, precision):
                reached.setdefault(form, []).append(cc.case_id(c))
    assert not set(reached) - set(INSTANTIATIONS), "the restated rules name kernels that do not exist: %s" % sorted(set(reached) - set(INSTANTIATIONS), key=str)
    missing = [i for i in INSTANTIATIONS if i not in reached]
    assert not missing, "add form cases that reach %s" % missing
    # the thresholds, from both sides: 2048 | 2047 rows, 16 | 17 and 32 | 33 columns, Ktot + 1 = 64 | 65 weight-gradient rows, the two fetches
    voxels = {int(np.prod(cc.out_shape(c))) for c in cc.FORMS}
    assert {2047, 2048} <= voxels and all(cc.out_shape(c) == cc.virtual_shape(c) for c in cc.FORMS)
    for v in (2047, 2048):
        assert {c[4] for c in cc.FORMS if int(np.prod(cc.out_shape(c))) == v} >= {16, 17, 32, 33}
        assert {cc.is_vec(c[2]) for c in cc.FORMS if int(np.prod(cc.out_shape(c))) == v and c[2] > 32} == {True, False}
    for rows in (64, 65):
        assert {c[4] for c in cc.FORMS if int(np.prod(c[1])) * (c[2] + c[3]) + 1 == rows} >= ({16, 17, 32, 33} if rows == 64 else {32, 33})
    # one result NULL lands in another form than the full call
    for c, needs in cc.FORMS_PARTIAL.items():
        assert c in cc.FORMS
        for need in needs:
            for precision in cc.PRECISIONS:
                part, full = forms_reached(c, precision, need), forms_reached(c, precision)
                # (the split weight gradient has one row form)
                assert part <= set(INSTANTIATIONS) and (part - full or (precision == "bf16x3" and c == cc.FORMS_SPLIT)), (cc.case_id(c), need, precision)
    assert {data_grad_form(cc.FORMS_NARROWING, "fp32", need)[2] for need in (("x",), ("x2",), ("x", "x2"))} == {1, 2, 4}
    assert weight_grad_form(cc.FORMS_SPLIT, "bf16x3", ("bias",)) == ("conv3d_bwd_weight_b_kernel", 3, 2, 1)  # one row, and still the 128-row form


# ---- the yardstick agrees with itself -------------------------------------------------------------------------------------------------------------

def _autograd(c):
    """Float64 autograd through conv3d_same(upsample(cat(x, x2))) on the real operands, the loss being sum(y * dy)."""
    x, x2, w, bias, dy = cc.operands(c)
    leaves = {n: t.double().requires_grad_() for n, t in (("x", x), ("x2", x2), ("w", w), ("bias", bias)) if t is not None}
    full = leaves["x"] if x2 is None else torch.cat([leaves["x"], leaves["x2"]], -1)
    y = ref.conv3d_same(ref.upsample(full, c[7]) if c[7] > 1 else full, leaves["w"], leaves["bias"], c[5], c[6])
    (y * dy.double()).sum().backward()
    return y.detach().numpy(), {n: t.grad.numpy() for n, t in leaves.items()}


@pytest.mark.parametrize("group", list(cc.GROUPS))
def test_the_gradient_references_equal_autograd(group):
    t0 = time.perf_counter()
    for c in cc.GROUPS[group]:
        exact = cc.references(c)[False]
        y, grads = _autograd(c)
        assert set(grads) == set(exact) - {"y"}
        for n, got in dict(grads, y=y).items():
            want = exact[n][0]
            assert got.shape == want.shape and np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), (cc.case_id(c), n)
    print("%s: %d cases, references and autograd in %.1f s" % (group, len(cc.GROUPS[group]), time.perf_counter() - t0))


def _before(n, k, stride, dilation):
    return ref.same_padding(n, k, stride, dilation)[1]


def header_conv(x, w, bias, stride, dilation, before=_before):
    """include/pointseg_saliency.h's formula as a plain loop: y[o] = bias + sum over taps of in[o * stride - pad_before + t * dilation] . w[t],
    taps outside the input reading 0.  x [B, D, H, W, C], w [kd, kh, kw, C, O], bias [O]: float64 numpy."""
    n, k = x.shape[1:4], w.shape[:3]
    out = [-(-m // stride) for m in n]
    pad = [before(m, e, stride, dilation) for m, e in zip(n, k)]
    y = np.empty((x.shape[0],) + tuple(out) + (w.shape[4],))
    y[...] = bias
    for od in range(out[0]):
        for oh in range(out[1]):
            for ow in range(out[2]):
                for td in range(k[0]):
                    for th in range(k[1]):
                        for tw in range(k[2]):
                            i = [o * stride - p + t * dilation for o, p, t in zip((od, oh, ow), pad, (td, th, tw))]
                            if all(0 <= v < m for v, m in zip(i, n)):
                                y[:, od, oh, ow] += x[:, i[0], i[1], i[2]] @ w[td, th, tw]
    return y


def header_data_grad(dy, w, n, stride, dilation, parity=True):
    """The data gradient the header's formula implies, as the kernels gather it: dx[i] = sum over taps of dy[(i + pad_before - t * dilation)
    / stride] . w[t]^T where that is a whole number inside the output.  parity=False drops "whole" (a deliberately wrong restatement)."""
    k = w.shape[:3]
    dx = np.zeros((dy.shape[0],) + tuple(n) + (w.shape[3],))
    taps = []
    for m, e, out in zip(n, k, dy.shape[1:4]):
        axis = []
        for t in range(e):
            zz = np.arange(m) + _before(m, e, stride, dilation) - t * dilation
            ok = (zz >= 0) & ((zz % stride == 0) | (not parity)) & (zz // stride < out)
            axis.append((np.nonzero(ok)[0], (zz // stride)[ok]))
        taps.append(axis)
    B = np.arange(dy.shape[0])
    for td, (iz, oz) in enumerate(taps[0]):
        for th, (iy, oy) in enumerate(taps[1]):
            for tw, (ix, ox) in enumerate(taps[2]):
                dx[np.ix_(B, iz, iy, ix)] += dy[np.ix_(B, oz, oy, ox)] @ w[td, th, tw].T
    return dx


def _f64(c):
    x, x2, w, bias, dy = cc.operands(c)
    return cc.materialised(x, x2, c[7]).double().numpy(), w.double().numpy(), bias.double().numpy(), dy.double().numpy()


def test_the_header_formula_as_a_loop_equals_the_reference_on_the_degenerate_extents():
    for c in cc.DEGENERATE:
        full, w, bias, dy = _f64(c)
        want = cc.references(c)[False]
        got = header_conv(full, w, bias, c[5], c[6])
        assert got.shape == want["y"][0].shape and np.abs(got - want["y"][0]).max() <= 1e-12 * np.abs(want["y"][0]).max(), cc.case_id(c)
        got = header_data_grad(dy, w, c[0], c[5], c[6])
        assert np.abs(got - want["x"][0]).max() <= 1e-12 * max(np.abs(want["x"][0]).max(), 1e-300), cc.case_id(c)
    # extent 1 under stride 2 gives one output voxel
    assert any(cc.out_shape(c) == (1, 1, 1) and c[5] == 2 for c in cc.DEGENERATE)


def test_the_exact_facts_are_the_references_zeros():
    """live_taps, reached_voxels and fed_outputs (what the GPU test holds to exact values) against the float64 references: a dead tap's dw
    and an unreached voxel's dx are exactly 0 there, everything else is not; every output is fed."""
    dead = unreached = 0
    for c in cc.ALL:
        want = cc.references(c)[False]
        live, reached = cc.live_taps(c), cc.reached_voxels(c)
        assert cc.fed_outputs(c).all() and cc.fed_outputs(c).shape == cc.out_shape(c), cc.case_id(c)
        dw = want["w"][0]
        assert live.shape == dw.shape[:3] and not dw[~live].any() and dw[live].all(), cc.case_id(c)
        for n in ("x", "x2"):
            if n in want:
                dx = np.moveaxis(want[n][0], 0, 3)  # [Ds, Hs, Ws, B, C]
                assert reached.shape == dx.shape[:3] and not dx[~reached].any() and dx[reached].all(), (cc.case_id(c), n)
        dead += int((~live).sum())
        unreached += int((~reached).sum())
    assert dead > 1000 and unreached > 1000, (dead, unreached)


# ---- the cases discriminate -----------------------------------------------------------------------------------------------------------------------------

def _larger_half(n, k, stride, dilation):
    out, before, after = ref.same_padding(n, k, stride, dilation)
    return after


def _unclamped(n, k, stride, dilation):
    """pad_total without the clamp, halved rounding DOWN (Python's //, a kernel's >> 1): the raw total is never below -1 -- 1 tap, stride 2,
    an even extent -- where it gives pad_before = -1.  (C's truncating / gives 0 there, as the clamp does.)"""
    return _raw_pad_total(n, k, stride, dilation) // 2


LARGER_HALF_CASE = cc.at(cc.JOINT, cc.SHAPE_B, (3, 3, 3), 2, 1)  # even extents on D and W: pad_total = 1, in front 0 and not 1
UNCLAMPED_CASE = cc.at(cc.JOINT, cc.SHAPE_B, (1, 1, 1), 2, 1)    # raw pad_total = -1 on D and W
NO_PARITY_CASE = cc.at(cc.JOINT, cc.SHAPE_A, (3, 3, 3), 2, 3)    # an odd dilation: the parity of t * dilation alternates with the tap


def _moved(c, role, got, what):
    want, cpu = cc.references(c)[False][role]
    moved, bar = float(np.abs(got - want).max()), cc.op_bar(want, cpu)
    print("%s, %s: %s stands %.3e from the reference, %.0f bars of %.3e" % (cc.case_id(c), role, what, moved, moved / bar, bar))
    return moved / bar


@pytest.mark.parametrize("c, wrong", [(LARGER_HALF_CASE, _larger_half), (UNCLAMPED_CASE, _unclamped)], ids=["larger-half", "unclamped"])
def test_a_wrong_pad_split_moves_a_named_case_by_100_bars(c, wrong):
    assert c in cc.ALL
    full, w, bias, _ = _f64(c)
    right = header_conv(full, w, bias, c[5], c[6])
    assert _moved(c, "y", right, "the header's loop") <= 1.0  # the loop itself is right
    assert _moved(c, "y", header_conv(full, w, bias, c[5], c[6], wrong), "the wrong pad split") > 100.0


def test_a_dropped_parity_test_moves_a_named_case_by_100_bars():
    c = NO_PARITY_CASE
    assert c in cc.ALL and c[5] == 2
    _, w, _, dy = _f64(c)
    assert _moved(c, "x", header_data_grad(dy, w, c[0], c[5], c[6]), "the header's gather") <= 1.0
    assert _moved(c, "x", header_data_grad(dy, w, c[0], c[5], c[6], parity=False), "the gather without the parity test") > 100.0
