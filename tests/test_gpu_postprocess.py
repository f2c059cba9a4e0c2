"""The kernels of csrc/postprocess.hip against the numpy restatement (postprocess_ref.py) and the recorded scipy / reference results
(golden/postprocess.npz).  Exact equality everywhere: every value is an integer.

The component kernel labels LDS tiles of (T0, T1, T2) = (4, 8, 64) voxels and unites them across tile faces in a second launch.  The
issue's shapes straddle T0 and T1 but not T2 = 64, so (5, 9, 65) = (T0 + 1, T1 + 1, T2 + 1) and (9, 17, 130) (three tiles along
every axis) are added to them."""
import ctypes
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import postprocess_ref as ref

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = (4, 8, 64)
SHAPES = [(1, 1, 1), (1, 1, 37), (1, 40, 40), (3, 5, 7), (9, 17, 33), (16, 16, 16), (33, 34, 35), (5, 9, 65), (9, 17, 130)]
FULL = (155, 240, 240)


@pytest.fixture(scope="module")
def pp():
    from point_unet_amd import postprocess
    return postprocess


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "postprocess.npz"))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


# voxel pairs that meet only across a tile EDGE diagonal (two coordinates differ, each across a tile face at 4, 8 or 64 / 128), both
# orientations on each pair of axes, and only across a tile CORNER (three differ); no two pairs are neighbours of each other
EDGE_PAIRS = [((3, 7, 10), (4, 8, 10)), ((3, 8, 20), (4, 7, 20)), ((3, 2, 63), (4, 2, 64)), ((3, 12, 64), (4, 12, 63)),
              ((0, 7, 63), (0, 8, 64)), ((8, 7, 64), (8, 8, 63))]
CORNER_PAIRS = [((3, 7, 63), (4, 8, 64)), ((3, 7, 127), (4, 8, 128)), ((3, 15, 128), (4, 16, 127)), ((7, 8, 127), (8, 7, 128)),
                ((7, 16, 128), (8, 15, 127))]


def diagonal_pairs(shape):
    """(mask, edge pairs placed, corner pairs placed): the pairs above that fit into the shape."""
    m = np.zeros(shape, np.uint8)
    placed = []
    for pairs in (EDGE_PAIRS, CORNER_PAIRS):
        placed.append(0)
        for a, b in pairs:
            if all(a[i] < shape[i] and b[i] < shape[i] for i in range(3)):
                m[a] = m[b] = 1
                placed[-1] += 1
    return m, placed[0], placed[1]


@functools.lru_cache(maxsize=None)
def inputs(shape):
    out = {"empty": np.zeros(shape, np.uint8), "full": np.ones(shape, np.uint8), "checker": ref.checkerboard(shape),
           "serpentine": ref.serpentine(shape), "blobs": ref.blobs_and_specks(shape), "faces": faces_mask(shape)}
    m, edges, corners = diagonal_pairs(shape)
    if edges + corners:
        out["diagonals"] = m
    return out


def faces_mask(shape):
    """Touches every face: the six face planes' checkerboards plus a block in the middle."""
    m = np.zeros(shape, np.uint8)
    c = ref.checkerboard(shape)
    for a in range(3):
        sl = [slice(None)] * 3
        for e in (0, -1):
            sl[a] = e
            m[tuple(sl)] = c[tuple(sl)]
    mid = tuple(slice(n // 3, max(n // 3 + 1, 2 * n // 3)) for n in shape)
    m[mid] = 1
    return m


@functools.lru_cache(maxsize=None)
def want_label(shape, name, c, bg):
    return ref.label(inputs(shape)[name], c, bg)


# ---- connected components -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES)
def test_label_components(pp, shape):
    for name, m in inputs(shape).items():
        t = dev(m)
        for c in (1, 2, 3):
            for bg in (False, True):
                labels, n, sizes, touches = pp.label_components(t, c, bg, return_touches=True)
                wl, wn, ws, wt = want_label(shape, name, c, bg)
                what = (shape, name, c, bg)
                assert labels.dtype == torch.int32 and tuple(labels.shape) == shape
                assert n == wn, what
                assert np.array_equal(host(labels), wl), what
                assert np.array_equal(host(sizes), ws) and np.array_equal(host(touches), wt), what


def test_the_inputs_separate_the_neighbourhoods():
    shape = (9, 17, 130)
    V = int(np.prod(shape))
    assert [want_label(shape, "checker", c, False)[1] for c in (1, 2, 3)] == [(V + 1) // 2, 1, 1]
    m, edges, corners = diagonal_pairs(shape)
    assert (edges, corners) == (len(EDGE_PAIRS), len(CORNER_PAIRS)) and diagonal_pairs((5, 9, 65))[1:] == (4, 1)
    for a, b in EDGE_PAIRS + CORNER_PAIRS:
        crossed = [a[i] // TILE[i] != b[i] // TILE[i] for i in range(3)]
        assert crossed == [a[i] != b[i] for i in range(3)] and sum(crossed) == (2 if (a, b) in EDGE_PAIRS else 3)
    # edge pairs are one component at connectivity >= 2 and two at 1; corner pairs are one component at 3 only
    assert [ref.label(m, c)[1] for c in (1, 2, 3)] == [2 * (edges + corners), edges + 2 * corners, edges + corners]
    assert [want_label(shape, "serpentine", c, False)[1] for c in (1, 2, 3)] == [1, 1, 1]


@pytest.mark.parametrize("c", (1, 2, 3))
def test_label_components_equals_scipy_golden(pp, golden, c):
    t = dev(golden["blobs"])
    labels, n, sizes = pp.label_components(t, c)
    assert np.array_equal(host(labels), golden["label_c%d" % c]) and n == int(golden["label_n_c%d" % c])
    assert np.array_equal(host(sizes), np.bincount(golden["label_c%d" % c].ravel())[1:])
    assert np.array_equal(host(pp.label_components(t, c, background=True)[0]), golden["label_bg_c%d" % c])


def test_label_components_takes_bool_and_wide_integers(pp, golden):
    want = golden["label_c2"]
    for t in (dev(golden["blobs"] != 0), dev(golden["blobs"].astype(np.int64) * 300), dev(golden["blobs"].astype(np.int16) * -1)):
        assert np.array_equal(host(pp.label_components(t, 2)[0]), want)


def _full_size_case():
    """Child process of test_full_size_serpentine_and_boxes: prints one JSON line."""
    sys.path.insert(0, ROOT)
    from point_unet_amd import postprocess
    m = np.zeros(FULL, np.uint8)
    m[:100] = ref.serpentine((100,) + FULL[1:])
    block = np.zeros(400, np.uint8)
    k = 0
    for i in range(19):
        for j in range(19):
            k += 1
            block[:] = 0
            block[:k] = 1  # k voxels in raster order of a 4 x 10 x 10 block: one component at every connectivity
            m[104:108, 12 * i + 1:12 * i + 11, 12 * j + 1:12 * j + 11] = block.reshape(4, 10, 10)
    t = torch.from_numpy(m).cuda()
    res = {"serpentine": int(m[:100].sum()), "runs": []}
    for c in (1, 3):
        a = postprocess.label_components(t, c, return_touches=True)
        b = postprocess.label_components(t, c, return_touches=True)
        res["runs"].append({"c": c, "n": a[1], "sizes": sorted(a[2].cpu().tolist()), "label_of_first": int(a[0][0, 0, 0]),
                            "label_max": int(a[0].max()), "touching": int(a[3].sum()),
                            "equal": bool(torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]) and a[1] == b[1])})
    print("RESULT " + json.dumps(res))


def test_full_size_serpentine_and_boxes():
    """155 x 240 x 240 with an analytic answer: a serpentine through the first 100 planes (one component that crosses every tile it
    meets several times: the long chain of the merge) and 361 separated boxes of 1 .. 361 voxels.  In a child process, under its own
    time limit: a merge that does not end would otherwise hang the suite."""
    code = "import sys; sys.path.insert(0, %r); import test_gpu_postprocess as t; t._full_size_case()" % os.path.join(ROOT, "tests")
    r = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120, cwd=ROOT)
    text = r.stdout.decode()
    assert r.returncode == 0, text[-2000:]
    res = json.loads([ln for ln in text.splitlines() if ln.startswith("RESULT ")][-1][7:])
    assert res["serpentine"] >= 50 * 120 * 240, "50 planes of 120 full rows, and the joints between them"
    for run in res["runs"]:
        assert run["n"] == 362 and run["label_max"] == 362 and run["label_of_first"] == 1, run["c"]
        assert run["sizes"] == list(range(1, 362)) + [res["serpentine"]], run["c"]
        assert run["touching"] == 1 and run["equal"], run["c"]


# ---- morphology -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES)
def test_binary_morphology(pp, shape):
    fns = {1: pp.binary_dilation, 2: pp.binary_erosion, 3: pp.binary_closing, 4: pp.binary_opening}
    for name in ("full", "blobs", "faces", "checker"):
        m = inputs(shape)[name]
        t = dev(m)
        for op, fn in fns.items():
            for c in (1, 2, 3):
                for it in (1, 2):
                    got = fn(t, c, it)
                    assert got.dtype == torch.uint8
                    assert np.array_equal(host(got), ref.MORPH[op](m, c, it)), (shape, name, op, c, it)


def test_morphology_equals_scipy_golden_and_border_facts(pp, golden):
    t = dev(golden["blobs"])
    for c in (1, 2, 3):
        assert np.array_equal(host(pp.binary_closing(t, c)), golden["close_c%d" % c])
        assert np.array_equal(host(pp.binary_opening(t, c)), golden["open_c%d" % c])
        assert np.array_equal(host(pp.binary_dilation(t, c, 2)), golden["dilate2_c%d" % c])
        assert np.array_equal(host(pp.binary_erosion(t, c, 2)), golden["erode2_c%d" % c])
    cube = host(pp.binary_closing(dev(np.ones((3, 3, 3), np.uint8)), 2))
    assert cube.sum() == 1 and cube[1, 1, 1] == 1
    corner = np.zeros((3, 3, 3), np.uint8)
    corner[0, 0, 0] = 1
    assert not host(pp.binary_closing(dev(corner), 2)).any()


# ---- selection ------------------------------------------------------------------------------------------------------------------------------

def test_selection_equals_the_reference_golden(pp, golden):
    for k in (0, 1):
        t = dev(golden["two_in_%d" % k])
        assert np.array_equal(host(pp.largest_two_components(t)), golden["two_largest_%d" % k])
        assert np.array_equal(host(pp.largest_two_components(t, threshold=20)), golden["two_above20_%d" % k])
    got = pp.remove_external_core(dev(golden["overlap_main"]), dev(golden["overlap_ext"]))
    assert np.array_equal(host(got), golden["overlap_out"])


@pytest.mark.parametrize("shape", [(3, 5, 7), (9, 17, 33), (33, 34, 35), (9, 17, 130)])
def test_selection_equals_the_restatement(pp, shape):
    main = dev(inputs(shape)["faces"])
    for name in ("blobs", "diagonals", "checker", "serpentine"):
        if name not in inputs(shape):
            continue
        m = inputs(shape)[name]
        t = dev(m)
        for c in (1, 2, 3):
            assert np.array_equal(host(pp.largest_two_components(t, connectivity=c)), ref.keep_components(m, ref.KEEP_LARGEST_TWO, c)), (name, c)
            for thr in (1, 5):
                assert np.array_equal(host(pp.largest_two_components(t, thr, c)), ref.keep_components(m, ref.KEEP_ABOVE, c, thr)), (name, c, thr)
        assert np.array_equal(host(pp.remove_external_core(main, t)), ref.keep_components(m, ref.KEEP_OVERLAP, 2, main=inputs(shape)["faces"])), name


def test_selection_edge_rules(pp):
    shape = (3, 5, 7)
    empty = np.zeros(shape, np.uint8)
    one = empty.copy()
    one[1, 1:4, 2] = 3  # a non-zero value other than 1: the output is still 0 / 1
    tie = (one != 0).astype(np.uint8)
    tie[1, 1:4, 5] = 1
    tie[0, 0, 0] = 1
    assert not host(pp.largest_two_components(dev(empty))).any() and not host(pp.largest_two_components(dev(empty), 5)).any()
    assert np.array_equal(host(pp.largest_two_components(dev(one), 1000)), one != 0), "a lone component is kept whatever its size"
    assert np.array_equal(host(pp.largest_two_components(dev(one))), one != 0)
    for m in (tie, tie[::-1].copy()):
        got = host(pp.largest_two_components(dev(m)))
        assert np.array_equal(got, ref.keep_components(m, ref.KEEP_LARGEST_TWO, 2)) and got.sum() == 6
        assert np.array_equal(host(pp.largest_two_components(dev(m), 2)), ref.keep_components(m, ref.KEEP_ABOVE, 2, 2))
    # three equal components and a larger one: the tie for second place goes to the lower label
    m = np.zeros((1, 9, 30), np.uint8)
    m[0, 0, 0:25] = 1
    for r in (2, 4, 6):
        m[0, r, 3:8] = 1
    got = host(pp.largest_two_components(dev(m)))
    assert np.array_equal(got, ref.keep_components(m, ref.KEEP_LARGEST_TWO, 2)) and got[0, 2].sum() == 5 and got[0, 4:].sum() == 0
    assert not host(pp.remove_external_core(dev(empty), dev(tie))).any()
    assert np.array_equal(host(pp.remove_external_core(dev(tie), dev(tie))), tie)


# ---- hole filling ---------------------------------------------------------------------------------------------------------------------------

def test_fill_holes(pp, golden):
    got = host(pp.fill_holes(dev(golden["holes_in"])))
    assert np.array_equal(got, golden["holes_out"]) and np.array_equal(got, ref.fill_holes(golden["holes_in"]))
    # enclosed cavity; cavity open through a tunnel; shell joined by diagonals alone; tunnel with a diagonal step; nested shells
    assert got[13, 5, 5] == 1 and got[3, 15, 5] == 0 and got[20, 5, 20] == 1 and got[1, 25, 5] == 1 and got[0, 26, 6] == 0
    assert got[12:23, 12:23, 20:31].all()


@pytest.mark.parametrize("shape", [(1, 1, 37), (3, 5, 7), (9, 17, 33), (5, 9, 65), (9, 17, 130)])
def test_fill_holes_equals_the_restatement(pp, shape):
    for name, m in inputs(shape).items():
        assert np.array_equal(host(pp.fill_holes(dev(m))), ref.fill_holes(m)), name
    if min(shape) >= 5:
        m = np.zeros(shape, np.uint8)
        m[1:-1, 1:-1, 1:-1] = 1
        m[2:-2, 2:-2, 2:-2] = 0  # a cavity that spans every tile of the shape
        assert host(pp.fill_holes(dev(m)))[1:-1, 1:-1, 1:-1].all()
        m[0:2, 2, 2] = 0
        assert np.array_equal(host(pp.fill_holes(dev(m))), m)


# ---- the chain ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("v", (0, 1))
def test_brats_chain_equals_the_reference_golden(pp, golden, v):
    pred, w = dev(golden["brats_pred_%d" % v]), dev(golden["brats_weight"])
    got = pp.brats_post_processing(pred, w)
    assert got.dtype == torch.uint8 and np.array_equal(host(got), golden["brats_out_%d_w" % v])
    assert np.array_equal(host(pp.brats_post_processing(pred)), golden["brats_out_%d_nw" % v])
    assert np.array_equal(host(pp.brats_post_processing(pred.to(torch.int64), w != 0)), golden["brats_out_%d_w" % v])
    assert torch.equal(got, pp.brats_post_processing(pred, w))


@pytest.mark.parametrize("shape", [(9, 17, 33), (9, 17, 130)])
def test_brats_chain_equals_the_restatement(pp, shape):
    h = ref._hash(shape, 3)
    pred = np.where(ref.blobs_and_specks(shape) != 0, np.array([2, 1, 4, 2], np.uint8)[h % 4], 0).astype(np.uint8)
    pred[ref.specks(shape, 29, 9) != 0] = 4
    weight = (ref.specks(shape, 11, 2) == 0).astype(np.uint8)
    for thr in (3, 40, 2000):
        for w in (None, weight):
            got = pp.brats_post_processing(dev(pred), None if w is None else dev(w), wt_threshold=thr)
            assert np.array_equal(host(got), ref.brats_post_processing(pred, w, thr)), (thr, w is None)


# ---- protocol -------------------------------------------------------------------------------------------------------------------------------

def pad256(n):
    return (n + 255) // 256 * 256


def test_scratch_protocol(pp, lib):
    from point_unet_amd import runtime
    shape = (9, 17, 33)
    V = int(np.prod(shape))
    m = inputs(shape)["blobs"]
    t, out = dev(m), torch.empty(shape, dtype=torch.uint8, device="cuda")
    ctx = runtime.default_context(0)
    need = ctypes.c_int64(0)
    assert lib.ps_fill_holes(ctx.handle, None, *shape, None, None, ctypes.byref(need)) == 0
    assert need.value == 256 + 2 * pad256(4 * V), "counters, parents, counts"
    assert lib.ps_binary_morph(None, None, *shape, 3, 2, 1, None, None, ctypes.byref(need)) == 0 and need.value == pad256(V)
    assert lib.ps_keep_components(None, None, *shape, 2, 3, 0, None, None, None, ctypes.byref(need)) == 0 and need.value == 256 + 3 * pad256(4 * V)
    assert lib.ps_brats_postprocess(None, None, None, *shape, 5, None, None, ctypes.byref(need)) == 0
    assert need.value == 256 + pad256(V) + 2 * pad256(4 * V)
    assert lib.ps_fill_holes(None, None, *shape, None, None, ctypes.byref(need)) == 0
    # exactly that many bytes are enough, and none behind them is written
    buf = torch.full((need.value + 4096,), 0xAB, dtype=torch.uint8, device="cuda")
    assert lib.ps_fill_holes(ctx.handle, runtime.ptr(t), *shape, runtime.ptr(out), runtime.ptr(buf), ctypes.byref(need)) == 0
    torch.cuda.synchronize()
    assert np.array_equal(host(out), ref.fill_holes(m)) and bool((buf[need.value:] == 0xAB).all())
    short = ctypes.c_int64(need.value - 1)
    assert lib.ps_fill_holes(ctx.handle, runtime.ptr(t), *shape, runtime.ptr(out), runtime.ptr(buf), ctypes.byref(short)) == 1
    assert b"ps_fill_holes" in lib.ps_last_error() and b"needs" in lib.ps_last_error()
    assert lib.ps_fill_holes(ctx.handle, runtime.ptr(t), *shape, runtime.ptr(out), ctypes.c_void_p(buf.data_ptr() + 8), ctypes.byref(need)) == 1
    assert lib.ps_fill_holes(ctx.handle, runtime.ptr(t), *shape, runtime.ptr(t), runtime.ptr(buf), ctypes.byref(need)) == 1
    assert b"overlap" in lib.ps_last_error()


def test_python_surface_errors_and_scratch_reuse(pp):
    m = dev(inputs((9, 17, 33))["blobs"])
    with pytest.raises(ValueError):
        pp.fill_holes(m.cpu())
    with pytest.raises(ValueError):
        pp.label_components(m.permute(2, 1, 0))
    with pytest.raises(ValueError):
        pp.label_components(m[:, :, ::2])
    with pytest.raises(ValueError):
        pp.binary_closing(m.float(), 2)
    with pytest.raises(ValueError):
        pp.binary_closing(m, 4)
    with pytest.raises(ValueError):
        pp.binary_closing(m, 2, 0)
    with pytest.raises(ValueError):
        pp.fill_holes(m[0])
    with pytest.raises(ValueError):
        pp.remove_external_core(m[:4].contiguous(), m)
    with pytest.raises(ValueError):
        pp.brats_post_processing(m, wt_threshold=-1)
    pp.fill_holes(m)
    key = [k for k in pp._scratch if k[0] == "ps_fill_holes" and k[2:] == (9, 17, 33)]
    before = pp._scratch[key[0]].data_ptr()
    pp.fill_holes(m)
    assert len(key) == 1 and pp._scratch[key[0]].data_ptr() == before


def test_output_feeds_segmentation_metrics(pp, golden):
    from point_unet_amd import metrics
    truth = dev(golden["brats_out_0_nw"])
    out = pp.brats_post_processing(dev(golden["brats_pred_0"]), dev(golden["brats_weight"]))
    assert out.dtype == torch.uint8 and out.is_cuda and out.is_contiguous() and metrics._as_u8(out, "pred").data_ptr() == out.data_ptr()
    res = metrics.segmentation_metrics(out, truth)
    want = host(out)
    for name, labs in metrics.BRATS_REGIONS.items():
        assert res[name]["n_pred"] == int(np.isin(want, list(labs)).sum())
    assert metrics.segmentation_metrics(out, out)[next(iter(metrics.BRATS_REGIONS))]["dice"] == 1.0
