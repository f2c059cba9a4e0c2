"""Writes tests/golden/postprocess.npz: scipy's and the reference's own results on the formula inputs of tests/postprocess_ref.py.
Run once, in the build container (needs scipy and the reference checkout); the tests only read the file.

  python tests/golden/make_postprocess_golden.py

Two kinds of record:
  * scipy's: ndimage.label at connectivity 1, 2, 3, binary_closing, binary_dilation / binary_erosion with iterations = 2, binary_fill_holes
  * the reference's post_processing (SaliencyAttention/eval.py), get_largest_two_component and remove_external_core
    (SaliencyAttention/utils.py): the three functions are cut out of the reference's files with `ast` when this script runs and
    executed with np and scipy.ndimage in scope.  None of their text is stored.
The script asserts that its inputs stay inside what the reference can run: it raises where two components a rule picks between have
equal sizes."""
import ast
import os
import sys

import numpy as np
from scipy import ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import postprocess_ref as ref  # noqa: E402

REFERENCE = os.path.join(os.environ.get("POINTSEG_REFERENCE", "/root/reference"), "SaliencyAttention")  # as make_golden.py


def reference_functions():
    env = dict(np=np, ndimage=ndimage, print=lambda *a, **k: None)
    for fname, names in (("utils.py", ("get_largest_two_component", "remove_external_core")), ("eval.py", ("post_processing",))):
        tree = ast.parse(open(os.path.join(REFERENCE, fname)).read())
        for node in ast.walk(tree):
            if isinstance(node, ast.FunctionDef) and node.name in names:
                exec(compile(ast.Module(body=[node], type_ignores=[]), fname, "exec"), env)
    return env


def struct(c):
    return ndimage.generate_binary_structure(3, c)


def main():
    env = reference_functions()
    out = {}
    s = ref.GOLDEN_SHAPE

    # ---- scipy on the formula inputs
    blobs = ref.blobs_and_specks(s)
    out["blobs"] = blobs
    for c in (1, 2, 3):
        lab, n = ndimage.label(blobs, struct(c))
        out["label_c%d" % c] = lab.astype(np.int32)
        out["label_n_c%d" % c] = np.int32(n)
        lab, n = ndimage.label(blobs == 0, struct(c))
        out["label_bg_c%d" % c] = lab.astype(np.int32)
        out["close_c%d" % c] = ndimage.binary_closing(blobs, structure=struct(c)).astype(np.uint8)
        out["open_c%d" % c] = ndimage.binary_opening(blobs, structure=struct(c)).astype(np.uint8)
        out["dilate2_c%d" % c] = ndimage.binary_dilation(blobs, structure=struct(c), iterations=2).astype(np.uint8)
        out["erode2_c%d" % c] = ndimage.binary_erosion(blobs, structure=struct(c), iterations=2).astype(np.uint8)
    shell = ref.hole_cases(s)
    out["holes_in"] = shell
    out["holes_out"] = ndimage.binary_fill_holes(shell).astype(np.uint8)
    assert out["holes_out"].sum() > shell.sum()

    # ---- the reference's selection rules
    for kept in (0, 1):
        m = ref.two_blob_mask(bool(kept))
        _, n = ndimage.label(m, struct(2))
        sizes = np.sort(ndimage.sum(m, ndimage.label(m, struct(2))[0], range(1, n + 1)))
        assert n > 3 and sizes[-1] != sizes[-2] and sizes[-2] != sizes[-3], "the reference raises on equal sizes"
        assert (10 * sizes[-2] > sizes[-1]) == bool(kept)
        out["two_in_%d" % kept] = m
        out["two_largest_%d" % kept] = np.asarray(env["get_largest_two_component"](m.copy(), False, None)).astype(np.uint8)
        big = sizes[sizes > 20]
        assert len(big) >= 2 and len(set(big.tolist())) == len(big) and (sizes <= 20).any()
        out["two_above20_%d" % kept] = np.asarray(env["get_largest_two_component"](m.copy(), False, 20)).astype(np.uint8)
    main_m, ext = ref.overlap_masks()
    lab, n = ndimage.label(ext, struct(2))
    sizes = ndimage.sum(ext, lab, range(1, n + 1))
    assert n == 5 and len(set(sizes.tolist())) == 5
    out["overlap_main"], out["overlap_ext"] = main_m, ext
    out["overlap_out"] = np.asarray(env["remove_external_core"](main_m.copy(), ext.copy())).astype(np.uint8)
    assert len(np.unique(lab[out["overlap_out"] != 0])) == 3

    # ---- the reference's chain, with the brain weight and with a weight of ones
    for v in (0, 1):
        pred = ref.brats_pred(v)
        out["brats_pred_%d" % v] = pred
        for wname, w in (("w", ref.brats_weight()), ("nw", np.ones(s, np.uint8))):
            p = pred.astype(np.int64) * w
            for stage in ("whole", "core"):  # the inputs of the two selections: the sizes the maker has to vouch for
                if stage == "whole":
                    m = ndimage.binary_closing(p > 0, structure=struct(2))
                    whole = np.asarray(env["get_largest_two_component"](m, False, 2000)) > 0
                else:
                    m = ndimage.binary_closing(((p > 0) & (p != 2)) & whole, structure=struct(2))
                lab, n = ndimage.label(m, struct(2))
                sizes = np.sort(ndimage.sum(m, lab, range(1, n + 1)))
                big = sizes[sizes > 2000]
                assert n > 1 and len(big) >= 1 and len(set(big.tolist())) == len(big), (v, wname, stage, sizes)
                if stage == "whole" and wname == "nw":
                    assert ((sizes > 100) & (sizes <= 2000)).any() and (sizes < 10).any(), sizes
            got = np.asarray(env["post_processing"](pred.astype(np.int64), w.astype(np.int64)))
            assert got.min() >= 0 and got.max() <= 4
            out["brats_out_%d_%s" % (v, wname)] = got.astype(np.uint8)
            assert (2 in got) and (1 in got)
            assert (4 in got) == (v == 0), "variant 0 keeps its enhancing region, variant 1 loses it to the < 100 rule"
        assert (pred == 4).sum() > 0
    out["brats_weight"] = ref.brats_weight()

    path = os.path.join(HERE, "postprocess.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d arrays, %d bytes" % (path, len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
