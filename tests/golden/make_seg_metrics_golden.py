#!/usr/bin/env python3
"""Generates tests/golden/seg_metrics.npz: the expected region metrics (counts, Dice, medpy's HD95) of the integer-formula label volumes
of tests/seg_metrics_oracle.py, computed with scipy (the restatement of medpy's hd95 that the reference's evaluation imports).  The
volumes are rebuilt from their formulas by every test; only the numbers are stored.

    python tests/golden/make_seg_metrics_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import seg_metrics_oracle as so  # noqa: E402

# name -> (shape, variant, spacing); the BraTS-sized pair at unit and at anisotropic spacing, small ones with every shape on the faces
CASES = {
    "brats": (so.BRATS_SHAPE, 0, (1.0, 1.0, 1.0)),
    "brats_aniso": (so.BRATS_SHAPE, 0, (0.8, 0.8, 2.5)),
    "small": ((24, 24, 24), 1, (1.0, 1.0, 1.0)),
    "small_aniso": ((24, 24, 24), 1, (1.5, 0.7, 1.1)),
    "thin": ((9, 17, 13), 0, (1.0, 1.0, 1.0)),
}


def compute():
    out = {}
    for name, (shape, variant, spacing) in list(CASES.items()) + [("chain", (so.BRATS_SHAPE, 0, (1.0, 1.0, 1.0)))]:
        pred, truth = so.label_pair(shape, variant)
        if name == "chain":  # point2prod -> probs_to_labels -> segmentation_metrics: 180 000 sampled voxels of pred, the rest label 0
            pred = so.chain_points(pred)[1]
        m = so.region_metrics(pred, truth, so.BRATS_REGIONS, spacing)
        regs = list(so.BRATS_REGIONS)
        out[name + "/counts"] = np.array([[m[r]["n_pred"], m[r]["n_truth"], m[r]["n_both"]] for r in regs], np.int64)
        out[name + "/dice"] = np.array([m[r]["dice"] for r in regs], np.float64)
        out[name + "/hd95"] = np.array([m[r]["hd95"] for r in regs], np.float64)
    return out


if __name__ == "__main__":
    res = compute()
    np.savez_compressed(os.path.join(HERE, "seg_metrics.npz"), **res)
    for k, v in res.items():
        print(k, v.tolist())
