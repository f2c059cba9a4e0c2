#!/usr/bin/env python3
"""Generates tests/golden/saliency_view.npz (run in the BUILD container only, like make_saliency_data_golden.py): the REAL sampler3d
(SaliencyAttention/data_sampler.py:169-214) with transpose_volumes, get_random_roi_sampling_center and extract_roi_from_volume
(SaliencyAttention/utils.py:80-104, 390-452) under it, cut out with ast (the modules themselves need tensorpack / nibabel) and run
UNMODIFIED with a stand-in `config` (DIRECTION, PATCH_SIZE) for the three directions, random.randint replaced by low / high / mid picks.
A second run has sampler3d's single assignment `flip = False` rewritten to `flip = True` in the syntax tree, everything else untouched:
it pins the flip of image, label and weight.  Only the resulting arrays are committed.

The reference's fill is np.random, so images are recorded inside the copied box only (zero elsewhere); the weight handed in is all ones,
so the weight that comes back marks the box.

    python tests/golden/make_saliency_view_golden.py <root of the reference repository>
"""
import ast
import copy
import os
import random
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = sys.argv[1]
CASES = (((9, 20, 23), (5, 6, 7)), ((4, 6, 30), (5, 6, 7)), ((17, 33, 19), (16, 16, 16)))  # (volume [d, h, w], patch in view axes): non-cubic
DIRECTIONS = ("axial", "sagittal", "coronal")
PICKS = {"lo": lambda a, b: a, "hi": lambda a, b: b, "mid": lambda a, b: (a + b) // 2}
C = 2


def cut(path, names):
    out = {}
    for node in ast.walk(ast.parse(open(path).read())):
        if isinstance(node, ast.FunctionDef) and node.name in names:
            out[node.name] = node
    assert set(out) == set(names), (path, sorted(out))
    return out


nodes = cut(os.path.join(REF, "SaliencyAttention/utils.py"), ("transpose_volumes", "get_random_roi_sampling_center", "extract_roi_from_volume"))
nodes.update(cut(os.path.join(REF, "SaliencyAttention/data_sampler.py"), ("sampler3d",)))

# sampler3d with its one `flip = False` turned into `flip = True`
flipped = copy.deepcopy(nodes["sampler3d"])
hits = [n for n in ast.walk(flipped) if isinstance(n, ast.Assign) and len(n.targets) == 1 and isinstance(n.targets[0], ast.Name)
        and n.targets[0].id == "flip"]
assert len(hits) == 1 and isinstance(hits[0].value, ast.Constant) and hits[0].value.value is False
hits[0].value = ast.Constant(value=True)
flipped.name = "sampler3d_flipped"

config = types.SimpleNamespace(DIRECTION="axial", PATCH_SIZE=None)
env = dict(np=np, random=random, config=config)
for node in list(nodes.values()) + [flipped]:
    exec(compile(ast.fix_missing_locations(ast.Module(body=[node], type_ignores=[])), "reference", "exec"), env)

# the centre sampler3d drew and the ranges it drew from, recorded around the reference's function (which runs as it is)
real_centre = env["get_random_roi_sampling_center"]
seen = {}


def recording_centre(*a, **kw):
    seen["centre"] = real_centre(*a, **kw)
    return seen["centre"]


env["get_random_roi_sampling_center"] = recording_centre

rng = np.random.default_rng(2024)
out = {"n_cases": np.int64(len(CASES)), "directions": np.array(DIRECTIONS), "picks": np.array(list(PICKS))}
real_randint = random.randint
for k, (shape, patch) in enumerate(CASES):
    vols = [rng.integers(-40, 40, shape).astype(np.float32) / 8 for _ in range(C)]
    label = ((rng.random(shape) < 0.3) * rng.integers(1, 4, shape)).astype(np.uint8)
    out.update({"shape%d" % k: np.array(shape, np.int64), "patch%d" % k: np.array(patch, np.int64), "image%d" % k: np.stack(vols, -1), "label%d" % k: label})
    config.PATCH_SIZE = list(patch)
    for direction in DIRECTIONS:
        config.DIRECTION = direction
        for pick, fn in PICKS.items():
            for flip in (0, 1):
                if flip and pick != "hi":  # (an odd extent at its highest centre leaves a row of fill at the far end: the box is off centre)
                    continue
                calls = []
                random.randint = lambda a, b, fn=fn: (calls.append((a, b)), fn(a, b))[1]
                try:
                    batch = env["sampler3d_flipped" if flip else "sampler3d"]([v.copy() for v in vols], label.copy(), np.ones(shape, np.uint8))
                finally:
                    random.randint = real_randint
                key = "%d_%s_%s_%d" % (k, direction, pick, flip)
                image, weight, lab = batch["images"], batch["weights"][..., 0], batch["labels"][..., 0]
                assert image.shape == tuple(patch) + (C,) and weight.shape == tuple(patch) and set(np.unique(weight)) <= {0, 1}
                out["centre_" + key] = np.array(seen["centre"], np.int64)
                out["ranges_" + key] = np.array(calls, np.int64).reshape(-1, 2)
                out["image_" + key] = (image * weight[..., None]).astype(np.float32)  # inside the copied box only
                out["weight_" + key] = weight.astype(np.uint8)
                out["label_" + key] = lab.astype(np.uint8)

path = os.path.join(HERE, "saliency_view.npz")
np.savez_compressed(path, **out)
print("saliency_view.npz", os.path.getsize(path))
assert os.path.getsize(path) < 300 * 1024
