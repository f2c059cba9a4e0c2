#!/usr/bin/env python3
"""Generates tests/golden/saliency_map_views.npz (run in the BUILD container only, like make_saliency_mixup_golden.py): the REAL
flip_lr and transpose_volumes (SaliencyAttention/utils.py:15-28, 80-104), overlapping_inference and segment_one_image
(SaliencyAttention/eval.py:103-193, 355-411), cut out with ast (the modules themselves need tensorpack / nibabel) and run UNMODIFIED with a
stand-in `config`, plus the fusion expression of eval.py:254 and the TEST_FLIP average of eval.py:463, compiled from their own syntax
trees.  The model function is cheap numpy (`model` below, restated by the test): a voxel's probabilities depend on its
value AND on its position inside the window, so a wrong orientation or a wrong mirror changes them.

The reference hard-codes the steps (48, 118, 118) and one input channel.  The volume is rebuilt from a seed; only the seed, the shapes and
the expected maps' class-1 probability at a few thousand recorded voxels (corners, window seams and random ones) are committed.

    python tests/golden/make_saliency_map_golden.py <root of the reference repository>
"""
import ast
import copy
import os
import sys
import time
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = sys.argv[1]

SEED = 254
SHAPE = (60, 135, 140)
PATCH = (48, 128, 128)
STEPS = (48, 118, 118)  # eval.py:108-109
VIEWS = ("axial", "sagittal", "coronal")


def make_volume(seed, shape):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


def model(window):
    """[B, p0, p1, p2, 1] -> two-class probabilities [B, p0, p1, p2, 2], float64."""
    _, p0, p1, p2, _ = window.shape
    i, j, k = np.meshgrid(np.arange(p0), np.arange(p1), np.arange(p2), indexing="ij")
    z = 1.3 * window[..., 0].astype(np.float64) + 0.013 * i - 0.007 * j + 0.003 * k + 0.0001 * i * k
    p = 1.0 / (1.0 + np.exp(-z))
    return np.stack([1.0 - p, p], -1)


def cut(path, names):
    out = {}
    for node in ast.walk(ast.parse(open(path).read())):
        if isinstance(node, ast.FunctionDef) and node.name in names:
            out[node.name] = ast.Module(body=[node], type_ignores=[])
    assert set(out) == set(names), (path, sorted(out))
    return out


def cut_expression(path, function, target, needs):
    """The right-hand side of `target = ...` inside `function` that mentions every name of `needs`, as a compiled expression."""
    found = []
    for fn in ast.walk(ast.parse(open(path).read())):
        if isinstance(fn, ast.FunctionDef) and fn.name == function:
            for node in ast.walk(fn):
                if isinstance(node, ast.Assign) and len(node.targets) == 1 and isinstance(node.targets[0], ast.Name) and node.targets[0].id == target:
                    names = {n.id for n in ast.walk(node.value) if isinstance(n, ast.Name)}
                    if set(needs) <= names:
                        found.append(node.value)
    assert len(found) == 1, (function, target, len(found))
    return compile(ast.fix_missing_locations(ast.Expression(body=found[0])), path, "eval")


config = types.SimpleNamespace(BATCH_SIZE=2, NUM_CLASS=2, DIRECTION="axial", PATCH_SIZE=list(PATCH), INFERENCE_PATCH_SIZE=list(PATCH),
                               ADVANCE_POSTPROCESSING=False, MULTI_VIEW=False, TEST_FLIP=True)
env = dict(np=np, copy=copy, time=time, config=config)
for path, names in (("SaliencyAttention/utils.py", ("flip_lr", "transpose_volumes")),
                    ("SaliencyAttention/eval.py", ("overlapping_inference", "segment_one_image"))):
    for name, mod in cut(os.path.join(REF, path), names).items():
        exec(compile(mod, path, "exec"), env)
fusion = cut_expression(os.path.join(REF, "SaliencyAttention/eval.py"), "segment_one_image_dynamic", "prob1", ("prob1_ax", "prob1_sa", "prob1_co"))
flip_mean = cut_expression(os.path.join(REF, "SaliencyAttention/eval.py"), "eval_pancreas", "final_prob", ("probs", "probs_flip"))

vol = make_volume(SEED, SHAPE)
data = {"images": vol[..., None], "weights": np.ones(SHAPE + (1,), np.float32)}
calls = []


def model_func(image_input):
    assert image_input.shape == (config.BATCH_SIZE,) + PATCH + (1,)
    calls.append(1)
    return model(image_input), None


# the shapes do what the test needs: in every view at least two windows along at least two axes, one of them overhanging, no hole
for view in VIEWS:
    n = np.transpose(vol, {"axial": (0, 1, 2), "sagittal": (2, 0, 1), "coronal": (1, 0, 2)}[view]).shape
    origins = [np.arange(0, max(1, n[a] - PATCH[a] + STEPS[a]), STEPS[a]) for a in range(3)]
    assert sum(len(o) >= 2 for o in origins) >= 2, (view, origins)
    assert any(o[-1] + PATCH[a] > n[a] for a, o in enumerate(origins) if len(o) >= 2), view
    assert all(o[-1] + PATCH[a] >= n[a] and STEPS[a] <= PATCH[a] for a, o in enumerate(origins)), view  # count.min() >= 1

maps = {}
for view in VIEWS:
    config.DIRECTION = view
    for flip in (0, 1):
        calls.clear()
        _, probs = env["segment_one_image"](env["flip_lr"](data) if flip else data, [model_func])
        assert probs.shape == SHAPE + (2,) and probs.dtype == np.float64 and np.isfinite(probs).all() and len(calls) >= 4
        maps[view, flip] = probs
    assert np.abs(maps[view, 0] - maps[view, 1]).max() > 1e-3  # the mirror is seen
assert np.abs(maps["axial", 0] - maps["sagittal", 0]).max() > 1e-3 and np.abs(maps["axial", 0] - maps["coronal", 0]).max() > 1e-3

# eval.py:254 takes the maps in VIEW orientation and turns them itself; segment_one_image has turned ours already, so undo that first
back = {"sagittal": (2, 0, 1, 3), "coronal": (1, 0, 2, 3)}
fused = {}
for flip in (0, 1):
    fused[flip] = eval(fusion, dict(np=np, prob1_ax=maps["axial", flip], prob1_sa=np.transpose(maps["sagittal", flip], back["sagittal"]),
                                    prob1_co=np.transpose(maps["coronal", flip], back["coronal"])))
    assert fused[flip].shape == SHAPE + (2,)
fused_flip = eval(flip_mean, dict(probs=fused[0], probs_flip=fused[1]))
view_flip = {view: eval(flip_mean, dict(probs=maps[view, 0], probs_flip=maps[view, 1])) for view in VIEWS}

# the recorded voxels: the corners, both sides of every window seam of every view, and random ones
rng = np.random.default_rng(SEED + 1)
marks = [set([0, n - 1]) for n in SHAPE]
for view, axes in (("axial", (0, 1, 2)), ("sagittal", (2, 0, 1)), ("coronal", (1, 0, 2))):
    for a, vol_axis in enumerate(axes):
        n = SHAPE[vol_axis]
        for o in np.arange(0, max(1, n - PATCH[a] + STEPS[a]), STEPS[a]):
            for at in (o - 1, o, o + PATCH[a] - 1, o + PATCH[a]):
                if 0 <= at < n:
                    marks[vol_axis] |= {int(at), int(n - 1 - at)}
grid = np.array([(d, h, w) for d in sorted(marks[0]) for h in sorted(marks[1]) for w in sorted(marks[2])], np.int64)
if len(grid) > 2000:
    grid = grid[np.sort(rng.choice(len(grid), 2000, replace=False))]
corners = np.array([(d, h, w) for d in (0, SHAPE[0] - 1) for h in (0, SHAPE[1] - 1) for w in (0, SHAPE[2] - 1)], np.int64)
pos = np.unique(np.concatenate([corners, grid, np.stack([rng.integers(0, n, 500) for n in SHAPE], 1)]), axis=0)
at = (pos[:, 0], pos[:, 1], pos[:, 2], 1)  # class 1 alone: the model's two probabilities add up to 1, and every step of the rule is linear

out = {"seed": np.int64(SEED), "shape": np.array(SHAPE, np.int64), "patch": np.array(PATCH, np.int64), "steps": np.array(STEPS, np.int64), "positions": pos,
       "fused": fused[0][at], "fused_flip": fused_flip[at]}
for view in VIEWS:
    out[view] = maps[view, 0][at]
    out[view + "_flip"] = view_flip[view][at]
path = os.path.join(HERE, "saliency_map_views.npz")
np.savez_compressed(path, **out)
print("saliency_map_views.npz", os.path.getsize(path), len(pos), "positions")
assert os.path.getsize(path) < 300 * 1024
