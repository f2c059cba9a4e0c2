#!/usr/bin/env python3
"""Generates tests/golden/pancreas_prepare.npz (run in the BUILD container only, like make_golden.py): the REAL reference functions of the
Pancreas preparation, cut out of their files with ast (the modules themselves need nibabel / SimpleITK) and run UNMODIFIED on a small
synthetic case with their file output captured.  Only the resulting arrays are committed.

    itensity_normalize_one_volume, sampling_convert_pc2ply   PointSegment/utils/dataPreparePancreas.py:34-46, 132-169
    genSegmentation                                          utils/genBinaryMap.py:67-80
    dilation_over_truth                                      PointSegment/utils/over_sampling.py:58-65

    python tests/golden/make_pancreas_golden.py
"""
import ast
import os
import random

import numpy as np
from scipy import ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"


def cut(path, names):
    out = {}
    for node in ast.walk(ast.parse(open(path).read())):
        if isinstance(node, ast.FunctionDef) and node.name in names:
            out[node.name] = ast.Module(body=[node], type_ignores=[])
    assert set(out) == set(names), (path, sorted(out))
    return out


shape = (40, 36, 28)
X, Y, Z = shape
rng = np.random.default_rng(41)
volume = np.clip(rng.normal(-200, 400, shape), -1024, 3000).astype(np.int16)  # Hounsfield-like, negative mean
g = np.stack(np.meshgrid(*[np.arange(s) for s in shape], indexing="ij"), -1).astype(np.float64)
label = ((((g - np.array([22, 15, 12])) / np.array([7, 6, 5])) ** 2).sum(-1) < 1.0).astype(np.uint8)  # a blob

# ---- normalisation + sampling --------------------------------------------------------------------------------------------------------------
saved, plys = {}, {}
env = dict(np=np, os=os, random=random, n_point=shape[0] * shape[1] * shape[2], out_format=".ply", original_pc_folder="full", sub_pc_folder="sub",
           write_ply=lambda path, fields, names: plys.__setitem__(os.path.basename(path), [np.asarray(f) for f in fields]),
           print=lambda *a, **k: None)
env["np"] = type("np_", (), {"__getattr__": lambda self, k: getattr(np, k)})()
type(env["np"]).save = staticmethod(lambda path, arr: saved.__setitem__(os.path.basename(path), np.asarray(arr)))
fns = cut(os.path.join(REF, "PointSegment/utils/dataPreparePancreas.py"), ("itensity_normalize_one_volume", "sampling_convert_pc2ply"))
for name in fns:
    exec(compile(fns[name], "dataPreparePancreas.py", "exec"), env)
img = env["itensity_normalize_one_volume"](volume)
random.seed(1)
env["sampling_convert_pc2ply"]([img, label], "case")  # n_point = X * Y * Z: the draw holds every voxel
origin = saved["case_xyz_origin_loop_0.npy"].astype(np.int64)
xyz, colors, labels = plys["case_loop_0.ply"]
flat = (origin[:, 0] * Y + origin[:, 1]) * Z + origin[:, 2]
assert len(np.unique(flat)) == X * Y * Z
order = np.argsort(flat)  # rows matched by origin, whatever random.sample did
full = dict(xyz=xyz[order].astype(np.float32), value=colors[order].reshape(-1).astype(np.float32), labels=labels[order].astype(np.uint8))
# one draw at a smaller n_point: the positives come first and ascending
saved.clear(); plys.clear()
env["n_point"] = int(label.sum()) + 3000
random.seed(2)
env["sampling_convert_pc2ply"]([img, label], "small")
o = saved["small_xyz_origin_loop_3.npy"].astype(np.int64)
small_flat = (o[:, 0] * Y + o[:, 1]) * Z + o[:, 2]

# ---- attention map -> binary map -> dilation OR truth ----------------------------------------------------------------------------------------
t = np.float32(0.9)
p1 = rng.integers(0, 61, shape).astype(np.float32) / np.float32(64)  # (a coarse lattice below the threshold: the file stays small)
edge = rng.random(shape) < 0.05
p1[edge] = np.array([np.nextafter(t, np.float32(0)), t, np.nextafter(t, np.float32(1))], np.float32)[rng.integers(0, 3, shape)[edge]]
for f in ((0, 5, 5), (X - 1, 5, 5), (5, 0, 5), (5, Y - 1, 5), (5, 5, 0), (5, 5, Z - 1), (0, 0, 0), (X - 1, Y - 1, Z - 1)):
    p1[f] = 1.0  # a mask touching every face of the array
probs = np.stack([1 - p1, p1], -1).astype(np.float32)
seg_out = {}
env2 = dict(np=type("np2", (), {"__getattr__": lambda self, k: getattr(np, k), "load": staticmethod(lambda path: probs.copy())})(),
            save_to_nii=lambda seg, name, out: seg_out.__setitem__("seg", np.asarray(seg)), print=lambda *a, **k: None)
exec(compile(cut(os.path.join(REF, "utils/genBinaryMap.py"), ("genSegmentation",))["genSegmentation"], "genBinaryMap.py", "exec"), env2)
env2["genSegmentation"](["maps/case.npy", "out", 0.9])
binary = seg_out["seg"].astype(np.uint8)
env3 = dict(np=np, ndimage=ndimage)
exec(compile(cut(os.path.join(REF, "PointSegment/utils/over_sampling.py"), ("dilation_over_truth",))["dilation_over_truth"], "over_sampling.py", "exec"), env3)
dilated_truth = np.asarray(env3["dilation_over_truth"](binary, label)).astype(np.uint8)

np.savez_compressed(os.path.join(HERE, "pancreas_prepare.npz"), volume=volume, label=label, xyz=np.ascontiguousarray(full["xyz"].T), value=full["value"], labels=full["labels"],
                    small_n_point=np.int64(env["n_point"]), small_flat=small_flat.astype(np.int32), probs1=p1, binary=binary, dilated_truth=dilated_truth)
print("pancreas_prepare.npz", os.path.getsize(os.path.join(HERE, "pancreas_prepare.npz")))
