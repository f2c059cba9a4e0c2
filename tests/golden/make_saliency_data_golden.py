#!/usr/bin/env python3
"""Generates tests/golden/saliency_data.npz (run in the BUILD container only, like make_pancreas_golden.py): the REAL reference functions
behind the saliency network's data, cut out of SaliencyAttention/utils.py with ast (the module itself needs nibabel / SimpleITK) and run
UNMODIFIED on small synthetic cases.  Only the resulting arrays are committed.

    get_none_zero_region, crop_ND_volume_with_bounding_box      utils.py:313-331, 362-388   (crop_brain_region's box and crop)
    itensity_normalize_one_volume, itensity_rescaling_one_volume utils.py:333-360
    get_random_roi_sampling_center, extract_roi_from_volume      utils.py:390-452            (sampler3d's centre and windows)

    python tests/golden/make_saliency_data_golden.py <root of the reference repository>
"""
import ast
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = sys.argv[1]
NAMES = ("get_none_zero_region", "crop_ND_volume_with_bounding_box", "itensity_normalize_one_volume", "itensity_rescaling_one_volume",
         "get_random_roi_sampling_center", "extract_roi_from_volume")


def cut(path, names):
    out = {}
    for node in ast.walk(ast.parse(open(path).read())):
        if isinstance(node, ast.FunctionDef) and node.name in names:
            out[node.name] = ast.Module(body=[node], type_ignores=[])
    assert set(out) == set(names), (path, sorted(out))
    return out


env = dict(np=np, random=random)
for name, mod in cut(os.path.join(REF, "SaliencyAttention/utils.py"), NAMES).items():
    exec(compile(mod, "utils.py", "exec"), env)
out = {}

# ---- crop_brain_region, step by step (utils.py:30-60) ------------------------------------------------------------------------------------------
rng = np.random.default_rng(77)
shape, margin = (12, 14, 15), 5
raw = np.zeros((4,) + shape, np.float32)
region = (slice(0, 5), slice(6, 9), slice(6, 8))  # touches the z = 0 face (the margin clamps), ends 7 rows inside the opposite one
raw[0][region] = rng.integers(-20, 200, (5, 3, 2)).astype(np.float32) / 4  # some voxels negative, some zero
raw[0, 0, 6, 6], raw[0, 4, 8, 7] = 3.25, -1.5  # the region's corners are non-zero whatever the draw
for c in (1, 2, 3):
    v = rng.integers(-30, 300, shape).astype(np.float32) / 8
    v[rng.random(shape) < 0.3] = 0
    raw[c] = v
assert raw[1, 11].any() and (raw[0] < 0).any() and (raw[2] < 0).any()  # non-zero outside the box; negative voxels
seg = np.zeros(shape, np.int16)
seg[0:5, 5:10, 5:9] = rng.choice([0, 1, 2, 4], (5, 5, 4))
assert set(np.unique(seg)) == {0, 1, 2, 4}
bbmin, bbmax = env["get_none_zero_region"](raw[0], margin)
assert bbmin[0] == 0 and bbmax[0] == 9 < shape[0] - 1
# (float64 in front of the reference's arithmetic, as nibabel's get_data hands it over; every value is exact in float32)
crop = [env["crop_ND_volume_with_bounding_box"](raw[c].astype(np.float64), bbmin, bbmax) for c in range(4)]
normalised = np.stack([env["itensity_normalize_one_volume"](v) for v in crop])
assert normalised.dtype == np.float64
out.update(raw=raw, seg=seg, margin=np.int64(margin), bbmin=np.array(bbmin, np.int64), bbmax=np.array(bbmax, np.int64),
           crop=np.stack(crop).astype(np.float32), weight=np.asarray(crop[0] > 0, np.float32), normalised=normalised.astype(np.float32))
for num_class, key in ((4, "label4"), (2, "label2")):
    label = seg.copy()
    if num_class == 4:  # (utils.py:51-55, verbatim)
        label[label == 4] = 3
    else:
        label[label == 4] = 1
        label[label == 2] = 1
    out[key] = env["crop_ND_volume_with_bounding_box"](label, bbmin, bbmax)

# ---- load_pancreas_img (utils.py:62-78) ----------------------------------------------------------------------------------------------------------
ct = np.clip(rng.normal(-100, 300, (6, 7, 8)), -1024, 3000).astype(np.int16)
out.update(ct=ct, ct_rescaled=env["itensity_rescaling_one_volume"](ct))

# ---- sampler3d's centre and windows (data_sampler.py:184-202: sample_mode "full", bounding_box None) -------------------------------------------
PAIRS = (((9, 20, 23), (5, 6, 7)), ((4, 6, 30), (5, 6, 7)), ((5, 6, 7), (5, 6, 7)), ((17, 33, 19), (16, 16, 16)), ((1, 1, 1), (8, 8, 8)))
real_randint = random.randint
for k, (n_in, n_out) in enumerate(PAIRS):
    calls = []

    def centre(pick, shape_in=n_in, shape_out=n_out):
        del calls[:]
        random.randint = lambda a, b: (calls.append((a, b)), pick(a, b))[1]
        try:
            return env["get_random_roi_sampling_center"](shape_in, list(shape_out), "full", None)
        finally:
            random.randint = real_randint

    ranges = np.full((3, 2), -1, np.int64)  # (-1, -1): the axis draws nothing
    for a in range(3):  # one axis at a time, so that a recorded call belongs to it
        centre(lambda a, b: a, (n_in[a],), (n_out[a],))
        assert len(calls) <= 1
        if calls:
            ranges[a] = calls[0]
    lo, hi, mid = centre(lambda a, b: a), centre(lambda a, b: b), centre(lambda a, b: (a + b) // 2)
    assert calls == [tuple(r) for r in ranges if r[0] >= 0]
    vol = rng.integers(-40, 40, n_in).astype(np.float32) / 8
    lab = (rng.random(n_in) < 0.3).astype(np.uint8) * rng.integers(1, 4, n_in).astype(np.uint8)
    rois = {"vol": [], "lab": [], "one": []}
    for c in (lo, hi, mid):
        rois["vol"].append(env["extract_roi_from_volume"](vol, c, list(n_out), fill="zero").astype(np.float32))
        rois["lab"].append(env["extract_roi_from_volume"](lab, c, list(n_out), fill="zero").astype(np.uint8))
        rois["one"].append(env["extract_roi_from_volume"](np.ones(n_in), c, list(n_out), fill="zero").astype(np.uint8))  # the copied box
    out.update({"in%d" % k: np.array(n_in, np.int64), "out%d" % k: np.array(n_out, np.int64), "ranges%d" % k: ranges,
                "centres%d" % k: np.array([lo, hi, mid], np.int64), "vol%d" % k: vol, "lab%d" % k: lab,
                "roi_vol%d" % k: np.stack(rois["vol"]), "roi_lab%d" % k: np.stack(rois["lab"]), "roi_one%d" % k: np.stack(rois["one"])})
out["n_pairs"] = np.int64(len(PAIRS))

path = os.path.join(HERE, "saliency_data.npz")
np.savez_compressed(path, **out)
print("saliency_data.npz", os.path.getsize(path))
assert os.path.getsize(path) < 300 * 1024
