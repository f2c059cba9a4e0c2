#!/usr/bin/env python3
"""Generates tests/golden/volume_zoom.npz (run in the BUILD container only, like make_golden.py; needs scipy): scipy.ndimage.zoom's own
results for the small cases of tests/zoom_ref.py (cases 0 - 8: int16 and float32 at order 3, uint8 at order 0), and the resampling of
one synthetic CT + label by each of the reference's two scripts -- their own lines, cut out of the files and run when this runs, as
make_pancreas_golden.py does.  Only arrays are committed.

    python tests/golden/make_zoom_golden.py
"""
import ast
import os
import sys
import textwrap

import numpy as np
from scipy import ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import zoom_ref as ref  # noqa: E402

out = {}
for k in range(ref.GOLDEN_CASES):
    shape, z = ref.CASES[k]
    ct, f32, seg = ref.case_inputs(k)
    out["in_i16_%d" % k] = ct
    out["in_u8_%d" % k] = seg  # (the float32 input is (ct * 0.37).astype(float32): not stored)
    out["i16_o3_%d" % k] = ndimage.zoom(ct, z, order=3)
    out["f32_o3_%d" % k] = ndimage.zoom(f32, z, order=3)
    out["u8_o0_%d" % k] = ndimage.zoom(seg, z, order=0)

# ---- the two scripts on one synthetic case ------------------------------------------------------------------------------------------------
# The loop bodies themselves, cut out of the reference's files when this runs (the modules need SimpleITK and a dataset on disk) and run
# UNMODIFIED: PointSegment/utils/cvt_CT_down.py:79-104 with FULL_SIZE = True, cvt_CT.py:79-105 with FULL_SIZE = False and a crop box.
REF = "/root/reference"
SETTINGS = ("upper", "lower", "down_scale", "slice_thickness")  # cvt_CT_down.py:24-30 == cvt_CT.py:24-30


class Spacing:
    """What the cut lines ask of the sitk image: the last entry of its spacing."""

    def __init__(self, z):
        self.z = z

    def GetSpacing(self):
        return (1.0, 1.0, self.z)


def run_script(name, first, last, count, ct_array, seg_array, spacing_z, **env):
    src = open(os.path.join(REF, "PointSegment/utils", name)).read()
    for node in ast.parse(src).body:
        if isinstance(node, ast.Assign) and node.targets[0].id in SETTINGS:
            env[node.targets[0].id] = ast.literal_eval(node.value)
    assert set(SETTINGS) <= set(env), sorted(env)
    body = textwrap.dedent("\n".join(src.split("\n")[first - 1:last]))
    nodes = ast.parse(body).body  # the cut is guarded by its shape: the z-zoom `if` first, the lower threshold's masked assignment last
    assert isinstance(nodes[0], ast.If) and isinstance(nodes[-1], ast.Assign) and isinstance(nodes[-1].targets[0], ast.Subscript), name
    assert len(nodes) == count and sum(isinstance(n, ast.If) for n in nodes) == 3, (name, len(nodes))
    env.update(np=np, ndimage=ndimage, ct=Spacing(spacing_z), ct_array=ct_array.copy(), seg_array=seg_array.copy())
    exec(compile(body, name, "exec"), env)
    return env["ct_array"], env["seg_array"], {k: env[k] for k in SETTINGS}


CHAIN_SHAPE, CHAIN_SPACING_Z, CHAIN_CROP = (20, 38, 35), 1.5, ((2, 27), (3, 40), (-4, 30))
rng = np.random.default_rng(77)
chain_ct = rng.integers(-400, 600, CHAIN_SHAPE).astype(np.int16)
chain_seg = np.zeros(CHAIN_SHAPE, np.uint8)  # a small organ: few enough positives for a 64-point cloud behind the chain
chain_seg[8:12, 14:20, 12:18] = rng.integers(1, 3, (4, 6, 6))

down_ct, down_seg, settings = run_script("cvt_CT_down.py", 79, 104, 5, chain_ct, chain_seg, CHAIN_SPACING_Z, FULL_SIZE=True)
crop_ct, crop_seg, settings2 = run_script("cvt_CT.py", 79, 105, 6, chain_ct, chain_seg, CHAIN_SPACING_Z, FULL_SIZE=False,
                                          start_slices=[c[0] for c in CHAIN_CROP], end_slices=[c[1] for c in CHAIN_CROP])
assert settings == settings2
lower, upper, slice_thickness, down_scale = (settings[k] for k in ("lower", "upper", "slice_thickness", "down_scale"))

# No voxel of either chain sits on a rounding tie (zoom_ref.TIE_WINDOW) in any of its int16 zooms, so the recorded volumes do not depend
# on the order of the float64 sums and a comparison may ask for equality -- also behind the intermediate rounding, where one flipped
# voxel would spread through the second zoom.
z_zoom = (CHAIN_SPACING_Z / slice_thickness, 1, 1)
stage1 = ndimage.zoom(chain_ct, z_zoom, order=3)  # the volume between the two zooms
assert not ref.ties(chain_ct, stage1.shape).any()
assert not ref.ties(stage1, ref.out_shape(stage1.shape, down_scale)).any()
box = ref.crop_box(stage1.shape, CHAIN_CROP)
cropped = np.flip(stage1, 1)[box]
assert not ref.ties(cropped, ref.out_shape(cropped.shape, down_scale)).any()

assert 0 < (down_seg > 0).sum() <= 64 and 0 < (crop_seg > 0).sum() <= 64
out.update(chain_ct=chain_ct, chain_seg=chain_seg, chain_spacing_z=np.float64(CHAIN_SPACING_Z), chain_crop=np.array(CHAIN_CROP, np.int64),
           chain_clip=np.array([lower, upper], np.int64), chain_down_scale=np.float64(down_scale), down_ct=down_ct, down_seg=down_seg, crop_ct=crop_ct,
           crop_seg=crop_seg)
path = os.path.join(HERE, "volume_zoom.npz")
np.savez_compressed(path, **out)
print("volume_zoom.npz", os.path.getsize(path), "chain shapes", down_ct.shape, crop_ct.shape)
