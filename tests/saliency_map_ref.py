"""numpy restatement of the rule of include/pointseg_saliency_map.h: segment_one_image (SaliencyAttention/eval.py:355-411) around
overlapping_inference (eval.py:103-193, restated in saliency_ref.py), with transpose_volumes (utils.py:80-104), flip_lr and TEST_FLIP
(utils.py:15-28, eval.py:461-463) and the MULTI_VIEW fusion (eval.py:254).  Float64 sums, as the reference's; `fuse32` is the fusion in
the float32 order the header states.  The reference's own functions, run unmodified, pin `one_view`, `flipped` and `fuse` through
tests/golden/saliency_map_views.npz (make_saliency_map_golden.py)."""
import numpy as np

import saliency_ref as ref

VIEWS = ("axial", "sagittal", "coronal")
TO_VIEW = {"axial": (0, 1, 2), "sagittal": (2, 0, 1), "coronal": (1, 0, 2)}      # transpose_volumes
FROM_VIEW = {"axial": (0, 1, 2), "sagittal": (1, 2, 0), "coronal": (1, 0, 2)}    # segment_one_image's way back


def to_view(volume, view):
    """volume [C, D, H, W] -> the view's [C, n0, n1, n2]."""
    return np.stack([np.transpose(x, TO_VIEW[view]) for x in volume])


def from_view(probs, view):
    """A map [n0, n1, n2, K] in view orientation -> [D, H, W, K]."""
    return np.transpose(probs, FROM_VIEW[view] + (3,))


def one_view(volume, probs_of, patch, steps, num_classes, view="axial"):
    """One unflipped pass: volume [C, D, H, W] -> (map [D, H, W, K] float64, count [D, H, W]); a voxel no window covers gives 0."""
    with np.errstate(invalid="ignore", divide="ignore"):
        mean, count = ref.overlapping_inference(to_view(volume, view), probs_of, patch, steps, num_classes)
    mean = np.where(count[..., None] > 0, mean, 0.0)
    return from_view(mean, view), np.transpose(count, FROM_VIEW[view])


def flipped(volume, probs_of, patch, steps, num_classes, view="axial"):
    """The flip pass: the volume mirrored along W BEFORE the view transform, its map mirrored back along W."""
    m, _ = one_view(np.flip(volume, axis=-1), probs_of, patch, steps, num_classes, view)
    return np.flip(m, axis=2)


def fuse(maps):
    """eval.py:254, float64: (m0 + m1 + ...) / n; one map is itself."""
    if len(maps) == 1:
        return maps[0]
    total = maps[0]
    for m in maps[1:]:
        total = total + m
    return total / float(len(maps))


def fuse32(maps):
    """The header's order in float32: fl32(fl32(...fl32(m0 + m1)...) / float(n)), a correctly rounded division."""
    maps = [np.asarray(m, np.float32) for m in maps]
    if len(maps) == 1:
        return maps[0]
    total = maps[0]
    for m in maps[1:]:
        total = total + m
    return total / np.float32(len(maps))


def flip_average32(m0, m1):
    return (np.asarray(m0, np.float32) + np.asarray(m1, np.float32)) * np.float32(0.5)


def saliency_map(volume, probs_of, patch, steps, num_classes, views=("axial",), flip=False, f32=False):
    """The whole rule.  probs_of: one function, or one per view.  f32: the per-pass maps rounded to float32 and fused in the header's
    float32 order (what the device does behind its float32 window sums); otherwise everything in float64."""
    fns = probs_of if isinstance(probs_of, (list, tuple)) else [probs_of] * len(views)
    fused = []
    for f in ((False, True) if flip else (False,)):
        maps = [(flipped if f else lambda *a: one_view(*a)[0])(volume, fn, patch, steps, num_classes, v) for v, fn in zip(views, fns)]
        fused.append(fuse32(maps) if f32 else fuse(maps))
    if not flip:
        return fused[0]
    return flip_average32(*fused) if f32 else (fused[0] + fused[1]) / 2.0
