"""Output side of the tester (the reference's PointSegment/testBraTS.py:83-101, 226-231 and testPancreas.py:71-85):
class probabilities of the sampled points scattered back into the image volume, on the device; and the clean-up of the predicted label
volume behind it (the reference's SaliencyAttention/eval.py:20-55, 402 and utils.py:106-164): connected components, binary morphology,
component selection, hole filling and the BraTS chain, include/pointseg_postprocess.h."""
import ctypes

import torch

from . import _lib, runtime


def point2prod(logits, p_idx, xyz_origin, volume_shape=(155, 240, 240)):
    """logits [n, C] (CUDA f32), p_idx [n] (int32 rows of the original cloud, or None), xyz_origin [total, 3] int32 voxel
    coordinates (x, y, z) of the original cloud.  Returns the volume f32 [Z, Y, X, C] -- what the reference saves after
    `np.moveaxis(volume, 1, 2)` (testBraTS.py:90), with softmax applied (testBraTS.py:183 `prob_logits`)."""
    logits = logits.contiguous()
    n, C = logits.shape
    xyz = xyz_origin.to(torch.int32).contiguous()
    total = xyz.shape[0]
    Z, X, Y = volume_shape
    vol = torch.empty((Z, Y, X, C), dtype=torch.float32, device=logits.device)
    scratch = torch.empty(total + Z * X * Y, dtype=torch.int32, device=logits.device)
    pi = p_idx.to(torch.int32).contiguous() if p_idx is not None else None
    ctx = runtime.default_context(logits.device.index)
    _lib.check(_lib.lib().ps_op_probs_to_volume(ctx.handle, runtime.ptr(logits), n, C, runtime.ptr(pi), runtime.ptr(xyz), total, Z, X, Y,
                                                runtime.ptr(vol), runtime.ptr(scratch)))
    return vol


# ---- the clean-up of a label volume (include/pointseg_postprocess.h, csrc/postprocess.hip) -------------------------------------------------

_scratch = {}  # (entry point, device index, sizing arguments) -> uint8 tensor, reused by every later call of that shape


def _mask_u8(t, who, name="mask", labels=False):
    """A contiguous CUDA integer / bool volume as uint8 without a copy where it already is one; other integer dtypes are converted
    (labels: by value, masks: to 0 / 1)."""
    if not isinstance(t, torch.Tensor):
        raise ValueError("%s: %s must be a torch tensor, got %s" % (who, name, type(t).__name__))
    if not t.is_cuda:
        raise ValueError("%s: %s must be a CUDA tensor" % (who, name))
    if t.dim() != 3 or t.numel() == 0:
        raise ValueError("%s: %s must be a non-empty 3-D volume, got shape %s" % (who, name, tuple(t.shape)))
    if t.is_floating_point() or t.is_complex():
        raise ValueError("%s: %s must have an integer or bool dtype, got %s" % (who, name, t.dtype))
    if not t.is_contiguous():
        raise ValueError("%s: %s must be contiguous" % (who, name))
    if t.numel() >= 2 ** 31:
        raise ValueError("%s: %s has %d voxels, the limit is 2^31 - 1" % (who, name, t.numel()))
    if t.dtype == torch.uint8:
        return t
    if t.dtype == torch.bool:
        return t.view(torch.uint8)
    return t.to(torch.uint8) if labels else (t != 0).view(torch.uint8)


def _same(a, b, who, name):
    if b.shape != a.shape or b.device != a.device:
        raise ValueError("%s: %s must have the shape and device of the first volume, %s on %s" % (who, name, tuple(a.shape), a.device))


def _call(fn_name, dev, key, *args):
    """The two-call protocol: size the scratch from the shapes, take it from the cache, run.  `args` holds the arguments between the
    context and the scratch pointer."""
    fn = getattr(_lib.lib(), fn_name)
    ctx = runtime.default_context(dev.index)
    need = ctypes.c_int64(0)
    _lib.check(fn(ctx.handle, *args, None, ctypes.byref(need)))
    k = (fn_name, dev.index) + key
    buf = _scratch.get(k)
    if buf is None or buf.numel() < need.value:
        buf = _scratch[k] = torch.empty(max(need.value, 1), dtype=torch.uint8, device=dev)
    _lib.check(fn(ctx.handle, *args, runtime.ptr(buf), ctypes.byref(need)))


def _connectivity(c, who):
    if c not in (1, 2, 3):
        raise ValueError("%s: connectivity must be 1, 2 or 3, got %r" % (who, c))
    return int(c)


def label_components(mask, connectivity=1, background=False, return_touches=False):
    """scipy.ndimage.label(mask, generate_binary_structure(3, connectivity)) with the component sizes, on the device: (labels int32 of
    the mask's shape, n, sizes int32[n]); background=True labels the zero voxels instead.  return_touches adds a uint8[n]: whether the
    component has a voxel on a face of the array.  n is read back (the one synchronisation here)."""
    who = "label_components"
    m = _mask_u8(mask, who)
    c = _connectivity(connectivity, who)
    V = m.numel()
    labels = torch.empty(m.shape, dtype=torch.int32, device=m.device)
    n = torch.empty(1, dtype=torch.int32, device=m.device)
    sizes = torch.empty((V + 1) // 2, dtype=torch.int32, device=m.device)
    touches = torch.empty((V + 1) // 2, dtype=torch.uint8, device=m.device)
    _call("ps_label_components", m.device, tuple(m.shape), runtime.ptr(m), *m.shape, c, 1 if background else 0, runtime.ptr(labels), runtime.ptr(n),
          runtime.ptr(sizes), runtime.ptr(touches))
    count = int(n.item())
    if return_touches:
        return labels, count, sizes[:count], touches[:count]
    return labels, count, sizes[:count]


def _morph(mask, op, connectivity, iterations, who):
    m = _mask_u8(mask, who)
    c = _connectivity(connectivity, who)
    if not isinstance(iterations, int) or iterations < 1:
        raise ValueError("%s: iterations must be an integer >= 1, got %r" % (who, iterations))
    out = torch.empty(m.shape, dtype=torch.uint8, device=m.device)
    _call("ps_binary_morph", m.device, tuple(m.shape), runtime.ptr(m), *m.shape, op, c, iterations, runtime.ptr(out))
    return out


def binary_dilation(mask, connectivity, iterations=1):
    """ndimage.binary_dilation(mask, generate_binary_structure(3, connectivity), iterations): uint8 0 / 1."""
    return _morph(mask, _lib.PS_MORPH_DILATE, connectivity, iterations, "binary_dilation")


def binary_erosion(mask, connectivity, iterations=1):
    """ndimage.binary_erosion(...): outside the array counts as 0, so every voxel with a neighbour outside goes."""
    return _morph(mask, _lib.PS_MORPH_ERODE, connectivity, iterations, "binary_erosion")


def binary_closing(mask, connectivity, iterations=1):
    """ndimage.binary_closing(...) with its defaults, border rule included: what touches a face of the array is eroded."""
    return _morph(mask, _lib.PS_MORPH_CLOSE, connectivity, iterations, "binary_closing")


def binary_opening(mask, connectivity, iterations=1):
    """ndimage.binary_opening(...) with its defaults."""
    return _morph(mask, _lib.PS_MORPH_OPEN, connectivity, iterations, "binary_opening")


def _keep(mask, rule, connectivity, threshold, main, who):
    m = _mask_u8(mask, who)
    c = _connectivity(connectivity, who)
    mm = None
    if main is not None:
        mm = _mask_u8(main, who, "main")
        _same(m, mm, who, "main")
    out = torch.empty(m.shape, dtype=torch.uint8, device=m.device)
    _call("ps_keep_components", m.device, tuple(m.shape) + (rule,), runtime.ptr(m), *m.shape, c, rule, int(threshold), runtime.ptr(mm), runtime.ptr(out))
    return out


def largest_two_components(mask, threshold=None, connectivity=2):
    """The reference's get_largest_two_component(mask, False, threshold) (SaliencyAttention/utils.py:127-164), uint8 0 / 1.  With a
    threshold (non-zero, as the reference tests it): every component larger than it -- but a lone component is kept whatever its size.
    Without: the largest component, and the second largest when ten times its size exceeds the largest's; at most one component: the
    mask as it is.  Equal sizes rank by label, the lower first."""
    who = "largest_two_components"
    if threshold:
        if int(threshold) != threshold or threshold < 0:
            raise ValueError("%s: threshold must be a non-negative integer, got %r" % (who, threshold))
        return _keep(mask, _lib.PS_KEEP_ABOVE, connectivity, threshold, None, who)
    return _keep(mask, _lib.PS_KEEP_LARGEST_TWO, connectivity, 0, None, who)


def remove_external_core(main, ext):
    """The reference's remove_external_core(lab_main, lab_ext) (SaliencyAttention/utils.py:106-124): the 18-connected components of
    `ext` of which at least half the voxels are set in `main`, uint8 0 / 1."""
    return _keep(ext, _lib.PS_KEEP_OVERLAP, 2, 0, main, "remove_external_core")


def fill_holes(mask):
    """scipy.ndimage.binary_fill_holes(mask): the mask plus every 6-connected component of its zero voxels that touches no face."""
    who = "fill_holes"
    m = _mask_u8(mask, who)
    out = torch.empty(m.shape, dtype=torch.uint8, device=m.device)
    _call("ps_fill_holes", m.device, tuple(m.shape), runtime.ptr(m), *m.shape, runtime.ptr(out))
    return out


def brats_post_processing(pred, weight=None, wt_threshold=2000):
    """The reference's post_processing(pred, weight) (SaliencyAttention/eval.py:20-55) in one call, no synchronisation: labels
    {0, 1, 2, 4} in, uint8 labels out -- what metrics.segmentation_metrics takes.  weight: non-zero = brain (None: everywhere)."""
    who = "brats_post_processing"
    p = _mask_u8(pred, who, "pred", labels=True)
    w = None
    if weight is not None:
        w = _mask_u8(weight, who, "weight")
        _same(p, w, who, "weight")
    if int(wt_threshold) != wt_threshold or wt_threshold < 0:
        raise ValueError("%s: wt_threshold must be a non-negative integer, got %r" % (who, wt_threshold))
    out = torch.empty(p.shape, dtype=torch.uint8, device=p.device)
    _call("ps_brats_postprocess", p.device, tuple(p.shape), runtime.ptr(p), runtime.ptr(w), *p.shape, int(wt_threshold), runtime.ptr(out))
    return out
