"""Dataset preparation on the device: MR volume -> full point cloud -> grid-subsampled cloud -> projection indices, the
pipeline of PointSegment/utils/dataPrepareBraTS.py (load_volume :31-72, convert_pc2ply :75-116) without the file I/O.

    volume_to_cloud      ps_volume_to_cloud   z-score per modality over its voxels > 0, non-zero voxels -> points (x-major)
    prepare_brats_volume                      + DataProcessing.grid_sub_sampling(sub_grid_size) and the 1-NN projection of the
                                              full cloud onto the sub-cloud (the reference asks sklearn's KDTree; here the
                                              exact HIP KNN -- equal distances, possibly a different index among exact ties)
    resample_pancreas_ct ps_volume_zoom       the spline zooms, flip, crop and HU clip of PointSegment/utils/cvt_CT_down.py:79-104 and
    zoom_volume                               cvt_CT.py:79-105 on a raw Pancreas CT + label (scipy.ndimage.zoom, order 3 / 0)
    prepare_pancreas_volume, pancreas_mask    ps_volume_sample: the resampled CT + positive set -> the network's clouds
"""
import ctypes

import numpy as np

from . import _lib, runtime
from .helper_tool import DataProcessing as DP


def volume_to_cloud(volumes, seg=None, device=0, ctx=None):
    """volumes: [4, X, Y, Z] raw intensities (any real dtype; taken as float32); seg: [X, Y, Z] integer labels or None.
    Returns xyz f32 [n,3], colors f32 [n,4], labels (uint8 [n], zeros without `seg`), xyz_origin int32 [n,3]."""
    vol = np.ascontiguousarray(volumes, dtype=np.float32)
    if vol.ndim != 4 or vol.shape[0] != 4:
        raise ValueError("volumes must have shape [4, X, Y, Z]")
    X, Y, Z = vol.shape[1:]
    s = None
    if seg is not None:
        s = np.ascontiguousarray(seg, dtype=np.int32)
        if s.shape != (X, Y, Z):
            raise ValueError("seg must have shape [X, Y, Z]")
    ctx = ctx or runtime.default_context(device)
    lib = _lib.lib()
    n = ctypes.c_int64(0)
    null = ctypes.c_void_p(0)
    _lib.check(lib.ps_volume_to_cloud(ctx.handle, runtime.ptr(vol), runtime.ptr(s), X, Y, Z, ctypes.byref(n), null, null, null, null))
    m = int(n.value)
    xyz = np.empty((m, 3), np.float32)
    colors = np.empty((m, 4), np.float32)
    labels = np.zeros(m, np.int32)
    origin = np.empty((m, 3), np.int32)
    if m:
        _lib.check(lib.ps_volume_to_cloud(ctx.handle, runtime.ptr(vol), runtime.ptr(s), X, Y, Z, ctypes.byref(n), runtime.ptr(xyz),
                                          runtime.ptr(colors), runtime.ptr(labels), runtime.ptr(origin)))
    return xyz, colors, labels.astype(np.uint8), origin


def prepare_brats_volume(volumes, seg=None, sub_grid_size=0.01, merge_label_4=True, chained=True, device=0, on_device=False):
    """The arrays convert_pc2ply writes for one case: the full cloud, the sub-cloud and `proj_idx` (index of the nearest
    sub-cloud point for every point of the full cloud).  merge_label_4 applies load_volume's `img[img == 4] = 3`.
    chained (default): ONE pipeline on the device, as dataPrepareBraTS.py:75-116 is one pipeline on the host -- the volume goes up
    once, ps_volume_to_cloud_dev -> ps_grid_subsample_dev -> ps_knn_batch(device pointers) hand their rows on in HBM, the results come
    down once.  chained=False: the three ops through their host-pointer entry points (three round trips over PCIe; same results, bit for bit).
    on_device=True (chained only): nothing comes down -- the same keys as CUDA tensors (labels and sub_labels int32), e.g. for
    dataset.CloudBank.add_prepared, so that volume -> bank stays in HBM."""
    if seg is not None and merge_label_4:
        seg = np.where(np.asarray(seg) == 4, 3, seg)
    if on_device and not chained:
        raise ValueError("prepare_brats_volume: on_device=True needs the chained path")
    if chained:
        return _prepare_chained(volumes, seg, sub_grid_size, device, on_device)
    xyz, colors, labels, origin = volume_to_cloud(volumes, seg)
    sub_xyz, sub_colors, sub_labels = DP.grid_sub_sampling(xyz, colors, labels.astype(np.int32), sub_grid_size)
    proj = DP.knn_search(sub_xyz[None], xyz[None], 1)[0, :, 0].astype(np.int32)
    return dict(xyz=xyz, colors=colors, labels=labels, xyz_origin=origin, sub_xyz=sub_xyz, sub_colors=sub_colors,
                sub_labels=np.asarray(sub_labels).reshape(-1).astype(np.uint8), proj_idx=proj)


def _prepare_chained(volumes, seg, sub_grid_size, device, on_device=False):
    import torch
    vol = np.ascontiguousarray(volumes, dtype=np.float32)
    if vol.ndim != 4 or vol.shape[0] != 4:
        raise ValueError("volumes must have shape [4, X, Y, Z]")
    X, Y, Z = vol.shape[1:]
    dev = torch.device("cuda", device)
    ctx = runtime.default_context(device)
    ctx.use_torch_stream()
    lib, h, p = _lib.lib(), ctx.handle, runtime.ptr
    d_vol = torch.from_numpy(vol).to(dev)
    d_seg = None
    if seg is not None:
        s = np.ascontiguousarray(seg, dtype=np.int32)
        if s.shape != (X, Y, Z):
            raise ValueError("seg must have shape [X, Y, Z]")
        d_seg = torch.from_numpy(s).to(dev)
    nvox = X * Y * Z
    xyz = torch.empty((nvox, 3), dtype=torch.float32, device=dev)
    colors = torch.empty((nvox, 4), dtype=torch.float32, device=dev)
    labels = torch.zeros(nvox, dtype=torch.int32, device=dev)
    origin = torch.empty((nvox, 3), dtype=torch.int32, device=dev)
    n = ctypes.c_int64(nvox)
    _lib.check(lib.ps_volume_to_cloud_dev(h, p(d_vol), p(d_seg), X, Y, Z, ctypes.byref(n), p(xyz), p(colors), p(labels), p(origin)))
    n = int(n.value)
    del d_vol
    if n == 0:
        raise RuntimeError("Error")  # (grid_sub_sampling's message for an empty result, wrapper.cpp:225-229)
    sub_xyz = torch.empty((n, 3), dtype=torch.float32, device=dev)
    sub_colors = torch.empty((n, 4), dtype=torch.float32, device=dev)
    sub_labels = torch.empty(n, dtype=torch.int32, device=dev)
    m = ctypes.c_int64(0)
    _lib.check(lib.ps_grid_subsample_dev(h, p(xyz), n, p(colors), 4, p(labels), 1, float(sub_grid_size), n, ctypes.byref(m), p(sub_xyz), p(sub_colors),
                                         p(sub_labels)))
    m = int(m.value)
    proj = torch.empty((n, 1), dtype=torch.int32, device=dev)
    _lib.check(lib.ps_knn_batch(h, p(sub_xyz), p(xyz), 1, m, n, 3, 1, p(proj), 1))
    if on_device:  # (stream-ordered on torch's current stream, like every tensor of the caller)
        return dict(xyz=xyz[:n], colors=colors[:n], labels=labels[:n], xyz_origin=origin[:n], sub_xyz=sub_xyz[:m], sub_colors=sub_colors[:m],
                    sub_labels=sub_labels[:m], proj_idx=proj[:, 0])
    torch.cuda.synchronize(dev)
    return dict(xyz=xyz[:n].cpu().numpy(), colors=colors[:n].cpu().numpy(), labels=labels[:n].cpu().numpy().astype(np.uint8),
                xyz_origin=origin[:n].cpu().numpy(), sub_xyz=sub_xyz[:m].cpu().numpy(), sub_colors=sub_colors[:m].cpu().numpy(),
                sub_labels=sub_labels[:m].cpu().numpy().reshape(-1).astype(np.uint8), proj_idx=proj[:, 0].cpu().numpy())


# ---- Pancreas: CT volume + positive set -> the network's clouds (ps_volume_sample, csrc/volume_sample.hip) -------------------------------

def _dev_tensor(a, dtype, dev):
    import torch
    if a is None:
        return None
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    return t.to(device=dev, dtype=dtype).contiguous()


def _volume_sample(shape, device, volume=None, mask=None, probs=None, channel=1, threshold=0.9, dilate=0, truth=None, label_src=None, n_point=0,
                   loops=1, seed=0, want_mask=False, ctx=None):
    """One ps_volume_sample call on device tensors (already of the wire dtypes).  Returns the dict of the outputs asked for."""
    import torch
    X, Y, Z = (int(s) for s in shape)
    dev = torch.device("cuda", device)
    ctx = ctx or runtime.default_context(device)
    a = _lib.PsVolumeSampleArgs()
    if volume is not None:
        a.volume = runtime.ptr(volume)
        a.volume_dtype = _lib.PS_VOLUME_I16 if volume.dtype == torch.int16 else _lib.PS_VOLUME_F32
    a.X, a.Y, a.Z = X, Y, Z
    a.mask, a.probs = runtime.ptr(mask), runtime.ptr(probs)
    if probs is not None:
        a.probs_C, a.probs_channel = int(probs.shape[-1]), int(channel)
    a.threshold, a.dilate = float(threshold), int(dilate)
    a.truth, a.label_src = runtime.ptr(truth), runtime.ptr(label_src)
    a.loops, a.N, a.seed = int(loops), int(n_point), int(seed) & 0xFFFFFFFF
    out = {"positives": torch.zeros(1, dtype=torch.int64, device=dev)}
    a.out_positives = runtime.ptr(out["positives"])
    if want_mask:
        out["mask"] = torch.empty((X, Y, Z), dtype=torch.uint8, device=dev)
        a.out_mask = runtime.ptr(out["mask"])
    if volume is not None:
        out["stats"] = torch.zeros(2, dtype=torch.float64, device=dev)
        a.out_stats = runtime.ptr(out["stats"])
    if n_point > 0:
        L, N = int(loops), int(n_point)
        out["xyz"] = torch.empty((L, N, 3), dtype=torch.float32, device=dev)
        out["labels"] = torch.empty((L, N), dtype=torch.int32, device=dev)
        out["xyz_origin"] = torch.empty((L, N, 3), dtype=torch.int32, device=dev)
        out["idx"] = torch.empty((L, N), dtype=torch.int32, device=dev)
        a.out_xyz, a.out_labels = runtime.ptr(out["xyz"]), runtime.ptr(out["labels"])
        a.out_origin, a.out_idx = runtime.ptr(out["xyz_origin"]), runtime.ptr(out["idx"])
        if volume is not None:
            out["features"] = torch.empty((L, N, 4), dtype=torch.float32, device=dev)
            a.out_features = runtime.ptr(out["features"])
    lib = _lib.lib()
    _lib.check(lib.ps_volume_sample(ctx.handle, ctypes.byref(a)))  # scratch == NULL: the size
    scratch = torch.empty(int(a.scratch_bytes), dtype=torch.uint8, device=dev)  # (stream-ordered like every tensor of the caller)
    a.scratch = runtime.ptr(scratch)
    _lib.check(lib.ps_volume_sample(ctx.handle, ctypes.byref(a)))
    if "features" in out:
        out["value"] = out["features"][..., 3:]
    return out


def _shape3(*arrays):
    for t in arrays:
        if t is not None:
            s = tuple(t.shape)[:3]
            if len(s) != 3:
                raise ValueError("expected a volume [X, Y, Z], got shape %s" % (tuple(t.shape),))
            return s
    raise ValueError("one of probs / mask is required")


def pancreas_mask(probs=None, mask=None, threshold=0.9, dilate=0, truth=None, channel=1, device=0):
    """The sampling mask of the Pancreas inference path, on the device: probs [X, Y, Z, C] (float32; channel `channel` >= threshold, compared
    in float32: genSegmentation, utils/genBinaryMap.py:67-80) or a ready mask [X, Y, Z] (!= 0), then `dilate` rounds of
    scipy.ndimage.binary_dilation's default structure, then OR truth (dilation_over_truth, PointSegment/utils/over_sampling.py:58-65).
    numpy or torch, host or device.  Returns the uint8 volume [X, Y, Z] (0 / 1) as a CUDA tensor."""
    import torch
    if (probs is None) == (mask is None):
        raise ValueError("pancreas_mask: exactly one of probs and mask")
    dev = torch.device("cuda", device)
    p = _dev_tensor(probs, torch.float32, dev)
    if p is not None and p.dim() != 4:
        raise ValueError("pancreas_mask: probs must have shape [X, Y, Z, C]")
    m, t = _as_u8_nonzero(mask, dev), _as_u8_nonzero(truth, dev)
    shape = _shape3(p, m)
    if t is not None and tuple(t.shape) != shape:
        raise ValueError("pancreas_mask: truth must have the volume's shape")
    runtime.default_context(device).use_torch_stream()
    return _volume_sample(shape, device, mask=m, probs=p, channel=channel, threshold=threshold, dilate=dilate, truth=t, want_mask=True)["mask"]


def _is_bool(a):
    return str(getattr(a, "dtype", "")) in ("bool", "torch.bool")


def _as_u8_nonzero(a, dev):
    """Any integer / bool volume -> device uint8 that is != 0 exactly where `a` is (a label 256 must not wrap to 0)."""
    import torch
    if a is None:
        return None
    if _is_bool(a):
        return _dev_tensor(a, torch.bool, dev).to(torch.uint8)
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    if t.dtype == torch.uint8:
        return t.to(dev).contiguous()
    return (t.to(dev) != 0).to(torch.uint8).contiguous()


def prepare_pancreas_volume(volume, label=None, mask=None, n_point=180000, loops=8, seed=0, probs=None, threshold=0.9, dilate=0, truth=None,
                            channel=1, device=0):
    """dataPreparePancreas.py's load_volume + sampling_convert_pc2ply (:34-46, 132-169) for one CT, on the device: `loops` clouds of
    `n_point` rows -- every positive voxel first and in voxel order, then a uniform sample of the rest, not shuffled.

    volume [X, Y, Z]: int16 or float32 (other dtypes are taken as float32), numpy or torch, host or device.
    The positive set, one of: label (the training form, :52-56: positive where label > 0, and out labels = the label's uint8 value);
    mask (the inference form, :189 "the binary of the attention network": labels 1 on the mask); probs [X, Y, Z, C] with threshold /
    channel; the last two with `dilate` rounds and an optional `truth` OR-ed in (pancreas_mask's steps, fused into the same call).

    Returns CUDA tensors with a leading `loops` axis: xyz f32 [L,N,3], features f32 [L,N,4] = [xyz | value], value f32 [L,N,1] (a view),
    labels i32 [L,N], xyz_origin i32 [L,N,3], idx i32 [L,N] (flat voxel index), and stats f64 [2] = {mean, std}, positives i64 [1].
    Loop l is the input of dataset.pancreas_cloud's consumers: build_pyramid(d["xyz"][l:l+1], cfg), features d["features"][l:l+1],
    point2prod(logits, None, d["xyz_origin"][l], volume_shape=(Z, X, Y))."""
    import torch
    if sum(x is not None for x in (label, mask, probs)) != 1:
        raise ValueError("prepare_pancreas_volume: exactly one of label, mask and probs gives the positive set")
    dev = torch.device("cuda", device)
    v = volume if isinstance(volume, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(volume))
    v = v.to(dev).contiguous() if v.dtype in (torch.int16, torch.float32) else v.to(device=dev, dtype=torch.float32).contiguous()
    if v.dim() != 3:
        raise ValueError("prepare_pancreas_volume: volume must have shape [X, Y, Z]")
    shape = tuple(v.shape)
    m = p = lab = None
    if label is not None:
        lt = label if isinstance(label, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(label))
        lab = lt.to(dev).to(torch.uint8).contiguous()  # (the reference's labels.astype(np.uint8), :152)
        m = lab
    elif mask is not None:
        m = _as_u8_nonzero(mask, dev)
    else:
        p = _dev_tensor(probs, torch.float32, dev)
        if p.dim() != 4:
            raise ValueError("prepare_pancreas_volume: probs must have shape [X, Y, Z, C]")
    t = _as_u8_nonzero(truth, dev)
    for name, x in (("label / mask", m), ("probs", p), ("truth", t)):
        if x is not None and tuple(x.shape)[:3] != shape:
            raise ValueError("prepare_pancreas_volume: %s must have the volume's shape %s" % (name, shape))
    runtime.default_context(device).use_torch_stream()
    return _volume_sample(shape, device, volume=v, mask=m, probs=p, channel=channel, threshold=threshold, dilate=dilate, truth=t, label_src=lab,
                          n_point=int(n_point), loops=int(loops), seed=seed)


# ---- Pancreas: raw CT -> the resampled volume prepare_pancreas_volume starts from (ps_volume_zoom, csrc/resample.hip) --------------------

_ZOOM_DTYPES = {"torch.int16": _lib.PS_VOLUME_I16, "torch.float32": _lib.PS_VOLUME_F32, "torch.uint8": _lib.PS_VOLUME_U8}


def _zoom_input(volume, dev, who):
    import torch
    t = volume if isinstance(volume, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(volume))
    if str(t.dtype) not in _ZOOM_DTYPES:
        raise ValueError("%s: dtype %s is none of int16, uint8, float32" % (who, t.dtype))
    if t.dim() != 3:
        raise ValueError("%s: expected a 3-D volume, got shape %s" % (who, tuple(t.shape)))
    return t.to(dev).contiguous()


def _zoom_shape(shape, zoom):
    z = (zoom,) * 3 if np.isscalar(zoom) else tuple(zoom)
    if len(z) != 3:
        raise ValueError("zoom must be a scalar or three factors")
    return tuple(int(round(n * float(f))) for n, f in zip(shape, z))  # scipy's own expression: Python's round, half to even


def _zoom_dev(v, out_shape, order, flip_mask, clip, device):
    """One ps_volume_zoom call on a contiguous device tensor."""
    import torch
    ctx = runtime.default_context(device)
    ctx.use_torch_stream()
    out = torch.empty(out_shape, dtype=v.dtype, device=v.device)
    lo, hi = (0.0, 0.0) if clip is None else (float(clip[0]), float(clip[1]))
    need = ctypes.c_int64(0)
    lib = _lib.lib()
    args = [ctx.handle, runtime.ptr(v), _ZOOM_DTYPES[str(v.dtype)], *(int(s) for s in v.shape), int(order), *(int(s) for s in out_shape), int(flip_mask),
            int(clip is not None), lo, hi, runtime.ptr(out)]
    _lib.check(lib.ps_volume_zoom(*args, None, ctypes.byref(need)))  # scratch == NULL: the size
    scratch = torch.empty(int(need.value), dtype=torch.uint8, device=v.device)  # (stream-ordered like every tensor of the caller)
    _lib.check(lib.ps_volume_zoom(*args, runtime.ptr(scratch), ctypes.byref(need)))
    return out


def _flip_mask(flip):
    axes = (flip,) if np.isscalar(flip) else tuple(flip)
    mask = 0
    for a in axes:
        if int(a) not in (0, 1, 2):
            raise ValueError("flip axes must be 0, 1 or 2, got %r" % (a,))
        mask |= 1 << int(a)
    return mask


def zoom_volume(volume, zoom, order=3, flip=(), clip=None, device=0):
    """scipy.ndimage.zoom(volume, zoom, order=order) with scipy's defaults (mode='constant', cval=0, prefilter=True, grid_mode=False), on
    the device: volume [n0, n1, n2] int16, uint8 or float32, numpy or torch, host or device; zoom a scalar or three factors; order 0 or 3.
    flip: axes read reversed (np.flip(volume, flip) in front of the zoom); clip = (lo, hi): np.clip behind it.  The output shape is
    scipy's, int(round(n * zoom)) per axis.  Returns a CUDA tensor of the input's dtype.  The rule, with the plane of zeros scipy leaves
    where j * (n - 1) / (m - 1) rounds above n - 1, is stated in include/pointseg_prepare.h."""
    import torch
    if order not in (0, 3):
        raise ValueError("zoom_volume: order must be 0 or 3")
    v = _zoom_input(volume, torch.device("cuda", device), "zoom_volume")
    shape = _zoom_shape(v.shape, zoom)
    if min(shape) < 1:
        raise ValueError("zoom_volume: zoom %r of shape %s leaves an empty volume %s" % (zoom, tuple(v.shape), shape))
    return _zoom_dev(v, shape, order, _flip_mask(flip), clip, device)


def resample_pancreas_ct(ct, seg=None, spacing_z=1.0, slice_thickness=1, down_scale=0.5, lower=-100, upper=240, flip_y=False, crop=None, device=0):
    """The resampling of one NIH Pancreas-CT case, on the device, step by step as the reference's two scripts do it:
    flip_y=False, crop=None is PointSegment/utils/cvt_CT_down.py:79-104; flip_y=True with crop is cvt_CT.py:79-105.

        1. spacing_z != slice_thickness: zoom by (spacing_z / slice_thickness, 1, 1), order 3 on the CT (rounded to int16 again, as
           scipy returns the input's dtype), order 0 on seg                                             (:80, 82)
        2. flip_y: np.flip(ct, 1) -- the CT alone, "the dataset mismatch between label and data"         (cvt_CT.py:85)
        3. crop = ((s0, e0), (s1, e1), (s2, e2)), inclusive ends, clamped to the volume, CT and seg      (cvt_CT.py:88-94)
        4. down_scale != 1: zoom by down_scale on every axis, order 3 / order 0                          (:97-99 / :98-100)
        5. clip the CT to [lower, upper]                                                                 (:103-104 / :104-105)

    The flip is an index map of step 4's read (the crop box is mirrored to match) and the clip follows step 4's rounding, so both are
    exact.  ct: int16 (other dtypes are taken as int16, as sitk.ReadImage(..., sitkInt16) does), seg: uint8 or None; numpy or torch,
    host or device.  Axis order: the arrays are SimpleITK's, [z, y, x]; spacing_z is ct.GetSpacing()[-1].  The NIfTI the scripts write
    from them and dataPreparePancreas.py then reads with nibabel is the transposed view [x, y, z].

    Returns {"ct": int16 [z, y, x], "seg": uint8 [z, y, x] or None, "spacing_scale": (int(1 / down_scale), int(1 / down_scale),
    slice_thickness / down_scale)} (the factors the scripts scale the x, y spacing by and the new z spacing, cvt_CT_down.py:148), the arrays as CUDA tensors.  They hand over
    to the sampling without leaving HBM:

        out = resample_pancreas_ct(ct, seg, spacing_z=2.5)
        clouds = prepare_pancreas_volume(out["ct"].permute(2, 1, 0).contiguous(), label=out["seg"].permute(2, 1, 0).contiguous())
    """
    import torch
    dev = torch.device("cuda", device)
    c = ct if isinstance(ct, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(ct))
    c = _zoom_input(c.to(dev).to(torch.int16), dev, "resample_pancreas_ct")
    s = None
    if seg is not None:
        s = seg if isinstance(seg, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(seg))
        s = _zoom_input(s.to(dev).to(torch.uint8), dev, "resample_pancreas_ct")
        if tuple(s.shape) != tuple(c.shape):
            raise ValueError("resample_pancreas_ct: seg must have the CT's shape")
    if spacing_z != slice_thickness:
        z = (spacing_z / slice_thickness, 1, 1)
        shape = _zoom_shape(c.shape, z)
        c = _zoom_dev(c, shape, 3, 0, None, device)
        if s is not None:
            s = _zoom_dev(s, shape, 0, 0, None, device)
    flip = 2 if flip_y else 0
    if crop is not None:
        box = [(max(0, int(a)), min(n - 1, int(b)) + 1) for n, (a, b) in zip(c.shape, crop)]
        if s is not None:
            s = s[box[0][0]:box[0][1], box[1][0]:box[1][1], box[2][0]:box[2][1]].contiguous()
        if flip_y:  # flip(ct, 1)[:, a:b] read through the flip is ct[:, n - b:n - a]
            n1 = c.shape[1]
            box[1] = (n1 - box[1][1], n1 - box[1][0])
        c = c[box[0][0]:box[0][1], box[1][0]:box[1][1], box[2][0]:box[2][1]].contiguous()
    clip = (lower, upper)
    if down_scale != 1:
        shape = _zoom_shape(c.shape, down_scale)
        c = _zoom_dev(c, shape, 3, flip, clip, device)
        if s is not None:
            s = _zoom_dev(s, shape, 0, 0, None, device)
    else:  # (no zoom left to carry the flip and the clip: an order-0 pass at the same shape is the copy that applies them)
        c = _zoom_dev(c, tuple(c.shape), 0, flip, clip, device)
    return {"ct": c, "seg": s, "spacing_scale": (int(1 / down_scale), int(1 / down_scale), slice_thickness / down_scale)}
