"""Evaluation on the device (csrc/metrics.hip): what turns logits and probability volumes into reported numbers.

    confusion / validate        Network.evaluate (PointSegment/RandLANet.py:208-264): argmax, confusion matrix, accuracy, IoU, mean IoU
    probs_to_labels             genSegmentation (utils/genSegmentationBraTS.py:67-79): probability volume -> label volume, 3 -> 4
    segmentation_metrics        Dice of label sets (utils/evaluationBraTS.py:22-64, evaluationPancreas.py:14-37) and medpy's
                                hd95(result, reference, voxelspacing, connectivity=1) (the scipy parts of evaluationBraTS.py:13-21)

Nothing here copies a volume or a cloud to the host: the confusion matrix stays on the device, and segmentation_metrics returns its
R x 5 numbers after one synchronisation.
"""
import ctypes
import math

import numpy as np
import torch

from . import _lib, runtime

BRATS_REGIONS = {"WT": (1, 2, 4), "TC": (1, 4), "ET": (4,)}  # evaluationBraTS.py:27-35 preprocess_label
PANCREAS_REGIONS = {"pancreas": (1,)}  # evaluationPancreas.py:14-37
BRATS_LABEL_VALUES = (0, 1, 2, 4)  # genSegmentationBraTS.py:73-76: class 3 -> label 4

_scratch = {}  # device -> the scratch tensor of segmentation_metrics (grows to the largest volume, then reused)


def _ctx(t):
    return runtime.default_context(t.device.index)


def _label_map(num_classes, ignored_label_inds):
    """Trainer.label_map's convention (RandLANet.py:68-81 reducing_list): raw label -> class index, -1 for an ignored label."""
    red = list(range(num_classes))
    for v in sorted(int(v) for v in ignored_label_inds):
        red = red[:v] + [-1] + red[v:]
    return red


def confusion(logits, labels, num_classes, ignored_label_inds=(), out=None):
    """Confusion matrix of a cloud on the device: logits [..., C] (CUDA float32), labels [...] (CUDA integer, raw labels).
    Rows are truth, columns prediction (sklearn's confusion_matrix).  The prediction is the argmax of the logits with ties to the lowest
    index (np.argmax; the reference's argmax of the softmax differs only where distinct logits round to equal fp32 probabilities).
    Labels in `ignored_label_inds` are dropped and the rest renumbered like the reference (RandLANet.py:226-233, generalised as the
    trainer's reducing list); a label outside [0, num_classes + len(ignored_label_inds)) is skipped.
    Returns a device int64 [C, C]; with `out` (a device int64 [C, C]) the counts are ADDED to it and `out` is returned."""
    C = int(num_classes)
    if not isinstance(logits, torch.Tensor) or not logits.is_cuda or logits.dtype != torch.float32:
        raise ValueError("confusion: logits must be a CUDA float32 tensor")
    if logits.shape[-1] != C:
        raise ValueError("confusion: logits have %d classes, num_classes is %d" % (logits.shape[-1], C))
    if not isinstance(labels, torch.Tensor) or labels.device != logits.device or labels.dtype.is_floating_point or labels.dtype == torch.bool:
        raise ValueError("confusion: labels must be an integer tensor on the logits' device")
    if labels.numel() * C != logits.numel():
        raise ValueError("confusion: %d labels for %d logit rows" % (labels.numel(), logits.numel() // C))
    if not 1 <= C <= 32:
        raise ValueError("confusion: num_classes must be in [1, 32]")
    if out is None:
        out = torch.zeros((C, C), dtype=torch.int64, device=logits.device)
    elif out.dtype != torch.int64 or tuple(out.shape) != (C, C) or out.device != logits.device or not out.is_contiguous():
        raise ValueError("confusion: out must be a contiguous int64 [%d, %d] tensor on the logits' device" % (C, C))
    lg = logits.contiguous()
    lab = labels.reshape(-1).to(torch.int32).contiguous()
    lmap = None
    if len(ignored_label_inds):
        lmap = torch.tensor(_label_map(C, ignored_label_inds), dtype=torch.int32, device=logits.device)
    _lib.check(_lib.lib().ps_confusion_accumulate(_ctx(lg).handle, runtime.ptr(lg), runtime.ptr(lab), lab.numel(), C, runtime.ptr(lmap),
                                                  lmap.numel() if lmap is not None else 0, runtime.ptr(out)))
    return out


def scores_from_confusion(cm):
    """accuracy, per-class IoU and mean IoU of a confusion matrix, as RandLANet.py:247-251 computes them.  A class that is neither in the
    truth nor predicted has IoU 0 / 0: it gets NaN here (the reference divides by zero), and mean_iou is the mean over the classes whose IoU
    is defined (NaN when none is).  accuracy is NaN when nothing was counted."""
    cm = np.asarray(cm.cpu() if isinstance(cm, torch.Tensor) else cm, dtype=np.int64)
    tp = np.diagonal(cm).astype(np.float64)
    gt, pos = cm.sum(1).astype(np.float64), cm.sum(0).astype(np.float64)
    den = gt + pos - tp
    with np.errstate(invalid="ignore", divide="ignore"):
        iou = np.where(den > 0, tp / np.where(den > 0, den, 1.0), np.nan)
    seen = float(cm.sum())
    defined = iou[~np.isnan(iou)]
    return {"accuracy": float(tp.sum() / seen) if seen else math.nan, "iou": iou,
            "mean_iou": float(defined.mean()) if defined.size else math.nan}


def validate(net, batches, ignored_label_inds=()):
    """Network.evaluate (RandLANet.py:208-264) on the device: runs `net.inference` over `(pyramid, features, labels)` batches, sums ONE
    confusion matrix on the device (no copy per batch) and returns {"accuracy", "iou", "mean_iou", "confusion"} (scores_from_confusion:
    an undefined IoU is NaN, mean_iou averages the defined ones; "confusion" is the device int64 [C, C]).

    The training-time pattern -- validate the weights a Trainer holds with an inference network:

        trainer = Trainer(cfg)
        ...
        net = Network(cfg, params=trainer.export_params())
        scores = metrics.validate(net, val_batches, cfg.ignored_label_inds)
    """
    C = int(net.config.num_classes)
    cm = None
    for pyr, feats, labels in batches:
        logits = net.inference({"pyramid": pyr, "features": feats})
        if cm is None:
            cm = torch.zeros((C, C), dtype=torch.int64, device=logits.device)
        confusion(logits, labels, C, ignored_label_inds, out=cm)
    if cm is None:
        raise ValueError("validate: no batches")
    out = scores_from_confusion(cm)
    out["confusion"] = cm
    return out


def probs_to_labels(volume, label_values=BRATS_LABEL_VALUES):
    """Probability volume [..., C] (CUDA float32, e.g. postprocess.point2prod's output) -> device uint8 label volume of shape
    volume.shape[:-1]: label_values[argmax], ties to the lowest index, so an all-zero (unsampled) voxel gets label_values[0]
    (genSegmentationBraTS.py:72-76 with its class 3 -> label 4 remap for the default table)."""
    if not isinstance(volume, torch.Tensor) or not volume.is_cuda or volume.dtype != torch.float32 or volume.dim() < 1:
        raise ValueError("probs_to_labels: volume must be a CUDA float32 tensor [..., C]")
    C = volume.shape[-1]
    vals = [int(v) for v in label_values]
    if len(vals) != C:
        raise ValueError("probs_to_labels: %d label values for %d classes" % (len(vals), C))
    if not 1 <= C <= 32 or any(not 0 <= v <= 255 for v in vals):
        raise ValueError("probs_to_labels: C must be in [1, 32] and every label value in [0, 255]")
    vol = volume.contiguous()
    out = torch.empty(vol.shape[:-1], dtype=torch.uint8, device=vol.device)
    table = (ctypes.c_int32 * C)(*vals)
    _lib.check(_lib.lib().ps_probs_to_labels(_ctx(vol).handle, runtime.ptr(vol), out.numel(), C, table, runtime.ptr(out)))
    return out


def _as_u8(t, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype.is_floating_point or t.dtype == torch.bool or t.dtype.is_complex:
        raise ValueError("segmentation_metrics: %s must be an integer CUDA tensor" % name)
    if t.dtype != torch.uint8:
        if t.numel() and (int(t.min()) < 0 or int(t.max()) > 255):
            raise ValueError("segmentation_metrics: %s holds labels outside [0, 255]" % name)
        t = t.to(torch.uint8)
    return t.contiguous()


def segmentation_metrics(pred, truth, regions=BRATS_REGIONS, spacing=(1.0, 1.0, 1.0), empty_hd95=None):
    """Dice and HD95 of label volumes pred, truth [D0, D1, D2] (CUDA integer tensors of one shape, any axis order; other integer dtypes
    are converted on the device) for every region of `regions` ({name: labels}; labels 0..31, at most 8 regions).  `spacing` is the voxel
    size per ARRAY axis.  Returns {name: {"dice", "hd95", "n_pred", "n_truth", "n_both"}}.

    dice follows evaluationBraTS.py:22-25: 1 when both masks are empty, else 2 n_both / (n_pred + n_truth).  hd95 is medpy's
    hd95(pred_mask, truth_mask, spacing, connectivity=1): the 95th percentile (numpy's linear rule) of the surface distances both ways
    between the 6-neighbourhood borders (a mask voxel on a face of the array is a border voxel).  medpy raises on an empty mask; here
    hd95 = 0 when both masks are empty and +inf when exactly one is -- or `empty_hd95` there when given (BraTS tooling uses 373.13)."""
    p, t = _as_u8(pred, "pred"), _as_u8(truth, "truth")
    if p.dim() != 3 or tuple(p.shape) != tuple(t.shape):
        raise ValueError("segmentation_metrics: pred and truth must be 3-d volumes of one shape (got %s and %s)"
                         % (tuple(p.shape), tuple(t.shape)))
    if p.device != t.device:
        raise ValueError("segmentation_metrics: pred and truth live on different devices")
    names = list(regions)
    if not 1 <= len(names) <= 8:
        raise ValueError("segmentation_metrics: 1 to 8 regions")
    masks = []
    for n in names:
        m = 0
        for lab in regions[n]:
            if not 0 <= int(lab) <= 31:
                raise ValueError("segmentation_metrics: region %r holds label %r (labels are 0..31)" % (n, lab))
            m |= 1 << int(lab)
        masks.append(m)
    sp = [float(s) for s in spacing]
    if len(sp) != 3 or any(not (math.isfinite(s) and s > 0) for s in sp):
        raise ValueError("segmentation_metrics: spacing must be three finite values > 0")
    D0, D1, D2 = p.shape
    R = len(names)
    lib = _lib.lib()
    need = lib.ps_seg_metrics_scratch_bytes(D0, D1, D2, R)
    if need < 0:
        raise ValueError("segmentation_metrics: unsupported volume shape %s" % (tuple(p.shape),))
    dev = p.device.index if p.device.index is not None else torch.cuda.current_device()
    buf = _scratch.get(dev)
    if buf is None or buf.numel() < need:
        buf = _scratch[dev] = torch.empty(int(need), dtype=torch.uint8, device=p.device)
    counts = (ctypes.c_int64 * (3 * R))()
    scores = (ctypes.c_double * (2 * R))()
    _lib.check(lib.ps_seg_metrics(_ctx(p).handle, runtime.ptr(p), runtime.ptr(t), D0, D1, D2, (ctypes.c_double * 3)(*sp),
                                  (ctypes.c_uint32 * R)(*masks), R, runtime.ptr(buf), int(buf.numel()), counts, scores))
    out = {}
    for r, n in enumerate(names):
        hd = scores[2 * r + 1]
        if empty_hd95 is not None and math.isinf(hd):
            hd = float(empty_hd95)
        out[n] = {"dice": scores[2 * r], "hd95": hd, "n_pred": counts[3 * r], "n_truth": counts[3 * r + 1], "n_both": counts[3 * r + 2]}
    return out
