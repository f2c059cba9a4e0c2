"""What include/pointseg_train_loss.h computes, restated in torch float64 from PointSegment/RandLANet.py:62-84 (the ignored labels and the
label reduction), :93-94 (the accuracy) and :276-312 (dice_loss, get_loss_dice_weight): the yardstick of tests/test_point_loss_rule.py and
tests/test_gpu_point_loss.py.  The losses are written as the reference writes them -- one-hot products over the valid rows, autograd for the
gradient -- and the closed form of the header stands next to them (closed_form), so that the two can be compared."""
import numpy as np
import torch

KINDS = ("dice", "dice_weighted")
BRATS_WEIGHTS = (4.0, 1.0, 1.0, 1.0)  # the constant get_loss_dice_weight hard-codes (RandLANet.py:295)
EPS = 0.00001


def reduce_labels(labels, num_classes, ignored_label_inds):
    """RandLANet.py:66-81: a label that is one of ignored_label_inds is an ignored row (-1 here); the others go through reducing_list =
    range(C) with a 0 inserted at every ignored index, ascending.  A label outside the list is ignored too (the trainer's label map)."""
    red = list(range(num_classes))
    for v in sorted(int(v) for v in ignored_label_inds):
        red = red[:v] + [-1] + red[v:]
    red = np.asarray(red, np.int64)
    lab = np.asarray(labels).astype(np.int64)
    inside = (lab >= 0) & (lab < len(red))
    return np.where(inside, red[np.clip(lab, 0, len(red) - 1)], -1).astype(np.int32)


def _valid(z, y):
    y = torch.as_tensor(np.asarray(y).reshape(-1)).long()
    keep = (y >= 0) & (y < z.shape[1])
    return z[keep], y[keep], keep


def dice_loss(logits, labels):
    """RandLANet.py:276-291 on the valid rows"""
    one_hot = torch.nn.functional.one_hot(labels, logits.shape[1]).to(logits.dtype)
    num = 2.0 * (one_hot * logits).sum(0)
    den = logits.square().sum(0) + one_hot.sum(0)
    return 1 - (num / (den + EPS)).mean()


def get_loss_dice_weight(logits, labels, class_weights=BRATS_WEIGHTS):
    """RandLANet.py:293-312 on the valid rows, its constant [[4, 1, 1, 1]] as an argument"""
    one_hot = torch.nn.functional.one_hot(labels, logits.shape[1]).to(logits.dtype)
    cw = torch.as_tensor(np.asarray(class_weights, np.float64)).to(logits.dtype).reshape(1, -1)
    num = 2.0 * (cw * one_hot * logits).sum(0)
    den = (cw * logits.square()).sum(0) + one_hot.sum(0)
    return 1 - (num / (den + EPS)).mean()


def loss_of(kind, zv, yv, class_weights):
    if kind == "dice":
        return dice_loss(zv, yv)
    if kind == "dice_weighted":
        return get_loss_dice_weight(zv, yv, class_weights)
    if kind == "ce":  # RandLANet.py:267-274
        w = torch.as_tensor(np.asarray(class_weights, np.float64)).to(zv.dtype)[yv]
        return (torch.nn.functional.cross_entropy(zv, yv, reduction="none") * w).mean()
    raise ValueError(kind)


def loss_and_grad(kind, logits, labels, class_weights=None, grad_scale=1.0, dtype=torch.float64):
    """(loss, dloss/dlogits * grad_scale) by autograd of the reference's expressions in `dtype`; labels outside [0, C) are ignored rows.
    With nothing valid the reference's sums are empty: the loss is 1 and the gradient 0."""
    z = torch.tensor(np.asarray(logits), dtype=dtype, requires_grad=True)
    zv, yv, _ = _valid(z, labels)
    cw = np.ones(z.shape[1]) if class_weights is None else class_weights
    loss = loss_of(kind, zv, yv, cw)
    loss.backward()
    g = z.grad if z.grad is not None else torch.zeros_like(z)
    return loss.detach().numpy(), (g * grad_scale).numpy()


def sums_of(logits, labels):
    """float64 [3 C + 2]: per class (S0, S1, S2), then n_valid, n_correct"""
    z = np.asarray(logits, np.float64)
    y = np.asarray(labels).reshape(-1).astype(np.int64)
    C = z.shape[1]
    keep = (y >= 0) & (y < C)
    zv, yv = z[keep], y[keep]
    oh = np.eye(C)[yv] if len(yv) else np.zeros((0, C))
    out = np.zeros(3 * C + 2)
    out[0:3 * C:3] = (oh * zv).sum(0)
    out[1:3 * C:3] = (zv * zv).sum(0)
    out[2:3 * C:3] = oh.sum(0)
    out[3 * C], out[3 * C + 1] = top1_counts(np.asarray(logits), labels)
    return out


def closed_form(kind, logits, labels, class_weights=None, grad_scale=1.0, sums=None):
    """The header's rule: (loss, gradient) from the three sums per class (of these rows, or the ones given) in float64"""
    z = np.asarray(logits, np.float64)
    y = np.asarray(labels).reshape(-1).astype(np.int64)
    C = z.shape[1]
    s = sums_of(z, y) if sums is None else np.asarray(sums, np.float64)
    u = np.ones(C) if kind == "dice" or class_weights is None else np.asarray(class_weights, np.float64)
    S0, S1, S2 = s[0:3 * C:3], s[1:3 * C:3], s[2:3 * C:3]
    D = u * S1 + S2 + 1e-5
    sc = 2 * u * S0 / D
    a = 2 * u / (C * D)
    b = a * sc
    keep = (y >= 0) & (y < C)
    oh = np.zeros_like(z)
    oh[np.nonzero(keep)[0], y[keep]] = 1.0
    grad = grad_scale * (b[None, :] * np.where(keep[:, None], z, 0.0) - a[None, :] * oh)
    grad[~keep] = 0.0
    return 1.0 - sc.mean(), grad


def top1_counts(logits, labels):
    """tf.nn.in_top_k(valid_logits, valid_labels, 1): a valid row is correct iff its target logit is finite and no class has a strictly
    larger logit (a tie is correct).  Returns (n_valid, n_correct)."""
    z = np.asarray(logits)
    y = np.asarray(labels).reshape(-1).astype(np.int64)
    keep = (y >= 0) & (y < z.shape[1])
    zv, yv = z[keep], y[keep]
    if not len(yv):
        return 0, 0
    zt = zv[np.arange(len(yv)), yv]
    with np.errstate(invalid="ignore"):
        correct = np.isfinite(zt) & ~(zv > zt[:, None]).any(1)
    return int(keep.sum()), int(correct.sum())


def accuracy(logits, labels):
    """float32(n_correct / n_valid); 0 where the reference's mean over nothing is NaN"""
    n, k = top1_counts(logits, labels)
    return np.float32(k / n) if n else np.float32(0.0)


def train_step_with_loss(kind, params, num_layers, xyz, neigh_idx, sub_idx, interp_idx, features, labels, class_weights, dtype=torch.float64):
    """oracle.randla_train_oracle's training-mode graph under the loss `kind` ("ce" | "dice" | "dice_weighted"); labels are the training
    labels (already reduced: outside [0, C) = ignored).  Returns dict(loss, logits, grads{name: array}) from autograd."""
    from oracle import randla_train_oracle as rto
    P = {}
    for k, v in params.items():
        t = torch.tensor(np.asarray(v), dtype=dtype)
        if not k.endswith(("moving_mean", "moving_variance")):
            t.requires_grad_(True)
        P[k] = t
    logits = rto._graph(P, num_layers, xyz, neigh_idx, sub_idx, interp_idx, features, dtype, True, {}, None)
    z = logits.reshape(-1, logits.shape[-1])
    zv, yv, _ = _valid(z, labels)
    loss = loss_of(kind, zv, yv, class_weights)
    loss.backward()
    grads = {k: v.grad.numpy().copy() for k, v in P.items() if v.requires_grad}
    return dict(loss=float(loss.detach()), logits=logits.detach().numpy(), grads=grads)
