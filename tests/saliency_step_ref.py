"""numpy float32 restatement of ps_saliency_sgd_update (include/pointseg_saliency_step.h): tf.train.MomentumOptimizer on the loss plus the
l2 regulariser of every `kernel` variable (SaliencyAttention/train.py:50-56, 83-110), per element, every product and every sum rounded to
float32 on its own -- which is what numpy does with float32 arrays and float32 scalars: it has no fused multiply-add."""
import numpy as np

F = np.float32


def decay_mask(shapes):
    """shapes: name -> shape in flat-buffer order (point_unet_amd.saliency.param_shapes) -> a bool array over the flat buffer, True on the
    elements of the tensors whose name ends in /kernel."""
    parts = [np.full(int(np.prod(shape)), name.endswith("/kernel")) for name, shape in shapes.items()]
    return np.concatenate(parts)


def sgd_update(params, grads, accum, decay, lr, momentum=0.9, l2=1e-5, grad_scale=1.0):
    """One update of float32 arrays (not in place): returns (params, accum)."""
    w, g, a = (np.asarray(t, dtype=F) for t in (params, grads, accum))
    g = g * F(grad_scale)
    g = np.where(decay, g + F(l2) * w, g)
    a = F(momentum) * a + g
    w = w - F(lr) * a
    assert w.dtype == F and a.dtype == F
    return w, a
