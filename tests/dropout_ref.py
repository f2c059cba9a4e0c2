"""numpy uint32 restatement of the dropout of the training step: hash32 and dropout_kernel of csrc/ops_train.hip, and the per-step seed
of the trainer (csrc/trainer.hip and the Python tape, train.py).  test_dropout_mask.py checks the statistics of the masks on the CPU;
test_gpu_train_ops.py checks the kernel against it bit for bit."""
import numpy as np

SEED_STEP = 0x9E3779B9  # seed of step s, rank r: SEED_STEP * (s + 1) + SEED_RANK * r (mod 2^32)
SEED_RANK = 0x85EBCA6B
INDEX_MUL = 2654435761  # the element index is multiplied by this before the seed is xor-ed in


def hash32(x):
    x = np.asarray(x, dtype=np.uint32).copy()
    with np.errstate(over="ignore"):
        _mix(x)
    return x


def _mix(x):
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x7FEB352D)
    x ^= x >> np.uint32(15)
    x *= np.uint32(0x846CA68B)
    x ^= x >> np.uint32(16)


def step_seed(step, rank=0):
    """The seed the trainer hands ps_op_dropout for the step that follows `step` completed steps."""
    return (SEED_STEP * (step + 1) + SEED_RANK * rank) & 0xFFFFFFFF


def uniform(n, seed):
    """u in [0, 1) with 24 bits, per element index e < n (the index wraps at 2^32 like the kernel's unsigned cast)."""
    e = np.arange(n, dtype=np.uint64).astype(np.uint32)
    with np.errstate(over="ignore"):
        h = hash32((e * np.uint32(INDEX_MUL)) ^ np.uint32(seed))
    return (h >> np.uint32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)


def keep_mask(n, seed, keep):
    """bool[n]: the elements dropout keeps (u < keep, compared in float32 like the kernel)."""
    return uniform(n, seed) < np.float32(keep)


def dropout_mask(n, seed, keep):
    """float32[n]: the mask ps_op_dropout writes, 0 or float32(1 / keep)."""
    scale = np.float32(1.0) / np.float32(keep)
    return np.where(keep_mask(n, seed, keep), scale, np.float32(0.0)).astype(np.float32)
