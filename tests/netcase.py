"""Shared construction of the network parity cases (BASELINE configs)."""
import numpy as np

from conftest import brats_cloud, uniform_cloud


def make_cfg(num_layers=2, d_out=(16, 64), ratios=(4, 4), k_n=16, num_classes=4, in_channels=7):
    class Cfg:
        pass

    c = Cfg()
    c.num_layers, c.d_out, c.sub_sampling_ratio = num_layers, list(d_out), list(ratios)
    c.k_n, c.num_classes, c.in_channels = k_n, num_classes, in_channels
    return c


def config1():
    """BASELINE config 1: single 18 000-point synthetic cloud, K=16, 2-layer RandLA-Net."""
    cfg = make_cfg()
    xyz = uniform_cloud(18000, 0)[None]
    feats = np.random.default_rng(1).standard_normal((1, 18000, 4)).astype(np.float32)
    return cfg, xyz, np.concatenate([xyz, feats], -1)


WIDE_ROWS_N0, WIDE_ROWS_B = 17000, 2


def wide_rows(seed=40, n0=WIDE_ROWS_N0, B=WIDE_ROWS_B):
    """The ladder's widths (16..512, K = 16) at subsampling ratios (2, 2, 2, 2, 2) on two clouds of 17 000 points (17 000 / 8 500 / 4 250 /
    2 125 / 1 062 / 531 per cloud): every level keeps enough rows to cross the row thresholds at which the training step and its ops
    switch kernels (level_rows; tests/test_wide_rows_case.py lists them), at a size the float64 autograd oracle still runs in seconds."""
    cfg = make_cfg(5, (16, 64, 128, 256, 512), (2, 2, 2, 2, 2), 16, 4, 7)
    xyz = np.stack([brats_cloud(n0, seed + b, grid=(40, 40, 30)) for b in range(B)])
    feats = np.random.default_rng(seed + 100).standard_normal((B, n0, 4)).astype(np.float32)
    return cfg, xyz, np.concatenate([xyz, feats], -1)


def level_rows(cfg, n0, B):
    """([N] rows, [N*K] rows) of every encoder level, from the config alone: level i holds B * n_i points, n_{i+1} = n_i // ratio_i
    (ps_pyramid_build), and its LFA branch runs on B * n_i * K rows."""
    n, rows = n0, []
    for r in list(cfg.sub_sampling_ratio)[:cfg.num_layers]:
        rows.append(B * n)
        n //= r
    return rows, [v * cfg.k_n for v in rows]

def small_deep(n0=6000, seed=0, k_n=16, B=1, classes=4, mods=4):
    """All five encoder widths (16..512) on a small lattice cloud: exercises every compiled kernel shape."""
    cfg = make_cfg(5, (16, 64, 128, 256, 512), (4, 4, 4, 4, 2), k_n, classes, 3 + mods)
    xyz = np.stack([brats_cloud(n0, seed + b, grid=(40, 40, 30)) for b in range(B)])
    feats = np.random.default_rng(seed + 100).standard_normal((B, n0, mods)).astype(np.float32)
    return cfg, xyz, np.concatenate([xyz, feats], -1)
