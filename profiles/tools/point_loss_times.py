"""The point network's loss stage and its training step under the objectives of include/pointseg_train_loss.h, timed.

    python profiles/tools/point_loss_times.py stage [--rows 1440000] [--classes 4] [--reps 50]
        the ops behind the three kinds on random logits, interleaved in ONE process, a hipEvent pair around each: "ce" (ps_op_weighted_ce,
        what the step ran before), "ce+acc" (with ps_op_top1_counts), "dice" and "dice_weighted" (ps_op_dice_sums + ps_op_dice_from_sums;
        the counts come with the sums)
    python profiles/tools/point_loss_times.py step [--loss ce] [--batch 8] [--points 180000] [--steps 30] [--root DIR]
        Trainer.train_step on a resident batch (the pyramid is built once, outside).  --root: import the package from another checkout
        of the repository (with its library built), e.g. the parent commit's -- a tree whose Trainer takes no loss= runs its one objective.

Prints one line per figure: the median and the range over the repetitions; nothing is asserted."""
import argparse
import ctypes
import os
import sys

import numpy as np


def _stats(v):
    v = np.sort(np.asarray(v))
    return "median %.4f min %.4f max %.4f ms (n = %d)" % (float(np.median(v)), v[0], v[-1], len(v))


def stage(args):
    import torch
    from point_unet_amd import _lib, runtime
    L = _lib.lib()
    ctx = runtime.default_context(0)
    ctx.use_torch_stream()
    h = ctx.handle
    R, C = args.rows, args.classes
    rng = np.random.default_rng(0)
    z = torch.from_numpy(rng.standard_normal((R, C)).astype(np.float32)).cuda()
    y = torch.from_numpy(rng.integers(0, C, R).astype(np.int32)).cuda()
    cw = torch.from_numpy(np.asarray([4.0] + [1.0] * (C - 1), np.float32)).cuda()
    loss = torch.zeros(1, dtype=torch.float32, device="cuda")
    dl = torch.empty_like(z)
    sums = torch.empty(3 * C + 2, dtype=torch.float64, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def ce():
        _lib.check(L.ps_op_weighted_ce(h, p(z), p(y), p(cw), R, C, p(loss), p(dl)))

    def ce_acc():
        ce()
        _lib.check(L.ps_op_top1_counts(h, p(z), p(y), R, C, p(sums)))

    def dice(kind):
        _lib.check(L.ps_op_dice_sums(h, p(z), p(y), R, C, p(sums)))
        _lib.check(L.ps_op_dice_from_sums(h, kind, p(z), p(y), p(cw), p(sums), 1.0, R, C, p(loss), p(dl)))

    runs = {"ce": ce, "ce+acc": ce_acc, "dice": lambda: dice(1), "dice_weighted": lambda: dice(2)}
    for _ in range(5):
        for fn in runs.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in runs}
    for _ in range(args.reps):
        for k, fn in runs.items():  # interleaved: every kind sees the same clocks and the same neighbours on the card
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b))
    for k, v in times.items():
        print("LOSS STAGE R %d C %d %-13s %s" % (R, C, k, _stats(v)))
    print("LOSS STAGE dice / ce = %.3f (medians)" % (np.median(times["dice"]) / np.median(times["ce"])))


def step(args):
    import inspect
    import torch
    from point_unet_amd import weights
    from point_unet_amd.pyramid import build_pyramid
    from point_unet_amd.train import Trainer

    class Cfg:
        num_layers, k_n, num_classes, in_channels = 5, 16, 4, 7
        sub_sampling_ratio = [4, 4, 4, 4, 2]
        d_out = [16, 64, 128, 256, 512]

    B, n0 = args.batch, args.points
    rng = np.random.default_rng(7)
    xyz = rng.random((B, n0, 3), dtype=np.float32)
    feats = np.concatenate([xyz, rng.standard_normal((B, n0, 4)).astype(np.float32)], -1)
    labels = rng.integers(0, 4, (B, n0)).astype(np.int32)
    kw = {}
    if "loss" in inspect.signature(Trainer.__init__).parameters:
        kw["loss"] = args.loss
    tr = Trainer(Cfg, params=weights.init_params(Cfg, seed=2), keep_prob=0.5, class_weights=np.asarray([4, 1, 1, 1], np.float32), **kw)
    d_feats, d_lab = torch.from_numpy(feats).cuda(), torch.from_numpy(labels).cuda()
    pyr = build_pyramid(torch.from_numpy(xyz).cuda(), Cfg)
    for _ in range(5):
        tr.train_step(pyr, d_feats, d_lab)
    torch.cuda.synchronize()
    times = []
    for _ in range(args.steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        tr.train_step(pyr, d_feats, d_lab)
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    print("TRAIN STEP %s batch %d points %d loss %s: %s" % (args.tag, B, n0, kw.get("loss", "ce (the tree's only one)"), _stats(times)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["stage", "step"])
    ap.add_argument("--rows", type=int, default=8 * 180000)
    ap.add_argument("--classes", type=int, default=4)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--loss", default="ce")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--points", type=int, default=180000)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--root", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
    ap.add_argument("--tag", default="this tree")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    (stage if args.what == "stage" else step)(args)


if __name__ == "__main__":
    main()
