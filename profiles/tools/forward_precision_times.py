"""The inference forward at its two precisions (include/pointseg_forward_precision.h), timed side by side in ONE process:
Network(precision="bf16x3") and Network(precision="bf16") on the same pyramid and features, forwards interleaved, on the 180 000-point
K = 16 BraTS cloud and the 262 144-point K = 32 cloud.  Preheat, then the best of three windows per mode (hipEvent pairs around `--reps`
interleaved forwards each), then the per-stage device times of one forward per mode through ps_timing_begin / _select / _end.

    python profiles/tools/forward_precision_times.py [--reps 20] [--clouds brats pancreas]

Prints one line per (cloud, mode) and one per (cloud, stage); nothing is asserted."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from point_unet_amd import weights  # noqa: E402
from point_unet_amd.RandLANet import Network  # noqa: E402
from point_unet_amd.pyramid import build_pyramid  # noqa: E402

MODES = ("bf16x3", "bf16")


def cfg_of(k_n, in_channels, num_classes):
    class Cfg:
        num_layers = 5
        sub_sampling_ratio = [4, 4, 4, 4, 2]
        d_out = [16, 64, 128, 256, 512]

    Cfg.k_n, Cfg.in_channels, Cfg.num_classes = k_n, in_channels, num_classes
    return Cfg


CLOUDS = {"brats": (180000, 16, 7, 4), "pancreas": (262144, 32, 4, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--clouds", nargs="+", default=list(CLOUDS))
    args = ap.parse_args()
    for name in args.clouds:
        n0, k_n, cin, ncls = CLOUDS[name]
        cfg = cfg_of(k_n, cin, ncls)
        rng = np.random.default_rng(0)
        xyz = rng.random((1, n0, 3), dtype=np.float32)
        feats = np.concatenate([xyz, rng.standard_normal((1, n0, cin - 3)).astype(np.float32)], -1)
        x, f = torch.from_numpy(xyz).cuda(), torch.from_numpy(feats).cuda()
        params = weights.init_params(cfg, seed=1, randomize_bn=True)
        nets = {m: Network(cfg, params=params, precision=m) for m in MODES}
        pyr = build_pyramid(x, cfg)
        inputs = {"pyramid": pyr, "features": f}
        out = {m: nets[m].inference(inputs) for m in MODES}  # (packs the one-plane images)
        torch.cuda.synchronize()
        agree = float((out["bf16"].argmax(-1) == out["bf16x3"].argmax(-1)).float().mean())
        for _ in range(5):  # preheat
            for m in MODES:
                nets[m].inference(inputs)
        torch.cuda.synchronize()
        best = {m: float("inf") for m in MODES}
        for _ in range(3):
            acc = {m: 0.0 for m in MODES}
            for _ in range(args.reps):
                for m in MODES:  # interleaved: both modes see the same clocks and the same neighbours on the card
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    nets[m].inference(inputs)
                    b.record()
                    b.synchronize()
                    acc[m] += a.elapsed_time(b)
            for m in MODES:
                best[m] = min(best[m], acc[m] / args.reps)
        for m in MODES:
            print("FORWARD %s n %d K %d %s: %.3f ms (best of 3 windows of %d)" % (name, n0, k_n, m, best[m], args.reps))
        print("FORWARD %s: bf16x3 / bf16 = %.3f, argmax agreement %.4f" % (name, best["bf16x3"] / best["bf16"], agree))
        stages = {}
        for m in MODES:
            ctx = nets[m].ctx
            ctx.timing_begin()
            nets[m].inference(inputs)
            for st, ms, launches in ctx.timing_end():
                stages.setdefault(st, {})[m] = (ms, launches)
        for st, v in stages.items():
            a, b = v.get("bf16x3", (0.0, 0)), v.get("bf16", (0.0, 0))
            print("STAGE %s %-12s bf16x3 %.4f ms (%d launches)  bf16 %.4f ms (%d launches)  ratio %.2f"
                  % (name, st, a[0], a[1], b[0], b[1], a[0] / b[0] if b[0] else 0.0))
        for m in MODES:
            nets[m].close()


if __name__ == "__main__":
    main()
