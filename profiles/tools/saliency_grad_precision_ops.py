"""The two convolution gradients at the three precisions of include/pointseg_saliency_train_precision.h
(point_unet_amd.saliency.conv3d_backward(precision=)), on saliency_grad_ops.py's five layers at the reference's [1, 64, 160, 160] patch,
with that tool's method: milliseconds from device events over 10 calls per window, 3 windows after 3 warm-up calls.  The three modes run
INTERLEAVED in one process -- window 1 of fp32, of bf16x3, of bf16, then window 2 of each, ... -- so the fp32 number every ratio is taken to
is this process's own, under the same clocks.  Per layer, gradient and mode: every window, the best, and the spread (slowest - fastest
window); per reduced mode the speed-up over fp32 and whether it exceeds both spreads (DESIGN.md 4.16's routing rule for "bf16x3").
Also the largest difference of each reduced mode's result from the fp32 one.  Behind the five layers, FORMS: one layer of the network for
each further kernel form the two launchers choose (narrow column tiles, the 4-byte fetch of dy, the 64-row forms of the deep levels, the
stride-2 gather), timed the same way.

The work runs in a child process under a time limit of its own, so a hang ends there.

usage (GPU box):
    python profiles/tools/saliency_grad_precision_ops.py --out DIR [--timeout 420]        # -> DIR/saliency_grad_precision_ops.json"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from saliency_grad_ops import LAYERS, PATCH, event_ms  # noqa: E402

MODES = ("fp32", "bf16x3", "bf16")
# name, kernel [kd, kh, kw, cin, cout], source extents, up-sampling, stride
FORMS = (("init_conv", (3, 3, 3, 1, 16), PATCH, 1, 1), ("down0_conv_0", (3, 3, 3, 16, 16), PATCH, 1, 1), ("stride2conv0", (3, 3, 3, 16, 32), PATCH, 1, 2),
         ("spatial_attention_1_conv2", (9, 1, 1, 32, 1), PATCH, 1, 1), ("final", (3, 3, 3, 128, 2), PATCH, 1, 1),
         ("down2_conv_0", (3, 3, 3, 64, 64), (16, 40, 40), 1, 1), ("stride2conv3", (3, 3, 3, 128, 256), (8, 20, 20), 1, 2),
         ("down4_conv_0", (3, 3, 3, 256, 256), (4, 10, 10), 1, 1), ("C5_cfe_cfe3_dilation", (3, 3, 3, 256, 32), (4, 10, 10), 1, 1))
WARM, REPS, WINDOWS = 3, 10, 3


def child(args):
    import torch
    from point_unet_amd import saliency as sal
    res = {"patch": PATCH, "modes": MODES, "reps": REPS, "windows": WINDOWS, "convs": {}, "forms": {}}
    for name, shape, src, up, stride in tuple((n, k, tuple(p // up for p in PATCH), up, 1) for n, k, up in LAYERS) + FORMS:
        out_ext = tuple(-(-n * up // stride) for n in src)
        g = torch.Generator().manual_seed(len(name))
        x = torch.randn((1,) + src + (shape[3],), generator=g).cuda()
        w = (torch.randn(shape, generator=g) * (2.0 / (shape[0] * shape[1] * shape[2] * shape[3])) ** 0.5).cuda()
        dy = torch.randn((1,) + out_ext + (shape[4],), generator=g).cuda()
        macs = out_ext[0] * out_ext[1] * out_ext[2] * shape[0] * shape[1] * shape[2] * shape[3] * shape[4]
        row = {"kernel": shape, "source": src, "up": up, "stride": stride, "gmac": round(macs / 1e9, 2)}
        for grad, need in (("bwd_data", ("x",)), ("bwd_weight", ("w", "bias"))):
            calls = {m: (lambda m=m: sal.conv3d_backward(dy, x, w, stride=stride, up=up, need=need, precision=m)) for m in MODES}
            out = {m: calls[m]() for m in MODES}
            for m in MODES:
                for _ in range(WARM):
                    calls[m]()
            torch.cuda.synchronize()
            ms = {m: [] for m in MODES}
            for _ in range(WINDOWS):
                for m in MODES:
                    ms[m].append(event_ms(torch, calls[m], REPS))
            r = {}
            for m in MODES:
                best = min(ms[m])
                r[m] = {"windows_ms": [round(v, 3) for v in ms[m]], "best_ms": round(best, 3), "spread_ms": round(max(ms[m]) - best, 3),
                        "tflops": round(2 * macs / (best * 1e-3) / 1e12, 2)}
            for m in MODES[1:]:
                gain = r["fp32"]["best_ms"] - r[m]["best_ms"]
                r[m]["speedup_over_fp32"] = round(r["fp32"]["best_ms"] / r[m]["best_ms"], 2)
                r[m]["faster_by_more_than_the_spread"] = bool(gain > max(r["fp32"]["spread_ms"], r[m]["spread_ms"]))
                r[m]["max_abs_diff_to_fp32"] = {n: float((out[m][n] - out["fp32"][n]).abs().max().item()) for n in need}
            r["max_abs"] = {n: float(out["fp32"][n].abs().max().item()) for n in need}
            row[grad] = r
            del out
        res["forms" if (name, shape, src, up, stride) in FORMS else "convs"][name] = row
        del x, w, dy
        torch.cuda.empty_cache()
    res["peak_device_memory_gb"] = round(torch.cuda.max_memory_allocated() / 1e9, 3)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "saliency_grad_precision_ops.json"), "w") as f:
            f.write(line + "\n")
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--timeout", type=int, default=420, help="seconds the child process may take")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        sys.exit(child(args))
    cmd = [sys.executable, os.path.abspath(__file__), "--child"] + (["--out", args.out] if args.out else [])
    sys.exit(subprocess.run(cmd, timeout=args.timeout).returncode)


if __name__ == "__main__":
    main()
