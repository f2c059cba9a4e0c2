"""One full-size patch of the saliency attention network (point_unet_amd.saliency, csrc/conv3d.hip, csrc/saliency.hip) on the GPU: the
reference's [64, 160, 160] Pancreas patch, one input channel, two classes.  Checks -- every result finite, the probabilities sum to 1, two
runs byte-equal, the scratch untouched behind the size the first call reported (a guard band behind it keeps its pattern) -- then
milliseconds per patch from device events after a warm-up, and the five costliest convolutions on their own next to
torch.nn.functional.conv3d on the same tensors (channels first, the input padded and up-sampled beforehand, neither inside the timed
region).  MACs per layer are counted from the layer table and the shapes.

The work runs in a child process under a time limit of its own, so a hang ends there.

--precision compares the arithmetic modes of include/pointseg_saliency_precision.h instead: the whole patch and the same five convolutions
in "fp32", "bf16x3" and "bf16", in ONE process, the modes interleaved round by round (a drift of the clock or the device hits all three
alike), device events after a warm-up, best-of and the spread of the rounds recorded; the baseline is the fp32 mode of the same session.

usage (GPU box):
    python profiles/tools/saliency_patch.py --out DIR [--timeout 420] [--no-torch]        # -> DIR/saliency_patch.json
    python profiles/tools/saliency_patch.py --precision [--out DIR]                       # -> DIR/saliency_patch_precision.json (DIR: profiles/)"""
import argparse
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PATCH = (64, 160, 160)
GUARD = 1 << 20


def level_of(name):
    """How often the layer's OUTPUT extents are halved."""
    if name.startswith("stride2conv"):
        return int(name[-1]) + 1
    if name.startswith("down"):
        return int(name[4])
    if name.startswith("C2_conv"):
        return 1
    if name.startswith(("C3_cfe", "up_conv1_C4_cfe", "up_conv1_C5_cfe", "C345_conv")):
        return 2
    if name.startswith("C4_cfe"):
        return 3
    if name.startswith("C5_cfe"):
        return 4
    return 0


def mac_table(sal, in_channels, classes, patch):
    v0 = patch[0] * patch[1] * patch[2]
    rows = []
    for name, shape, _, _ in sal.layer_table(in_channels, classes):
        if len(shape) != 5:
            continue
        taps = shape[0] * shape[1] * shape[2]
        rows.append((name, shape, (v0 >> (3 * level_of(name))) * taps * shape[3] * shape[4]))
    return rows


def event_ms(torch, fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / reps


def interleaved_ms(torch, fns, rounds, reps):
    """fns: mode -> callable.  `rounds` rounds, each timing every mode once (reps calls between two events), in the dict's order.
    Returns mode -> {best, median, worst} in ms."""
    for fn in fns.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    runs = {m: [] for m in fns}
    for _ in range(rounds):
        for m, fn in fns.items():
            runs[m].append(event_ms(torch, fn, reps))
    return {m: {"best": round(min(r), 3), "median": round(sorted(r)[len(r) // 2], 3), "worst": round(max(r), 3)} for m, r in runs.items()}


def child_precision(args):
    import numpy as np
    import torch
    from point_unet_amd import saliency as sal
    modes = ("fp32", "bf16x3", "bf16")
    res = {"patch": PATCH, "in_channels": 1, "num_classes": 2, "modes": modes,
           "method": "one process, modes interleaved per round, device events around 3 calls, 2 warm-up calls per mode; ms: best / median / worst of the rounds"}
    params = sal.init_params(1, 2, seed=0)
    nets = {m: sal.SaliencyNet(params, 1, 2, precision=m) for m in modes}
    x = torch.from_numpy(np.random.default_rng(1).standard_normal((1,) + PATCH + (1,)).astype(np.float32)).cuda()
    ok = True
    probs = {}
    for m in modes:
        p = nets[m].probs(x)
        good = bool(torch.isfinite(p).all().item()) and float((p.sum(-1) - 1.0).abs().max().item()) <= 1e-6 and torch.equal(nets[m].probs(x), p)
        ok = ok and good
        probs[m] = p
    res["checks_pass"] = ok
    res["max_abs_prob_diff_to_fp32"] = {m: float((probs[m] - probs["fp32"]).abs().max().item()) for m in modes[1:]}
    del probs
    rows = mac_table(sal, 1, 2, PATCH)
    total = sum(r[2] for r in rows)
    res["gmac_total"] = round(total / 1e9, 1)
    res["ms_per_patch"] = interleaved_ms(torch, {m: (lambda n=nets[m]: n.probs(x)) for m in modes}, 7, 3)
    res["convs"] = {}
    for name, shape, macs in sorted(rows, key=lambda r: -r[2])[:5]:
        up = 4 if "up4" in name else (2 if "up2" in name else 1)
        src = tuple(p // up for p in PATCH)
        g = torch.Generator().manual_seed(len(name))
        xi = torch.randn((1,) + src + (shape[3],), generator=g).cuda()
        w = (torch.randn(shape, generator=g) * (2.0 / (shape[0] * shape[1] * shape[2] * shape[3])) ** 0.5).cuda()
        ms = interleaved_ms(torch, {m: (lambda m=m: sal.conv3d(xi, w, up=up, precision=m)) for m in modes}, 5, 3)
        res["convs"][name] = {"kernel": shape, "up": up, "gmac": round(macs / 1e9, 2), "ms": ms,
                              "tflops_best": {m: round(2 * macs / (ms[m]["best"] * 1e-3) / 1e12, 1) for m in modes}}
        del xi, w
    res["ok"] = bool(ok)
    line = json.dumps(res)
    print(line)
    out = args.out or os.path.join(ROOT, "profiles")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "saliency_patch_precision.json"), "w") as f:
        f.write(line + "\n")
    return 0 if ok else 1


def child(args):
    if args.precision:
        return child_precision(args)
    import numpy as np
    import torch
    import torch.nn.functional as F
    import saliency_ref as ref
    from point_unet_amd import _lib, runtime
    from point_unet_amd import saliency as sal
    res = {"patch": PATCH, "in_channels": 1, "num_classes": 2}
    params = sal.init_params(1, 2, seed=0)
    net = sal.SaliencyNet(params, 1, 2)
    x = torch.from_numpy(np.random.default_rng(1).standard_normal((1,) + PATCH + (1,)).astype(np.float32)).cuda()

    # the scratch behind a guard band
    ctx = runtime.default_context(0)
    ctx.use_torch_stream()
    fn = _lib.lib().ps_saliency_forward
    need = ctypes.c_int64(0)
    n = net.weights.numel()
    _lib.check(fn(ctx.handle, None, 1, *PATCH, 1, 2, None, n, None, None, None, None, ctypes.byref(need)))
    buf = torch.empty(need.value + GUARD, dtype=torch.uint8, device="cuda")
    buf[need.value:] = 0xA5
    logits = torch.empty((1,) + PATCH + (2,), dtype=torch.float32, device="cuda")
    probs = torch.empty_like(logits)
    _lib.check(fn(ctx.handle, runtime.ptr(x), 1, *PATCH, 1, 2, runtime.ptr(net.weights), n, runtime.ptr(logits), runtime.ptr(probs), None, runtime.ptr(buf),
                  ctypes.byref(need)))
    torch.cuda.synchronize()
    res["scratch_bytes"] = need.value
    res["scratch_guard_intact"] = bool((buf[need.value:] == 0xA5).all().item())
    del buf
    res["all_finite"] = bool(torch.isfinite(logits).all().item() and torch.isfinite(probs).all().item())
    res["max_abs_logit"] = float(logits.abs().max().item())
    res["probs_sum_max_dev"] = float((probs.sum(-1) - 1.0).abs().max().item())
    again = net.probs(x)
    res["two_runs_byte_equal"] = bool(torch.equal(again, probs) and torch.equal(net.probs(x), again))
    ok = res["scratch_guard_intact"] and res["all_finite"] and res["probs_sum_max_dev"] <= 1e-6 and res["two_runs_byte_equal"]

    # the patch
    for _ in range(3):
        net.probs(x)
    torch.cuda.synchronize()
    runs = [event_ms(torch, lambda: net.probs(x), 5) for _ in range(3)]
    rows = mac_table(sal, 1, 2, PATCH)
    total = sum(r[2] for r in rows)
    res["ms_per_patch"] = round(min(runs), 3)
    res["ms_per_patch_runs"] = [round(r, 3) for r in runs]
    res["gmac_total"] = round(total / 1e9, 1)
    res["tflops_whole_patch"] = round(2 * total / (min(runs) * 1e-3) / 1e12, 2)
    res["gmac_per_layer"] = {r[0]: round(r[2] / 1e9, 2) for r in rows}

    # the five costliest convolutions on their own
    res["convs"] = {}
    for name, shape, macs in sorted(rows, key=lambda r: -r[2])[:5]:
        up = 4 if "up4" in name else (2 if "up2" in name else 1)
        src = tuple(p // up for p in PATCH)
        g = torch.Generator().manual_seed(len(name))
        xi = torch.randn((1,) + src + (shape[3],), generator=g).cuda()
        w = (torch.randn(shape, generator=g) * (2.0 / (shape[0] * shape[1] * shape[2] * shape[3])) ** 0.5).cuda()
        ours = lambda: sal.conv3d(xi, w, up=up)  # noqa: E731
        y = ours()
        for _ in range(2):
            ours()
        torch.cuda.synchronize()
        ms = min(event_ms(torch, ours, 3) for _ in range(2))
        row = {"kernel": shape, "up": up, "gmac": round(macs / 1e9, 2), "ms": round(ms, 3), "tflops": round(2 * macs / (ms * 1e-3) / 1e12, 2)}
        if not args.no_torch:
            pads = [ref.same_padding(PATCH[a], shape[a]) for a in range(3)]
            xt = F.pad(ref.upsample(xi, up).permute(0, 4, 1, 2, 3), (pads[2][1], pads[2][2], pads[1][1], pads[1][2], pads[0][1], pads[0][2])).contiguous()
            wt = w.permute(4, 3, 0, 1, 2).contiguous()
            theirs = lambda: F.conv3d(xt, wt)  # noqa: E731
            yt = theirs()
            for _ in range(2):
                theirs()
            torch.cuda.synchronize()
            tms = min(event_ms(torch, theirs, 3) for _ in range(2))
            row.update(torch_ms=round(tms, 3), torch_tflops=round(2 * macs / (tms * 1e-3) / 1e12, 2),
                       max_abs_diff_to_torch=float((yt.permute(0, 2, 3, 4, 1) - y).abs().max().item()))
            del xt, yt
        res["convs"][name] = row
        del xi, y
    res["peak_device_memory_gb"] = round(torch.cuda.max_memory_allocated() / 1e9, 3)
    res["ok"] = bool(ok)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "saliency_patch.json"), "w") as f:
            f.write(line + "\n")
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--timeout", type=int, default=420, help="seconds the child process may take")
    ap.add_argument("--no-torch", action="store_true", help="skip the torch.nn.functional.conv3d comparison")
    ap.add_argument("--precision", action="store_true", help="compare the fp32, bf16x3 and bf16 modes -> saliency_patch_precision.json")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        sys.exit(child(args))
    cmd = [sys.executable, os.path.abspath(__file__), "--child"] + (["--out", args.out] if args.out else []) + (["--no-torch"] if args.no_torch else []) \
        + (["--precision"] if args.precision else [])
    sys.exit(subprocess.run(cmd, timeout=args.timeout).returncode)


if __name__ == "__main__":
    main()
