"""The gradients of the saliency network's five costliest convolutions and of one full-resolution instance norm + ReLU on the GPU
(point_unet_amd.saliency.conv3d_backward / instance_norm_relu_backward, csrc/conv3d_train.hip), at the reference's [1, 64, 160, 160]
patch: milliseconds from device events over 10 calls after 3 warm-up calls, best of 3 windows (torch: 3 calls after 2, best of 2), for
ps_conv3d_bwd_data, ps_conv3d_bwd_weight and -- re-measured in the same run -- the forward ps_conv3d, each gradient also as a ratio to
that forward (a gradient is the forward's MAC count), next to
torch.nn.grad.conv3d_input / conv3d_weight on the same tensors on the same GPU (channels first; the SAME padding of these odd kernels
at stride 1 is symmetric, so torch takes it as `padding=`; an up-sampled input is materialised beforehand, outside the timed region, and
torch's data gradient then stops at the up-sampled tensor).  The method is profiles/tools/saliency_patch.py's.

The work runs in a child process under a time limit of its own, so a hang ends there.

usage (GPU box):
    python profiles/tools/saliency_grad_ops.py --out DIR [--timeout 420] [--no-torch]        # -> DIR/saliency_grad_ops.json"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PATCH = (64, 160, 160)
# DESIGN.md 4.9's second table: name, kernel [kd, kh, kw, cin, cout], up-sampling inside the fetch
LAYERS = (("C12_conv", (3, 3, 3, 128, 64), 1), ("spatial_attention_1_conv1", (1, 9, 9, 64, 32), 1), ("spatial_attention_2_conv1", (9, 1, 9, 64, 32), 1),
          ("spatial_attention_3_conv1", (9, 9, 1, 64, 32), 1), ("up_conv1_C345_up4", (3, 3, 3, 64, 64), 4))


def event_ms(torch, fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / reps


def best_ms(torch, fn, warm=3, reps=10, runs=3, spread=None, key=None):
    """The best of `runs` windows of `reps` calls after `warm` calls; every window's time goes to spread[key]."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = [event_ms(torch, fn, reps) for _ in range(runs)]
    if spread is not None:
        spread[key] = [round(m, 3) for m in ms]
    return min(ms)


def child(args):
    import torch
    import saliency_ref as ref
    from point_unet_amd import saliency as sal
    res = {"patch": PATCH, "convs": {}}
    v0 = PATCH[0] * PATCH[1] * PATCH[2]
    for name, shape, up in LAYERS:
        src = tuple(p // up for p in PATCH)
        g = torch.Generator().manual_seed(len(name))
        x = torch.randn((1,) + src + (shape[3],), generator=g).cuda()
        w = (torch.randn(shape, generator=g) * (2.0 / (shape[0] * shape[1] * shape[2] * shape[3])) ** 0.5).cuda()
        dy = torch.randn((1,) + PATCH + (shape[4],), generator=g).cuda()
        macs = v0 * shape[0] * shape[1] * shape[2] * shape[3] * shape[4]
        runs = {}
        fwd = best_ms(torch, lambda: sal.conv3d(x, w, up=up), spread=runs, key="forward")
        data = best_ms(torch, lambda: sal.conv3d_backward(dy, x, w, up=up, need=("x",)), spread=runs, key="bwd_data")
        weight = best_ms(torch, lambda: sal.conv3d_backward(dy, x, w, up=up, need=("w", "bias")), spread=runs, key="bwd_weight")
        row = {"kernel": shape, "up": up, "gmac": round(macs / 1e9, 2), "forward_ms": round(fwd, 3), "bwd_data_ms": round(data, 3),
               "bwd_weight_ms": round(weight, 3), "bwd_data_over_forward": round(data / fwd, 2), "bwd_weight_over_forward": round(weight / fwd, 2),
               "bwd_data_tflops": round(2 * macs / (data * 1e-3) / 1e12, 2), "bwd_weight_tflops": round(2 * macs / (weight * 1e-3) / 1e12, 2), "runs_ms": runs}
        if not args.no_torch:
            ours = sal.conv3d_backward(dy, x, w, up=up, need=("x", "w"))
            pad = tuple(k // 2 for k in shape[:3])
            xt = ref.upsample(x, up).permute(0, 4, 1, 2, 3).contiguous()
            wt = w.permute(4, 3, 0, 1, 2).contiguous()
            dyt = dy.permute(0, 4, 1, 2, 3).contiguous()
            t_data = best_ms(torch, lambda: torch.nn.grad.conv3d_input(xt.shape, wt, dyt, padding=pad), warm=2, reps=3, runs=2)
            t_weight = best_ms(torch, lambda: torch.nn.grad.conv3d_weight(xt, wt.shape, dyt, padding=pad), warm=2, reps=3, runs=2)
            row.update(torch_conv3d_input_ms=round(t_data, 3), torch_conv3d_weight_ms=round(t_weight, 3))
            tw = torch.nn.grad.conv3d_weight(xt, wt.shape, dyt, padding=pad).permute(2, 3, 4, 1, 0)
            row["dw_max_abs_diff_to_torch"] = float((tw - ours["w"]).abs().max().item())
            row["dw_max_abs"] = float(tw.abs().max().item())
            if up == 1:
                tx = torch.nn.grad.conv3d_input(xt.shape, wt, dyt, padding=pad).permute(0, 2, 3, 4, 1)
                row["dx_max_abs_diff_to_torch"] = float((tx - ours["x"]).abs().max().item())
                row["dx_max_abs"] = float(tx.abs().max().item())
                del tx
            del xt, wt, dyt, tw, ours
        res["convs"][name] = row
        del x, w, dy
        torch.cuda.empty_cache()

    # the norm's gradient on one full-resolution 64-channel activation
    g = torch.Generator().manual_seed(7)
    x = torch.randn((1, v0, 64), generator=g).cuda()
    dy = torch.randn((1, v0, 64), generator=g).cuda()
    gamma, beta = (torch.rand(64, generator=g) + 0.5).cuda(), torch.zeros(64).cuda()
    y = sal.instance_norm_relu(x, gamma, beta)
    res["instance_norm_relu"] = {"shape": (1, v0, 64), "forward_ms": round(best_ms(torch, lambda: sal.instance_norm_relu(x, gamma, beta)), 3),
                                 "bwd_ms": round(best_ms(torch, lambda: sal.instance_norm_relu_backward(dy, x, y, gamma)), 3)}
    res["peak_device_memory_gb"] = round(torch.cuda.max_memory_allocated() / 1e9, 3)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "saliency_grad_ops.json"), "w") as f:
            f.write(line + "\n")
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--timeout", type=int, default=420, help="seconds the child process may take")
    ap.add_argument("--no-torch", action="store_true", help="skip torch.nn.grad.conv3d_input / conv3d_weight")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        sys.exit(child(args))
    cmd = [sys.executable, os.path.abspath(__file__), "--child"] + (["--out", args.out] if args.out else []) + (["--no-torch"] if args.no_torch else [])
    sys.exit(subprocess.run(cmd, timeout=args.timeout).returncode)


if __name__ == "__main__":
    main()
