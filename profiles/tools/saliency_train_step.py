"""The channel attention, the spatial gate and softmax + weighted Dice on the GPU (point_unet_amd.saliency, csrc/saliency_train.hip), forward
and backward at the reference's shapes -- C345 [2, 16*40*40, 384] (96 hidden units), the gate [2, 64*160*160, 64], the loss
[2, 64*160*160, 2] -- and one training step of TrainableSaliencyNet at the reference's batch [2, 64, 160, 160, 1].

Stage `ops`: milliseconds from device events over 100 calls after 10 warm-up calls, best of 3 windows (saliency_grad_ops.py's method), each
op next to the SAME op composed from torch's elementwise and reduction ops on the same GPU (its backward by torch.autograd through that
composition, over 50 calls after 5, best of 2): the comparison, not the code under test.  With every time the bytes the pass must move
(each large tensor read or written once per pass the header names) and the share of the 8 TB/s HBM peak that makes.
Stage `step`: forward + backward + reference_optimizer step, the mean of 5 steps after 1 warm-up step; peak device memory; and the share of
the step's device time spent inside the six new entry points (device events around the wrappers' calls).

Stages `opbyop` and `onecall`: the same step at the same batch two ways in one session -- TrainableSaliencyNet under torch.autograd and
reference_optimizer as it stands, and SaliencyTrainer.step (ps_saliency_train_step, include/pointseg_saliency_step.h) -- each the mean
step over `--steps` steps between device events, 1 warm-up step, 3 windows; peak device memory (torch's allocator; for `onecall` also the
step's scratch); and, from one more step under the context's stage timing, the launches and device time per entry point.  The yardstick
of `onecall` is `opbyop` of the same session, never itself.

Stage `onecall_precision`: SaliencyTrainer.step at the same batch in four combinations of (forward, data gradient, weight gradient)
precision -- "fp32", "bf16x3", "bf16" and ("bf16x3", "bf16", "bf16") (include/pointseg_saliency_step_precision.h) -- in ONE process, their
windows interleaved (window 1 of each, then window 2 of each, ...) so that a drift of the device meets all four alike; the same window
discipline (device events, 1 warm-up step each, `--steps` steps per window, 3 windows).  The four trainers share one scratch (its size is
the same in every combination).  Per combination: the windows, the best one, the peak device memory and the first three losses.  Its
yardstick is `onecall` of the same session (name both in --stages): "fp32" runs the same code.  -> DIR/saliency_train_step_precision.json

Each stage runs in a child process under a time limit of its own; after a stage that fails or runs out of time nothing more starts.

usage (GPU box):
    python profiles/tools/saliency_train_step.py --out DIR [--stages ops,step,opbyop,onecall,onecall_precision] [--timeout 300]
                                                                                                         # -> DIR/saliency_train_step.json"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from saliency_grad_ops import best_ms  # noqa: E402  (the same directory: the method is shared, not restated)

PATCH = (64, 160, 160)
HBM_PEAK = 8.0e12  # bytes / s, MI355X


def _timed(torch, fn, nbytes):
    """An op of ours: the time, the bytes it must move and the share of the HBM peak that makes."""
    spread = {}
    ms = best_ms(torch, fn, warm=10, reps=100, runs=3, spread=spread, key="ms")
    return {"ms": round(ms, 4), "mbytes": round(nbytes / 1e6, 1), "hbm_share": round(nbytes / (ms * 1e-3) / HBM_PEAK, 3), "runs_ms": spread["ms"]}


def _measure(torch, name, res, ours_fwd, ours_bwd, torch_fwd, torch_leaves, dy, bytes_fwd, bytes_bwd):
    row = {"forward": _timed(torch, ours_fwd, bytes_fwd), "backward": _timed(torch, ours_bwd, bytes_bwd)}
    with torch.no_grad():
        row["torch_forward_ms"] = round(best_ms(torch, torch_fwd, warm=5, reps=50, runs=2), 4)
    y = torch_fwd()
    row["torch_backward_ms"] = round(best_ms(torch, lambda: torch.autograd.grad(y, torch_leaves, dy, retain_graph=True), warm=5, reps=50, runs=2), 4)
    row["at_or_under_torch"] = {"forward": row["forward"]["ms"] <= row["torch_forward_ms"], "backward": row["backward"]["ms"] <= row["torch_backward_ms"]}
    res[name] = row


def stage_ops(args):
    import torch
    import saliency_train_ref as tref
    from point_unet_amd import saliency as sal
    res = {}
    g = torch.Generator().manual_seed(1)
    rand = lambda *shape: torch.randn(shape, generator=g).cuda()
    v0, v2 = PATCH[0] * PATCH[1] * PATCH[2], PATCH[0] * PATCH[1] * PATCH[2] // 64

    # channel attention at C345: forward = the sum pass + the apply pass (x twice, y once); backward = dy and x, then dy and dx
    B, V, C, Ch = 2, v2, 384, 96
    x, dy = rand(B, V, C), rand(B, V, C)
    w1, b1, w2, b2 = rand(C, Ch) * (2.0 / C) ** 0.5, rand(Ch) * 0.1, rand(Ch, C) * (2.0 / Ch) ** 0.5, rand(C) * 0.1
    _, mean, hidden, scale = sal.channel_attention(x, w1, b1, w2, b2)
    leaves = [t.clone().requires_grad_() for t in (x, w1, b1, w2, b2)]
    n = B * V * C * 4
    _measure(torch, "channel_attention", res, lambda: sal.channel_attention(x, w1, b1, w2, b2),
             lambda: sal.channel_attention_backward(dy, x, mean, hidden, scale, w1, w2), lambda: tref.channel_attention(*leaves), leaves, dy, 3 * n, 4 * n)
    res["channel_attention"]["shape"] = (B, V, C, Ch)
    del x, dy, leaves
    torch.cuda.empty_cache()

    # the gate: forward reads f, a1, a2, a3 and writes y, sa; backward reads dy, f, sa and writes df, da
    B, V, C = 2, v0, 64
    a = [rand(B, V) for _ in range(3)]
    f, dy = rand(B, V, C), rand(B, V, C)
    _, sa = sal.spatial_gate(a[0], a[1], a[2], f)
    leaves = [t.clone().requires_grad_() for t in a + [f]]
    r = B * V * 4
    _measure(torch, "spatial_gate", res, lambda: sal.spatial_gate(a[0], a[1], a[2], f), lambda: sal.spatial_gate_backward(dy, f, sa),
             lambda: tref.spatial_gate(*leaves), leaves, dy, (2 * C + 4) * r, (3 * C + 2) * r)
    res["spatial_gate"]["shape"] = (B, V, C)
    del f, dy, leaves, a, sa
    torch.cuda.empty_cache()

    # the loss: forward reads logits, labels, weight; backward reads them again and writes dlogits
    B, V, C = 2, v0, 2
    logits, weight = rand(B, V, C), torch.rand((B, V), generator=g).cuda() + 0.2
    labels = torch.randint(0, C, (B, V), generator=g, dtype=torch.int32).cuda()
    _, sums = sal.softmax_dice_loss(logits, labels, weight)
    z = logits.clone().requires_grad_()
    _measure(torch, "softmax_dice_loss", res, lambda: sal.softmax_dice_loss(logits, labels, weight),
             lambda: sal.softmax_dice_loss_backward(logits, labels, weight, sums), lambda: tref.softmax_dice_loss(z, labels, weight), [z], None, (C + 2) * r,
             (2 * C + 2) * r)
    res["softmax_dice_loss"]["shape"] = (B, V, C)
    res["peak_device_memory_gb"] = round(torch.cuda.max_memory_allocated() / 1e9, 3)
    return res


def stage_step(args):
    import torch
    from point_unet_amd import saliency as sal
    spans = []

    def timed(name):
        inner = getattr(sal, name)

        def call(*a, **kw):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            out = inner(*a, **kw)
            e.record()
            spans.append((name, s, e))
            return out
        setattr(sal, name, call)

    for name in ("channel_attention", "channel_attention_backward", "spatial_gate", "spatial_gate_backward", "softmax_dice_loss", "softmax_dice_loss_backward"):
        timed(name)
    g = torch.Generator().manual_seed(2)
    shape = (2,) + PATCH
    net = sal.TrainableSaliencyNet(sal.init_params(1, 2, seed=0), 1, 2)
    opt = sal.reference_optimizer(net)
    x = torch.randn(shape + (1,), generator=g).cuda()
    labels = torch.randint(0, 2, shape, generator=g, dtype=torch.int32).cuda()
    weight = torch.rand(shape, generator=g).cuda() + 0.2

    def step():
        opt.zero_grad()
        loss = net.loss(x, labels, weight)
        loss.backward()
        opt.step()
        return loss.detach()

    losses = [float(step())]  # warm-up: the scratch buffers and torch's allocator grow here
    torch.cuda.synchronize()
    del spans[:]
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(args.steps):
        last = step()
    e.record()
    e.synchronize()
    losses.append(float(last))
    total = s.elapsed_time(e)
    per_op = {}
    for name, a, b in spans:
        per_op[name] = per_op.get(name, 0.0) + a.elapsed_time(b) / args.steps
    new_ops = sum(per_op.values())
    return {"batch": shape, "steps": args.steps, "step_ms": round(total / args.steps, 1), "new_ops_ms": {k: round(v, 3) for k, v in per_op.items()},
            "new_ops_share": round(new_ops / (total / args.steps), 4), "peak_device_memory_gb": round(torch.cuda.max_memory_allocated() / 1e9, 2),
            "losses_first_and_last": losses}


def _step_inputs(torch):
    g = torch.Generator().manual_seed(2)
    shape = (2,) + PATCH
    x = torch.randn(shape + (1,), generator=g).cuda()
    labels = torch.randint(0, 2, shape, generator=g, dtype=torch.int32).cuda()
    weight = torch.rand(shape, generator=g).cuda() + 0.2
    return shape, x, labels, weight


def _window(torch, step, steps):
    """(the mean step of one window of `steps` steps in ms, between device events; the steps' results)."""
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    got = [step() for _ in range(steps)]
    e.record()
    e.synchronize()
    return round(s.elapsed_time(e) / steps, 2), got


def _windows(torch, step, steps, windows=3):
    """(the mean step of each window in ms, the first and the last loss): 1 warm-up step, then `windows` windows of `steps` steps."""
    losses = [float(step())]  # warm-up: scratch buffers and torch's allocator grow here
    torch.cuda.synchronize()
    out = []
    for _ in range(windows):
        ms, got = _window(torch, step, steps)
        out.append(ms)
    losses.append(float(got[-1]))
    return out, losses


def _stage_rows(torch, step):
    """One more step under the context's stage timing: entry point -> (launches, device ms), and the totals."""
    from point_unet_amd import runtime
    ctx = runtime.default_context(0)
    ctx.use_torch_stream()
    ctx.timing_begin()
    step()
    torch.cuda.synchronize()
    rows = {}
    for name, ms, launches in ctx.timing_end():
        r = rows.setdefault(name, [0, 0.0])
        r[0], r[1] = r[0] + launches, r[1] + ms
    return {"entries": {k: [v[0], round(v[1], 3)] for k, v in rows.items()}, "launches": sum(v[0] for v in rows.values()),
            "device_ms": round(sum(v[1] for v in rows.values()), 2)}


def _step_result(torch, shape, args, windows, losses, rows):
    return {"batch": shape, "steps_per_window": args.steps, "windows_ms": windows, "step_ms": min(windows),
            "spread": round((max(windows) - min(windows)) / min(windows), 4), "peak_device_memory_gb": round(torch.cuda.max_memory_allocated() / 1e9, 2),
            "losses_first_and_last": losses, "stage_timing": rows}


def stage_opbyop(args):
    import torch
    from point_unet_amd import saliency as sal
    shape, x, labels, weight = _step_inputs(torch)
    net = sal.TrainableSaliencyNet(sal.init_params(1, 2, seed=0), 1, 2)
    opt = sal.reference_optimizer(net)

    def step():
        opt.zero_grad()
        loss = net.loss(x, labels, weight)
        loss.backward()
        opt.step()
        return loss.detach()

    windows, losses = _windows(torch, step, args.steps)
    res = _step_result(torch, shape, args, windows, losses, None)  # (the peak before the stage-timing step)
    res["stage_timing"] = _stage_rows(torch, step)  # (torch's own kernels -- cat, add, the optimiser -- are not entries and not counted)
    return res


def stage_onecall(args):
    import torch
    from point_unet_amd import saliency as sal
    shape, x, labels, weight = _step_inputs(torch)
    tr = sal.SaliencyTrainer(sal.init_params(1, 2, seed=0), 1, 2)
    step = lambda: tr.step(x, labels, weight, 0.01).clone()
    windows, losses = _windows(torch, step, args.steps)
    res = _step_result(torch, shape, args, windows, losses, None)
    res["scratch_gb"] = round(tr.scratch_bytes / 1e9, 2)
    res["stage_timing"] = _stage_rows(torch, step)
    return res


PRECISIONS = ("fp32", "bf16x3", "bf16", ("bf16x3", "bf16", "bf16"))


def stage_onecall_precision(args, windows=3):
    import torch
    from point_unet_amd import saliency as sal
    shape, x, labels, weight = _step_inputs(torch)
    params = sal.init_params(1, 2, seed=0)
    rows = []
    for precision in PRECISIONS:
        tr = sal.SaliencyTrainer(params, 1, 2, precision=precision)
        if rows:
            tr.scratch = rows[0]["trainer"].scratch  # (the same size in every combination; the first warm-up step made it)
        step = lambda tr=tr: tr.step(x, labels, weight, 0.01).clone()
        torch.cuda.reset_peak_memory_stats()
        losses = [step()]  # warm-up
        torch.cuda.synchronize()
        rows.append({"trainer": tr, "step": step, "losses": losses, "windows_ms": [], "peak": torch.cuda.max_memory_allocated()})
    for _ in range(max(windows, 3)):
        for row in rows:
            ms, got = _window(torch, row["step"], args.steps)
            row["windows_ms"].append(ms)
            row["losses"] += got
    res = {"batch": shape, "steps_per_window": args.steps, "scratch_gb": round(rows[0]["trainer"].scratch_bytes / 1e9, 2), "combinations": []}
    for precision, row in zip(PRECISIONS, rows):
        w = row["windows_ms"]
        res["combinations"].append({"precision": precision, "windows_ms": w, "step_ms": min(w), "spread": round((max(w) - min(w)) / min(w), 4),
                                    "peak_device_memory_gb": round(row["peak"] / 1e9, 2), "first_three_losses": [float(l) for l in row["losses"][:3]]})
    base = res["combinations"][0]["step_ms"]
    for row in res["combinations"]:
        row["fp32_over_this"] = round(base / row["step_ms"], 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--stages", default="ops,step")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=300, help="seconds each stage's child process may take")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        print("RESULT " + json.dumps({"ops": stage_ops, "step": stage_step, "opbyop": stage_opbyop, "onecall": stage_onecall,
                                      "onecall_precision": stage_onecall_precision}[args.child](args)))
        return 0
    res = {"patch": PATCH}
    for stage in args.stages.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", stage, "--steps", str(args.steps)]
        try:
            done = subprocess.run(cmd, timeout=args.timeout, stdout=subprocess.PIPE, text=True)
        except subprocess.TimeoutExpired:
            print("stage %s ran out of its %d s: nothing more is started" % (stage, args.timeout))
            return 1
        lines = [l for l in done.stdout.splitlines() if l.startswith("RESULT ")]
        if done.returncode != 0 or not lines:
            print("stage %s ended with status %d: nothing more is started" % (stage, done.returncode))
            return 1
        res[stage] = json.loads(lines[-1][7:])
    if "opbyop" in res and "onecall" in res:
        a, b = res["opbyop"], res["onecall"]
        res["onecall_vs_opbyop"] = {"step_ms_ratio": round(b["step_ms"] / a["step_ms"], 4), "spread_of_the_session": max(a["spread"], b["spread"]),
                                    "memory_gb": [b["peak_device_memory_gb"], a["peak_device_memory_gb"]]}
    if "onecall" in res and "onecall_precision" in res:
        a, b = res["onecall"], res["onecall_precision"]["combinations"][0]
        res["fp32_vs_onecall"] = {"step_ms": [b["step_ms"], a["step_ms"]], "step_ms_ratio": round(b["step_ms"] / a["step_ms"], 4),
                                  "spread_of_the_session": max(a["spread"], b["spread"])}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "saliency_train_step.json"), "w") as f:
            f.write(line + "\n")
        if "onecall_precision" in res:
            keep = {k: res[k] for k in ("patch", "onecall", "onecall_precision", "fp32_vs_onecall") if k in res}
            with open(os.path.join(args.out, "saliency_train_step_precision.json"), "w") as f:
                f.write(json.dumps(keep) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
