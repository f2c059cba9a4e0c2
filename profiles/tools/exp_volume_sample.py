"""ps_volume_sample (prepare.prepare_pancreas_volume / pancreas_mask) timed on the GPU, in one process, device events after warm-up, at the
reference's Pancreas size: a 512 x 512 x 240 int16 CT, ~40 000 positives, loops 8, N 180 000; the mask stage alone (probabilities ->
threshold -> one dilation -> OR truth); and the numpy restatement of the same call (tests/volume_sample_ref.py) on the host, one thread.
Per-kernel times come from two separate runs under `rocprofv3 --kernel-trace --stats --output-format csv`: --sample-only (the draw from a
ready u8 mask) and --mask-only (the mask stage: probabilities [n, 2] -> threshold -> one dilation -> OR truth -> out_mask).  --merge joins
their kernel_stats CSVs and the timing run's JSON with the algorithmic bytes of each pass (n = voxels, T = loops * N rows) and writes
volume_sample_exp.json, the file kept under profiles/:
    statistics 2 n | u8 mask -> work bytes 2 n | probabilities -> work bytes (4 C + 1) n | dilation round 2 n | work bytes + truth ->
    work bytes + out_mask 4 n | select round n | compaction n + 12 T | sort pass 8 T (histogram) + 24 T (scatter) | gather 55 T

usage (GPU box):
    python profiles/tools/exp_volume_sample.py --out DIR                                   # timings -> DIR/exp_volume_sample.json
    rocprofv3 --kernel-trace --stats --output-format csv -d A -o vs -- python profiles/tools/exp_volume_sample.py --sample-only
    rocprofv3 --kernel-trace --stats --output-format csv -d B -o vs -- python profiles/tools/exp_volume_sample.py --mask-only
    python profiles/tools/exp_volume_sample.py --merge DIR/exp_volume_sample.json --kernel-stats A/vs_kernel_stats.csv \
        --mask-kernel-stats B/vs_kernel_stats.csv --out DIR                                # -> DIR/volume_sample_exp.json"""
import argparse
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

SHAPE, LOOPS, N = (512, 512, 240), 8, 180000
HBM_ACHIEVABLE_GBS = 6300.0  # the rate a streaming kernel reaches on this part (float4 copy)


def inputs():
    rng = np.random.default_rng(0)
    vol = rng.integers(-1024, 1500, SHAPE, dtype=np.int16)
    g = np.stack(np.meshgrid(*[np.arange(s) for s in SHAPE], indexing="ij"), -1).astype(np.float32)
    r = np.array(SHAPE, np.float32) * np.float32(0.0545)
    blob = ((((g - np.array(SHAPE, np.float32) / 2) / r) ** 2).sum(-1) < 1.0).astype(np.uint8)
    return vol, blob


def algorithmic_bytes(n, loops, n_rows, probs_c=2):
    """Bytes each pass has to move, by the kernel's name as the profiler prints it.  The first match wins."""
    T = loops * n_rows
    return [("vs_stats_i16_kernel", 2 * n), ("vs_mask_kernel<0, true>", 2 * n), ("vs_mask_kernel<1, false>", (4 * probs_c + 1) * n),
            ("vs_mask_kernel<2, true>", 4 * n), ("vs_dilate_kernel", 2 * n), ("vs_hist_kernel", n), ("vs_compact_kernel", n + 12 * T),
            ("radix_hist_kernel", 8 * T), ("radix_scatter_kernel", 24 * T), ("vs_gather_kernel", T * (7 + 48))]


def event_ms(fn, reps):
    import torch
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / reps


def kernel_table(path, n, loops, n_rows):
    """rocprofv3's kernel_stats CSV -> per-kernel average time, algorithmic GB/s and share of the achievable HBM rate."""
    alg = algorithmic_bytes(n, loops, n_rows)
    rows = []
    for r in csv.DictReader(open(path)):
        name = r.get("Name") or r.get("KernelName") or ""
        calls = int(r.get("Calls") or r.get("Count") or 0)
        avg_us = float(r.get("AverageNs") or r.get("Average") or 0) / 1e3
        if "ps::" not in name:
            continue
        nbytes = next((b for k, b in alg if k in name), None)
        row = {"kernel": name[:80], "calls": calls, "avg_us": round(avg_us, 2)}
        if nbytes and avg_us > 0:
            gbs = nbytes / (avg_us * 1e-6) / 1e9
            row.update(algorithmic_bytes=nbytes, gb_per_s=round(gbs, 1), share_of_achievable_hbm=round(gbs / HBM_ACHIEVABLE_GBS, 3))
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sample-only", action="store_true")
    ap.add_argument("--mask-only", action="store_true")
    ap.add_argument("--merge", default=None, help="the timing run's JSON")
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--mask-kernel-stats", default=None)
    args = ap.parse_args()
    n = int(np.prod(SHAPE))
    if args.merge:
        res = json.loads(open(args.merge).read())
        res["hbm_achievable_gb_per_s"] = HBM_ACHIEVABLE_GBS
        if args.kernel_stats:
            res["kernels_draw"] = kernel_table(args.kernel_stats, n, LOOPS, N)
        if args.mask_kernel_stats:
            res["kernels_mask_stage"] = kernel_table(args.mask_kernel_stats, n, LOOPS, N)
        line = json.dumps(res)
        print(line)
        if args.out:
            os.makedirs(args.out, exist_ok=True)
            with open(os.path.join(args.out, "volume_sample_exp.json"), "w") as f:
                f.write(line + "\n")
        return
    import torch
    from point_unet_amd.prepare import pancreas_mask, prepare_pancreas_volume
    vol, blob = inputs()
    d_vol, d_blob = torch.from_numpy(vol).cuda(), torch.from_numpy(blob).cuda()
    seed = [0]

    def draw():
        seed[0] += 1
        return prepare_pancreas_volume(d_vol, mask=d_blob, n_point=N, loops=LOOPS, seed=seed[0])

    def mask_inputs():
        return torch.stack([1 - d_blob.float(), d_blob.float()], -1).contiguous()

    if args.mask_only:  # (the rocprofv3 run of the mask stage)
        probs = mask_inputs()
        for _ in range(23):
            pancreas_mask(probs=probs, threshold=0.9, dilate=1, truth=d_blob)
        torch.cuda.synchronize()
        print(json.dumps({"mask_only": True}))
        return
    if args.sample_only:  # (the rocprofv3 run of the draw)
        for _ in range(3):
            draw()
        for _ in range(20):
            draw()
        torch.cuda.synchronize()
        print(json.dumps({"sample_only": True}))
        return
    res = {"shape": SHAPE, "loops": LOOPS, "N": N, "positives": int(blob.sum()), "algorithmic_bytes": dict(algorithmic_bytes(n, LOOPS, N))}
    for _ in range(3):
        draw()
    torch.cuda.synchronize()
    runs = [event_ms(draw, 10) for _ in range(3)]
    res["device_call_ms"] = {"ms": round(min(runs), 4), "ms_runs": [round(r, 4) for r in runs]}
    probs = mask_inputs()
    mask_fn = lambda: pancreas_mask(probs=probs, threshold=0.9, dilate=1, truth=d_blob)  # noqa: E731
    for _ in range(3):
        mask_fn()
    torch.cuda.synchronize()
    runs = [event_ms(mask_fn, 10) for _ in range(3)]
    res["device_mask_stage_ms"] = {"ms": round(min(runs), 4), "ms_runs": [round(r, 4) for r in runs]}
    del probs
    import volume_sample_ref as ref
    t0 = time.perf_counter()
    ref.sample(vol, blob, N, LOOPS, 1)
    res["host_numpy_restatement_s"] = round(time.perf_counter() - t0, 2)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "exp_volume_sample.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
