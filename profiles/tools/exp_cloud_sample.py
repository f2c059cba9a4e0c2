"""Device batch sampling (dataset.CloudBank / ps_cloud_sample) timed on the GPU, in one process, device events after warm-up:
  (1) sample() for B = 1 and 8 at N = 180 000 and 365 000 from synthetic 1.5 M-point clouds (~90 k positives each);
  (2) the host sampler (dataset.sample_brats_cloud, numpy, one thread) on one such cloud, for comparison;
  (3) a 20-step fp32 B = 8 x 180 000 training loop fed a FRESH bank batch every step through PyramidPrefetcher, alternated with the same
      loop on ONE resident batch (bench.py --mode train's setting).
Per-kernel times come from a separate run under `rocprofv3 --kernel-trace --stats` with --sample-only (sample() alone, B = 8, N = 180 000).

usage (GPU box): python profiles/tools/exp_cloud_sample.py [--out DIR] [--sample-only]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

N_CLOUD, N_POS, GRID = 1500000, 90000, (240, 240, 155)


def synthetic_cloud(seed):
    """1.5 M distinct voxels of the BraTS grid (xyz = ijk / grid), four modalities, 90 000 tumour points (labels 1..3)."""
    rng = np.random.default_rng(seed)
    g = np.asarray(GRID)
    flat = rng.choice(int(np.prod(g)), N_CLOUD, replace=False)
    ijk = np.stack([flat % g[0], (flat // g[0]) % g[1], flat // (g[0] * g[1])], 1)
    xyz = (ijk / g).astype(np.float32)
    mods = rng.standard_normal((N_CLOUD, 4)).astype(np.float32)
    labels = np.zeros(N_CLOUD, np.int32)
    labels[rng.choice(N_CLOUD, N_POS, replace=False)] = rng.integers(1, 4, N_POS)
    return xyz, mods, labels


def event_ms(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sample-only", action="store_true")
    ap.add_argument("--steps", type=int, default=20)
    args = ap.parse_args()
    from point_unet_amd.dataset import CloudBank, sample_brats_cloud
    bank = CloudBank(channels=4)
    clouds = []
    for c in range(8):
        xyz, mods, labels = synthetic_cloud(c)
        bank.add(xyz, mods, labels)
        if c == 0:
            clouds.append((xyz, mods, labels))
    torch.cuda.synchronize()
    res = {"clouds": 8, "points_per_cloud": N_CLOUD, "positives_per_cloud": [bank.positives(c) for c in range(8)]}
    seed = [0]

    def draw(B, N):
        seed[0] += 1
        return bank.sample(list(range(B)), N, seed[0])

    if args.sample_only:  # (the rocprofv3 run: warm-up, then 50 draws of the B = 8 x 180 000 batch)
        for _ in range(5):
            draw(8, 180000)
        for _ in range(50):
            draw(8, 180000)
        bank.synchronize()
        print(json.dumps({"sample_only": True}))
        return
    # (1) device sampling
    samp = {}
    for B in (1, 8):
        for N in (180000, 365000):
            for _ in range(5):
                draw(B, N)
            torch.cuda.synchronize()
            runs = [event_ms(lambda: draw(B, N), 20) for _ in range(3)]
            samp["B%d_N%d" % (B, N)] = {"ms": round(min(runs), 4), "ms_runs": [round(r, 4) for r in runs]}
    bank.synchronize()
    res["device_sample"] = samp
    # (2) the host sampler, one cloud, one thread
    xyz, mods, labels = clouds[0]
    dt = [("x", "f4"), ("y", "f4"), ("z", "f4"), ("t1ce", "f4"), ("t1", "f4"), ("flair", "f4"), ("t2", "f4"), ("class", "i4")]
    data = np.zeros(N_CLOUD, dtype=dt)
    for k, name in enumerate(("x", "y", "z")):
        data[name] = xyz[:, k]
    for k, name in enumerate(("t1ce", "t1", "flair", "t2")):
        data[name] = mods[:, k]
    data["class"] = labels
    host = {}
    for N in (180000, 365000):
        rng = np.random.default_rng(0)
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            sample_brats_cloud(data, N, rng)
            ts.append(1e3 * (time.perf_counter() - t0))
        host["N%d" % N] = {"ms_per_cloud": round(min(ts), 2), "ms_runs": [round(t, 2) for t in ts]}
    res["host_sample"] = host
    # (3) the training loop: fresh bank batches vs one resident batch, alternated
    from point_unet_amd import weights
    from point_unet_amd.helper_tool import ConfigBraTS as cfg
    from point_unet_amd.pipeline import PyramidPrefetcher
    from point_unet_amd.train import Trainer
    B, N = 8, 180000
    tr = Trainer(cfg, params=weights.init_params(cfg, seed=2), keep_prob=0.5, mlp_dtype="fp32")
    pre = PyramidPrefetcher(cfg)
    resident = draw(B, N)

    def loop(fresh, steps):
        cur = draw(B, N) if fresh else resident
        pre.submit(cur.xyz)
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for k in range(steps):
            nxt = (draw(B, N) if fresh else resident) if k + 1 < steps else None
            if nxt is not None:
                pre.submit(nxt.xyz)
            pyr, slot = pre.next()
            loss = tr.train_step(pyr, cur.features, cur.labels)
            pre.release(slot)
            cur = nxt
        e.record()
        e.synchronize()
        pre.synchronize()
        assert bool(torch.isfinite(loss).all())
        return s.elapsed_time(e) / steps

    loop(True, 3)
    loop(False, 3)
    runs = {"fresh": [], "resident": []}
    for _ in range(3):
        runs["resident"].append(round(loop(False, args.steps), 3))
        runs["fresh"].append(round(loop(True, args.steps), 3))
    bank.synchronize()
    res["train_loop_b8_fp32"] = {"steps": args.steps, "ms_per_step": runs,
                                 "note": "fresh = a new bank batch (ps_cloud_sample) every step on the training stream; resident = one batch reused"}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "exp_cloud_sample.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
