"""The label clean-up (postprocess.label_components, postprocess.brats_post_processing; csrc/postprocess.hip) timed on the GPU, in one
process, device events after the warm-up bench.py uses (20 calls), at the BraTS size 155 x 240 x 240: a synthetic prediction (a large
tumour with core and enhancing region, a second blob of a few hundred voxels, label noise) under a brain mask, and the same chain in
scipy on the host (--scipy, one run: it takes seconds) -- the reference's post_processing, SaliencyAttention/eval.py:20-55, written out
with ndimage calls.  The launch counts come from the library's own stage records (ps_timing_begin / ps_timing_end).

usage (GPU box):
    python profiles/tools/exp_postprocess.py --out DIR [--scipy]        # timings -> DIR/exp_postprocess.json"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

SHAPE = (155, 240, 240)
WT_THRESHOLD = 2000


def inputs():
    x, y, z = np.meshgrid(*[np.arange(n, dtype=np.float32) for n in SHAPE], indexing="ij")

    def ball(c, r):
        return ((x - c[0]) / r[0]) ** 2 + ((y - c[1]) / r[1]) ** 2 + ((z - c[2]) / r[2]) ** 2 <= 1.0

    rng = np.random.default_rng(0)
    pred = np.zeros(SHAPE, np.uint8)
    pred[ball((80, 120, 130), (30, 40, 45))] = 2
    pred[ball((80, 120, 130), (18, 25, 28))] = 1
    pred[ball((80, 120, 130), (9, 12, 14))] = 4
    pred[ball((30, 60, 60), (5, 6, 6))] = 2
    noise = rng.random(SHAPE) < 0.002
    pred[noise] = rng.choice(np.array([1, 2, 4], np.uint8), int(noise.sum()))
    weight = ball((77, 120, 120), (70, 100, 95)).astype(np.uint8)
    return pred, weight


def event_ms(fn, reps):
    import torch
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / reps


def scipy_chain(pred, weight):
    from scipy import ndimage
    s = ndimage.generate_binary_structure(3, 2)

    def above(m):
        lab, n = ndimage.label(m, s)
        if n == 1:
            return m
        sizes = np.bincount(lab.ravel())
        sizes[0] = 0
        return (sizes > WT_THRESHOLD)[lab]

    p = pred * (weight != 0)
    whole = above(ndimage.binary_closing(p > 0, structure=s))
    core = above(ndimage.binary_closing((p > 0) & (p != 2) & whole, structure=s))
    enh = (p == 4) & core
    if whole.sum() > 100 and 0 < enh.sum() < 100:
        enh[...] = False
    out = 2 * whole.astype(np.uint8)
    out[core] = 1
    out[enh] = 4
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--scipy", action="store_true", help="also time the chain in scipy on the host and compare the volumes")
    args = ap.parse_args()
    import torch
    from point_unet_amd import postprocess, runtime
    pred, weight = inputs()
    d_pred, d_weight = torch.from_numpy(pred).cuda(), torch.from_numpy(weight).cuda()
    d_whole = (d_pred > 0).to(torch.uint8)
    chain = lambda: postprocess.brats_post_processing(d_pred, d_weight, WT_THRESHOLD)  # noqa: E731
    label = lambda: postprocess.label_components(d_whole, 2)  # noqa: E731
    res = {"shape": SHAPE, "wt_threshold": WT_THRESHOLD}
    ctx = runtime.default_context(0)
    for name, fn in (("brats_post_processing", chain), ("label_components", label)):
        for _ in range(20):
            fn()
        torch.cuda.synchronize()
        runs = [event_ms(fn, 10) for _ in range(3)]
        ctx.timing_begin()
        fn()
        rows = ctx.timing_end()
        res[name] = {"device_ms": round(min(runs), 4), "device_ms_runs": [round(r, 4) for r in runs],
                     "launches": int(sum(r[2] for r in rows)), "stage_ms": {r[0]: round(r[1], 4) for r in rows}}
    res["label_components"]["components"] = label()[1]
    res["label_components"]["note"] = "includes the read-back of n, the one synchronisation of the Python wrapper"
    if args.scipy:
        t0 = time.perf_counter()
        want = scipy_chain(pred, weight)
        res["brats_post_processing"]["host_scipy_s"] = round(time.perf_counter() - t0, 2)
        res["brats_post_processing"]["equal_to_scipy"] = bool(np.array_equal(chain().cpu().numpy(), want))
        from scipy import ndimage
        t0 = time.perf_counter()
        _, n = ndimage.label(pred > 0, ndimage.generate_binary_structure(3, 2))
        res["label_components"]["host_scipy_s"] = round(time.perf_counter() - t0, 2)
        res["label_components"]["equal_count_to_scipy"] = bool(n == res["label_components"]["components"])
    res["peak_device_memory_gb"] = round(torch.cuda.max_memory_allocated() / 1e9, 3)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "exp_postprocess.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
