"""ps_volume_zoom (prepare.resample_pancreas_ct) timed on the GPU, in one process, device events after the warm-up bench.py uses (20
calls), at the NIH Pancreas-CT size: one 240 x 512 x 512 int16 CT and its uint8 label through both forms of the reference's resampling,
PointSegment/utils/cvt_CT_down.py:79-104 (z zoom 1.25 -> 300 slices, then 0.5 on every axis) and cvt_CT.py:79-105 (the same with the CT
flipped along y and both cropped in front of the second zoom), and the same calls in scipy on the host (one run each: they take seconds).
Per-kernel times come from a separate run under `rocprofv3 --kernel-trace --output-format csv` (--profile: the first form, 5 times);
--merge joins that run's kernel trace, in dispatch order, with the bytes each pass moves by construction and writes volume_zoom_exp.json,
the file kept under profiles/.  Bytes per pass, v = voxels of the pass's input volume, w = voxels of its output, S = bytes of the dtype:
    first prefilter (reads the caller's volume, writes float64)  (S + 8) v + 16 v (the anticausal pass reads and writes the coefficients)
    later prefilter (float64 in place)                           32 v
    interpolation                                                32 w read (four taps, neighbours share cache lines: 8 v at least) + 8 w | S w written
    order 0 gather                                               2 S w

usage (GPU box):
    python profiles/tools/exp_volume_zoom.py --out DIR [--scipy]                          # timings -> DIR/exp_volume_zoom.json
    rocprofv3 --kernel-trace --output-format csv -d A -o vz -- python profiles/tools/exp_volume_zoom.py --profile
    python profiles/tools/exp_volume_zoom.py --merge DIR/exp_volume_zoom.json --kernel-trace A/vz_kernel_trace.csv --out DIR"""
import argparse
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

SHAPE, SPACING_Z, CROP = (240, 512, 512), 1.25, ((10, 289), (40, 471), (40, 471))
# The yardstick of DESIGN.md 4.4 and 4.6 (exp_volume_sample.py uses the same figure): 8 TB/s is the part's specified HBM3E peak, about
# 6.3 TB/s is what a streaming kernel reaches of it; in this tree probs_to_labels was measured at that rate (152 MB in 24 us, 4.4).
HBM_ACHIEVABLE_GBS = 6300.0
PROFILE_REPS = 5


def inputs():
    rng = np.random.default_rng(0)
    ct = rng.integers(-1024, 1500, SHAPE, dtype=np.int16)
    seg = np.zeros(SHAPE, np.uint8)
    seg[100:140, 200:300, 220:330] = 1
    return ct, seg


def passes_of_the_first_form():
    """(kernel name fragment, bytes by construction) of one cvt_CT_down chain, in dispatch order."""
    n = SHAPE[0] * SHAPE[1] * SHAPE[2]
    z1 = int(round(SHAPE[0] * SPACING_Z))
    v1 = z1 * SHAPE[1] * SHAPE[2]                     # after the z zoom
    a, b, c = v1 // 2, v1 // 4, v1 // 8               # the 0.5 zoom, axis after axis
    return [
        ("rz_taps_kernel", 0), ("rz_filter_strided_kernel<short>", 26 * n), ("rz_interp_kernel<short>", 8 * n + 2 * v1),   # CT, z zoom
        ("rz_taps_kernel", 0), ("rz_gather_kernel<unsigned char>", 2 * v1),                                               # label, z zoom
        ("rz_taps_kernel", 0), ("rz_filter_strided_kernel<short>", 26 * v1), ("rz_interp_kernel<double>", 8 * v1 + 8 * a),  # CT, 0.5: axis 0
        ("rz_filter_strided_kernel<double>", 32 * a), ("rz_interp_kernel<double>", 8 * a + 8 * b),                          # axis 1
        ("rz_filter_rows_kernel", 32 * b), ("rz_interp_kernel<short>", 8 * b + 2 * c),                                      # axis 2
        ("rz_taps_kernel", 0), ("rz_gather_kernel<unsigned char>", 2 * c),                                                # label, 0.5
    ]


def event_ms(fn, reps):
    import torch
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / reps


def kernel_table(path):
    """rocprofv3's kernel trace -> the passes of one chain in dispatch order: average time over the profiled repetitions (the first one
    left out), algorithmic GB/s and share of the achievable HBM rate."""
    rows = [r for r in csv.DictReader(open(path)) if "ps::" in (r.get("Kernel_Name") or "") and "rz_" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    plan = passes_of_the_first_form()
    assert len(rows) == PROFILE_REPS * len(plan), (len(rows), len(plan))
    out = []
    for i, (frag, nbytes) in enumerate(plan):
        us = []
        for rep in range(1, PROFILE_REPS):
            r = rows[rep * len(plan) + i]
            assert frag in r["Kernel_Name"], (frag, r["Kernel_Name"])
            us.append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
        row = {"pass": i, "kernel": frag, "avg_us": round(sum(us) / len(us), 1)}
        if nbytes:
            gbs = nbytes / (row["avg_us"] * 1e-6) / 1e9
            row.update(algorithmic_bytes=nbytes, gb_per_s=round(gbs, 1), share_of_achievable_hbm=round(gbs / HBM_ACHIEVABLE_GBS, 3))
        out.append(row)
    return out


def scipy_chain(ct, seg, flip_y, crop):
    from scipy import ndimage
    ct = ndimage.zoom(ct, (SPACING_Z, 1, 1), order=3)
    seg = ndimage.zoom(seg, (SPACING_Z, 1, 1), order=0)
    if flip_y:
        ct = np.flip(ct, 1)
    if crop:
        box = tuple(slice(max(0, a), min(n - 1, b) + 1) for n, (a, b) in zip(seg.shape, crop))
        ct, seg = ct[box], seg[box]
    ct = ndimage.zoom(ct, 0.5, order=3)
    seg = ndimage.zoom(seg, 0.5, order=0)
    return np.clip(ct, -100, 240), seg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--scipy", action="store_true", help="also time the two chains in scipy on the host and compare the volumes")
    ap.add_argument("--merge", default=None, help="the timing run's JSON")
    ap.add_argument("--kernel-trace", default=None)
    args = ap.parse_args()
    if args.merge:
        res = json.loads(open(args.merge).read())
        res["hbm_achievable_gb_per_s"] = HBM_ACHIEVABLE_GBS
        res["passes_cvt_ct_down"] = kernel_table(args.kernel_trace)
        res["passes_sum_us"] = round(sum(r["avg_us"] for r in res["passes_cvt_ct_down"]), 1)
        line = json.dumps(res)
        print(line)
        if args.out:
            os.makedirs(args.out, exist_ok=True)
            with open(os.path.join(args.out, "volume_zoom_exp.json"), "w") as f:
                f.write(line + "\n")
        return
    import torch
    from point_unet_amd.prepare import resample_pancreas_ct
    ct, seg = inputs()
    d_ct, d_seg = torch.from_numpy(ct).cuda(), torch.from_numpy(seg).cuda()
    down = lambda: resample_pancreas_ct(d_ct, d_seg, spacing_z=SPACING_Z)  # noqa: E731
    crop = lambda: resample_pancreas_ct(d_ct, d_seg, spacing_z=SPACING_Z, flip_y=True, crop=CROP)  # noqa: E731
    if args.profile:
        for _ in range(PROFILE_REPS):
            down()
        torch.cuda.synchronize()
        print(json.dumps({"profile": True}))
        return
    res = {"shape": SHAPE, "spacing_z": SPACING_Z, "crop": CROP}
    for name, fn in (("cvt_ct_down", down), ("cvt_ct", crop)):
        for _ in range(20):
            fn()
        torch.cuda.synchronize()
        runs = [event_ms(fn, 10) for _ in range(3)]
        out = fn()
        res[name] = {"device_ms": round(min(runs), 4), "device_ms_runs": [round(r, 4) for r in runs], "out_shape": list(out["ct"].shape)}
        if args.scipy:
            t0 = time.perf_counter()
            want_ct, want_seg = scipy_chain(ct, seg, name == "cvt_ct", CROP if name == "cvt_ct" else None)
            res[name]["host_scipy_s"] = round(time.perf_counter() - t0, 2)
            got = out["ct"].cpu().numpy()
            res[name]["ct_voxels_differing_from_scipy"] = int((got != want_ct).sum())
            res[name]["seg_equal_to_scipy"] = bool(np.array_equal(out["seg"].cpu().numpy(), want_seg))
    res["peak_device_memory_gb"] = round(torch.cuda.max_memory_allocated() / 1e9, 3)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "exp_volume_zoom.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
