"""The patch sampler through the three anatomical views (include/pointseg_saliency_view.h) on the GPU, timed per CALL of
the C entry as DESIGN 4.14 timed ps_patch_sample -- the host's table and its upload with the two launches, on outputs allocated once:
T = 8, one_positive, view patch [64, 160, 160], C = 1 on a bank of four Pancreas-sized volumes (110-131, 512, 512).  One process, the
variants interleaved window by window, device events around `reps` calls after a warm-up, three windows; best, median and worst window in
microseconds per call.

    old_3slots, old_mixed               ps_patch_sample at 3 slots and ps_patch_sample_mixup at B = 2: the calls DESIGN 4.14 timed
    axial / coronal / sagittal          ps_patch_sample_view at B = 2, and the same with every sample flipped
    *_3slots, *_mixed                   the view entry at 3 slots; ps_patch_sample_mixup_view at B = 2 (3 drawn samples), K = 2
    permute_then_axial                  the route the view entries replace: permute(...).contiguous() of ONE volume's image, label and
                                        weight, then the axial call on a bank of such copies; with it the bytes that route keeps resident
                                        per view

--old-only times the first two alone: they exist in every build of the library, so the same tool measures an older one.

usage (GPU box):
    python profiles/tools/saliency_view_sample.py [--out DIR] [--reps 50] [--old-only]     # -> DIR/saliency_view_sample.json (DIR: profiles/)"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

PATCH = (64, 160, 160)
DEPTHS = (110, 117, 124, 131)
VIEWS = {"axial": 0, "sagittal": 1, "coronal": 2}


def event_us(torch, fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--old-only", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch
    from point_unet_amd import _lib, runtime
    from point_unet_amd import saliency_data as sd

    lib = _lib.lib()
    g = torch.Generator(device="cuda").manual_seed(1)
    bank, copies = sd.PatchBank(1), sd.PatchBank(1)
    vols = []
    for d in DEPTHS:
        image = torch.randn((d, 512, 512, 1), generator=g, device="cuda")
        label = (torch.rand((d, 512, 512), generator=g, device="cuda") < 0.01).to(torch.uint8)
        weight = torch.ones((d, 512, 512), dtype=torch.uint8, device="cuda")
        bank.add_prepared(image, label, weight)
        if not args.old_only:
            copies.add_prepared(image.permute(2, 0, 1, 3).contiguous(), label.permute(2, 0, 1).contiguous(), weight.permute(2, 0, 1).contiguous())
        vols.append((image, label, weight))
    rng = np.random.default_rng(0)
    cands = {2: np.ascontiguousarray(rng.integers(0, 4, (2, 8)), np.int32), 3: np.ascontiguousarray(rng.integers(0, 4, (3, 8)), np.int32)}
    out = {k: torch.empty((3,) + PATCH + (2,), dtype=torch.float32, device="cuda") for k in ("images", "weights", "labels")}
    out["info"] = torch.empty((3, 8), dtype=torch.int32, device="cuda")
    outs = [runtime.ptr(out[k]) for k in ("images", "weights", "labels", "info")]
    P = (ctypes.c_int64 * 3)(*PATCH)
    gamma = (ctypes.c_double * 2)(0.3, 0.6)
    ones = (ctypes.c_int32 * 3)(1, 1, 1)

    def call(b, slots, mixed=False, view=None, flip=None):
        """One C call on bank b: `slots` rows of cand; view None: the old entry."""
        tables = b.c_tables()
        head = [b.ctx.handle, *tables, 1, cands[slots].ctypes.data_as(_lib.c_i32p), slots - (1 if mixed else 0), 8, P, 5, 2] + ([2, gamma] if mixed else [])
        if view is None:
            fn = lib.ps_patch_sample_mixup if mixed else lib.ps_patch_sample
            return lambda: _lib.check(fn(*head, *outs))
        fn = lib.ps_patch_sample_mixup_view if mixed else lib.ps_patch_sample_view
        return lambda: _lib.check(fn(*head, VIEWS[view], flip, *outs))

    bank.ctx.use_torch_stream()
    fns = {"old_3slots": call(bank, 3), "old_mixed": call(bank, 3, mixed=True)}
    ok = True
    if not args.old_only:
        copies.ctx.use_torch_stream()
        for view in VIEWS:
            fns[view] = call(bank, 2, view=view)
            fns[view + "_flipped"] = call(bank, 2, view=view, flip=ones)
            fns[view + "_3slots"] = call(bank, 3, view=view)
            fns[view + "_mixed"] = call(bank, 3, mixed=True, view=view)
        image, label, weight = vols[0]
        axial_on_copies = call(copies, 2, view="axial")

        def route():
            image.permute(2, 0, 1, 3).contiguous(), label.permute(2, 0, 1).contiguous(), weight.permute(2, 0, 1).contiguous()
            axial_on_copies()

        fns["permute_then_axial"] = route
        # the identity the tests hold, once more at this size
        a, b = bank.sample(cands[2], PATCH, 5, direction="sagittal"), copies.sample(cands[2], PATCH, 5)
        ok = all(torch.equal(a[k], b[k]) for k in ("images", "weights", "labels", "info"))
    for fn in fns.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    runs = {k: [] for k in fns}
    for _ in range(args.windows):
        for k, fn in fns.items():
            runs[k].append(event_us(torch, fn, args.reps))
    res = {"patch": PATCH, "T": 8, "mode": "one_positive", "volumes": [(d, 512, 512) for d in DEPTHS], "reps": args.reps,
           "method": "one process, variants interleaved per window, device events around `reps` C calls, 5 warm-up calls each; us per call: best / median / worst window",
           "sagittal_equals_permuted_copies": ok,
           "us_per_call": {k: {"best": round(min(r), 1), "median": round(sorted(r)[len(r) // 2], 1), "worst": round(max(r), 1)} for k, r in runs.items()},
           "resident_bytes_per_view_of_the_copy_route": int(sum(d * 512 * 512 * 6 for d in DEPTHS)),
           "bytes_permuted_per_volume": int(DEPTHS[0] * 512 * 512 * 6)}
    line = json.dumps(res)
    print(line)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "saliency_view_sample.json"), "w") as f:
        f.write(line + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
