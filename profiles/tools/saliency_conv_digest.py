"""The bytes of the 3-D convolution and its gradients, as digests: saliency.conv3d and saliency.conv3d_backward over every case of
tests/saliency_conv_cases.ALL (the joint geometries, the degenerate extents, the k walk, the fused inputs, the batches and one case per
kernel instantiation) at the three precisions, and the SHA-256 of every result tensor (y, dx, dx2, dw, dbias).  A change that reorders no
floating-point sum leaves every digest as it was: run the tool on a build of the tree before the change and on the tree after it, then
compare the two files.  The comparison is made tensor by tensor; the file it writes for the repository holds the comparison and, per case
group and precision, each run's SHA-256 over its tensor digests -- the per-tensor lists (0.4 MB a run) stay in the run files.

The cases and their operands are this tree's (tests/saliency_conv_cases.py, seeded by the case); --root names the tree whose package and
library compute the results (default: this one).  The work runs in a child process under a time limit of its own, so a hang ends there.

usage (GPU box):
    python profiles/tools/saliency_conv_digest.py --out DIR --label NAME [--root TREE] [--timeout 420]     # -> DIR/saliency_conv_digest_NAME.json
    python profiles/tools/saliency_conv_digest.py --compare A.json B.json --out FILE        # tensor by tensor; FILE: both runs per group and precision"""
import argparse
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def child(args):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.abspath(args.root))
    import saliency_conv_cases as cc
    from point_unet_amd import saliency as sal
    roles = ("y", "x", "x2", "w", "bias")
    digests = []
    for c in cc.ALL:
        x, x2, w, bias, dy = (None if t is None else t.cuda() for t in cc.operands(c))
        per_precision = []
        for precision in cc.PRECISIONS:
            got = sal.conv3d_backward(dy, x, w, c[5], c[6], x2, c[7], precision=precision)
            got["y"] = sal.conv3d(x, w, bias, c[5], c[6], x2, c[7], precision=precision)
            per_precision.append(" ".join(hashlib.sha256(got[n].cpu().numpy().tobytes()).hexdigest() for n in roles if n in got))
        digests.append(per_precision)
    res = {"label": args.label, "roles": "the digests of a case at a precision, in the order y, x, x2 (with x2 alone), w, bias", "precisions": cc.PRECISIONS,
           "groups": [[name, len(group)] for name, group in cc.GROUPS.items()], "cases": [cc.case_id(c) for c in cc.ALL], "digests": digests}
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "saliency_conv_digest_%s.json" % args.label), "w") as f:
        json.dump(res, f)
    print("%s: %d cases x %d precisions, %d digests" % (args.label, len(digests), len(cc.PRECISIONS), sum(len(p.split()) for d in digests for p in d)))
    return 0


def compare(a_path, b_path, out):
    """Compares every tensor digest of the two runs, names the (case, precision) pairs that differ, and writes the short file that is kept:
    per case group and precision the number of tensors and, for each run, the SHA-256 over that group's tensor digests in case order."""
    a, b = (json.load(open(p)) for p in (a_path, b_path))
    same_cases = a["cases"] == b["cases"] and a["precisions"] == b["precisions"] and a["groups"] == b["groups"]
    differing = [] if not same_cases else [
        "%s %s" % (case, precision) for case, da, db in zip(a["cases"], a["digests"], b["digests"]) for precision, pa, pb in zip(a["precisions"], da, db) if pa != pb]
    n = sum(len(p.split()) for d in a["digests"] for p in d)
    rows, first = [], 0
    for name, count in a["groups"]:
        for i, precision in enumerate(a["precisions"]):
            row = {"group": name, "cases": count, "precision": precision, "tensors": sum(len(d[i].split()) for d in a["digests"][first:first + count])}
            for run in (a, b):
                row[run["label"]] = hashlib.sha256(" ".join(d[i] for d in run["digests"][first:first + count]).encode()).hexdigest()
            rows.append(row)
        first += count
    res = {"what": "per case group of tests/saliency_conv_cases.py and precision: the SHA-256 over the SHA-256 digests of every result tensor (per case y, x, x2, "
                   "w, bias), in case order, for each run; the comparison is made tensor by tensor",
           "comparison": {"same_case_list": same_cases, "cases": len(a["cases"]), "tensor_digests_per_run": n, "differing": differing,
                          "all_equal": bool(same_cases and not differing)},
           "rows": rows}
    with open(out, "w") as f:
        f.write('{\n"what": %s,\n"comparison": %s,\n"rows": [\n%s\n]\n}\n' % (json.dumps(res["what"]), json.dumps(res["comparison"]),
                                                                             ",\n".join(json.dumps(r) for r in rows)))
    print("%s against %s: %d digests per list, %d (case, precision) pairs differ" % (a["label"], b["label"], n, len(differing)))
    return 0 if res["comparison"]["all_equal"] else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="a directory (run) or a file (--compare)")
    ap.add_argument("--label", default="tree")
    ap.add_argument("--root", default=ROOT, help="the tree whose point_unet_amd package and library compute the results")
    ap.add_argument("--timeout", type=int, default=420, help="seconds the child process may take")
    ap.add_argument("--compare", nargs=2, metavar=("A.json", "B.json"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if not args.out:
        ap.error("--out is required")
    if args.compare:
        sys.exit(compare(args.compare[0], args.compare[1], args.out))
    if args.child:
        sys.exit(child(args))
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--out", args.out, "--label", args.label, "--root", args.root]
    sys.exit(subprocess.run(cmd, timeout=args.timeout).returncode)


if __name__ == "__main__":
    main()
