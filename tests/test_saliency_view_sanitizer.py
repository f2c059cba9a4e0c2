"""The candidate table of the patch sampler -- the centre, the window, the copied box in view and in volume axes
(csrc/saliency_sampler_plan.h) -- in a stand-alone program under -fsanitize=address,undefined, compared with the numpy restatement
(saliency_view_ref.box): no GPU, no HIP call, nothing loaded into Python."""
import os
import subprocess

import saliency_view_ref as vref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((9, 20, 23), (4, 6, 30), (17, 33, 19), (1, 1, 1), (3, 2, 4), (7, 41, 37), (64, 160, 160), (2147483647, 1, 1))
PATCHES = ((5, 6, 7), (16, 16, 16), (8, 8, 8), (36, 5, 40), (1, 1, 1), (64, 160, 160), (1, 1, 2147483647))
HASHES = ((0, 0, 0), (0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF), (0x80000000, 0x12345678, 0xDEADBEEF), (1, 0xFFFFFFFE, 0x7FFFFFFF))


def test_candidate_table_under_asan_ubsan_equals_the_restatement():
    csrc = os.path.join(ROOT, "point-unet_amd", "csrc")
    subprocess.check_call(["make", "-C", csrc, "-s", "asan-sampler"])
    cases = [(view, s, p, h) for view in vref.VIEWS for s in SHAPES for p in PATCHES for h in HASHES]
    args = [str(v) for view, s, p, h in cases for v in (vref.VIEW_ID[view],) + s + p + h]
    p = subprocess.run([os.path.join(csrc, "build", "sampler_asan_check")] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0, "rc %d:\n%s" % (p.returncode, p.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-4000:]
    lines = p.stdout.splitlines()
    assert lines[-1] == "asan_sampler_main ok" and len(lines) == len(cases) + 1
    for line, (view, s, patch, h) in zip(lines, cases):
        want = [v for part in vref.box(s, patch, view, h) for v in part]
        assert [int(v) for v in line.split()] == want, (view, s, patch, h, line)
    # a view out of range and a broken argument list are refused, not run
    for bad in (["3"] + args[1:10], args[:9]):
        q = subprocess.run([os.path.join(csrc, "build", "sampler_asan_check")] + bad, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
        assert q.returncode == 1 and "asan_sampler_main:" in q.stderr and "runtime error" not in q.stderr
