"""The host plan of ps_saliency_map -- the view axes, the window table and the scratch plan (csrc/saliency_map_plan.h) -- in a stand-alone
program under -fsanitize=address,undefined: no GPU, no HIP call, nothing loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_window_table_and_scratch_plan_under_asan_ubsan():
    csrc = os.path.join(ROOT, "point-unet_amd", "csrc")
    subprocess.check_call(["make", "-C", csrc, "-s", "asan-map"])
    p = subprocess.run([os.path.join(csrc, "build", "map_asan_check")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0, "rc %d:\n%s" % (p.returncode, p.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-4000:]
    assert "asan_map_main ok" in p.stdout
