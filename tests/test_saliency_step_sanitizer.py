"""The host side of the saliency training step -- the layer table, the optimiser's decay table and the scratch plan
(csrc/saliency_net.h, csrc/saliency_step_plan.h) -- in a stand-alone program under -fsanitize=address,undefined: no GPU, no HIP call, nothing
loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_step_plan_and_decay_table_under_asan_ubsan():
    csrc = os.path.join(ROOT, "point-unet_amd", "csrc")
    subprocess.check_call(["make", "-C", csrc, "-s", "asan-step"])
    p = subprocess.run([os.path.join(csrc, "build", "step_asan_check")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0, "rc %d:\n%s" % (p.returncode, p.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-4000:]
    assert "asan_step_main ok" in p.stdout
