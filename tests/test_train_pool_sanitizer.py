"""The device-memory pool of the native training step (csrc/train_pool.h) -- first fit over address-ordered blocks, coalescing inside a chunk
and never across two, the steady state of a repeated step, the reset behind a failed step, a source that refuses -- in a stand-alone program
under -fsanitize=address,undefined over a source of numbered addresses: no GPU, no HIP call, nothing loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_training_pool_under_asan_ubsan():
    csrc = os.path.join(ROOT, "point-unet_amd", "csrc")
    subprocess.check_call(["make", "-C", csrc, "-s", "asan-pool"])
    p = subprocess.run([os.path.join(csrc, "build", "pool_asan_check")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0, "rc %d:\n%s" % (p.returncode, p.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-4000:]
    assert "asan_pool_main ok" in p.stdout
