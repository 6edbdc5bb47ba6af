"""blk::transpose64 on its own, as the kernels call it: 16 waves of one workgroup, each with its private LDS region, each
transposing a 64 x 64 block of distinct values and transposing it back (tests/isa/probe_transpose.hip).  The host compares both
images exactly: the routine is pure data movement, whatever the width of its LDS reads and the lane exchange in front of them."""
import os
import shutil
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sixteen_waves_transpose_and_back_exactly(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "probe_transpose")
    subprocess.check_call([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=on", "-fno-slp-vectorize", "-w",
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "enph459-super-resolution_amd", "csrc"),
                           os.path.join(ROOT, "tests", "isa", "probe_transpose.hip"), "-o", exe])
    out = subprocess.run(["timeout", "-k", "10", "120", exe], capture_output=True, text=True, timeout=150)
    print(out.stdout, out.stderr)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "transpose probe OK" in out.stdout and " 0 wrong transposed, 0 wrong after the way back" in out.stdout
