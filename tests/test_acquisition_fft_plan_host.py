"""The pure plan of gat_acquire_fft (csrc/gat_acq_fft_plan.h) and the host loops of its rule (csrc/gat_acq_fft.h), compiled
stand-alone with their own main (tests/acqfftplan/acqfftplan_main.cpp) under AddressSanitizer and UBSan, and run: a few thousand
random plans (the cheapest transform length, segments that give every bin exactly one owner and read no lag outside [0, Jseg), a
scratch carve-up of disjoint regions inside the bound, every (block, antenna) unit walked once and in order), every refusal with
nothing planned, and the host loops on heap buffers of the descriptors' exact extents.  The program stands alone; nothing is
loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plan_and_host_loops_under_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ not found: the plan header cannot be checked")
    exe = str(tmp_path / "acqfftplan")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "gpuacceleratedtracking_amd", "csrc"),
                    os.path.join(ROOT, "tests", "acqfftplan", "acqfftplan_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "planned " in r.stdout and " 0 failures" in r.stdout, r.stdout[-500:]
