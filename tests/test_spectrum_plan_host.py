"""The pure plan of gat_sample_spectrum (csrc/gat_spec_plan.h) and the host loop of its rule (csrc/gat_spec.h), compiled stand-alone
with their own main (tests/specplan/specplan_main.cpp) under AddressSanitizer and UBSan, and run: the kernel's walk over every
transform size (each point held once a pass, every twiddle the rule's), a few thousand random plans with every (block, antenna)
pair covered exactly once, every documented refusal with nothing planned, and the host loop on heap buffers of the descriptors'
exact extents, so that a read before a block's first sample or past its last one is seen.  The program stands alone; nothing is
loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plan_and_host_loop_under_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ not found: the plan header cannot be checked")
    exe = str(tmp_path / "specplan")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "gpuacceleratedtracking_amd", "csrc"),
                    os.path.join(ROOT, "tests", "specplan", "specplan_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "planned 3000 calls" in r.stdout and " 0 failures" in r.stdout, r.stdout[-500:]
