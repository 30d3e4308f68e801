"""The pure plans of gat_spacetime_filter and gat_spacetime_covariance (csrc/gat_st_plan.h) and the host loop of the filter's rule
(csrc/gat_st.h), compiled stand-alone with their own main (tests/stplan/stplan_main.cpp) under AddressSanitizer and UBSan, and
run: a few thousand random plans, every (block, output) covered exactly once, the covariance's LDS geometry for every (M, T),
every documented refusal with nothing planned, and the host loop on heap buffers of the descriptors' exact extents -- shapes at the
edges of every chunk, tile and halo among them --, so that a read before a block's first sample or past its last one is seen.
The program stands alone; nothing is loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plan_and_host_loop_under_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ not found: the plan header cannot be checked")
    exe = str(tmp_path / "stplan")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "gpuacceleratedtracking_amd", "csrc"),
                    os.path.join(ROOT, "tests", "stplan", "stplan_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "planned 3000 calls" in r.stdout and " 0 failures" in r.stdout, r.stdout[-500:]
