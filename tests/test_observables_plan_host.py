"""The pure plan of gat_observables (csrc/gat_obs_plan.h) and the host twin's loops over it (the rule of csrc/gat_obs.h), compiled
stand-alone with their own main (tests/obsplan/obsplan_main.cpp) under AddressSanitizer and UBSan, and run: a few thousand random
plans walked as the kernels walk them, with every (block, channel) covered by exactly one run and every epoch written exactly
once, every documented refusal with nothing planned, and the host twin on heap buffers of exactly the described extents with each
output alone and all but each.  The program stands alone; nothing is loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ not found: the plan header cannot be checked")
    out = str(tmp_path_factory.mktemp("obsplan") / "obsplan")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "gpuacceleratedtracking_amd", "csrc"),
                    os.path.join(ROOT, "tests", "obsplan", "obsplan_main.cpp"), "-o", out], check=True)
    return out


def test_plan_and_twin_under_sanitizers(exe):
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "planned 3000 calls" in r.stdout and " 0 failures" in r.stdout, r.stdout[-500:]
