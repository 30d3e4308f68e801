"""The pure plan of gat_nav_decode (csrc/gat_nav_plan.h) and the host twin's loops over it (the rule of csrc/gat_nav.h), compiled
stand-alone with their own main (tests/navplan/navplan_main.cpp) under AddressSanitizer and UBSan, and run: a few thousand random
plans, every (k, symbol), (k, candidate) and (k, frame) covered exactly once by the planned geometry, the scratch carve-up within
the planned bytes, every documented refusal with nothing planned, and the host twin on heap buffers of exactly the extents the
call describes -- a capacity above the counts, counts from monitor records, subsets of the outputs, streams with frames --, so
that a read or a write outside them is seen.  The program stands alone; nothing is loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plan_and_host_twin_under_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ not found: the plan header cannot be checked")
    exe = str(tmp_path / "navplan")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "gpuacceleratedtracking_amd", "csrc"),
                    os.path.join(ROOT, "tests", "navplan", "navplan_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "planned 3000 calls" in r.stdout and " 0 failures" in r.stdout, r.stdout[-500:]
