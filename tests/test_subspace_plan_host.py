"""The pure plans of gat_accumulator_covariance and gat_hermitian_eig (csrc/gat_eig_plan.h) and the host twins' loops over them (the
rule of csrc/gat_eig.h), compiled stand-alone with their own main (tests/subplan/subplan_main.cpp) under AddressSanitizer and UBSan,
and run: a few thousand random plans, every (estimate, channel, chunk, entry) and every (matrix, round, item) covered exactly once
by the planned geometry in either work split, the scratch and the LDS carve-up within the planned bytes, every documented refusal
with nothing planned, and both twins on heap buffers of exactly the extents the calls describe -- padded block strides, a last
partial chunk, a last partial estimate, R = 0, subsets of the outputs --, so that a read or a write outside them is seen.  The
program stands alone; nothing is loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plans_and_host_twins_under_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ not found: the plan header cannot be checked")
    exe = str(tmp_path / "subplan")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "gpuacceleratedtracking_amd", "csrc"),
                    os.path.join(ROOT, "tests", "subplan", "subplan_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "planned 3000 calls" in r.stdout and " 0 failures" in r.stdout, r.stdout[-500:]
