"""The pure plans of the operators over raw samples -- gat_condition_samples (csrc/gat_cond_plan.h), gat_beamform_samples
(csrc/gat_beam_plan.h) and what they share (csrc/gat_sig_plan.h: descriptor check, fast-path rule, overlap test, the chunk split)
-- compiled stand-alone with their own main (tests/condplan/condplan_main.cpp) under AddressSanitizer and UBSan, and run: a few
thousand random cases each, every (block, sample) covered exactly once, every documented refusal with nothing planned.  The
estimating operators' split and batches are tests/test_estimate_plan_host.py's.  The program stands alone; nothing is loaded
into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plan_program_under_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ not found: the plan header cannot be checked")
    exe = str(tmp_path / "condplan")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "gpuacceleratedtracking_amd", "csrc"),
                    os.path.join(ROOT, "tests", "condplan", "condplan_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "planned 4000 calls" in r.stdout and " 0 failures" in r.stdout, r.stdout[-500:]
