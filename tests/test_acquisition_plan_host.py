"""The direct acquisition search's pure plan (csrc/gat_acq_plan.h: the call check it shares with gat_acquire_fft, and acq_plan)
compiled stand-alone with its own main (tests/acqplan/acqplan_main.cpp) under AddressSanitizer and UBSan, and run: every
documented refusal with its code, its message and nothing written, in the entry point's order where two faults meet; a few
thousand random accepted calls whose groups, tiles, scratch regions and replica reach are walked as the kernel and its launcher
walk them; and G and the scratch bytes of a handful of shapes as literal numbers.  The program stands alone; nothing is loaded
into Python."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plan_program_under_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ not found: the plan header cannot be checked")
    exe = str(tmp_path / "acqplan")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "gpuacceleratedtracking_amd", "csrc"),
                    os.path.join(ROOT, "tests", "acqplan", "acqplan_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "pinned 19 plans" in r.stdout, r.stdout[-1000:]
    m = re.search(r"planned (\d+) calls \((\d+) with unit groups, (\d+) with a caller's grid\), every refusal from (\d+) of them, 0 failures", r.stdout)
    assert m, r.stdout[-1000:]
    assert int(m.group(1)) >= 4000 and int(m.group(2)) > 0 and int(m.group(3)) > 0 and int(m.group(4)) >= 400
