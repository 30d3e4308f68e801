"""The correlator call's pure plan (csrc/gat_corr_plan.h: corr_check_call, corr_plan, corr_plan_resident) compiled stand-alone
with its own main (tests/corrplan/corrplan_main.cpp) under AddressSanitizer and UBSan, and run: every refusal a call can reach
with its code and message; a few thousand random calls whose planned launches keep what the kernels assume of a launch
(tests/corr_launch_contract.h, shared with the host simulator) and own every tap exactly once; every branch of the plan reached;
and the geometry of the benchmark's shapes at 256 CUs as literal numbers.  The header must compile without any HIP header.  The
program stands alone; nothing is loaded into Python."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gpuacceleratedtracking_amd", "csrc")


def test_plan_header_includes_no_hip_header():
    with open(os.path.join(CSRC, "gat_corr_plan.h")) as f:
        includes = re.findall(r'^\s*#\s*include\s*[<"]([^>"]+)[>"]', f.read(), flags=re.M)
    assert includes and not [i for i in includes if "hip" in i.lower()], includes
    assert "gat_sig_plan.h" in includes and "gat.h" in includes


def test_plan_program_under_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ not found: the plan header cannot be checked")
    exe = str(tmp_path / "corrplan")
    # (no -I of a ROCm tree: the header and the launch contract are plain C++)
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                    os.path.join(ROOT, "tests", "corrplan", "corrplan_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "pinned 8 plans" in r.stdout, r.stdout[-1000:]
    m = re.search(r"planned (\d+) calls \((\d+) refused, (\d+) resident plans\), (\d+) refusals provoked, 0 failures", r.stdout)
    assert m, r.stdout[-1000:]
    assert int(m.group(1)) >= 4000 and int(m.group(3)) > 100 and int(m.group(4)) >= 20
