"""The pure plan of gat_position_fix_raim (csrc/gat_raim_plan.h) and the host twin's loops over it (the rules of csrc/gat_fix.h and
csrc/gat_raim.h), compiled stand-alone with their own main (tests/raimplan/raimplan_main.cpp) under AddressSanitizer and UBSan with
float-cast-overflow, and run: every documented refusal with nothing planned, a few thousand random plans with every lane's frozen channel inside the wave's
LDS, the host twin on heap buffers of exactly the described extents with every subset of the optional outputs -- it must leave out
the channel that was moved by a code period and find the receiver --, and a round walked lane-per-candidate the way the kernel runs
it, which must give the twin's trial statistics and its choice to the bit.  The program stands alone; nothing is loaded into Python."""
import os
import subprocess

import pytest

from tests.fix_domain import sanitizing_compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("raimplan") / "raimplan")
    subprocess.run([sanitizing_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off",
                    "-fsanitize=address,undefined,float-cast-overflow",
                    "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "gpuacceleratedtracking_amd", "csrc"),
                    os.path.join(ROOT, "tests", "raimplan", "raimplan_main.cpp"), "-o", out], check=True)
    return out


def test_plan_twin_and_wave_round_under_sanitizers(exe):
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "planned 3000 calls" in r.stdout and " 0 failures" in r.stdout, r.stdout[-500:]
