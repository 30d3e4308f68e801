"""The pure plan of gat_snapshot_fix (csrc/gat_snap_plan.h) and the host twin's loops over it (the rules of csrc/gat_fix.h,
csrc/gat_vel.h and csrc/gat_snap.h), compiled stand-alone with their own main (tests/snapplan/snapplan_main.cpp) under
AddressSanitizer and UBSan with float-cast-overflow, and run: every documented refusal with nothing planned, a few thousand random
plans that cover every (epoch, channel) once, the host twin on heap buffers of exactly the described extents with every subset of the
optional outputs, of ``prior_xyz`` and of the weights -- it must find the receivers and the whole milliseconds --, an epoch walked
lane by lane the way the kernel runs it, which must give the twin's record and outputs to the bit, and the hostile entries.  The
program stands alone; nothing is loaded into Python."""
import os
import subprocess

import pytest

from tests.fix_domain import sanitizing_compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("snapplan") / "snapplan")
    subprocess.run([sanitizing_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off",
                    "-fsanitize=address,undefined,float-cast-overflow",
                    "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "gpuacceleratedtracking_amd", "csrc"),
                    os.path.join(ROOT, "tests", "snapplan", "snapplan_main.cpp"), "-o", out], check=True)
    return out


def test_plan_twin_and_wave_walk_under_sanitizers(exe):
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout[-600:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "planned 3000 calls" in r.stdout and " 0 failures" in r.stdout, r.stdout[-500:]
