"""The pure plan of gat_smooth_observables (csrc/gat_smooth_plan.h) and the host twin's loops over it (the rule of
csrc/gat_smooth.h), compiled stand-alone with their own main (tests/smoothplan/smoothplan_main.cpp) under AddressSanitizer and UBSan
with float-cast-overflow, and run: every documented refusal with nothing planned, 3000 random plans in which every (epoch, channel)
lies in exactly one thread of each stage, the segment combine's associativity on random triples, the host twin on heap buffers of
exactly the described extents with every subset of the optional outputs, the device split's four stages walked in plain loops
against the twin's bytes, and the hostile entries.  The program stands alone; nothing is loaded into Python."""
import os
import subprocess

import pytest

from tests.fix_domain import sanitizing_compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("smoothplan") / "smoothplan")
    subprocess.run([sanitizing_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off",
                    "-fsanitize=address,undefined,float-cast-overflow",
                    "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "gpuacceleratedtracking_amd", "csrc"),
                    os.path.join(ROOT, "tests", "smoothplan", "smoothplan_main.cpp"), "-o", out], check=True)
    return out


def test_plan_twin_and_hostile_entries_under_sanitizers(exe):
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout[-600:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "planned 3000 calls" in r.stdout and " 0 failures" in r.stdout, r.stdout[-500:]
