"""The channel-record rules (csrc/gat_chan_rules.h: the kernels' predicates and the host checks that negate them) and the code
tables' layout (csrc/gat_code_tables.h: strides, refusals, packers) compiled stand-alone with their own main
(tests/chanrules/chanrules_main.cpp) under AddressSanitizer and UBSan, without contraction, and run: every refusal with its code
and message; 120 000 random draws in which no accepted record is one a kernel poisons; each rule broken alone; the bounds one ulp
either side; the packed tables of 1 .. 130, 1023, 10230 and 120000 chips in exactly sized buffers; pinned strides.  Both headers
must compile alone without any HIP header.  The program stands alone; nothing is loaded into Python."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gpuacceleratedtracking_amd", "csrc")
HEADERS = ("gat_hd.h", "gat_chan_rules.h", "gat_code_tables.h")


def _gxx():
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ not found: the headers cannot be checked")
    return gxx


@pytest.mark.parametrize("header", HEADERS)
def test_header_compiles_alone_without_hip(header, tmp_path):
    with open(os.path.join(CSRC, header)) as f:
        includes = re.findall(r'^\s*#\s*include\s*[<"]([^>"]+)[>"]', f.read(), flags=re.M)
    assert not [i for i in includes if "hip" in i.lower()], includes
    src = tmp_path / "alone.cpp"
    src.write_text('#include "%s"\nint main() { return 0; }\n' % header)
    # (no -I of a ROCm tree)
    subprocess.run([_gxx(), "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                    "-fsyntax-only", str(src)], check=True)


def test_one_definition_of_the_host_device_marker():
    """GAT_HD is defined in gat_hd.h alone, and the code-span bounds are literals in gat_chan_rules.h alone."""
    defs, bounds = [], []
    for name in sorted(os.listdir(CSRC)):
        with open(os.path.join(CSRC, name)) as f:
            text = f.read()
        if re.search(r"^\s*#\s*define\s+GAT_HD\b", text, flags=re.M):
            defs.append(name)
        if "2097152.0" in text:
            bounds.append(name)
    assert defs == ["gat_hd.h"], defs
    assert bounds == ["gat_chan_rules.h"], bounds


def test_rules_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "chanrules")
    subprocess.run([_gxx(), "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                    os.path.join(ROOT, "tests", "chanrules", "chanrules_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    m = re.search(r"packed (\d+) tables \((\d+) with sign-bit rows\), pinned (\d+) stride pairs", r.stdout)
    assert m and int(m.group(1)) == 4 * 133 and int(m.group(2)) >= 133 and int(m.group(3)) >= 8, r.stdout[-1000:]
    m = re.search(r"drew (\d+) calls, (\d+) refusals provoked, 0 failures", r.stdout)
    assert m and int(m.group(1)) >= 100000 and int(m.group(2)) >= 40, r.stdout[-1000:]
