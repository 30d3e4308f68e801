"""The pure plan of gat_position_fix (csrc/gat_fix_plan.h), the host twin's loops over it (the rule of csrc/gat_fix.h) and the
ephemeris table (csrc/gat_fix_eph.h), compiled stand-alone with their own main (tests/fixplan/fixplan_main.cpp) under
AddressSanitizer and UBSan, and run: a few thousand random plans with every (epoch, channel) covered exactly once, every documented
refusal with nothing planned, the host twin on heap buffers of exactly the described extents with every subset of the optional
outputs, and the ephemeris through encoder and decoder.  The same program, asked for it, writes fix_sincos over a dense grid and
around every multiple of pi/4 up to 64 rad; the values are compared here with numpy's long double sine and cosine within 1e-15.
The program stands alone; nothing is loaded into Python."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ not found: the plan header cannot be checked")
    out = str(tmp_path_factory.mktemp("fixplan") / "fixplan")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "gpuacceleratedtracking_amd", "csrc"),
                    os.path.join(ROOT, "tests", "fixplan", "fixplan_main.cpp"), "-o", out], check=True)
    return out


def test_plan_twin_and_ephemeris_under_sanitizers(exe):
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "planned 3000 calls" in r.stdout and " 0 failures" in r.stdout, r.stdout[-500:]


def test_sincos_against_long_double(exe, tmp_path):
    """|error| <= 1e-15 absolute on |x| <= 64: the bound that keeps a satellite position good to 3e-8 m an angle"""
    if np.finfo(np.longdouble).eps > 1e-18:
        pytest.fail("numpy's long double is no wider than double here: no reference for the sine")
    path = str(tmp_path / "sincos.bin")
    subprocess.run([exe, "sincos", path], check=True)
    v = np.fromfile(path, dtype=np.float64).reshape(-1, 3)
    assert v.shape[0] > 400000 and np.abs(v[:, 0]).max() <= 64.5
    x = v[:, 0].astype(np.longdouble)
    err_c = np.abs(v[:, 1].astype(np.longdouble) - np.cos(x)).max()
    err_s = np.abs(v[:, 2].astype(np.longdouble) - np.sin(x)).max()
    print(f"fix_sincos: max |cos error| {float(err_c):.3e}, max |sin error| {float(err_s):.3e} over {v.shape[0]} points")
    assert err_c <= 1e-15 and err_s <= 1e-15
