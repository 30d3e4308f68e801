"""The pure plan of gat_position_fix (csrc/gat_fix_plan.h), the host twin's loops over it (the rule of csrc/gat_fix.h) and the
ephemeris table (csrc/gat_fix_eph.h), compiled stand-alone with their own main (tests/fixplan/fixplan_main.cpp) under
AddressSanitizer and UBSan with float-cast-overflow (which g++'s ``undefined`` leaves out; ROCm's clang++ where g++ lacks it), and
run: a few thousand random plans with every (epoch, channel) covered exactly once, every documented refusal with nothing planned,
the host twin on heap buffers of exactly the described extents with every subset of the optional outputs, and the ephemeris through encoder and decoder.  The same program, asked for it, writes fix_sincos over a dense grid and
around every multiple of pi/4 up to 72 rad, and at +-2^k with four neighbours each for k = 6 .. 1023; the values are compared here
with numpy's long double sine and cosine within 1e-15 wherever |x| <= 2^20, beyond that the sweep must only run clean under the
sanitizer (the quadrant's conversion).  The program stands alone; nothing is loaded into Python."""
import os
import subprocess

import numpy as np
import pytest

from tests.fix_domain import sanitizing_compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZERS = "address,undefined,float-cast-overflow"


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("fixplan") / "fixplan")
    subprocess.run([sanitizing_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=" + SANITIZERS,
                    "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "gpuacceleratedtracking_amd", "csrc"),
                    os.path.join(ROOT, "tests", "fixplan", "fixplan_main.cpp"), "-o", out], check=True)
    return out


def test_plan_twin_and_ephemeris_under_sanitizers(exe):
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "planned 3000 calls" in r.stdout and " 0 failures" in r.stdout, r.stdout[-500:]


def test_sincos_against_long_double(exe, tmp_path):
    """|error| <= 1e-15 absolute on |x| <= 72 (Omega reaches +-69.3) and at the powers of two up to 2^20: the bound that keeps a
    satellite position good to 3e-8 m an angle.  Beyond 2^20 the reduction's products are no longer exact and the values are no
    sine; there the sweep to +-2^1023, the infinities and NaN must only run clean under the sanitizers: the quadrant is taken
    without a conversion that is undefined from 2^63 on."""
    if np.finfo(np.longdouble).eps > 1e-18:
        pytest.fail("numpy's long double is no wider than double here: no reference for the sine")
    path = str(tmp_path / "sincos.bin")
    r = subprocess.run([exe, "sincos", path], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    v = np.fromfile(path, dtype=np.float64).reshape(-1, 3)
    swept = np.abs(v[:, 0])
    assert (swept == 2.0 ** 1023).sum() == 2 and (swept == 2.0 ** 63).sum() == 2 and np.isnan(v[-1, 0]) and np.isinf(v[-3:-1, 0]).all()
    v = v[swept <= 2.0 ** 20]
    # the grid, 185 multiples of pi/4 and 15 powers of two of both signs with their neighbours (2^20's upper ones lie beyond)
    assert v.shape[0] == 450001 + 185 * 9 + 15 * 2 * 9 - 8 and np.abs(v[:, 0]).max() == 2.0 ** 20 and (np.abs(v[:, 0]) > 72.0).sum() >= 14 * 18
    x = v[:, 0].astype(np.longdouble)
    err_c = np.abs(v[:, 1].astype(np.longdouble) - np.cos(x)).max()
    err_s = np.abs(v[:, 2].astype(np.longdouble) - np.sin(x)).max()
    print(f"fix_sincos: max |cos error| {float(err_c):.3e}, max |sin error| {float(err_s):.3e} over {v.shape[0]} points")
    assert err_c <= 1e-15 and err_s <= 1e-15
