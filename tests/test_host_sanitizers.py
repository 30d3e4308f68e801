"""Host-only code under AddressSanitizer + UndefinedBehaviorSanitizer (CPU build only -- GPU sanitizers do not exist on this
pool): `make -C oracle sanitize` compiles the oracle and libgat's host-only translation unit (csrc/gat_codes.cpp: PRN
generators, tap-shift helper) with -fsanitize=address,undefined,float-cast-overflow and drives them through the cases in
oracle/sanitize/sanitize_main.c (ragged sizes, negative taps at n = 0, ratio = 1/16 with code phases within an ulp of
chip edges, carrier phases that round to a whole cycle, GPS L5 lengths).  Any report aborts the run.

`make -C tests/hostsim run` does the same for the REST of the library's host code -- csrc/gat_api.cpp (validation, launch
planning, scratch management, graph cache, device groups) and csrc/gat_resident_api.cpp (the resident correlator's host side) and csrc/gat_acq_api.cpp (the acquisition search's validation,
work split and scratch carve-up) and csrc/gat_array_api.cpp (the antenna-array entry points: validation, the covariance's work split and
estimate batches) -- by linking it against a
host-only stand-in of the HIP runtime ("device" memory = host memory: every copy size is checked) and of the kernel
launchers, which check each planned launch against what the kernel assumes about its arguments (LDS carve-up, replica
room, grid decode, tap tables) and play the device's side of the resident correlator's doorbell protocol in a thread."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("gcc") is None or shutil.which("make") is None, reason="needs gcc + make")
def test_oracle_and_host_only_library_code_under_asan_ubsan():
    p = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "sanitize"], capture_output=True, text=True, timeout=900)
    out = p.stdout + p.stderr
    assert p.returncode == 0, out[-3000:]
    assert "sanitize: ok" in out and "runtime error" not in out and "AddressSanitizer" not in out, out[-3000:]


@pytest.mark.skipif(shutil.which("g++") is None or shutil.which("make") is None or not os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"),
                    reason="needs g++, make and the HIP headers")
def test_library_host_code_on_a_simulated_device_under_asan_ubsan():
    p = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tests", "hostsim"), "run", "CALLS=2500"], capture_output=True, text=True, timeout=1200)
    out = p.stdout + p.stderr
    assert p.returncode == 0, out[-4000:]
    assert "ok: 0 failures, 0 broken invariants" in out and "runtime error" not in out and "AddressSanitizer" not in out, out[-3000:]
    # the sweep really went through the planner and the resident protocol
    import re
    m = re.search(r"correlate sweep: (\d+) calls planned and launched, (\d+) rejected.*?(\d+) matrix-core launches, (\d+) second stages, (\d+) tails", out)
    assert m and int(m.group(1)) > 2000 and int(m.group(2)) > 20 and int(m.group(3)) > 10 and int(m.group(4)) > 100 and int(m.group(5)) > 5, out[-2000:]
    m = re.search(r"resident correlator: (\d+) opened, (\d+) refused as unsupported \(\+ \d+ for want of room\), (\d+) calls answered; the emulated kernel was started (\d+) times", out)
    assert m and int(m.group(1)) > 10 and int(m.group(3)) > 500 and int(m.group(4)) > int(m.group(1)), out[-2000:]
    # ... on caller's code tables of every length and chip kind: the fixed grid and the random sweep's tables, long int8 tables
    # among them, and no valid call refused (the planner once chose a tile that no longer fitted: 280 refusals in this grid)
    m = re.search(r"code tables: (\d+) tables bound, (\d+) grid calls, (\d+) calls on int8 tables of >= 20000 chips, (\d+) valid calls refused", out)
    assert m and int(m.group(1)) >= 35 and int(m.group(2)) >= 32400 and int(m.group(3)) >= 5400 and int(m.group(4)) == 0, out[-2000:]
    # ... on the tap lists of the GPU tests by layout, antennas, channels and kernel selection: every valid call launched, with
    # the launches covering each of the caller's taps exactly once (checked per call: a broken coverage is a failure above)
    m = re.search(r"tap grid: (\d+) calls, (\d+) tap launches, (\d+) valid calls refused", out)
    assert m and int(m.group(1)) >= 18048 and int(m.group(2)) >= 18048 and int(m.group(3)) == 0, out[-2000:]
    # ... and through the acquisition search's host side (csrc/gat_acq_api.cpp): launches, rejections and split grids
    m = re.search(r"acquisition sweep: (\d+) calls launched, (\d+) rejected, (\d+) with G > 1", out)
    assert m and int(m.group(1)) > 150 and int(m.group(2)) > 150 and int(m.group(3)) > 50, out[-2000:]
    # ... and through the antenna-array entry points (csrc/gat_array_api.cpp): every (block, sample) of every launched covariance
    # read exactly once and its outputs written whole (checked per call), refusals without a launch, and the work split's regimes
    # as shares of the launched calls.  Observed at CALLS=2500: 2168 / 333 / 665 / 292 / 832 on the default seed, 2215 / 286 /
    # 745 / 311 / 847 on seed 7; the shares asked for are about half the smaller of the two (0.31, 0.13 and 0.38 of the launched).
    m = re.search(r"array sweep: (\d+) covariance calls launched, (\d+) rejected, (\d+) with splits > 1, (\d+) with more units than workgroups, "
                  r"(\d+) through the streaming kernel", out)
    assert m, out[-2000:]
    launched, refused, split, multi_unit, streaming = (int(v) for v in m.groups())
    assert launched > 1500 and refused > 150, out[-2000:]
    assert split >= 0.15 * launched and multi_unit >= 0.065 * launched and streaming >= 0.19 * launched, out[-2000:]
