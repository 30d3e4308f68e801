"""Timings of the carrier smoothing (include/gat.h gat_smooth_observables) next to what a user of the library did before it
existed, on the same observables in the same run, with scripts/atm_bench.py's protocol:

  the device call on observables in device memory -- settle launches, then timed launches, one HIP-event interval per launch
  (all four kernels), median;
  the yardstick: a device-to-host copy of the observables followed by the host twin (gat_smooth_observables_host: the same rule
  in plain loops, one thread) -- wall time of the two steps, each timed, median over `--host-reps` repetitions.

Shapes (epochs, channels), every output asked for, the rate test and a lock mask on, a window of 100, synthetic observables with
noise, slips, gaps and masked cells (tests/smooth_cases.py):
  (65536, 12)    a 12-channel receiver
  (65536, 64)    64 channels

Per shape: ms of the device call with the plan, ms of the copy and of the twin, their ratio, and the bytes the call moves at the
least (inputs once, scratch written and read once, outputs once) over the device time.  The outputs of both paths are compared
bit for bit before anything is timed.

  python scripts/smooth_bench.py [--out profiles/smooth/smooth_bench.json] [--settle 3] [--steps 10] [--host-reps 2] [--warm 10]
Reported, not required: no figure here gates anything."""
from __future__ import annotations

import argparse
import ctypes as C
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scripts.array_bench import median_ms  # noqa: E402
from scripts.spectrum_bench import lib_record  # noqa: E402

SOURCES = ("gat_smooth.hip", "gat_smooth.h", "gat_smooth_plan.h", "gat_smooth_kernels.h", "gat_smooth_api.cpp")
SHAPES = ((65536, 12), (65536, 64))
WINDOW = 100


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "smooth", "smooth_bench.json"))
    ap.add_argument("--settle", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--warm", type=int, default=10)
    args = ap.parse_args()
    import torch

    import gpuacceleratedtracking_amd as g
    from gpuacceleratedtracking_amd import _lib
    from gpuacceleratedtracking_amd.smoothing import smoothing_plan
    from tests import smooth_cases as sc

    lib = g.load_library()
    ctx = g.get_context()
    dev = ctx.device
    csrc = os.path.join(ROOT, "gpuacceleratedtracking_amd", "csrc")
    sha = hashlib.sha256()
    for name in SOURCES:
        with open(os.path.join(csrc, name), "rb") as fh:
            sha.update(fh.read())
    res = {"protocol": "device: settle launches, then timed launches, one HIP-event interval each, median; host: wall time, median", "settle": args.settle,
           "steps": args.steps, "host_reps": args.host_reps, "warm_launches": args.warm, "window": WINDOW, "build": g.build.build_info(),
           "library": lib_record(_lib.library_path()), "smooth_sources_sha256": sha.hexdigest(), "shapes": {}}
    order = ("tx_frac_out", "count", "cmc_s", "status", "channels")

    for E, K in SHAPES:
        case = sc.synthetic(E + K, E, K, window=WINDOW, rate_gate_cycles=0.5, slips=[(e, e % K, 300) for e in range(997, E, 997)], gap_p=0.002, mask_p=0.002)
        cfg = sc.smooth_cfg(**case.config())
        h_in = dict(zip(sc.ARRAYS, [np.ascontiguousarray(v) for v in case.arrays()]))
        d_in = {k: torch.from_numpy(v).to(dev) for k, v in h_in.items()}
        sizes = {n: ((K * 16, np.uint8) if n == "channels" else (E * K, sc.OUT_DTYPES[n])) for n in order}
        d_out = {k: torch.zeros(v[0], dtype=getattr(torch, np.dtype(v[1]).name), device=dev) for k, v in sizes.items()}
        h_out = {k: np.zeros(v[0], v[1]) for k, v in sizes.items()}
        p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

        def launch():
            rc = lib.gat_smooth_observables(ctx._h, *[p(d_in[k]) for k in sc.ARRAYS], E, K, C.byref(cfg), *[p(d_out[k]) for k in order])
            if rc != 0:
                ctx.check(rc, "gat_smooth_observables")

        def host():
            t0 = time.perf_counter()
            ctx.sync()
            h = {k: d_in[k].cpu().numpy() for k in sc.ARRAYS}
            t1 = time.perf_counter()
            rc = lib.gat_smooth_observables_host(*[h[k].ctypes.data for k in sc.ARRAYS], E, K, C.byref(cfg), *[h_out[k].ctypes.data for k in order])
            assert rc == 0, rc
            return (t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3

        launch()
        ctx.sync()
        host()
        same = all(np.array_equal(d_out[k].cpu().numpy().view(np.uint8), h_out[k].view(np.uint8)) for k in order)
        if not res["shapes"]:  # the process's first timing: bring the device up to its clocks first
            for _ in range(args.warm):
                launch()
            ctx.sync()
        ms = median_ms(ctx, launch, args.settle, args.steps)
        reps = np.array([host() for _ in range(args.host_reps)])
        copy_ms, twin_ms = float(np.median(reps[:, 0])), float(np.median(reps[:, 1]))
        chan = h_out["channels"].view(_lib.SMOOTH_CHANNEL_DTYPE)
        # inputs: two passes over 45 bytes a cell (the sum and the emit walk) and tx_frac once more; scratch: 20 bytes a cell written,
        # 36 read (C, SS, a at e, SS at e - n, C at a); outputs: 21 bytes a cell
        least = E * K * (2 * 45 + 8 + 20 + 36 + 21)
        rec = {"E": E, "K": K, "same_bits": bool(same), "measured": int(chan["measured"].sum()), "arcs": int(chan["arcs"].sum()),
               "cmc_resets": int(chan["cmc_resets"].sum()), "rate_resets": int(chan["rate_resets"].sum()), "device_ms": ms, "copy_ms": copy_ms,
               "twin_ms": twin_ms, "host_path_ms": copy_ms + twin_ms, "host_over_device": (copy_ms + twin_ms) / ms,
               "cells_per_second": E * K / (ms * 1e-3), "bytes_moved_at_least": least, "gb_per_second_at_least": least / (ms * 1e-3) / 1e9,
               "plan": smoothing_plan(E, K, window=WINDOW, rate_gate_cycles=0.5)}
        res["shapes"][f"E{E}_K{K}"] = rec
        print(json.dumps(rec), flush=True)
        del d_in, d_out

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
