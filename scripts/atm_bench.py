"""Timings of the range corrections (include/gat.h gat_range_corrections) next to what a user of the library did before they
existed, on the same observables in the same run, with scripts/vel_bench.py's protocol:

  the device call on observables and fixes in device memory -- settle launches, then timed launches, one HIP-event interval per
  launch, median; gat_position_fix on the same inputs is timed the same way beside it;
  the yardstick: a device-to-host copy of the observables and the fixes followed by the host twin (gat_range_corrections_host:
  the same rule in plain loops, one thread) -- wall time of the two steps, each timed, median over `--host-reps` repetitions.

Shapes (epochs, channels), every output asked for, ionosphere and troposphere on, a zenith array, a synthetic constellation seen
from eight sites (tests/fix_cases.py); the fixes are those of gat_position_fix on the device:
  (65536, 12)    a 12-channel receiver
  (65536, 64)    64 channels, about a third of them above the horizon

Per shape: ms of the device call with the plan, ms of gat_position_fix, ms of the copy and of the twin, and their ratio.  The
outputs of both paths are compared bit for bit before anything is timed.

  python scripts/atm_bench.py [--out profiles/atm/atm_bench.json] [--settle 3] [--steps 10] [--host-reps 2] [--warm 10]
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

SOURCES = ("gat_atm.hip", "gat_atm.h", "gat_atm_plan.h", "gat_atm_kernels.h", "gat_atm_api.cpp", "gat_fix.h", "gat_vel.h")
SHAPES = ((65536, 12), (65536, 64))
ALPHA = (12 * 2.0 ** -30, 2 * 2.0 ** -27, -1 * 2.0 ** -24, -1 * 2.0 ** -24)
BETA = (44 * 2.0 ** 11, 8 * 2.0 ** 14, -1 * 2.0 ** 16, -6 * 2.0 ** 16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "atm", "atm_bench.json"))
    ap.add_argument("--settle", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--warm", type=int, default=10)
    args = ap.parse_args()
    import torch

    import gpuacceleratedtracking_amd as g
    from gpuacceleratedtracking_amd import _lib
    from gpuacceleratedtracking_amd.atmosphere import atm_config, atmosphere_plan
    from gpuacceleratedtracking_amd.positioning import fix_config
    from tests import fix_cases as fc

    lib = g.load_library()
    ctx = g.get_context()
    dev = ctx.device
    csrc = os.path.join(ROOT, "gpuacceleratedtracking_amd", "csrc")
    sha = hashlib.sha256()
    for name in SOURCES:
        with open(os.path.join(csrc, name), "rb") as fh:
            sha.update(fh.read())
    res = {"protocol": "device: settle launches, then timed launches, one HIP-event interval each, median; host: wall time, median", "settle": args.settle,
           "steps": args.steps, "host_reps": args.host_reps, "warm_launches": args.warm, "build": g.build.build_info(),
           "library": lib_record(_lib.library_path()), "atm_sources_sha256": sha.hexdigest(), "shapes": {}}
    fcfg = fix_config()
    acfg = atm_config(g.Klobuchar(ALPHA, BETA), True)
    fix_order = ("fixes", "sat", "resid", "sin_el", "used")
    order = ("tx_frac_out", "delay", "geom", "channel_status", "epoch_status")

    for E, K in SHAPES:
        case = (fc.case("short", 30, K, 64) if K < 30 else fc.case("mid", K, None, 64)).tiled(E)
        ephs = np.ascontiguousarray(case.ephs)
        rng = np.random.default_rng(E + K)
        h_in = {"tx_ms": case.tx_ms, "tx_frac": case.tx_frac, "rx_ms": case.rx_ms, "rx_frac": case.rx_frac,
                "zenith": np.stack([rng.uniform(2.0, 2.4, E), rng.uniform(0.02, 0.3, E)], axis=1)}
        d_eph = torch.from_numpy(ephs.view(np.uint8).reshape(K, -1).copy()).to(dev)
        d_in = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in h_in.items()}
        fix_sizes = {"fixes": (E * 80, np.uint8), "sat": (E * K * 4, np.float64), "resid": (E * K, np.float64), "sin_el": (E * K, np.float64),
                     "used": (E * K, np.uint8)}
        d_fix = {k: torch.zeros(v[0], dtype=getattr(torch, np.dtype(v[1]).name), device=dev) for k, v in fix_sizes.items()}
        sizes = {"tx_frac_out": (E * K, np.float64), "delay": (E * K * 2, np.float64), "geom": (E * K * 3, np.float64), "channel_status": (E * K, np.uint8),
                 "epoch_status": (E, np.int32)}
        d_out = {k: torch.zeros(v[0], dtype=getattr(torch, np.dtype(v[1]).name), device=dev) for k, v in sizes.items()}
        h_out = {k: np.zeros(v[0], v[1]) for k, v in sizes.items()}
        times = ("tx_ms", "tx_frac", "rx_ms", "rx_frac")
        p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

        def launch_fix():
            rc = lib.gat_position_fix(ctx._h, p(d_eph), *[p(d_in[k]) for k in times], None, E, K, C.byref(fcfg), *[p(d_fix[k]) for k in fix_order])
            if rc != 0:
                ctx.check(rc, "gat_position_fix")

        def launch():
            rc = lib.gat_range_corrections(ctx._h, p(d_eph), *[p(d_in[k]) for k in times], p(d_fix["fixes"]), p(d_in["zenith"]), E, K, C.byref(acfg),
                                           *[p(d_out[k]) for k in order])
            if rc != 0:
                ctx.check(rc, "gat_range_corrections")

        def host():
            t0 = time.perf_counter()
            ctx.sync()
            h = {k: d_in[k].cpu().numpy() for k in times + ("zenith",)}
            h["fixes"] = d_fix["fixes"].cpu().numpy()
            t1 = time.perf_counter()
            rc = lib.gat_range_corrections_host(ephs.ctypes.data, *[h[k].ctypes.data for k in times + ("fixes", "zenith")], E, K, C.byref(acfg),
                                                *[h_out[k].ctypes.data for k in order])
            assert rc == 0, rc
            return (t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3

        launch_fix()
        launch()
        ctx.sync()
        host()
        same = all(np.array_equal(d_out[k].cpu().numpy().view(np.uint8), h_out[k].view(np.uint8)) for k in order)
        if not res["shapes"]:  # the process's first timing: bring the device up to its clocks first
            for _ in range(args.warm):
                launch()
            ctx.sync()
        ms = median_ms(ctx, launch, args.settle, args.steps)
        fix_ms = median_ms(ctx, launch_fix, args.settle, args.steps)
        reps = np.array([host() for _ in range(args.host_reps)])
        copy_ms, twin_ms = float(np.median(reps[:, 0])), float(np.median(reps[:, 1]))
        corrected = h_out["channel_status"] == _lib.GAT_ATM_CH_CORRECTED
        d = h_out["delay"].reshape(-1, 2).sum(axis=1)
        rec = {"E": E, "K": K, "same_bits": bool(same), "corrected_channels": int(corrected.sum()), "counting_channels": int((h_out["channel_status"] != 0).sum()),
               "epochs_with_a_frame": int((h_out["epoch_status"] == 0).sum()), "mean_delay_m": float(d[corrected].mean()), "max_delay_m": float(d.max()),
               "device_ms": ms, "position_fix_ms": fix_ms, "copy_ms": copy_ms, "twin_ms": twin_ms, "host_path_ms": copy_ms + twin_ms,
               "host_over_device": (copy_ms + twin_ms) / ms, "cells_per_second": E * K / (ms * 1e-3), "plan": atmosphere_plan(E, K)}
        res["shapes"][f"E{E}_K{K}"] = rec
        print(json.dumps(rec), flush=True)
        del d_in, d_out, d_fix

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
