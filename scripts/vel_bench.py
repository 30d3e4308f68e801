"""Timings of the velocity fix (include/gat.h gat_velocity_fix) next to what a user of the library did before it existed, on the
same observables in the same run, with scripts/fix_bench.py's protocol:

  the device call on observables and fixes in device memory -- settle launches, then timed launches, one HIP-event interval per
  launch, median; gat_position_fix on the same inputs is timed the same way beside it;
  the yardstick: a device-to-host copy of the observables, the fixes and the used set followed by the host twin
  (gat_velocity_fix_host: the same rule in plain loops, one thread) -- wall time of the two steps, each timed, median over
  `--host-reps` repetitions.

Shapes (epochs, channels), every output asked for, a synthetic constellation seen from eight sites by moving receivers
(tests/fix_cases.py, tests/vel_cases.py); the fixes and the used set are those of gat_position_fix on the device:
  (65536, 12)    a 12-channel receiver
  (65536, 64)    64 channels, about a third of them above the horizon

Per shape: ms of the device call with the plan, ms of gat_position_fix, ms of the copy and of the twin, and their ratio.  The
outputs of both paths are compared bit for bit before anything is timed.

  python scripts/vel_bench.py [--out profiles/vel/vel_bench.json] [--settle 3] [--steps 10] [--host-reps 2] [--warm 10]
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

SOURCES = ("gat_vel.hip", "gat_vel.h", "gat_vel_plan.h", "gat_vel_kernels.h", "gat_vel_api.cpp", "gat_fix.h", "gat_fix_wave.h")
SHAPES = ((65536, 12), (65536, 64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vel", "vel_bench.json"))
    ap.add_argument("--settle", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--warm", type=int, default=10)
    args = ap.parse_args()
    import torch

    import gpuacceleratedtracking_amd as g
    from gpuacceleratedtracking_amd import _lib
    from gpuacceleratedtracking_amd.positioning import fix_config
    from gpuacceleratedtracking_amd.velocity import vel_config, velocity_plan
    from tests import fix_cases as fc
    from tests import vel_cases as vc

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
           "library": lib_record(_lib.library_path()), "vel_sources_sha256": sha.hexdigest(), "shapes": {}}
    fcfg, vcfg = fix_config(), vel_config()
    fix_order = ("fixes", "sat", "resid", "sin_el", "used")
    order = ("velocities", "sat_vel", "resid")

    for E, K in SHAPES:
        moving = vc.moving(fc.case("short", 30, K, 64) if K < 30 else fc.case("mid", K, None, 64))
        idx = np.arange(E) % moving.E
        case = moving.case.tiled(E)
        ephs = np.ascontiguousarray(case.ephs)
        h_in = {"tx_ms": case.tx_ms, "tx_frac": case.tx_frac, "rx_ms": case.rx_ms, "rx_frac": case.rx_frac,
                "doppler": np.ascontiguousarray(moving.doppler[idx])}
        d_eph = torch.from_numpy(ephs.view(np.uint8).reshape(K, -1).copy()).to(dev)
        d_in = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in h_in.items()}
        fix_sizes = {"fixes": (E * 80, np.uint8), "sat": (E * K * 4, np.float64), "resid": (E * K, np.float64), "sin_el": (E * K, np.float64),
                     "used": (E * K, np.uint8)}
        d_fix = {k: torch.zeros(v[0], dtype=getattr(torch, np.dtype(v[1]).name), device=dev) for k, v in fix_sizes.items()}
        sizes = {"velocities": (E * _lib.VELOCITY_DTYPE.itemsize, np.uint8), "sat_vel": (E * K * 4, np.float64), "resid": (E * K, np.float64)}
        d_out = {k: torch.zeros(v[0], dtype=getattr(torch, np.dtype(v[1]).name), device=dev) for k, v in sizes.items()}
        h_out = {k: np.zeros(v[0], v[1]) for k, v in sizes.items()}
        p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

        def launch_fix():
            rc = lib.gat_position_fix(ctx._h, p(d_eph), *[p(d_in[k]) for k in ("tx_ms", "tx_frac", "rx_ms", "rx_frac")], None, E, K, C.byref(fcfg),
                                      *[p(d_fix[k]) for k in fix_order])
            if rc != 0:
                ctx.check(rc, "gat_position_fix")

        def launch():
            rc = lib.gat_velocity_fix(ctx._h, p(d_eph), p(d_in["tx_ms"]), p(d_in["tx_frac"]), p(d_in["doppler"]), p(d_fix["fixes"]), p(d_fix["used"]), None,
                                      E, K, C.byref(vcfg), *[p(d_out[k]) for k in order])
            if rc != 0:
                ctx.check(rc, "gat_velocity_fix")

        def host():
            t0 = time.perf_counter()
            ctx.sync()
            h = {k: d_in[k].cpu().numpy() for k in ("tx_ms", "tx_frac", "doppler")}
            h["fixes"], h["used"] = d_fix["fixes"].cpu().numpy(), d_fix["used"].cpu().numpy()
            t1 = time.perf_counter()
            rc = lib.gat_velocity_fix_host(ephs.ctypes.data, *[h[k].ctypes.data for k in ("tx_ms", "tx_frac", "doppler", "fixes", "used")], None, E, K,
                                           C.byref(vcfg), *[h_out[k].ctypes.data for k in order])
            assert rc == 0, rc
            return (t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3

        launch_fix()
        launch()
        ctx.sync()
        host()
        same = all(np.array_equal(d_out[k].cpu().numpy().view(np.uint8), h_out[k].view(np.uint8)) for k in order)
        vel = h_out["velocities"].view(_lib.VELOCITY_DTYPE)
        if not res["shapes"]:  # the process's first timing: bring the device up to its clocks first
            for _ in range(args.warm):
                launch()
            ctx.sync()
        ms = median_ms(ctx, launch, args.settle, args.steps)
        fix_ms = median_ms(ctx, launch_fix, args.settle, args.steps)
        reps = np.array([host() for _ in range(args.host_reps)])
        copy_ms, twin_ms = float(np.median(reps[:, 0])), float(np.median(reps[:, 1]))
        err = float(np.abs(np.stack([vel["vx"], vel["vy"], vel["vz"]], axis=1) - moving.v_ecef[idx]).max())
        rec = {"E": E, "K": K, "same_bits": bool(same), "good_velocities": int((vel["status"] == 0).sum()), "mean_used": float(vel["num_used"].mean()),
               "max_error_mps": err, "device_ms": ms, "position_fix_ms": fix_ms, "copy_ms": copy_ms, "twin_ms": twin_ms,
               "host_path_ms": copy_ms + twin_ms, "host_over_device": (copy_ms + twin_ms) / ms, "epochs_per_second": E / (ms * 1e-3),
               "plan": velocity_plan(E, K)}
        res["shapes"][f"E{E}_K{K}"] = rec
        print(json.dumps(rec), flush=True)
        del d_in, d_out, d_fix

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
