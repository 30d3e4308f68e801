"""Timings of the position fix (include/gat.h gat_position_fix) next to what a user of the library did before it existed, on the
same observables in the same run:

  the device call on observables in device memory -- settle launches, then timed launches, one HIP-event interval per launch, median
  (the protocol of scripts/nav_bench.py);
  the yardstick: a device-to-host copy of the observables followed by the host twin (gat_position_fix_host: the same rule in plain
  loops, one thread) -- wall time of the two steps, each timed, median over `--host-reps` repetitions.

Shapes (epochs, channels), every output asked for, a synthetic constellation seen from eight sites (tests/fix_cases.py):
  (65536, 12)    a 12-channel receiver
  (65536, 64)    the monitor's headline shape: 64 channels, about a third of them above the horizon

Per shape: ms of the device call with the plan, ms of the copy and of the twin, and their ratio.  The outputs of both paths are
compared bit for bit before anything is timed.

  python scripts/fix_bench.py [--out profiles/fix/fix_bench.json] [--settle 3] [--steps 10] [--host-reps 2] [--warm 10]
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

SOURCES = ("gat_fix.hip", "gat_fix.h", "gat_fix_plan.h", "gat_fix_kernels.h", "gat_fix_api.cpp")
SHAPES = ((65536, 12), (65536, 64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fix", "fix_bench.json"))
    ap.add_argument("--settle", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--warm", type=int, default=10)
    args = ap.parse_args()
    import torch

    import gpuacceleratedtracking_amd as g
    from gpuacceleratedtracking_amd import _lib
    from gpuacceleratedtracking_amd.positioning import fix_config, position_plan
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
           "library": lib_record(_lib.library_path()), "fix_sources_sha256": sha.hexdigest(), "shapes": {}}
    cfg = fix_config()
    order = ("fixes", "sat", "resid", "sin_el", "used")

    for E, K in SHAPES:
        case = (fc.case("short", 30, K, 64) if K < 30 else fc.case("mid", K, None, 64)).tiled(E)
        ephs = np.ascontiguousarray(case.ephs)
        h_in = {"tx_ms": case.tx_ms, "tx_frac": case.tx_frac, "rx_ms": case.rx_ms, "rx_frac": case.rx_frac}
        d_eph = torch.from_numpy(ephs.view(np.uint8).reshape(K, -1).copy()).to(dev)
        d_in = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in h_in.items()}
        sizes = {"fixes": (E * 80, np.uint8), "sat": (E * K * 4, np.float64), "resid": (E * K, np.float64), "sin_el": (E * K, np.float64),
                 "used": (E * K, np.uint8)}
        d_out = {k: torch.zeros(v[0], dtype=getattr(torch, np.dtype(v[1]).name), device=dev) for k, v in sizes.items()}
        h_out = {k: np.zeros(v[0], v[1]) for k, v in sizes.items()}
        names = ("tx_ms", "tx_frac", "rx_ms", "rx_frac")

        def launch():
            rc = lib.gat_position_fix(ctx._h, C.c_void_p(d_eph.data_ptr()), *[C.c_void_p(d_in[k].data_ptr()) for k in names], None, E, K, C.byref(cfg),
                                      *[C.c_void_p(d_out[k].data_ptr()) for k in order])
            if rc != 0:
                ctx.check(rc, "gat_position_fix")

        def host():
            t0 = time.perf_counter()
            ctx.sync()
            h = {k: d_in[k].cpu().numpy() for k in names}
            t1 = time.perf_counter()
            rc = lib.gat_position_fix_host(ephs.ctypes.data, *[h[k].ctypes.data for k in names], None, E, K, C.byref(cfg),
                                           *[h_out[k].ctypes.data for k in order])
            assert rc == 0, rc
            return (t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3

        launch()
        ctx.sync()
        host()
        same = all(np.array_equal(d_out[k].cpu().numpy().view(np.uint8), h_out[k].view(np.uint8)) for k in order)
        fixes = h_out["fixes"].view(_lib.FIX_DTYPE)
        if not res["shapes"]:  # the process's first timing: bring the device up to its clocks first
            for _ in range(args.warm):
                launch()
            ctx.sync()
        ms = median_ms(ctx, launch, args.settle, args.steps)
        reps = np.array([host() for _ in range(args.host_reps)])
        copy_ms, twin_ms = float(np.median(reps[:, 0])), float(np.median(reps[:, 1]))
        err = float(np.linalg.norm(np.stack([fixes["x"], fixes["y"], fixes["z"]], axis=1) - case.truth_xyz, axis=1).max())
        rec = {"E": E, "K": K, "same_bits": bool(same), "good_fixes": int((fixes["status"] == 0).sum()), "mean_used": float(fixes["num_used"].mean()),
               "mean_iterations": float(fixes["iterations"].mean()), "max_error_m": err, "device_ms": ms, "copy_ms": copy_ms, "twin_ms": twin_ms,
               "host_path_ms": copy_ms + twin_ms, "host_over_device": (copy_ms + twin_ms) / ms, "epochs_per_second": E / (ms * 1e-3),
               "plan": position_plan(E, K)}
        res["shapes"][f"E{E}_K{K}"] = rec
        print(json.dumps(rec), flush=True)
        del d_in, d_out

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
