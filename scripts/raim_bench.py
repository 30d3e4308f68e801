"""Timings of the fix integrity call (include/gat.h gat_position_fix_raim) next to gat_position_fix on the same observables in the
same run -- what integrity costs -- and next to what a user does without the device call: a device-to-host copy of the observables
followed by the host twin (gat_position_fix_raim_host: the same rule in plain loops, one thread).

  the device calls on observables in device memory -- settle launches, then timed launches, one HIP-event interval per launch,
  median (the protocol of scripts/fix_bench.py);
  the host path: wall time of the copy and of the twin, each timed, median over `--host-reps` repetitions.

Shapes (epochs, channels) as in scripts/fix_bench.py, pseudorange noise of 3 m (tests/raim_cases.py), thresholds at p_fa = 1e-3,
every output asked for but `trial`, one round of exclusion:
  (65536, 12)    a 12-channel receiver
  (65536, 64)    64 channels, about a third of them above the horizon
each with 0 %, 1 % and 100 % of the epochs faulted: the highest satellite of the epoch a code period off.

Per shape and share: ms of both device calls and their ratio, ms of the copy and of the twin and the ratio of the host path to the
device call, the counts of detected and repaired epochs.  The outputs of device and twin are compared bit for bit before anything
is timed.

  python scripts/raim_bench.py [--out profiles/raim/raim_bench.json] [--settle 3] [--steps 10] [--host-reps 2] [--warm 10]
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

SOURCES = ("gat_raim.hip", "gat_raim.h", "gat_raim_plan.h", "gat_raim_kernels.h", "gat_raim_api.cpp", "gat_fix_wave.h", "gat_fix.h", "gat_fix_plan.h")
SHAPES = ((65536, 12), (65536, 64))
SHARES = (0.0, 0.01, 1.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raim", "raim_bench.json"))
    ap.add_argument("--settle", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--warm", type=int, default=10)
    args = ap.parse_args()
    import torch

    import gpuacceleratedtracking_amd as g
    from gpuacceleratedtracking_amd import _lib
    from gpuacceleratedtracking_amd.positioning import fix_config, raim_config, raim_plan
    from tests import fix_cases as fc
    from tests import raim_cases as rc

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
           "library": lib_record(_lib.library_path()), "raim_sources_sha256": sha.hexdigest(), "sigma_m": rc.SIGMA_M, "p_fa": rc.P_FA,
           "max_exclude": 1, "trial_iter": 8, "shapes": {}}
    cfg, rcfg = fix_config(), raim_config(rc.thresholds(), 1, 8)
    fix_order = ("fixes", "sat", "resid", "sin_el", "used")
    order = ("fixes", "integrity", "sat", "resid", "sin_el", "used")
    names = ("tx_ms", "tx_frac", "rx_ms", "rx_frac")
    warmed = False

    for E, K in SHAPES:
        base = rc.noisy(fc.case("short", 30, K, 64) if K < 30 else fc.case("mid", K, None, 64), 17).tiled(E)
        ephs = np.ascontiguousarray(base.ephs)
        d_eph = torch.from_numpy(ephs.view(np.uint8).reshape(K, -1).copy()).to(dev)
        top = np.argmax(np.where(base.tx_ms >= 0, base.sin_el, -2.0), axis=1)
        for share in SHARES:
            tx_ms = base.tx_ms.copy()
            hit = np.flatnonzero(np.arange(E) % 100 == 37) if share == 0.01 else (np.arange(E) if share == 1.0 else np.zeros(0, np.int64))
            tx_ms[hit, top[hit]] = (tx_ms[hit, top[hit]] + 1) % 604800000
            h_in = {"tx_ms": tx_ms, "tx_frac": base.tx_frac, "rx_ms": base.rx_ms, "rx_frac": base.rx_frac}
            d_in = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in h_in.items()}
            sizes = {"fixes": (E * 80, np.uint8), "integrity": (E * 64, np.uint8), "sat": (E * K * 4, np.float64), "resid": (E * K, np.float64),
                     "sin_el": (E * K, np.float64), "used": (E * K, np.uint8)}
            d_out = {k: torch.zeros(v[0], dtype=getattr(torch, np.dtype(v[1]).name), device=dev) for k, v in sizes.items()}
            h_out = {k: np.zeros(v[0], v[1]) for k, v in sizes.items()}

            def launch():
                rc_ = lib.gat_position_fix_raim(ctx._h, C.c_void_p(d_eph.data_ptr()), *[C.c_void_p(d_in[k].data_ptr()) for k in names], None, E, K,
                                                C.byref(cfg), C.byref(rcfg), *[C.c_void_p(d_out[k].data_ptr()) for k in order], None)
                if rc_ != 0:
                    ctx.check(rc_, "gat_position_fix_raim")

            def launch_fix():
                rc_ = lib.gat_position_fix(ctx._h, C.c_void_p(d_eph.data_ptr()), *[C.c_void_p(d_in[k].data_ptr()) for k in names], None, E, K,
                                           C.byref(cfg), *[C.c_void_p(d_out[k].data_ptr()) for k in fix_order])
                if rc_ != 0:
                    ctx.check(rc_, "gat_position_fix")

            def host():
                t0 = time.perf_counter()
                ctx.sync()
                h = {k: d_in[k].cpu().numpy() for k in names}
                t1 = time.perf_counter()
                rc_ = lib.gat_position_fix_raim_host(ephs.ctypes.data, *[h[k].ctypes.data for k in names], None, E, K, C.byref(cfg), C.byref(rcfg),
                                                     *[h_out[k].ctypes.data for k in order], None)
                assert rc_ == 0, rc_
                return (t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3

            launch()
            ctx.sync()
            first = host()
            same = all(np.array_equal(d_out[k].cpu().numpy().view(np.uint8), h_out[k].view(np.uint8)) for k in order)
            fixes, integ = h_out["fixes"].view(_lib.FIX_DTYPE), h_out["integrity"].view(_lib.INTEGRITY_DTYPE)
            if not warmed:  # the process's first timing: bring the device up to its clocks first
                for _ in range(args.warm):
                    launch()
                ctx.sync()
                warmed = True
            ms = median_ms(ctx, launch, args.settle, args.steps)
            fix_ms = median_ms(ctx, launch_fix, args.settle, args.steps)
            reps = np.array([first] + [host() for _ in range(args.host_reps - 1)])
            copy_ms, twin_ms = float(np.median(reps[:, 0])), float(np.median(reps[:, 1]))
            err = np.linalg.norm(np.stack([fixes["x"], fixes["y"], fixes["z"]], axis=1) - base.truth_xyz, axis=1)
            rec = {"E": E, "K": K, "faulted_share": share, "faulted_epochs": int(len(hit)), "same_bits": bool(same),
                   "detected": int(((integ["status"] & _lib.GAT_RAIM_DETECTED) != 0).sum()),
                   "excluded": int(((integ["status"] & _lib.GAT_RAIM_EXCLUDED) != 0).sum()),
                   "right_channel": int((integ["excluded"][hit, 0] == top[hit]).sum()) if len(hit) else 0,
                   "unresolved": int(((integ["status"] & _lib.GAT_RAIM_UNRESOLVED) != 0).sum()), "mean_used": float(fixes["num_used"].mean()),
                   "mean_iterations": float(fixes["iterations"].mean()), "max_error_m": float(err.max()), "raim_device_ms": ms, "fix_device_ms": fix_ms,
                   "raim_over_fix": ms / fix_ms, "copy_ms": copy_ms, "twin_ms": twin_ms, "host_path_ms": copy_ms + twin_ms,
                   "host_over_device": (copy_ms + twin_ms) / ms, "epochs_per_second": E / (ms * 1e-3), "plan": raim_plan(E, K, thresholds=rc.thresholds())}
            res["shapes"][f"E{E}_K{K}_faulted{share:g}"] = rec
            print(json.dumps(rec), flush=True)
            del d_in, d_out

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
