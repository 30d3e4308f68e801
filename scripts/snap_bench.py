"""Timings of the snapshot fix (include/gat.h gat_snapshot_fix) next to what a user of the library had without it, on the same
inputs in the same run, with scripts/smooth_bench.py's protocol:

  the device call on inputs in device memory -- settle launches, then timed launches, one HIP-event interval per launch, median;
  the yardstick: a device-to-host copy of the inputs followed by the host twin (gat_snapshot_fix_host: the same rule in plain
  loops, one thread) -- wall time of the two steps, each timed, median over `--host-reps` repetitions;
  as context, gat_position_fix on the same shapes (the transmit times the snapshot fix hands on), timed the same way: what the
  satellite evaluated again in every iteration costs.

Shapes (epochs, channels), every output asked for, priors 30 km and clocks 20 s off (tests/snap_cases.py, tiled):
  (65536, 12)    a 12-channel receiver
  (65536, 64)    64 channels

The outputs of the device call and of the twin are compared bit for bit before anything is timed.

  python scripts/snap_bench.py [--out profiles/snap/snap_bench.json] [--settle 3] [--steps 10] [--host-reps 2] [--warm 10]
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

SOURCES = ("gat_snap.hip", "gat_snap.h", "gat_snap_plan.h", "gat_snap_kernels.h", "gat_snap_api.cpp")
SHAPES = ((65536, 12), (65536, 64))
OUTPUTS = (("tx_ms", np.int32, True), ("rx_ms_out", np.int32, False), ("n_ms", np.int32, True), ("resid", np.float64, True),
           ("sin_el", np.float64, True), ("used", np.uint8, True))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "snap", "snap_bench.json"))
    ap.add_argument("--settle", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--warm", type=int, default=10)
    args = ap.parse_args()
    import torch

    import gpuacceleratedtracking_amd as g
    from gpuacceleratedtracking_amd import _lib
    from gpuacceleratedtracking_amd.positioning import fix_config
    from gpuacceleratedtracking_amd.snapshot import snap_config, snapshot_plan
    from tests import snap_cases as sc

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
           "library": lib_record(_lib.library_path()), "snap_sources_sha256": sha.hexdigest(), "shapes": {}}
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    for E, K in SHAPES:
        base = sc.case("short", 30, 12, 8, check=False) if K == 12 else sc.case("mid", 64, None, 8, check=False)
        case = base.tiled(E)
        cfg, fcfg = snap_config(), fix_config(init_xyz=tuple(case.prior[0]))
        names = ("ephs", "code_frac", "rx_ms", "rx_frac", "prior")
        h_in = dict(zip(names, [np.ascontiguousarray(v) for v in case.args()]))
        d_in = {k: torch.from_numpy(v.view(np.uint8) if k == "ephs" else v).to(dev) for k, v in h_in.items()}
        d_fix = torch.zeros(E * _lib.SNAP_FIX_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        h_fix = np.zeros(E, _lib.SNAP_FIX_DTYPE)
        d_out = {n: torch.zeros(E * K if cells else E, dtype=getattr(torch, np.dtype(t).name), device=dev) for n, t, cells in OUTPUTS}
        h_out = {n: np.zeros(E * K if cells else E, t) for n, t, cells in OUTPUTS}
        d_pfix = torch.zeros(E * _lib.FIX_DTYPE.itemsize, dtype=torch.uint8, device=dev)

        def launch():
            rc = lib.gat_snapshot_fix(ctx._h, *[p(d_in[k]) for k in names], None, E, K, C.byref(cfg), p(d_fix), *[p(d_out[n]) for n, _, _ in OUTPUTS])
            if rc != 0:
                ctx.check(rc, "gat_snapshot_fix")

        def launch_fix():  # the position fix on the times the snapshot fix handed on, every output but sat
            rc = lib.gat_position_fix(ctx._h, p(d_in["ephs"]), p(d_out["tx_ms"]), p(d_in["code_frac"]), p(d_out["rx_ms_out"]), p(d_in["rx_frac"]), None, E,
                                      K, C.byref(fcfg), p(d_pfix), None, p(d_out["resid"]), p(d_out["sin_el"]), p(d_out["used"]))
            if rc != 0:
                ctx.check(rc, "gat_position_fix")

        def host():
            t0 = time.perf_counter()
            ctx.sync()
            h = {k: d_in[k].cpu().numpy() for k in names}
            t1 = time.perf_counter()
            rc = lib.gat_snapshot_fix_host(*[h[k].ctypes.data for k in names], None, E, K, C.byref(cfg), h_fix.ctypes.data,
                                           *[h_out[n].ctypes.data for n, _, _ in OUTPUTS])
            assert rc == 0, rc
            return (t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3

        launch()
        ctx.sync()
        host()
        same = d_fix.cpu().numpy().tobytes() == h_fix.tobytes() and all(d_out[n].cpu().numpy().tobytes() == h_out[n].tobytes() for n, _, _ in OUTPUTS)
        if not res["shapes"]:  # the process's first timing: bring the device up to its clocks first
            for _ in range(args.warm):
                launch()
            ctx.sync()
        ms = median_ms(ctx, launch, args.settle, args.steps)
        fix_ms = median_ms(ctx, launch_fix, args.settle, args.steps)
        launch()  # the position fix wrote resid, sin_el and used: leave the snapshot fix's
        ctx.sync()
        reps = np.array([host() for _ in range(args.host_reps)])
        copy_ms, twin_ms = float(np.median(reps[:, 0])), float(np.median(reps[:, 1]))
        rec = {"E": E, "K": K, "same_bits": bool(same), "status_zero": int((h_fix["status"] == 0).sum()), "iterations_mean": float(h_fix["iterations"].mean()),
               "used_mean": float(h_fix["num_used"].mean()), "device_ms": ms, "position_fix_ms": fix_ms, "snapshot_over_position_fix": ms / fix_ms,
               "copy_ms": copy_ms, "twin_ms": twin_ms, "host_path_ms": copy_ms + twin_ms, "host_over_device": (copy_ms + twin_ms) / ms,
               "epochs_per_second": E / (ms * 1e-3), "plan": snapshot_plan(E, K)}
        res["shapes"][f"E{E}_K{K}"] = rec
        print(json.dumps(rec), flush=True)
        del d_in, d_out

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
