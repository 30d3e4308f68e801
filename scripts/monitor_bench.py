"""Timings of the tracking monitor (include/gat.h gat_track_monitor) next to what a user of the library did before it existed, on
the same accumulators in the same run:

  the device call on the accumulator history where gat_tracking_run left it -- settle launches, then timed launches, one HIP-event
  interval per launch, median (the protocol of scripts/spectrum_bench.py);
  the yardstick: a device-to-host copy of both accumulator planes followed by the host twin (gat_track_monitor_host: the same rule
  in plain loops, one thread) -- wall time of the two steps, each timed, median over `--host-reps` repetitions.

Shapes (B, K, M), L = 3 taps, GPS L1 C/A symbols of 20 blocks, windows of 20 blocks, every output asked for:
  (1000, 12, 4)     one second of a 12-channel, 4-antenna receiver
  (65536, 64, 16)   a long history of a large array (1.6 GB of accumulators)

Per shape: ms of the device call with the plan's workgroups and scratch, ms of the copy and of the twin, and their ratio.  The
outputs of both paths are compared bit for bit before anything is timed.

  python scripts/monitor_bench.py [--out profiles/monitor/monitor_bench.json] [--settle 5] [--steps 20] [--host-reps 3] [--warm 50]
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

SOURCES = ("gat_mon.hip", "gat_mon.h", "gat_mon_plan.h", "gat_mon_kernels.h", "gat_mon_api.cpp")
SHAPES = ((1000, 12, 4), (65536, 64, 16))
L, PROMPT, W, PD = 3, 1, 20, 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "monitor", "monitor_bench.json"))
    ap.add_argument("--settle", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--warm", type=int, default=50)
    args = ap.parse_args()
    import torch

    import gpuacceleratedtracking_amd as g
    from gpuacceleratedtracking_amd import _lib
    from gpuacceleratedtracking_amd.monitor import monitor_config, monitor_plan

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
           "library": lib_record(_lib.library_path()), "monitor_sources_sha256": sha.hexdigest(), "shapes": {}}
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    cfg = monitor_config(L, PROMPT, W, np.ones(PD, np.int8), None, 0)

    for B, K, M in SHAPES:
        n = K * L * M
        NW, cap = (B + W - 1) // W, B // PD
        acc = [torch.randn((B, K, L, M), generator=gen, device=dev, dtype=torch.float32) for _ in range(2)]
        sizes = {"windows": K * NW * 6, "energy": K * PD, "channels": K * 4, "sym_re": K * cap, "sym_im": K * cap, "sym_wbp": K * cap}
        d_out = {k: torch.zeros(v, dtype=torch.float64, device=dev) for k, v in sizes.items()}
        h_out = {k: np.zeros(v) for k, v in sizes.items()}
        order = ("windows", "energy", "channels", "sym_re", "sym_im", "sym_wbp")

        def launch():
            rc = lib.gat_track_monitor(ctx._h, C.c_void_p(acc[0].data_ptr()), C.c_void_p(acc[1].data_ptr()), n, B, K, M, C.byref(cfg), None, None, None, None,
                                       *[C.c_void_p(d_out[k].data_ptr()) for k in order])
            if rc != 0:
                ctx.check(rc, "gat_track_monitor")

        def host():
            t0 = time.perf_counter()
            ctx.sync()
            h = [a.cpu().numpy() for a in acc]
            t1 = time.perf_counter()
            rc = lib.gat_track_monitor_host(h[0].ctypes.data, h[1].ctypes.data, n, B, K, M, C.byref(cfg), None, None, None, None,
                                            *[h_out[k].ctypes.data for k in order])
            assert rc == 0, rc
            return (t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3

        launch()
        ctx.sync()
        host()
        same = all(np.array_equal(d_out[k].cpu().numpy().view(np.int64), h_out[k].view(np.int64)) for k in order)
        if not res["shapes"]:  # the process's first timing: bring the device up to its clocks first
            for _ in range(args.warm):
                launch()
            ctx.sync()
        ms = median_ms(ctx, launch, args.settle, args.steps)
        reps = np.array([host() for _ in range(args.host_reps)])
        copy_ms, twin_ms = float(np.median(reps[:, 0])), float(np.median(reps[:, 1]))
        rec = {"B": B, "K": K, "M": M, "L": L, "window_blocks": W, "symbol_blocks": PD, "accumulator_bytes": 8 * B * n, "same_bits": bool(same),
               "device_ms": ms, "copy_ms": copy_ms, "twin_ms": twin_ms, "host_path_ms": copy_ms + twin_ms, "host_over_device": (copy_ms + twin_ms) / ms,
               "plan": monitor_plan(B, K, M, L, PROMPT, W, np.ones(PD, np.int8))}
        res["shapes"][f"B{B}_K{K}_M{M}"] = rec
        print(json.dumps(rec), flush=True)
        del acc, d_out

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
