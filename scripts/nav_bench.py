"""Timings of the navigation data layer (include/gat.h gat_nav_decode) next to what a user of the library did before it existed, on
the same symbols in the same run:

  the device call on the monitor's symbols where gat_track_monitor left them -- settle launches, then timed launches, one HIP-event
  interval per launch, median (the protocol of scripts/monitor_bench.py);
  the yardstick: a device-to-host copy of sym_re followed by the host twin (gat_nav_decode_host: the same rule in plain loops, one
  thread) -- wall time of the two steps, each timed, median over `--host-reps` repetitions.

Shapes (K, symbols), both formats, every output asked for, streams of back-to-back frames at 7 dB Es/N0 behind a junk prefix:
  (12, 1000)     a 12-channel receiver: 20 s of L1 C/A bits, 5 s of L5 symbols
  (64, 6553)     64 channels over 65 s of signal: 131 s of L1 C/A bits, 33 s of L5 symbols

Per shape and format: ms of the device call with the plan's workgroups and scratch, ms of the copy and of the twin, and their ratio.
The outputs of both paths are compared bit for bit before anything is timed.

  python scripts/nav_bench.py [--out profiles/nav/nav_bench.json] [--settle 5] [--steps 20] [--host-reps 3] [--warm 50]
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

SOURCES = ("gat_nav.hip", "gat_nav.h", "gat_nav_plan.h", "gat_nav_kernels.h", "gat_nav_api.cpp")
SHAPES = ((12, 1000), (64, 6553))
SIGMA = float(np.sqrt(1.0 / (2.0 * 10.0 ** 0.7)))  # Es/N0 = 7 dB on unit symbols


def symbols(g, fmt, K, n, rng):
    """[K, n] symbols: per channel a junk prefix, then frames back to back with consecutive TOW counts, noisy; eight distinct streams"""
    rows = []
    for k in range(min(K, 8)):
        bits_needed = n // (2 if fmt else 1)
        parts = [rng.integers(0, 2, 17 + 31 * k)]
        f = 0
        while sum(len(p) for p in parts) < bits_needed:
            parts.append(g.cnav_message(3 + k, 10 + f % 4, 600 + f, rng.integers(0, 2, 239)) if fmt
                         else g.lnav_subframe(600 + f, f % 5 + 1, rng.integers(0, 2, 190)))
            f += 1
        bits = np.concatenate(parts)[:bits_needed]
        s = (g.cnav_fec_encode(bits) if fmt else bits).astype(np.float64)
        x = np.zeros(n)
        x[:len(s)] = 1.0 - 2.0 * s
        rows.append((x + SIGMA * rng.standard_normal(n)) * (-1.0 if k & 1 else 1.0))
    return np.stack([rows[k % len(rows)] for k in range(K)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nav", "nav_bench.json"))
    ap.add_argument("--settle", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--warm", type=int, default=50)
    args = ap.parse_args()
    import torch

    import gpuacceleratedtracking_amd as g
    from gpuacceleratedtracking_amd import _lib
    from gpuacceleratedtracking_amd.navigation import nav_config, nav_plan

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
           "library": lib_record(_lib.library_path()), "nav_sources_sha256": sha.hexdigest(), "shapes": {}}
    rng = np.random.default_rng(1)

    for K, n in SHAPES:
        for fmt, name in ((_lib.GAT_NAV_LNAV, "lnav"), (_lib.GAT_NAV_CNAV, "cnav")):
            cfg = nav_config(fmt, n, None, 1)
            P, F = (2 if fmt else 1), int(cfg.max_frames)
            sym = torch.from_numpy(symbols(g, fmt, K, n, rng)).to(dev)
            sizes = {"channels": (K * 8, np.int32), "frames": (K * F * 14, np.int32), "decoded": (K * P * (n // P), np.uint8), "path_metric": (K * P, np.int32)}
            order = ("channels", "frames", "decoded", "path_metric")
            d_out = {k: torch.zeros(v[0], dtype=getattr(torch, np.dtype(v[1]).name), device=dev) for k, v in sizes.items()}
            h_out = {k: np.zeros(v[0], v[1]) for k, v in sizes.items()}

            def launch():
                rc = lib.gat_nav_decode(ctx._h, C.c_void_p(sym.data_ptr()), None, K, C.byref(cfg), *[C.c_void_p(d_out[k].data_ptr()) for k in order])
                if rc != 0:
                    ctx.check(rc, "gat_nav_decode")

            def host():
                t0 = time.perf_counter()
                ctx.sync()
                h = sym.cpu().numpy()
                t1 = time.perf_counter()
                rc = lib.gat_nav_decode_host(h.ctypes.data, None, K, C.byref(cfg), *[h_out[k].ctypes.data for k in order])
                assert rc == 0, rc
                return (t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3

            launch()
            ctx.sync()
            host()
            same = all(np.array_equal(d_out[k].cpu().numpy(), h_out[k]) for k in order)
            chans = h_out["channels"].view(_lib.NAV_CHANNEL_DTYPE)
            if not res["shapes"]:  # the process's first timing: bring the device up to its clocks first
                for _ in range(args.warm):
                    launch()
                ctx.sync()
            ms = median_ms(ctx, launch, args.settle, args.steps)
            reps = np.array([host() for _ in range(args.host_reps)])
            copy_ms, twin_ms = float(np.median(reps[:, 0])), float(np.median(reps[:, 1]))
            rec = {"format": name, "K": K, "symbols": n, "max_frames": F, "symbol_bytes": 8 * K * n, "same_bits": bool(same),
                   "synced_channels": int((chans["frame_offset"] >= 0).sum()), "frames_found": int(chans["score"].sum()),
                   "device_ms": ms, "copy_ms": copy_ms, "twin_ms": twin_ms, "host_path_ms": copy_ms + twin_ms, "host_over_device": (copy_ms + twin_ms) / ms,
                   "plan": nav_plan(K, n, fmt)}
            res["shapes"][f"{name}_K{K}_S{n}"] = rec
            print(json.dumps(rec), flush=True)
            del sym, d_out

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
