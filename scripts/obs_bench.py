"""Timings of the observables (include/gat.h gat_observables) next to what a user of the library did before they existed, on the
same history in the same run:

  the device call on a history in device memory -- settle launches, then timed launches, one HIP-event interval per launch, median
  (the protocol of scripts/fix_bench.py);
  the yardstick: a device-to-host copy of the history followed by the host twin (gat_observables_host: the same rule in plain
  loops, one thread) -- wall time of the two steps, each timed, median over `--host-reps` repetitions;
  the read-only kernel (gat_debug_read_stream, best variant) over the history's bytes in the same run: the call reads the history
  twice (the sums, then the epochs), so its time is set against two such reads.

Shapes (blocks, channels), every output asked for, histories of tests/obs_cases.py with wraps of 0, 1 and 2 periods and Dopplers of
both signs, an epoch every 20 blocks and at every block:
  (65536, 12)    a 12-channel receiver, 65.5 s
  (65536, 64)    the monitor's headline shape

Per shape and stride: ms of the device call with the plan, ms of the copy and of the twin, their ratio, the bytes of the history and
the read ceiling.  The outputs of both paths are compared bit for bit before anything is timed.

  python scripts/obs_bench.py [--out profiles/obs/obs_bench.json] [--settle 3] [--steps 10] [--host-reps 2] [--warm 10]
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

SOURCES = ("gat_obs.hip", "gat_obs.h", "gat_obs_plan.h", "gat_obs_kernels.h", "gat_obs_api.cpp")
SHAPES = ((65536, 12), (65536, 64))
STRIDES = (20, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "obs", "obs_bench.json"))
    ap.add_argument("--settle", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--warm", type=int, default=10)
    args = ap.parse_args()
    import torch

    import gpuacceleratedtracking_amd as g
    from gpuacceleratedtracking_amd import _lib
    from gpuacceleratedtracking_amd.observables import OUTPUTS, obs_config, observables_plan
    from tests import obs_cases as oc

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
           "library": lib_record(_lib.library_path()), "obs_sources_sha256": sha.hexdigest(), "shapes": {}}
    dtypes = {"tx_ms": np.int32, "rx_ms": np.int32, "carrier_cycles": np.int64, "channels": np.uint8}

    for B, K in SHAPES:
        h, mon, nav, frames, _ = oc.standard(B, K, frame_lead=1000)
        hist = np.ascontiguousarray(h.records)
        as_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)  # noqa: E731
        d_hist, d_mon, d_nav, d_frames = as_dev(hist), as_dev(mon), as_dev(nav), as_dev(frames)
        for stride in STRIDES:
            E = B // stride + 1
            kw = oc.base_config(max_frames=frames.shape[1], epoch_stride=stride)
            cfg = obs_config(**kw)
            sizes = {n: (E if n in ("rx_ms", "rx_frac") else K * 32 if n == "channels" else E * K, dtypes.get(n, np.float64)) for n in OUTPUTS}
            d_out = {n: torch.zeros(s[0], dtype=getattr(torch, np.dtype(s[1]).name), device=dev) for n, s in sizes.items()}
            h_out = {n: np.zeros(s[0], s[1]) for n, s in sizes.items()}

            def launch():
                rc = lib.gat_observables(ctx._h, C.c_void_p(d_hist.data_ptr()), C.c_void_p(d_mon.data_ptr()), C.c_void_p(d_nav.data_ptr()),
                                         C.c_void_p(d_frames.data_ptr()), B, K, E, C.byref(cfg), *[C.c_void_p(d_out[n].data_ptr()) for n in OUTPUTS])
                if rc != 0:
                    ctx.check(rc, "gat_observables")

            def host():
                t0 = time.perf_counter()
                ctx.sync()
                hh = d_hist.cpu().numpy()
                t1 = time.perf_counter()
                rc = lib.gat_observables_host(hh.ctypes.data, mon.ctypes.data, nav.ctypes.data, frames.ctypes.data, B, K, E, C.byref(cfg),
                                              *[h_out[n].ctypes.data for n in OUTPUTS])
                assert rc == 0, rc
                return (t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3

            launch()
            ctx.sync()
            host()
            same = all(np.array_equal(d_out[n].cpu().numpy().view(np.uint8), h_out[n].view(np.uint8)) for n in OUTPUTS)
            truth = bool(np.array_equal(h_out["tx_ms"].reshape(E, K), h.ms[::stride]))
            if not res["shapes"]:  # the process's first timing: bring the device up to its clocks first
                for _ in range(args.warm):
                    launch()
                ctx.sync()
            ms = median_ms(ctx, launch, args.settle, args.steps)
            reps = np.array([host() for _ in range(args.host_reps)])
            copy_ms, twin_ms = float(np.median(reps[:, 0])), float(np.median(reps[:, 1]))
            nbytes = int(hist.nbytes)
            read_ms = min(float(np.median(ctx.read_stream_ms(d_hist, nbytes, variant=v, launches=args.steps))) for v in (0, 1))
            out_bytes = int(sum(np.dtype(s[1]).itemsize * s[0] for s in sizes.values()))
            rec = {"B": B, "K": K, "E": E, "epoch_stride": stride, "same_bits": bool(same), "tx_ms_is_truth": truth,
                   "measured_channels": int((h_out["channels"].view(_lib.OBS_CHANNEL_DTYPE)["status"] == 0).sum()), "device_ms": ms, "copy_ms": copy_ms,
                   "twin_ms": twin_ms, "host_path_ms": copy_ms + twin_ms, "host_over_device": (copy_ms + twin_ms) / ms, "history_bytes": nbytes,
                   "output_bytes": out_bytes, "history_passes": 2, "read_once_ms": read_ms, "read_gb_per_s": nbytes / (read_ms * 1e6),
                   "device_over_two_reads": ms / (2.0 * read_ms), "history_gb_per_s": 2.0 * nbytes / (ms * 1e6),
                   "plan": observables_plan(B, K, E, **kw)}
            res["shapes"][f"B{B}_K{K}_stride{stride}"] = rec
            print(json.dumps(rec), flush=True)
            del d_out
        del d_hist

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
