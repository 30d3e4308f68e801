"""Timings of the FFT acquisition search (include/gat.h gat_acquire_fft) next to the direct search (gat_acquire) on the same grid
in the same process, by the protocol of scripts/spectrum_bench.py (settle launches, then timed launches, one HIP-event interval
per launch, median; the two methods in the order fft, direct, direct, fft and each one's figure the lower of its two medians; the
first case is launched `--warm` times before anything is timed).  Both calls synchronise, so an interval is a whole search: its
launches, the statistics and the results' copy.

  l1_s10     GPS L1, 32 PRNs x 29 Doppler bins (+-7 kHz in 500 Hz) x 2000 half-chip bins (s = 10), 4 antennas, 20 MHz, 1 ms
  l1_s1      the same at sample spacing: 20000 code bins
  l5_50MHz   GPS L5, 12 PRNs x 29 x 25000 bins (s = 2), 4 antennas, 50 MHz, 1 ms (N = 50000, F = 2^17)
  l1_10blk   l1_s10 over 10 blocks, non-coherent

Per case: ms of both methods and their ratio, the FFT plan (gat_acquire_fft_plan) and the bytes its launches move by the plan's own
count (every pass reads and writes its transforms once; the product reads C and W), with the rate that makes of the FFT's time.
`--only fft|direct --case NAME --launches K` runs K launches of one method without timing: the run to put under
`rocprofv3 --kernel-trace --stats` (the per-kernel split) or `rocprofv3 --pmc ...` (counters, in a run of their own).

  python scripts/acquisition_fft_bench.py [--out profiles/acquisition_fft/acquisition_fft_bench.json] [--settle 3] [--steps 10] [--warm 20]
Reported, not required: no figure here gates anything."""
from __future__ import annotations

import argparse
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scripts.array_bench import median_ms  # noqa: E402
from scripts.spectrum_bench import lib_record  # noqa: E402

SOURCES = ("gat_acq_fft.hip", "gat_acq_fft.h", "gat_acq_fft_plan.h", "gat_acq_fft_kernels.h", "gat_acq_fft_api.cpp", "gat_acq.hip", "gat_acq_api.cpp")
#          system, fs, N, M, B, PRNs, s, J
CASES = {"l1_s10": ("GPSL1", 20.0e6, 20000, 4, 1, 32, 10, 2000),
         "l1_s1": ("GPSL1", 20.0e6, 20000, 4, 1, 32, 1, 20000),
         "l5_50MHz": ("GPSL5", 50.0e6, 50000, 4, 1, 12, 2, 25000),
         "l1_10blk": ("GPSL1", 20.0e6, 20000, 4, 10, 32, 10, 2000)}


def plan_bytes(pl, P, D, J, M, B, N, sample_bytes):
    """bytes the FFT search's launches read and write, by the plan: per transform and pass F float pairs in and out (the signal's
    first pass reads N samples instead, the replica's reads no array), the product's first pass reads two spectra, its last pass
    writes none but reads and writes the grid once per unit"""
    F8, two = 8.0 * (1 << pl["fft_log2"]), pl["passes"] == 2
    G, units = pl["num_segments"], M * B
    rep = P * B * G * F8 * (3 if two else 1)
    sig = units * D * (N * sample_bytes + F8 * (3 if two else 1))
    prod = P * D * G * units * F8 * (4 if two else 2) + 2.0 * 4 * P * D * J * units
    return {"replica": rep, "signal": sig, "product": prod, "total": rep + sig + prod}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "acquisition_fft", "acquisition_fft_bench.json"))
    ap.add_argument("--settle", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warm", type=int, default=20)
    ap.add_argument("--case", default=None)
    ap.add_argument("--only", default=None, choices=("fft", "direct"))
    ap.add_argument("--launches", type=int, default=3)
    ap.add_argument("--doppler-batch", type=int, default=0)
    args = ap.parse_args()
    import torch

    import gpuacceleratedtracking_amd as g
    from gpuacceleratedtracking_amd import _lib
    from gpuacceleratedtracking_amd.acquisition import _as_desc, acquire_fft_plan

    g.load_library()
    ctx = g.get_context()
    dev = ctx.device
    cus = ctx.device_info()["num_cus"]
    if args.doppler_batch:
        ctx.set_option("acq_fft_doppler_batch", args.doppler_batch)
    csrc = os.path.join(ROOT, "gpuacceleratedtracking_amd", "csrc")
    sha = hashlib.sha256()
    for name in SOURCES:
        with open(os.path.join(csrc, name), "rb") as fh:
            sha.update(fh.read())
    res = {"protocol": "each method: settle launches, then timed launches, one HIP-event interval each, median; a launch is a whole synchronising search",
           "settle": args.settle, "steps": args.steps, "order": "fft, direct, direct, fft; the lower median of a method's two rounds", "warm_launches": args.warm,
           "doppler_batch_option": args.doppler_batch, "num_cus": cus, "build": g.build.build_info(), "library": lib_record(_lib.library_path()),
           "sources_sha256": sha.hexdigest(), "cases": {}}
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    for label, (sysname, fs, N, M, B, P, s, J) in CASES.items():
        if args.case and label != args.case:
            continue
        system = g.GNSSDICT[sysname]()
        ctx.set_codes(system.codes)
        re = torch.randn((M, B * N), generator=gen, device=dev, dtype=torch.float32)
        im = torch.randn((M, B * N), generator=gen, device=dev, dtype=torch.float32)
        desc = _as_desc((re, im), N, B, N)
        D = 29
        cfg = _lib.AcqConfig()
        cfg.struct_size = C.sizeof(_lib.AcqConfig)
        cfg.num_doppler_bins, cfg.num_code_bins, cfg.code_step_samples = D, J, s
        cfg.if_hz, cfg.code_freq_hz, cfg.doppler_first_hz, cfg.doppler_step_hz = 0.0, system.code_frequency, -7000.0, 500.0
        cfg.first_shift, cfg.min_peak_ratio, cfg.code_length = 0, 2.0, int(system.code_length)
        prns = np.arange(P, dtype=np.int32)
        out = np.zeros(P, dtype=_lib.ACQ_RESULT_DTYPE)
        power = torch.empty((P, D, J), dtype=torch.float32, device=dev)
        launches = {}
        for method, fn in (("fft", ctx.lib.gat_acquire_fft), ("direct", ctx.lib.gat_acquire)):
            cargs = (ctx._h, C.byref(desc), B, prns.ctypes.data_as(C.POINTER(C.c_int32)), P, fs, C.byref(cfg), C.c_void_p(power.data_ptr()), C.c_void_p(out.ctypes.data))

            def launch(fn=fn, cargs=cargs, method=method):
                rc = fn(*cargs)
                if rc != 0:
                    ctx.check(rc, method)
            launches[method] = launch
        pl = acquire_fft_plan(desc, B, P, fs, cfg, num_cus=cus, doppler_batch=args.doppler_batch)
        if args.only:
            for _ in range(args.launches):
                launches[args.only]()
            ctx.sync()
            print(label, args.only, args.launches, "launches", json.dumps(pl), flush=True)
            continue
        if not res["cases"]:
            for _ in range(args.warm):
                launches["fft"]()
            ctx.sync()
        rec = {m: {"rounds": []} for m in launches}
        for method in ("fft", "direct", "direct", "fft"):
            rec[method]["rounds"].append(median_ms(ctx, launches[method], args.settle, args.steps))
            rec[method]["ms"] = min(rec[method]["rounds"])
        nb = plan_bytes(pl, P, D, J, M, B, N, 8)
        rec.update({"system": sysname, "fs": fs, "N": N, "M": M, "B": B, "P": P, "D": D, "J": J, "s": s, "plan": pl, "plan_bytes": nb,
                    "fft_GBps_of_plan_bytes": nb["total"] / (rec["fft"]["ms"] * 1e-3) / 1e9, "direct_over_fft": rec["direct"]["ms"] / rec["fft"]["ms"],
                    "direct_mac": float(P) * D * J * N * M * B, "direct_TFLOPs": 4.0 * P * D * J * N * M * B / (rec["direct"]["ms"] * 1e-3) / 1e12})
        res["cases"][label] = rec
        print(label, json.dumps(rec), flush=True)
        del re, im, power
    if args.only:
        return
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
