"""Acquisition search (gat_acquire) at a cold start of configs[1]'s shape: GPS L1 C/A, 32 PRNs, 4 antennas, 20 MHz, one
1 ms block, +-7 kHz in 500 Hz steps (29 bins), code step s = 10 samples, J = 2000 bins (one code period).

Reports the HIP-event median of the whole call (grid, group sum, statistics, results to the host), the grid kernel's
share of the FP32 vector roof (T = P D J N M B sign-multiply-accumulates at 4 FLOP each over 157.3 TFLOP/s: 3.8 ms here),
and the same grid through the existing correlator -- channels = PRN x Doppler, taps in calls of 32 -- as a user can do it
without the search (correlation time only; squaring and summing would come on top).
usage: python scripts/acquisition_bench.py [--iters K] [--kernel-stats <rocprofv3 kernel_stats.csv>] [--out FILE]
Kernel times come from a separate run under `rocprofv3 --kernel-trace --stats -- python scripts/acquisition_bench.py
--iters 5`; --kernel-stats then reads that run's kernel_stats.csv into the report."""
import argparse
import csv
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import gpuacceleratedtracking_amd as g

PEAK_FP32 = 157.3e12  # MI355X FP32 vector, FLOP/s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-correlator", action="store_true")
    args = ap.parse_args()

    system = g.GPSL1()
    P, M, fs, N, B = 32, 4, 20e6, 20000, 1
    fc = 1.023e6
    sats = [(2, 1500.0, 100.265), (7, -2000.0, 511.53), (12, 3000.0, 900.27), (19, -500.0, 33.27)]
    prm = g.make_params(np.array([p for p, _, _ in sats]), np.array([fc * (1 + d / 1575.42e6) for _, d, _ in sats]),
                        np.array([d for _, d, _ in sats]), np.array([t for _, _, t in sats]), 0.0, shape=(1, len(sats)))
    ctx = g.get_context()
    ctx.set_codes(system.codes)
    re = torch.empty((M, N), dtype=torch.float32, device="cuda")
    im = torch.empty_like(re)
    ctx.gen_signal(re, im, g.GAT_LAYOUT_PLANAR, N, M, N, N, 1, len(sats), ctx.params_to_device(prm), fs, amplitude=1.0,
                   steering_cycles=torch.rand(M, device="cuda"), noise_sigma=float(np.sqrt(fs / (2 * 10 ** 4.5))), seed=5)
    kw = dict(num_samples=N, max_doppler=7000.0, doppler_step=500.0, code_step_chips=0.5, keep_power=True)
    res = g.acquire(system, (re, im), fs, range(P), **kw)
    D, J = res[0].power_bins.shape
    s = max(1, int(round(0.5 * fs / fc)))
    assert (D, J, s) == (29, 2000, 10), (D, J, s)
    T = P * D * J * N * M * B
    roof_ms = 4.0 * T / PEAK_FP32 * 1e3

    for _ in range(3):
        g.acquire(system, (re, im), fs, range(P), **kw)
    times = []
    for _ in range(args.iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.acquire(system, (re, im), fs, range(P), **kw)
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    call_ms = float(np.median(times))
    out = {"scenario": "GPS L1 C/A, 32 PRN x 29 Doppler x 2000 code bins (s = 10), M = 4, fs = 20 MHz, N = 20000, B = 1",
           "sign_macs": T, "roof_ms": roof_ms, "call_ms_median": call_ms, "call_ms_min": float(np.min(times)),
           "call_fraction_of_roof": roof_ms / call_ms, "iters": args.iters,
           "detected": [r.prn for r in res if r.detected == 1], "library": g.load_library().gat_version().decode()}

    if not args.no_correlator:
        # the same grid through the correlator: channels = PRN x Doppler (928), taps in calls of 32 (63 calls)
        dop = -7000.0 + 500.0 * np.arange(D)
        cp = g.make_params(np.repeat(np.arange(P), D), fc, np.tile(dop, P), 0.0, 0.0, shape=(1, P * D))
        cp_dev = ctx.params_to_device(cp)
        from gpuacceleratedtracking_amd.streams import signal_desc
        desc = signal_desc(re, im, N)
        K = P * D
        o_re = torch.empty((K * 32 * M,), dtype=torch.float32, device="cuda")
        o_im = torch.empty_like(o_re)
        calls = [np.arange(j0, min(J, j0 + 32), dtype=np.int32) * s for j0 in range(0, J, 32)]

        def route():
            for sh in calls:
                ctx.downconvert_and_correlate(desc, cp_dev, 1, K, sh, fs, o_re, o_im)
        route()
        torch.cuda.synchronize()
        ct = []
        for _ in range(max(3, args.iters // 5)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            route()
            e1.record()
            e1.synchronize()
            ct.append(e0.elapsed_time(e1))
        out["correlator_route_ms_median"] = float(np.median(ct))
        out["correlator_route_calls"] = len(calls)
        out["speedup_vs_correlator_route"] = out["correlator_route_ms_median"] / call_ms

    if args.kernel_stats:
        with open(args.kernel_stats) as f:
            rows = list(csv.DictReader(f))
        ks = {}
        for r in rows:
            name = r.get("Name", "")
            ks[name] = {"calls": int(r["Calls"]), "avg_us": float(r["AverageNs"]) / 1e3}
        grid = [v for k, v in ks.items() if "acq_grid_kernel" in k]
        out["kernel_stats"] = {k: v for k, v in ks.items() if "acq_" in k}
        if grid:
            kms = grid[0]["avg_us"] / 1e3
            out["grid_kernel_ms"] = kms
            out["grid_kernel_fraction_of_roof"] = roof_ms / kms
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
