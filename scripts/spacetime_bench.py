"""Timings of space-time adaptive processing (include/gat.h gat_spacetime_covariance, gat_spacetime_filter), next to their
yardsticks in the same run, by the protocol of scripts/spectrum_bench.py (settle launches, then timed launches, one HIP-event
interval per launch, median):

  the headline stream -- antennas at 20 MHz, blocks of 1 ms = 20000 samples -- as planar float and as int8 pairs, for M = 4 with
  T = 1, 3, 5, 7, 16 taps an antenna and for M = 16 with T = 4; one beam; one covariance estimate over all blocks.

Per shape: ms of the filter and of the covariance on the aligned path, their input rates over the rate of the read-only kernel
(gat_debug_read_stream, best variant) on the same input in the same run, and their FP32 rates (filter: 8 Q flop an output;
covariance: 8 flop an upper-triangle element pair and snapshot, Q (Q + 1) / 2 of them) over the 157.3 TFLOP/s vector roof.  For T = 1
the same data also go through gat_beamform_samples and gat_spatial_covariance: one tap is where a regression against them would show
(both operators forward one tap to them, so each pair of figures is one kernel timed twice: what differs is the run's scatter).

The operators of a shape are timed in the order A, B, B, A, and each one's figure is the lower of its two medians (`rounds` keeps
all); the first shape is launched `--warm` times before anything is timed.  Every input is larger than the 256 MB of last-level
cache (the int8 shapes take four times the blocks for that), so the reader's rate is a memory rate in every row.

  python scripts/spacetime_bench.py [--out profiles/spacetime/spacetime_bench.json] [--settle 5] [--steps 10] [--warm 100] [--blocks 1024]
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

FP32_ROOF = 157.3e12
SOURCES = ("gat_st.hip", "gat_st.h", "gat_st_plan.h", "gat_st_kernels.h", "gat_st_api.cpp", "gat_sample_load.h")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spacetime", "spacetime_bench.json"))
    ap.add_argument("--settle", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warm", type=int, default=100)
    ap.add_argument("--blocks", type=int, default=1024)
    args = ap.parse_args()
    import torch

    import gpuacceleratedtracking_amd as g
    from gpuacceleratedtracking_amd import _lib
    from gpuacceleratedtracking_amd.streams import alloc_stream, input_desc

    g.load_library()
    ctx = g.get_context()
    dev = ctx.device
    csrc = os.path.join(ROOT, "gpuacceleratedtracking_amd", "csrc")
    sha = hashlib.sha256()
    for name in SOURCES:
        with open(os.path.join(csrc, name), "rb") as fh:
            sha.update(fh.read())
    res = {"protocol": "every kernel: settle launches, then timed launches, one HIP-event interval each, median", "settle": args.settle, "steps": args.steps,
           "order": "A, B, B, A; the lower median of an operator's two rounds", "warm_launches": args.warm, "fp32_roof_TFLOPs": FP32_ROOF / 1e12,
           "build": g.build.build_info(), "library": lib_record(_lib.library_path()), "spacetime_sources_sha256": sha.hexdigest(), "shapes": {}}
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)

    def vp(t):
        return C.c_void_p(t.data_ptr())

    def bench(label, signal, reader_ms, M, N, B, T):
        first, desc = input_desc(signal, N, B, 0, None)
        Q, No = M * T, N - T + 1
        w = torch.randn((2, 1, Q), generator=gen, device=dev, dtype=torch.float64) / Q
        out, odesc = alloc_stream(1, No, B, dev, planar=True)
        cov = torch.zeros((2, 1, Q, Q), dtype=torch.float32, device=dev)
        launches = {}

        def call(name, fn, *a):
            def launch():
                rc = fn(ctx._h, *a)
                if rc != 0:
                    ctx.check(rc, name)
            launches[name] = launch

        call("filter", ctx.lib.gat_spacetime_filter, C.byref(desc), B, vp(w[0]), vp(w[1]), T, 1, C.byref(odesc))
        call("covariance", ctx.lib.gat_spacetime_covariance, C.byref(desc), B, B, T, vp(cov[0]), vp(cov[1]))
        order = ["filter", "covariance", "covariance", "filter"]
        if T == 1:  # the operators one tap must not fall behind
            call("beamform_samples", ctx.lib.gat_beamform_samples, C.byref(desc), B, vp(w[0]), vp(w[1]), 1, C.byref(odesc))
            call("spatial_covariance", ctx.lib.gat_spatial_covariance, C.byref(desc), B, B, vp(cov[0]), vp(cov[1]))
            order = ["filter", "beamform_samples", "beamform_samples", "filter", "covariance", "spatial_covariance", "spatial_covariance", "covariance"]
        if not res["shapes"]:  # the process's first timing: bring the device up to its clocks first
            for _ in range(args.warm):
                launches["filter"]()
            ctx.sync()
        rec = {name: {"rounds": []} for name in launches}
        for name in order:
            ms = median_ms(ctx, launches[name], args.settle, args.steps)
            rec[name]["rounds"].append(ms)
            rec[name]["ms"] = min(rec[name]["rounds"])
            if name in ("filter", "beamform_samples"):
                info = ctx.last_launch_info()
                rec[name].update({"vec": info["vec"], "workgroups": info["workgroups"], "splits": info["splits"], "lds_bytes": info["lds_bytes"]})
        nbytes = first.numel() * first.element_size() * (2 if isinstance(signal, tuple) else 1)
        read_rate = first.numel() * first.element_size() / (reader_ms * 1e-3)
        flop = {"filter": 8.0 * Q * No * B, "covariance": 8.0 * (Q * (Q + 1) // 2) * No * B}
        for name in rec:
            ms = rec[name]["ms"]
            rec[name].update({"input_GBps": nbytes / (ms * 1e-3) / 1e9, "of_reader": nbytes / (ms * 1e-3) / read_rate})
            if name in flop:
                rec[name].update({"TFLOPs": flop[name] / (ms * 1e-3) / 1e12, "of_fp32_roof": flop[name] / (ms * 1e-3) / FP32_ROOF})
        rec.update({"M": M, "T": T, "Q": Q, "N": N, "B": B, "input_bytes": nbytes, "output_bytes": 8 * No * B, "reader_GBps": read_rate / 1e9})
        res["shapes"][label] = rec
        print(label, json.dumps(rec), flush=True)

    def reader(first):
        return min(float(np.median(ctx.read_stream_ms(first, first.numel() * first.element_size(), variant=v, launches=args.steps))) for v in (0, 1))

    N = 20000
    for M, taps in ((4, (1, 3, 5, 7, 16)), (16, (4,))):
        B = args.blocks * 4 // M
        re = torch.randn((M, B * N), generator=gen, device=dev, dtype=torch.float32)
        im = torch.randn((M, B * N), generator=gen, device=dev, dtype=torch.float32)
        r_ms = reader(re)
        for T in taps:
            bench(f"float_M{M}_T{T}", (re, im), r_ms, M, N, B, T)
        del re, im
        B *= 4  # 2 bytes a sample: four times the blocks keep the input beyond the last-level cache
        x8 = torch.randint(-127, 128, (M, B * N, 2), generator=gen, device=dev, dtype=torch.int8)
        r_ms = reader(x8)
        for T in taps:
            bench(f"int8_M{M}_T{T}", x8, r_ms, M, N, B, T)
        del x8

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
