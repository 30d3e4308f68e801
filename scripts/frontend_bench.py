"""Timings of the sample conditioner (include/gat.h gat_condition_samples, gat_sample_stats) on the headline stream (M = 4,
B = 4096 x N = 20000), next to their yardsticks in the same run, by the protocol of scripts/array_bench.py (settle launches,
then timed launches, one HIP-event interval per launch, median):

  planar float -> int8, int16 pairs -> int8, and the statistics alone on the planar stream: ms, GB/s over the algorithmic bytes
      (in_bytes * M + out_bytes * M per sample; the statistics: in_bytes * M), and that rate over the rate of the read-only
      kernel (gat_debug_read_stream, best variant) on the planar stream;
  the headline correlator on the float stream and on its int8 conditioning: the pair that says after how many reads of a
      stream the conversion has paid for itself, break_even_reads = conversion ms / (float ms - int8 ms).

  python scripts/frontend_bench.py [--out profiles/frontend/frontend_bench.json] [--settle 64] [--steps 30]
Reported, not required: no figure here gates anything."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scripts.array_bench import median_ms  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frontend", "frontend_bench.json"))
    ap.add_argument("--settle", type=int, default=64)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--blocks", type=int, default=4096)
    args = ap.parse_args()
    import torch

    import gpuacceleratedtracking_amd as g
    from gpuacceleratedtracking_amd import frontend, streams

    N, M, L, K, B = 20000, 4, 3, 2, args.blocks
    op, desc, sig, prm = g.build_stream("GPSL1", N, M, L, K, B)
    ctx = g.get_context()
    samples = float(M) * B * N
    res = {"shape": {"N": N, "M": M, "B": B}, "settle": args.settle, "steps": args.steps, "build": g.build.build_info()}

    reader = min(float(np.median(ctx.read_stream_ms(sig[0], sig[0].numel() * 4, variant=v, launches=args.steps))) for v in (0, 1))
    read_rate = sig[0].numel() * 4 / (reader * 1e-3)
    res["reader"] = {"ms": reader, "GBps": read_rate / 1e9}

    # records from the stream itself, as a receiver would make them
    st = frontend.sample_stats(sig, N, B, ctx=ctx)
    params = frontend.agc_params(st, 16.0, 0.0, ctx=ctx)

    def bench_condition(signal, in_bytes, label):
        out, odesc, counts = frontend.condition_samples(signal, params, N, B, torch.int8, ctx=ctx)
        _, idesc = streams.input_desc(signal, N, B, 0, None)
        fn = ctx.lib.gat_condition_samples
        cargs = (ctx._h, C.byref(idesc), B, C.c_void_p(params.data_ptr()), 0, C.byref(odesc), C.c_void_p(counts.data_ptr()))

        def launch():
            rc = fn(*cargs)
            if rc != 0:
                ctx.check(rc, "gat_condition_samples")
        ms = median_ms(ctx, launch, args.settle, args.steps)
        rate = samples * (in_bytes + 2) / (ms * 1e-3)
        res[label] = {"ms": ms, "GBps": rate / 1e9, "of_reader": rate / read_rate, "vec": ctx.last_launch_info()["vec"]}
        return out, odesc

    sig8, desc8 = bench_condition(sig, 8, "planar_to_int8")  # (sig8 owns the memory desc8 points into)
    p16 = frontend.agc_params(st, 2000.0, 0.0, ctx=ctx)
    sig16, _, _ = frontend.condition_samples(sig, p16, N, B, torch.int16, ctx=ctx)
    ctx.sync()
    bench_condition(sig16, 4, "int16_to_int8")

    _, idesc = streams.input_desc(sig, N, B, 0, None)
    sfn, sargs = ctx.lib.gat_sample_stats, (ctx._h, C.byref(idesc), B, B, None, 0, C.c_void_p(st.raw.data_ptr()))

    def stats_launch():
        rc = sfn(*sargs)
        if rc != 0:
            ctx.check(rc, "gat_sample_stats")
    ms = median_ms(ctx, stats_launch, args.settle, args.steps)
    rate = samples * 8 / (ms * 1e-3)
    res["stats_planar"] = {"ms": ms, "GBps": rate / 1e9, "of_reader": rate / read_rate, "vec": ctx.last_launch_info()["vec"]}

    # the headline correlator on the float stream and on its int8 image
    f_ms = median_ms(ctx, lambda: op.launch(desc), args.settle, args.steps)
    q_ms = median_ms(ctx, lambda: op.launch(desc8), args.settle, args.steps)
    res["correlator"] = {"float_ms": f_ms, "int8_ms": q_ms}
    saved = f_ms - q_ms
    res["break_even_reads"] = res["planar_to_int8"]["ms"] / saved if saved > 0 else None

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
