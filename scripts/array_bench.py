"""Timings of the spatial covariance kernels (include/gat.h gat_spatial_covariance) and of the sample beamformer
(gat_beamform_samples) on the device, next to their yardsticks in the same run:

  small arrays -- the headline stream (M = 4, B = 4096 x N = 20000; planar float 2.62 GB, then int16 and int8 pairs): the
      covariance, the headline correlator and the read-only kernel (gat_debug_read_stream, best variant) over the same
      samples, each by bench.py's protocol (settle launches, then timed launches, one HIP-event interval per launch,
      median).  Requirement (planar): covariance bytes/s x 1.12 >= the reader's bytes/s -- the guard
      tests/test_measurement_gpu.py holds the headline correlator to.
  large arrays -- the configs[3] (M = 16, 128 x 50000) and configs[4] (M = 64, 1 x 2 000 000) signals: the covariance's time
      and its share of the FP32 vector roof (8 M (M + 1) / 2 flop per sample over 157.3 TFLOP/s), and, reported only,
      torch.view_as_complex(x) @ x.mH on the interleaved layout.

  beams -- the headline stream in the three ingest formats into 1 and 4 planar beams (the streaming kernel), and the M = 16
      and M = 64 signals into 1 and 4 beams (the general kernel): ms, GB/s over the algorithmic bytes in_bytes * M + 8 * beams
      per sample, and that rate over the reader's of the same run.  Reported, not required.

  python scripts/array_bench.py [--out profiles/array/array_bench.json] [--only small|large|beams|trace] [--settle 64] [--steps 30]
--only trace: a few launches of every measured covariance shape and nothing else, for a rocprofv3 --kernel-trace --stats (or
--pmc) run of its own.  Exit status 1 when the small-array requirement is missed."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FP32_VECTOR_ROOF = 157.3e12  # MI355X peak FP32 vector rate (FLOP/s)


def median_ms(ctx, launch, settle, steps):
    for _ in range(settle):
        launch()
    ctx.timer_lap()
    for _ in range(steps):
        launch()
        ctx.timer_lap()
    return float(np.median(ctx.timer_laps()))


def covariance_call(g, ctx, desc, B, M):
    import torch
    c_re = torch.empty((1, M, M), dtype=torch.float32, device=ctx.device)
    c_im = torch.empty_like(c_re)
    fn, args = ctx.lib.gat_spatial_covariance, (ctx._h, C.byref(desc), B, B, C.c_void_p(c_re.data_ptr()), C.c_void_p(c_im.data_ptr()))

    def launch(_keep=(c_re, c_im, desc)):
        rc = fn(*args)
        if rc != 0:
            ctx.check(rc, "gat_spatial_covariance")
    return launch


def small(g, settle, steps):
    import torch
    N, M, L, K, B = 20000, 4, 3, 1, 4096
    rows = []
    for name, layout in (("planar float", 0), ("int16 pairs", 2), ("int8 pairs", 3)):
        op, desc, sig, prm = g.build_stream("GPSL1", N, M, L, K, B, layout=layout)
        ctx = op.ctx
        nbytes = B * N * M * g.SAMPLE_BYTES[layout]
        t_cov = median_ms(ctx, covariance_call(g, ctx, desc, B, M), settle, steps)
        t_cor = median_ms(ctx, lambda: op.launch(desc), settle, steps)
        rbytes = sig[0].numel() * sig[0].element_size()  # one plane (planar) or the whole interleaved buffer
        t_read = min(float(np.median(ctx.read_stream_ms(sig[0], rbytes, variant=v, launches=7)[1:])) for v in (0, 1, 2, 4, 8))
        cov_rate, cor_rate, read_rate = nbytes / t_cov / 1e6, nbytes / t_cor / 1e6, rbytes / t_read / 1e6
        rows.append(dict(shape=f"M={M} B={B} N={N} {name}", bytes=nbytes, covariance_ms=t_cov, correlator_ms=t_cor, covariance_GBps=cov_rate,
                         correlator_GBps=cor_rate, reader_GBps=read_rate, covariance_fraction_of_read_ceiling=cov_rate / read_rate,
                         reader_over_covariance=read_rate / cov_rate))
        print(json.dumps(rows[-1]), flush=True)
        del op, desc, sig
        torch.cuda.empty_cache()
    return rows


def beams_call(g, ctx, desc, B, M, J, N):
    """gat_beamform_samples of `desc` into J planar beams, blocks back to back; random weights"""
    import torch
    gen = torch.Generator().manual_seed(J * 100 + M)
    w_re = torch.randn((J, M), generator=gen, dtype=torch.float64).to(ctx.device)
    w_im = torch.randn((J, M), generator=gen, dtype=torch.float64).to(ctx.device)
    ld = B * N
    o_re = torch.empty((J, ld), dtype=torch.float32, device=ctx.device)
    o_im = torch.empty_like(o_re)
    out = g._lib.SignalDesc(o_re.data_ptr(), o_im.data_ptr(), 0, J, N, ld, N, 0)
    fn, args = ctx.lib.gat_beamform_samples, (ctx._h, C.byref(desc), B, C.c_void_p(w_re.data_ptr()), C.c_void_p(w_im.data_ptr()), J, C.byref(out))

    def launch(_keep=(w_re, w_im, o_re, o_im, out, desc)):
        rc = fn(*args)
        if rc != 0:
            ctx.check(rc, "gat_beamform_samples")
    return launch


BEAMS = (("planar float", ("GPSL1", 20000, 4, 3, 1, 4096), 0, {}), ("int16 pairs", ("GPSL1", 20000, 4, 3, 1, 4096), 2, {}),
         ("int8 pairs", ("GPSL1", 20000, 4, 3, 1, 4096), 3, {}), ("ComplexF32 pairs", ("GPSL1", 50000, 16, 3, 32, 128), 1, {}),
         ("ComplexF32 pairs", ("GPSL1", 2000000, 64, 3, 64, 1), 1, dict(block_seconds=20e-3)))


def beams(g, settle, steps):
    import torch
    rows = []
    for name, args, layout, kw in BEAMS:
        _, N, M, L, K, B = args
        op, desc, sig, prm = g.build_stream(*args, layout=layout, **kw)
        ctx = op.ctx
        rbytes = sig[0].numel() * sig[0].element_size()
        t_read = min(float(np.median(ctx.read_stream_ms(sig[0], rbytes, variant=v, launches=7)[1:])) for v in (0, 1, 2, 4, 8))
        read_rate = rbytes / t_read / 1e6
        t_cov = median_ms(ctx, covariance_call(g, ctx, desc, B, M), settle, steps)
        for J in (1, 4):
            t = median_ms(ctx, beams_call(g, ctx, desc, B, M, J, N), settle, steps)
            info = ctx.last_launch_info()
            nbytes = B * N * (M * g.SAMPLE_BYTES[layout] + 8 * J)
            rows.append(dict(shape=f"M={M} B={B} N={N} {name}", beams=J, kernel="streaming" if info["vec"] == 4 else "general", bytes=nbytes,
                             beams_ms=t, beams_GBps=nbytes / t / 1e6, reader_GBps=read_rate, beams_fraction_of_read_ceiling=nbytes / t / 1e6 / read_rate,
                             covariance_ms=t_cov, beams_over_covariance_time=t / t_cov,
                             byte_ratio_to_covariance=nbytes / (B * N * M * g.SAMPLE_BYTES[layout])))
            print(json.dumps(rows[-1]), flush=True)
        del op, desc, sig
        torch.cuda.empty_cache()
    return rows


LARGE = (("configs[3] signal", ("GPSL1", 50000, 16, 3, 32, 128), {}), ("configs[4] signal", ("GPSL1", 2000000, 64, 3, 64, 1), dict(block_seconds=20e-3)))


def large(g, settle, steps):
    import torch
    rows = []
    for name, args, kw in LARGE:
        _, N, M, L, K, B = args
        op, desc, sig, prm = g.build_stream(*args, layout=1, **kw)  # ComplexF32 pairs: the layout the torch comparator needs
        ctx = op.ctx
        t_cov = median_ms(ctx, covariance_call(g, ctx, desc, B, M), settle, steps)
        flop = 8.0 * M * (M + 1) / 2 * N * B
        nbytes = B * N * M * 8
        x = torch.view_as_complex(sig[0])
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
        stream = torch.cuda.current_stream(ctx.device)
        for _ in range(max(3, settle // 8)):
            r = x @ x.mH
        ev[0].record(stream)
        for i in range(steps):
            r = x @ x.mH
            ev[i + 1].record(stream)
        stream.synchronize()
        t_torch = float(np.median([ev[i].elapsed_time(ev[i + 1]) for i in range(steps)]))
        rows.append(dict(shape=f"{name}: M={M} B={B} N={N} ComplexF32 pairs", bytes=nbytes, flop=flop, covariance_ms=t_cov,
                         covariance_TFLOPs=flop / t_cov / 1e9, fraction_of_fp32_vector_roof=flop / (t_cov * 1e-3) / FP32_VECTOR_ROOF,
                         covariance_GBps=nbytes / t_cov / 1e6, torch_matmul_ms=t_torch))
        print(json.dumps(rows[-1]), flush=True)
        del op, desc, sig, x, r
        torch.cuda.empty_cache()
    return rows


def trace(g):
    """a few launches of every measured covariance shape: what a profiler run of its own looks at"""
    import torch
    for args, layout, kw in ((("GPSL1", 20000, 4, 3, 1, 4096), 0, {}), (("GPSL1", 20000, 4, 3, 1, 4096), 2, {}), (("GPSL1", 20000, 4, 3, 1, 4096), 3, {}),
                             (LARGE[0][1], 1, LARGE[0][2]), (LARGE[1][1], 1, LARGE[1][2])):
        op, desc, sig, prm = g.build_stream(*args, layout=layout, **kw)
        launch = covariance_call(g, op.ctx, desc, args[5], args[2])
        for _ in range(8):
            launch()
        op.ctx.sync()
        del op, desc, sig
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "array", "array_bench.json"))
    ap.add_argument("--only", choices=("small", "large", "beams", "trace"))
    ap.add_argument("--settle", type=int, default=64)
    ap.add_argument("--steps", type=int, default=30)
    a = ap.parse_args()
    import torch

    import gpuacceleratedtracking_amd as g
    if not torch.cuda.is_available():
        raise SystemExit("array_bench.py needs a HIP device: there is no CPU fallback")
    if a.only == "trace":
        trace(g)
        return 0
    ctx = g.get_context()
    res = dict(library=g.load_library().gat_version().decode(), device=ctx.device_info(), settle=a.settle, steps=a.steps)
    if a.only in (None, "small"):
        res["small_arrays"] = small(g, a.settle, a.steps)
    if a.only in (None, "large"):
        res["large_arrays"] = large(g, a.settle, a.steps)
    if a.only in (None, "beams"):
        res["sample_beams"] = beams(g, a.settle, a.steps)
    ok = True
    if "small_arrays" in res:
        ok = res["small_arrays"][0]["covariance_GBps"] * 1.12 >= res["small_arrays"][0]["reader_GBps"]
        res["small_array_requirement_met"] = bool(ok)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(dict(requirement_met=ok, out=a.out)))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
