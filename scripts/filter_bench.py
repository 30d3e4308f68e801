"""Timings of the sample filter (include/gat.h gat_filter_samples), next to their yardsticks in the same run, by the protocol of
scripts/array_bench.py (settle launches, then timed launches, one HIP-event interval per launch, median):

  a 4-antenna wideband front end, 100 MHz -> 20 MHz (D = 5, T = 64), blocks of 1 ms, from planar float, int16 pairs and int8 pairs;
  a notch at the stream's own rate (D = 1, T = 32) over the headline stream (M = 4, blocks of N = 20000 planar float).

Per shape: ms of the tiled kernel, its FP32 rate (8 T flop per output and antenna) over the 157.3 TFLOP/s vector roof, its input
rate over the rate of the read-only kernel (gat_debug_read_stream, best variant) on the same input in the same run, and ms of the
general kernel on the same data (the same call with the output one sample off its alignment).

Every input is larger than the 256 MB of last-level cache (the int8 shape takes twice the blocks for that), so the reader's rate is
a memory rate in every row.  The record names the text it timed: the SHA-256 of the filter's sources next to the build's identity.

  python scripts/filter_bench.py [--out profiles/filter/filter_bench.json] [--settle 20] [--steps 20] [--wide-blocks 256] [--blocks 1024]
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

FP32_ROOF = 157.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "filter", "filter_bench.json"))
    ap.add_argument("--settle", type=int, default=20)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--wide-blocks", type=int, default=256)
    ap.add_argument("--blocks", type=int, default=1024)
    args = ap.parse_args()
    import torch

    import gpuacceleratedtracking_amd as g
    from gpuacceleratedtracking_amd import _lib, filtering, streams

    g.load_library()
    ctx = g.get_context()
    dev = ctx.device
    csrc = os.path.join(ROOT, "gpuacceleratedtracking_amd", "csrc")
    sha = hashlib.sha256()
    for name in ("gat_fir.hip", "gat_fir.h", "gat_fir_plan.h", "gat_fir_kernels.h", "gat_fir_api.cpp"):
        with open(os.path.join(csrc, name), "rb") as fh:
            sha.update(fh.read())
    res = {"protocol": "every kernel: settle launches, then timed launches, one HIP-event interval each, median", "settle": args.settle, "steps": args.steps,
           "fp32_roof_TFLOPs": FP32_ROOF / 1e12, "build": g.build.build_info(), "filter_sources_sha256": sha.hexdigest(), "shapes": {}}
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)

    def bench(label, signal, in_bytes, M, N, B, T, D, step):
        taps = filtering.shift_taps(filtering.lowpass_taps(T, 0.25 / D), step)
        g_re, g_im = filtering._tap_planes(taps)
        t_re, t_im = torch.from_numpy(g_re).to(dev), torch.from_numpy(g_im).to(dev)
        first, desc = streams.input_desc(signal, N, B, 0, None)
        Q = filtering.num_outputs(N, T, D)
        ostride = (Q + 3) // 4 * 4
        o_re, o_im = (torch.zeros(M * B * ostride + 4, dtype=torch.float32, device=dev) for _ in range(2))
        cfg = filtering._config(T, D, step, 0.0)
        out = {}
        for kernel, off in (("tiled", 0), ("general", 4)):  # (4 bytes: one float of each plane)
            odesc = _lib.SignalDesc(o_re.data_ptr() + off, o_im.data_ptr() + off, _lib.GAT_LAYOUT_PLANAR, M, Q, B * ostride, ostride, 0)
            cargs = (ctx._h, C.byref(desc), B, C.c_void_p(t_re.data_ptr()), C.c_void_p(t_im.data_ptr()), C.byref(cfg), C.byref(odesc))

            def launch():
                rc = ctx.lib.gat_filter_samples(*cargs)
                if rc != 0:
                    ctx.check(rc, "gat_filter_samples")
            ms = median_ms(ctx, launch, args.settle, args.steps)  # (one protocol for both kernels)
            info = ctx.last_launch_info()
            assert (info["vec"] > 1) == (kernel == "tiled"), info
            out[kernel] = {"ms": ms, "vec": info["vec"], "workgroups": info["workgroups"], "splits": info["splits"]}
        nbytes = first.numel() * first.element_size() * (2 if isinstance(signal, tuple) else 1)
        reader = min(float(np.median(ctx.read_stream_ms(first, first.numel() * first.element_size(), variant=v, launches=args.steps))) for v in (0, 1))
        read_rate = first.numel() * first.element_size() / (reader * 1e-3)
        flop = 8.0 * T * Q * M * B
        ms = out["tiled"]["ms"]
        out.update({"M": M, "N": N, "B": B, "T": T, "D": D, "Q": Q, "input_bytes": nbytes, "reader_GBps": read_rate / 1e9,
                    "TFLOPs": flop / (ms * 1e-3) / 1e12, "of_fp32_roof": flop / (ms * 1e-3) / FP32_ROOF, "input_GBps": nbytes / (ms * 1e-3) / 1e9,
                    "of_reader": nbytes / (ms * 1e-3) / read_rate, "general_over_tiled_ms": out["general"]["ms"] / ms})
        assert in_bytes * M * B * N == nbytes
        res["shapes"][label] = out
        print(label, json.dumps(out), flush=True)

    M, N, B = 4, 100000, args.wide_blocks
    re = torch.randn((M, B * N), generator=gen, device=dev, dtype=torch.float32)
    im = torch.randn((M, B * N), generator=gen, device=dev, dtype=torch.float32)
    bench("wide_float_100_to_20", (re, im), 8, M, N, B, 64, 5, 0.125)
    x16 = (torch.stack((re, im), dim=-1) * 2000.0).round().clamp(-32767, 32767).to(torch.int16).contiguous()
    bench("wide_int16_100_to_20", x16, 4, M, N, B, 64, 5, 0.125)
    del re, im, x16
    B = 2 * args.wide_blocks  # 2 bytes a sample: twice the blocks keep the input beyond the last-level cache
    x8 = (torch.randn((M, B * N, 2), generator=gen, device=dev, dtype=torch.float32) * 16.0).round().clamp(-127, 127).to(torch.int8).contiguous()
    bench("wide_int8_100_to_20", x8, 2, M, N, B, 64, 5, 0.125)
    del x8
    M, N, B = 4, 20000, args.blocks
    re = torch.randn((M, B * N), generator=gen, device=dev, dtype=torch.float32)
    im = torch.randn((M, B * N), generator=gen, device=dev, dtype=torch.float32)
    bench("notch_float_20", (re, im), 8, M, N, B, 32, 1, 0.0)

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
