"""Timings of the sample spectrum (include/gat.h gat_sample_spectrum), next to their yardsticks in the same run, by the protocol of
scripts/filter_bench.py (settle launches, then timed launches, one HIP-event interval per launch, median):

  the headline stream -- 4 antennas at 20 MHz, blocks of 1 ms = 20000 samples -- as planar float and as int8 pairs, through
  F = 1024 with H = 512 (38 segments a block), F = 4096 with H = 4096 (4) and F = 256 with H = 128 (155).

Per shape: ms of the aligned path (16-byte loads), its FP32 rate (5 F log2 F flop a segment) over the 157.3 TFLOP/s vector roof,
its input rate over the rate of the read-only kernel (gat_debug_read_stream, best variant) on the same input in the same run, and
ms of the general path on the same data (the same call with the base one sample on and a block one sample shorter: the same
segments).

The two paths are timed in the order aligned, general, general, aligned, and each path's figure is the lower of its two medians
(`rounds` keeps all four); the first shape is launched `--warm` times before anything is timed.  Whatever is timed first in a
process runs up to 7 % slow -- the same general kernel on the same data took 0.455 ms as the run's first timing and 0.423 ms as
its second -- and a fixed order charged that to the aligned path.

Every input is larger than the 256 MB of last-level cache (the int8 shape takes four times the blocks for that), so the reader's
rate is a memory rate in every row.  The record names the text it timed: the SHA-256 of the spectrum's sources next to the
build's identity.

  python scripts/spectrum_bench.py [--out profiles/spectrum/spectrum_bench.json] [--settle 10] [--steps 20] [--warm 300] [--blocks 1024]
Reported, not required: no figure here gates anything."""
from __future__ import annotations

import argparse
import ctypes as C
import hashlib
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scripts.array_bench import median_ms  # noqa: E402

FP32_ROOF = 157.3e12
SOURCES = ("gat_spec.hip", "gat_spec.h", "gat_spec_plan.h", "gat_spec_kernels.h", "gat_spec_api.cpp", "gat_sample_load.h")


def lib_record(path):
    """the library that was loaded and timed: its path relative to the repository and the SHA-256 of the file (the `build` field
    describes the package's own library, which GAT_LIBRARY may have replaced)"""
    with open(path, "rb") as fh:
        digest = hashlib.sha256(fh.read()).hexdigest()
    return {"path": os.path.relpath(path, ROOT), "sha256": digest, "gat_library_override": bool(os.environ.get("GAT_LIBRARY"))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spectrum", "spectrum_bench.json"))
    ap.add_argument("--settle", type=int, default=10)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=300)
    ap.add_argument("--blocks", type=int, default=1024)
    args = ap.parse_args()
    import torch

    import gpuacceleratedtracking_amd as g
    from gpuacceleratedtracking_amd import _lib, spectrum
    from gpuacceleratedtracking_amd.streams import input_desc

    g.load_library()
    ctx = g.get_context()
    dev = ctx.device
    csrc = os.path.join(ROOT, "gpuacceleratedtracking_amd", "csrc")
    sha = hashlib.sha256()
    for name in SOURCES:
        with open(os.path.join(csrc, name), "rb") as fh:
            sha.update(fh.read())
    res = {"protocol": "every kernel: settle launches, then timed launches, one HIP-event interval each, median", "settle": args.settle, "steps": args.steps,
           "order": "aligned, general, general, aligned; the lower median of a path's two rounds", "warm_launches": args.warm, "fp32_roof_TFLOPs": FP32_ROOF / 1e12, "build": g.build.build_info(), "library": lib_record(_lib.library_path()), "spectrum_sources_sha256": sha.hexdigest(), "shapes": {}}
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)

    def bench(label, signal, reader_ms, M, N, B, F, H):
        first, desc = input_desc(signal, N, B, 0, None)
        w = torch.from_numpy(spectrum.window_values("hann", F)).to(dev)
        power = torch.zeros((B, M, F), dtype=torch.float32, device=dev)
        cfg = spectrum._config(F, H)
        S = spectrum.num_segments(N, F, H)
        assert spectrum.num_segments(N - 1, F, H) == S
        step = _lib.SAMPLE_BYTES[desc.layout] if desc.im is None else 4
        out, launches = {}, {}
        for path, off in (("aligned", 0), ("general", 1)):
            d = _lib.SignalDesc(desc.re + off * step, None if desc.im is None else desc.im + off * step, desc.layout, M, N - off, desc.ant_stride,
                                desc.block_stride, 0)
            cargs = (ctx._h, C.byref(d), B, C.c_void_p(w.data_ptr()), C.byref(cfg), C.c_void_p(power.data_ptr()))

            def launch(cargs=cargs, _keep=d):
                rc = ctx.lib.gat_sample_spectrum(*cargs)
                if rc != 0:
                    ctx.check(rc, "gat_sample_spectrum")
            launches[path] = launch
            out[path] = {"rounds": []}
        if not res["shapes"]:  # the process's first timing: bring the device up to its clocks first
            for _ in range(args.warm):
                launches["aligned"]()
            ctx.sync()
        for path in ("aligned", "general", "general", "aligned"):
            ms = median_ms(ctx, launches[path], args.settle, args.steps)  # (one protocol for both paths)
            info = ctx.last_launch_info()
            assert (info["vec"] > 1) == (path == "aligned"), info
            out[path]["rounds"].append(ms)
            out[path].update({"ms": min(out[path]["rounds"]), "vec": info["vec"], "workgroups": info["workgroups"],
                              "pairs_per_workgroup": info["channels_per_wg"], "lds_bytes": info["lds_bytes"]})
        nbytes = first.numel() * first.element_size() * (2 if isinstance(signal, tuple) else 1)
        read_rate = first.numel() * first.element_size() / (reader_ms * 1e-3)
        flop = 5.0 * F * math.log2(F) * S * M * B
        ms = out["aligned"]["ms"]
        out.update({"M": M, "N": N, "B": B, "F": F, "H": H, "S": S, "input_bytes": nbytes, "reader_GBps": read_rate / 1e9,
                    "TFLOPs": flop / (ms * 1e-3) / 1e12, "of_fp32_roof": flop / (ms * 1e-3) / FP32_ROOF, "input_GBps": nbytes / (ms * 1e-3) / 1e9,
                    "of_reader": nbytes / (ms * 1e-3) / read_rate, "general_over_aligned_ms": out["general"]["ms"] / ms,
                    "general_of_reader": nbytes / (out["general"]["ms"] * 1e-3) / read_rate})
        res["shapes"][label] = out
        print(label, json.dumps(out), flush=True)

    def reader(first):
        return min(float(np.median(ctx.read_stream_ms(first, first.numel() * first.element_size(), variant=v, launches=args.steps))) for v in (0, 1))

    shapes = ((1024, 512), (4096, 4096), (256, 128))
    M, N, B = 4, 20000, args.blocks
    re = torch.randn((M, B * N), generator=gen, device=dev, dtype=torch.float32)
    im = torch.randn((M, B * N), generator=gen, device=dev, dtype=torch.float32)
    r_ms = reader(re)
    for F, H in shapes:
        bench(f"float_F{F}_H{H}", (re, im), r_ms, M, N, B, F, H)
    del re, im
    B = 4 * args.blocks  # 2 bytes a sample: four times the blocks keep the input beyond the last-level cache
    x8 = torch.randint(-127, 128, (M, B * N, 2), generator=gen, device=dev, dtype=torch.int8)
    r_ms = reader(x8)
    for F, H in shapes:
        bench(f"int8_F{F}_H{H}", x8, r_ms, M, N, B, F, H)

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
