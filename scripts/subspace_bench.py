"""Timings of the subspace layer (include/gat.h gat_accumulator_covariance, gat_hermitian_eig) next to what a user of the library
did before it existed, on the same data in the same run:

  the device calls -- settle launches, then timed launches, one HIP-event interval per launch, median (the protocol of
  scripts/spectrum_bench.py);
  the yardstick: for the covariance a device-to-host copy of both accumulator planes followed by numpy's einsum over the prompt tap
  in complex128; for the eigensolver a device-to-host copy of the matrices followed by numpy.linalg.eigh -- wall time of the two
  steps, each timed, median over `--host-reps` repetitions.

Shapes: the covariance at (B, K, M) = (1000, 12, 4) and (65536, 64, 16), L = 3 taps, one estimate of all blocks; the eigensolver at
(n, Q) = (12, 4), (64, 16) and (64, 64) on Wishart matrices with every eigenvector asked for, and with one.

Per shape: ms of the device call with the plan, ms of the copy and of numpy, and their ratio.  The device results are compared with
the host twins bit for bit (the eigensolver) or on the first two channels (the covariance) before anything is timed.

  python scripts/subspace_bench.py [--out profiles/subspace/subspace_bench.json] [--settle 5] [--steps 20] [--host-reps 3] [--warm 50]
Reported, not required: no figure here gates anything."""
from __future__ import annotations

import argparse
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

SOURCES = ("gat_eig.hip", "gat_eig.h", "gat_eig_plan.h", "gat_eig_kernels.h", "gat_eig_api.cpp")
COV_SHAPES = ((1000, 12, 4), (65536, 64, 16))
EIG_SHAPES = ((12, 4), (64, 16), (64, 64))
L, TAP = 3, 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "subspace", "subspace_bench.json"))
    ap.add_argument("--settle", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--warm", type=int, default=50)
    args = ap.parse_args()
    import torch

    import gpuacceleratedtracking_amd as g
    from gpuacceleratedtracking_amd import _lib

    g.load_library()
    ctx = g.get_context()
    dev = ctx.device
    csrc = os.path.join(ROOT, "gpuacceleratedtracking_amd", "csrc")
    sha = hashlib.sha256()
    for name in SOURCES:
        with open(os.path.join(csrc, name), "rb") as fh:
            sha.update(fh.read())
    res = {"protocol": "device: settle launches, then timed launches, one HIP-event interval each, median; host: wall time, median", "settle": args.settle,
           "steps": args.steps, "host_reps": args.host_reps, "warm_launches": args.warm, "build": g.build.build_info(),
           "library": lib_record(_lib.library_path()), "subspace_sources_sha256": sha.hexdigest(), "covariance": {}, "eigensolver": {}}
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    warmed = False

    for B, K, M in COV_SHAPES:
        acc = [torch.randn((B, K, L, M), generator=gen, device=dev, dtype=torch.float32) for _ in range(2)]
        out = [None]

        def launch():
            out[0] = g.accumulator_covariance(acc[0], acc[1], tap_index=TAP, ctx=ctx)

        def host():
            t0 = time.perf_counter()
            ctx.sync()
            h = [a.cpu().numpy() for a in acc]
            t1 = time.perf_counter()
            x = h[0][:, :, TAP, :].astype(np.complex128)
            x.imag = h[1][:, :, TAP, :]
            cov = np.einsum("bki,bkj->kij", x, x.conj())
            return (t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3, cov

        launch()
        ctx.sync()
        got = out[0].cpu().numpy()[0]
        twin = g.accumulator_covariance_host(acc[0][:, :2].cpu().numpy(), acc[1][:, :2].cpu().numpy(), tap_index=TAP)[0]
        same = np.array_equal(got[:2].real.copy().view(np.int64), twin.real.copy().view(np.int64)) and \
            np.array_equal(got[:2].imag.copy().view(np.int64), twin.imag.copy().view(np.int64))
        plain = host()[2]
        err = float(np.abs(got - plain).max() / np.abs(plain).max())
        if not warmed:  # the process's first timing: bring the device up to its clocks first
            for _ in range(args.warm):
                launch()
            ctx.sync()
            warmed = True
        ms = median_ms(ctx, launch, args.settle, args.steps)
        reps = np.array([host()[:2] for _ in range(args.host_reps)])
        copy_ms, numpy_ms = float(np.median(reps[:, 0])), float(np.median(reps[:, 1]))
        rec = {"B": B, "K": K, "M": M, "L": L, "accumulator_bytes": 8 * B * K * L * M, "tap_bytes": 8 * B * K * M, "same_bits_as_twin": bool(same),
               "against_einsum_rel": err, "device_ms": ms, "copy_ms": copy_ms, "einsum_ms": numpy_ms, "host_path_ms": copy_ms + numpy_ms,
               "host_over_device": (copy_ms + numpy_ms) / ms, "plan": g.subspace_plan(B, K, L, M, TAP)}
        res["covariance"][f"B{B}_K{K}_M{M}"] = rec
        print(json.dumps(rec), flush=True)
        del acc, out

    rng = np.random.default_rng(2)
    for n, Q in EIG_SHAPES:
        x = rng.standard_normal((n, Q, 3 * Q)) + 1j * rng.standard_normal((n, Q, 3 * Q))
        a = torch.from_numpy(x @ x.conj().transpose(0, 2, 1)).to(dev)
        for R in (Q, 1):
            out = [None]

            def launch():
                out[0] = g.hermitian_eig(a, R, ctx=ctx)

            def host():
                t0 = time.perf_counter()
                ctx.sync()
                h = a.cpu().numpy()
                t1 = time.perf_counter()
                w, v = np.linalg.eigh(h)
                return (t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3, w

            launch()
            ctx.sync()
            lam, vec, status = (t.cpu().numpy() for t in out[0])
            t_lam, t_vec, t_status = g.hermitian_eig_host(a.cpu().numpy(), R)
            same = np.array_equal(lam.view(np.int64), t_lam.view(np.int64)) and np.array_equal(status, t_status) and \
                np.array_equal(vec.real.copy().view(np.int64), t_vec.real.copy().view(np.int64)) and \
                np.array_equal(vec.imag.copy().view(np.int64), t_vec.imag.copy().view(np.int64))
            w = host()[2]
            err = float(np.abs(lam - w[:, ::-1]).max() / np.abs(w).max())
            ms = median_ms(ctx, launch, args.settle, args.steps)
            reps = np.array([host()[:2] for _ in range(args.host_reps)])
            copy_ms, numpy_ms = float(np.median(reps[:, 0])), float(np.median(reps[:, 1]))
            rec = {"n": n, "Q": Q, "vectors": R, "same_bits_as_twin": bool(same), "against_eigh_rel": err, "sweeps": int(status.max()), "device_ms": ms,
                   "copy_ms": copy_ms, "eigh_ms": numpy_ms, "host_path_ms": copy_ms + numpy_ms, "host_over_device": (copy_ms + numpy_ms) / ms,
                   "plan": g.subspace_plan(eig_matrices=n, eig_order=Q, eig_vectors=R)}
            res["eigensolver"][f"n{n}_Q{Q}_R{R}"] = rec
            print(json.dumps(rec), flush=True)

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
