"""CPU forecast of tests/test_beam_stream_gpu.py::test_cold_start_under_the_jammer, on the library's own conventions and
without a device: the scene of tests/test_array_gpu.py with the satellite at --amp (default 0.25; the FP64 oracle's generator
times the scene's steering vector) plus scene_interference, FP64 power-inversion weights from the covariance of the first 8
blocks, tests/helpers.acq_power_oracle over the default grid (29 Doppler bins of 500 Hz x 2000 code bins, s = 2) of block 0
for PRNs 7, 3 and 20, on the 4 antennas and on the beam w^H x, and gat_acq_stats_host on each grid.  Prints one line per
search and PRN: detected, peak / second, refined Doppler and code phase, C/N0.  A few minutes of CPU time.

  python scripts/beam_cold_start_forecast.py [--amp 0.25]"""
from __future__ import annotations

import argparse
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--amp", type=float, default=0.25)
    amp = ap.parse_args().amp
    import oracle
    from gpuacceleratedtracking_amd import _lib
    from gpuacceleratedtracking_amd.acquisition import acquisition_stats_host
    from tests import array_ref
    from tests.helpers import acq_power_oracle
    from tests.test_array_gpu import SCENE, scene_directions, scene_interference

    N, M, fs, fc, nblk = SCENE["N"], SCENE["M"], SCENE["fs"], SCENE["fc"], 8
    dop, tau0, phi0 = SCENE["dop"], SCENE["tau0"], SCENE["phi0"]
    codes = oracle.codes("GPSL1", 32)
    fcode = fc * (1 + dop / 1575.42e6)
    ss, _ = scene_directions(SCENE["seed"])
    a = np.exp(2j * np.pi * ss.astype(np.float32).astype(np.float64))
    x = scene_interference(SCENE["seed"], nblk).numpy().astype(np.complex128)
    for b in range(nblk):
        tau = np.mod(tau0 + fcode * (N / fs) * b, 1023.0)
        phi = np.mod(phi0 + dop * (N / fs) * b, 1.0)
        re, im = oracle.gen_signal(codes, SCENE["prn"] - 1, fcode, fs, dop, tau, 2 * np.pi * phi, N, 1)
        x[:, b * N:(b + 1) * N] += amp * a[:, None] * (re[0] + 1j * im[0])[None, :]
    x = x.real.astype(np.float32).astype(np.float64) + 1j * x.imag.astype(np.float32).astype(np.float64)  # as the device holds it
    R = array_ref.covariance(x, N, nblk, nblk)[0]
    v = np.linalg.solve(R, np.eye(M)[0])
    w = v / np.conj(v[0])  # power inversion: R^-1 e0 / (e0^H R^-1 e0)
    y = (w.conj() @ x)[None, :]
    D, J, s = 29, 2000, 2
    cfg = _lib.AcqConfig()
    cfg.struct_size = ctypes.sizeof(_lib.AcqConfig)
    cfg.num_doppler_bins, cfg.num_code_bins, cfg.code_step_samples = D, J, s
    cfg.if_hz, cfg.code_freq_hz, cfg.doppler_first_hz, cfg.doppler_step_hz = 0.0, fc, -7000.0, 500.0
    cfg.first_shift, cfg.min_peak_ratio, cfg.code_length = 0, 2.0, 1023
    for name, sig in (("antennas", x), ("beam", y)):
        re, im = sig.real.astype(np.float32)[:, :N], sig.imag.astype(np.float32)[:, :N]
        grids = [acq_power_oracle(re, im, codes, col, fc, 1023, fs, 0.0, -7000.0, 500.0, np.arange(D), 0, s, np.arange(J), N, 1, N)
                 for col in (SCENE["prn"] - 1, 2, 19)]
        for prn, r in zip((SCENE["prn"], 3, 20), acquisition_stats_host(np.stack(grids).astype(np.float32), cfg, fs, N)):
            print(f"amp {amp} {name}: PRN {prn} detected {r['detected']} peak/second {r['peak_to_second']:.3f} "
                  f"Doppler {r['carrier_doppler_hz']:.1f} Hz code phase {r['code_phase_chips']:.3f} chips C/N0 {r['cn0_dbhz']:.1f} dB-Hz", flush=True)


if __name__ == "__main__":
    main()
