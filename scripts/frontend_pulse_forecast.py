"""CPU forecast of tests/test_condition_pipeline_gpu.py::test_blanking_uncovers_the_satellites_under_pulsed_interference, on the
library's own conventions and without a device: the test's two satellites from the FP64 oracle's generator, numpy noise of the
test's sigma, the test's pulses; the numpy restatement (tests/cond_ref.py) of {statistics under the last threshold, AGC} x
iterations and of the conditioning to int8; tests/helpers.acq_power_oracle over the whole search grid of the raw stream and of
the blanked int8 stream; gat_acq_stats_host on each grid.  Prints per stream and PRN column: detected, peak / second, Doppler,
code phase; and the blanked fraction.  About a minute of CPU time.

  python scripts/frontend_pulse_forecast.py [--noise-seed 5]"""
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
    ap.add_argument("--noise-seed", type=int, default=5)
    args = ap.parse_args()
    import oracle
    from gpuacceleratedtracking_amd import _lib, frontend
    from gpuacceleratedtracking_amd.acquisition import acquisition_stats_host
    from tests import cond_ref as ref
    from tests.cond_ref import PULSED as s, pulsed_params, pulses
    from tests.helpers import acq_power_oracle

    N, B, fs, fc = s["N"], s["B"], s["fs"], s["fc"]
    codes = oracle.codes("GPSL1", 32)
    prn0, fcode, dop, tau, phi = pulsed_params()
    rng = np.random.default_rng(args.noise_seed)
    x = s["sigma"] * (rng.standard_normal(B * N) + 1j * rng.standard_normal(B * N)) + pulses()
    for b in range(B):
        for k in range(prn0.size):
            re, im = oracle.gen_signal(codes, int(prn0[k]), fcode[k], fs, dop[k], tau[b, k], 2 * np.pi * phi[b, k], N, 1)
            x[b * N:(b + 1) * N] += re[0] + 1j * im[0]
    re, im = x.real.astype(np.float32)[None, :], x.imag.astype(np.float32)[None, :]  # as the device holds it

    # requantize(blank_factor, iterations): statistics under the last threshold, AGC, ... then the conversion
    vr, vi = (v.reshape(1, B, N).transpose(1, 0, 2) for v in (re, im))
    rec = None
    for it in range(s["iterations"]):
        st = ref.stats(vr, vi, None if rec is None else rec["threshold"])
        p64 = ref.agc(st, 16.0, s["blank_factor"])
        rec = np.zeros(1, dtype=frontend.COND_PARAMS_DTYPE)
        rec["scale"], rec["dc_re"], rec["dc_im"], rec["threshold"] = (p64[:, i].astype(np.float32) for i in range(4))
        print(f"round {it}: kept {int(st['kept'][0])} threshold {float(rec['threshold'][0]) / s['sigma']:.2f} sigma", flush=True)
    qr, qi, cnt = ref.condition(vr, vi, rec, ref.I8)
    print(f"blanked {int(cnt[0, 0])} of {B * N} ({cnt[0, 0] / (B * N):.3%}), clipped {int(cnt[0, 1])}", flush=True)
    q_re, q_im = (q.transpose(1, 0, 2).reshape(1, B * N).astype(np.float32) for q in (qr, qi))

    step = fs / (2.0 * N)
    nd = int(np.floor(s["max_doppler"] / step + 1e-9))
    D, J = 2 * nd + 1, N
    cfg = _lib.AcqConfig()
    cfg.struct_size = ctypes.sizeof(_lib.AcqConfig)
    cfg.num_doppler_bins, cfg.num_code_bins, cfg.code_step_samples = D, J, 1
    cfg.if_hz, cfg.code_freq_hz, cfg.doppler_first_hz, cfg.doppler_step_hz = 0.0, fc, -nd * step, step
    cfg.first_shift, cfg.min_peak_ratio, cfg.code_length = 0, 2.0, 1023
    for name, (a, b_) in (("raw", (re, im)), ("blanked int8", (q_re, q_im))):
        grids = [acq_power_oracle(a, b_, codes, col, fc, 1023, fs, 0.0, -nd * step, step, np.arange(D), 0, 1, np.arange(J), N, B, N)
                 for col in s["cols"]]
        for col, r in zip(s["cols"], acquisition_stats_host(np.stack(grids).astype(np.float32), cfg, fs, N)):
            print(f"{name}: column {col} detected {r['detected']} peak/second {r['peak_to_second']:.3f} Doppler {r['carrier_doppler_hz']:.1f} Hz "
                  f"code phase {r['code_phase_chips']:.3f} chips", flush=True)


if __name__ == "__main__":
    main()
