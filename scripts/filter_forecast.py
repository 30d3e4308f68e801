"""CPU forecast of tests/test_filter_pipeline_gpu.py, on the library's own conventions and without a device: the tests' satellites
from the FP64 oracle's generator, numpy noise of the tests' sigma, the tests' tone; gat_filter_samples_host (the bit-exact twin of
the device filter) with the tests' taps; a numpy search -- per Doppler bin a circular FFT correlation with the code replica over
one code period, |R|^2 added over antennas and blocks, subsampled to the search's code bins -- and gat_acq_stats_host on each
grid (detected = peak / second >= 2.0).  Prints per stream and code-table column: detected, peak / second, Doppler, code phase.

  python scripts/filter_forecast.py [--seed-offset 0]"""
from __future__ import annotations

import argparse
import ctypes
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def scene_stream(s, seed_offset):
    """complex128 [M, gen_blocks * N]: satellites (identical on every antenna) plus independent noise"""
    import oracle
    from tests import fir_ref as ref
    codes = oracle.codes("GPSL1", 32)
    prn0, fcode, f, tau, phi = ref.scene_params(s)
    N, B, M = s["N"], s["gen_blocks"], s["M"]
    rng = np.random.default_rng(s["noise_seed"] + seed_offset)
    x = ref.scene_sigma(s) * (rng.standard_normal((M, B * N)) + 1j * rng.standard_normal((M, B * N)))
    for b in range(B):
        for k in range(prn0.size):
            re, im = oracle.gen_signal(codes, int(prn0[k]), fcode[k], s["fs"], f[k], tau[b, k], 2 * np.pi * phi[b, k], N, 1)
            x[:, b * N:(b + 1) * N] += (re[0] + 1j * im[0])[None, :]
    return x, codes


def host_filter(x, taps, D, step):
    """the stream (complex [M, n], narrowed to float32 as the device holds it) through gat_filter_samples_host as one block"""
    from gpuacceleratedtracking_amd import filtering as f
    M, n = x.shape
    re, im = np.ascontiguousarray(x.real.astype(np.float32)), np.ascontiguousarray(x.imag.astype(np.float32))
    Q = f.num_outputs(n, len(taps), D)
    o_re, o_im = np.zeros((M, Q), np.float32), np.zeros((M, Q), np.float32)
    rc = f.filter_samples_host(f.host_desc(re, im, 0, M, n, n, n), 1, taps, f.host_desc(o_re, o_im, 0, M, Q, Q, Q), D, step, 0.0)
    assert rc == 0, rc
    return o_re.astype(np.float64) + 1j * o_im.astype(np.float64)


def search(y, codes, cols, fs, N, B, max_doppler, label):
    """the search of gpuacceleratedtracking_amd.acquire with its default grid on y [M, B * N] at baseband; prints the verdicts and
    returns the records"""
    from gpuacceleratedtracking_amd import _lib
    from gpuacceleratedtracking_amd.acquisition import acquisition_stats_host
    from tests.fir_ref import FC, LC
    s = max(1, int(round(0.5 * fs / FC)))
    J = int(math.ceil(LC * fs / (FC * s)))
    step = fs / (2.0 * N)
    nd = int(math.floor(max_doppler / step + 1e-9))
    dop = np.arange(-nd, nd + 1) * step
    n = np.arange(N)
    grids = np.zeros((len(cols), dop.size, J))
    for ci, col in enumerate(cols):
        rep = codes[col][np.floor(FC / fs * n).astype(np.int64) % LC].astype(np.float64)  # tau_b = 0: a block is one code period
        R = np.fft.fft(rep)
        for di, fd in enumerate(dop):
            mix = np.exp(-2j * np.pi * fd / fs * n)
            for m in range(y.shape[0]):
                for b in range(B):
                    a = y[m, b * N:(b + 1) * N] * mix                       # sum_n a[n] rep[n + k]
                    corr = np.fft.ifft(np.conj(np.fft.fft(np.conj(a))) * R)
                    grids[ci, di] += (np.abs(corr) ** 2)[np.arange(J) * s]
    cfg = _lib.AcqConfig()
    cfg.struct_size = ctypes.sizeof(_lib.AcqConfig)
    cfg.num_doppler_bins, cfg.num_code_bins, cfg.code_step_samples = dop.size, J, s
    cfg.if_hz, cfg.code_freq_hz, cfg.doppler_first_hz, cfg.doppler_step_hz = 0.0, FC, float(dop[0]), step
    cfg.first_shift, cfg.min_peak_ratio, cfg.code_length = 0, 2.0, LC
    res = acquisition_stats_host(grids.astype(np.float32), cfg, fs, N)
    for col, r in zip(cols, res):
        print(f"{label}: column {col} detected {r['detected']} peak/second {r['peak_to_second']:.3f} Doppler {r['carrier_doppler_hz']:.1f} Hz "
              f"code phase {r['code_phase_chips']:.3f} chips", flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed-offset", type=int, default=0)
    args = ap.parse_args()
    from gpuacceleratedtracking_amd import filtering as f
    from tests import fir_ref as ref

    # channelise: 100 MHz on a 12.5 MHz IF -> 20 MHz baseband
    s = ref.CHANNEL
    x, codes = scene_stream(s, args.seed_offset)
    nu = s["if_hz"] / s["fs"]
    taps = f.shift_taps(f.lowpass_taps(s["T"], s["cutoff_hz"] / s["fs"]), nu)
    y = host_filter(x[:, :ref.scene_used_samples(s)], taps, s["D"], nu)
    fs_out, N_out = s["fs"] / s["D"], s["N"] // s["D"]
    delay = (s["T"] - 1) / 2.0 / s["D"]
    tau, dop = ref.scene_truth(s, delay, fs_out)
    print(f"channelise: sigma {ref.scene_sigma(s):.2f}, {y.shape[1]} outputs at {fs_out / 1e6:.0f} MHz, group delay {delay:.2f} output samples; "
          f"truth: " + ", ".join(f"column {c}: {d:.0f} Hz {t:.3f} chips" for c, d, t in zip(s["present"], dop, tau)), flush=True)
    search(y, codes, s["cols"], fs_out, N_out, s["out_blocks"], s["max_doppler"], "channelised")

    # a CW tone at 20 MHz and its notch
    s = ref.NOTCH
    x, codes = scene_stream(s, args.seed_offset)
    x = x + ref.scene_tone(s)[None, :]
    used = ref.scene_used_samples(s)
    search(x[:, :s["out_blocks"] * s["N"]].astype(np.complex64).astype(np.complex128), codes, s["cols"], s["fs"], s["N"], s["out_blocks"], s["max_doppler"], "raw with tone")
    y = host_filter(x[:, :used], f.notch_taps(s["T"], s["nu"], s["width"]), 1, 0.0)
    tau, dop = ref.scene_truth(s, (s["T"] - 1) / 2.0, s["fs"])
    print(f"notch: sigma {ref.scene_sigma(s):.2f}, tone amplitude {np.abs(ref.scene_tone(s)[0]):.1f}; truth: " +
          ", ".join(f"column {c}: {d:.0f} Hz {t:.3f} chips" for c, d, t in zip(s["present"], dop, tau)), flush=True)
    search(y, codes, s["cols"], s["fs"], s["N"], s["out_blocks"], s["max_doppler"], "notched")
    # the notched stream requantised to int8 (target_rms 16: the statistics' sigma, round to nearest, clamp)
    sig = np.sqrt((np.abs(y) ** 2).mean() / 2.0)
    q = np.clip(np.rint(y.real * (16.0 / sig)), -127, 127) + 1j * np.clip(np.rint(y.imag * (16.0 / sig)), -127, 127)
    search(q, codes, s["cols"], s["fs"], s["N"], s["out_blocks"], s["max_doppler"], "notched int8")


if __name__ == "__main__":
    main()
