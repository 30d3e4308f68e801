"""numpy FP64 restatement of the sample filter (include/gat.h, "sample filtering"), independent of libgat: the "valid"
convolution, the decimation and the oscillator on the stream position, with the library's definition of theta -- step reduced
to [-1/2, 1/2] and phase to [0, 1], theta = P * step + phase -- evaluated in extended precision, and the sum of absolute
products S the error bound is stated in.  Samples are logical arrays [B, M, N]; the layout helpers (tests/cond_ref.py's) put them
into the four memory layouts with any strides."""
from __future__ import annotations

import numpy as np

from tests.cond_ref import (CF32, DTYPE, I8, I16, LAYOUTS, LIMIT, PLANAR, get, index, make_buffers, put, random_samples,  # noqa: F401
                            same_bits)

OUT_LAYOUTS = (PLANAR, CF32)
VEC_SAMPLES = {PLANAR: 4, CF32: 2, I16: 4, I8: 8}  # samples of a 16-byte load or store


def num_outputs(N, T, D):
    return (N - T) // D + 1


def narrow_taps(taps):
    """complex128 of the float32 values the library works with"""
    g = np.asarray(taps).astype(np.complex128)
    return g.real.astype(np.float32).astype(np.float64) + 1j * g.imag.astype(np.float32).astype(np.float64)


def fir(xr, xi, taps, D=1, step=0.0, phase=0.0, block_stride=None):
    """xr, xi: [B, M, N] of any real dtype (converted exactly); taps: complex [T] (narrowed to float32 first).  Returns (y, S, P):
    complex128 [B, M, Q], S = sum_t (|g_re| + |g_im|)(|x_re| + |x_im|) [B, M, Q] and the stream positions P [B, Q] (float64)."""
    x = np.asarray(xr, np.float64) + 1j * np.asarray(xi, np.float64)
    B, M, N = x.shape
    g = narrow_taps(taps)
    T = g.size
    bs = N if block_stride is None else block_stride
    win = np.lib.stride_tricks.sliding_window_view(x, T, axis=-1)[:, :, ::D, :]  # [B, M, Q, T]: x[q D + k]
    z = win @ g[::-1]                                                           # sum_t g[t] x[q D + T - 1 - t]
    ax = np.abs(np.asarray(xr, np.float64)) + np.abs(np.asarray(xi, np.float64))
    S = np.lib.stride_tricks.sliding_window_view(ax, T, axis=-1)[:, :, ::D, :] @ (np.abs(g.real) + np.abs(g.imag))[::-1]
    Q = z.shape[2]
    P = np.arange(B, dtype=np.float64)[:, None] * bs + np.arange(Q, dtype=np.float64)[None, :] * D + (T - 1)
    if step == 0.0 and phase == 0.0:
        return z, S, P
    ld = np.longdouble
    st, ph = ld(step) - ld(np.rint(step)), ld(phase) - ld(np.floor(phase))
    theta = P.astype(ld) * st + ph
    theta -= np.rint(theta)
    ang = (2 * ld(np.pi)) * theta  # (np.pi is a double: its error, 1.2e-16 rad relative, is far below the bound's terms)
    rot = np.cos(ang).astype(np.float64) - 1j * np.sin(ang).astype(np.float64)
    return z * rot[:, None, :], S, P


def bound(T, S, P):
    """per component: [(2T + 8) 2^-24 + 2 pi 2^-53 (P/2 + 2)] S -- 2T sequential FMAs, the rotation's polynomial and roundings, the
    double rounding of theta (the sample filter)"""
    return ((2 * T + 8) * 2.0 ** -24 + 2 * np.pi * 2.0 ** -53 * (P[:, None, :] / 2 + 2)) * S


def guard_of(bufs):
    return [b.copy() for b in bufs]


def unchanged_outside(bufs, before, layout, idx):
    """every element of the buffers outside the indexed ones still holds what it held"""
    for b, b0 in zip(bufs, before):
        mask = np.ones(b.shape[0], bool)
        mask[idx.reshape(-1)] = False
        if not same_bits(b[mask], b0[mask]):
            return False
    return True


# ---- the pipeline scenes (tests/test_filter_pipeline_gpu.py and their CPU forecast, scripts/filter_forecast.py) ------------------
# GPS L1, satellites of amplitude 1 in complex white noise of sigma per component: C/N0 = fs / (2 sigma^2).  Blocks of 1 ms; the
# generators make `gen_blocks` of them and the filters use the first out_blocks * N_out * D + T - 1 samples, so that the filtered
# stream is out_blocks whole code periods.  `cols` are the code-table columns searched: `present` and as many absent ones.
FC, LC, L1 = 1.023e6, 1023, 1575.42e6
# a wideband front end: 100 MHz, the band of interest on a 12.5 MHz IF; channelised to 20 MHz baseband (D = 5, 64 taps, cutoff
# 5 MHz: flat over the C/A main lobe, 80 dB down from 9 MHz on, where the band begins to alias into 20 MHz)
CHANNEL = dict(fs=100e6, if_hz=12.5e6, M=2, N=100000, gen_blocks=3, out_blocks=2, D=5, T=64, cutoff_hz=5e6, present=[4, 12, 25], cols=[4, 9, 12, 17, 25, 30],
               dop=[1800.0, -3100.0, 400.0], tau0=[211.3, 640.75, 999.1], phi0=[0.1, 0.45, 0.8], cn0_dbhz=45.0, max_doppler=5000.0, noise_seed=3)
# a 20 MHz stream with a CW tone 40 dB over the noise power in 20 MHz, 3.1 MHz off the carrier; the notch: 65 taps, 200 kHz wide
NOTCH = dict(fs=20e6, if_hz=0.0, M=2, N=20000, gen_blocks=3, out_blocks=2, D=1, T=65, width=0.01, nu=0.155, tone_db=40.0, tone_phase=0.3,
             present=[2, 21], cols=[2, 7, 21, 28], dop=[-2250.0, 3900.0], tau0=[87.6, 512.2], phi0=[0.6, 0.05], cn0_dbhz=47.0, max_doppler=5000.0,
             noise_seed=4)


def scene_sigma(s):
    return float(np.sqrt(s["fs"] / (2.0 * 10.0 ** (s["cn0_dbhz"] / 10.0))))


def scene_used_samples(s):
    """input samples the filter takes: out_blocks code periods of outputs"""
    return s["out_blocks"] * (s["N"] // s["D"]) * s["D"] + s["T"] - 1


def scene_params(s):
    """[gen_blocks, K] channel values, block b continuing block b - 1: (prn0, fcode, carrier f, tau, phi in cycles)"""
    dop, b = np.array(s["dop"]), np.arange(s["gen_blocks"], dtype=np.float64)[:, None]
    fcode = FC * (1 + dop / L1)
    f = s["if_hz"] + dop
    dt = s["N"] / s["fs"]
    tau = np.mod(np.array(s["tau0"])[None, :] + fcode[None, :] * dt * b, float(LC))
    phi = np.mod(np.array(s["phi0"])[None, :] + f[None, :] * dt * b, 1.0)
    return np.array(s["present"]), fcode, f, tau, phi


def scene_tone(s):
    """complex128 [gen_blocks * N]: the CW tone, `tone_db` over the noise power 2 sigma^2"""
    n = np.arange(s["gen_blocks"] * s["N"], dtype=np.float64)
    return np.sqrt(2.0) * scene_sigma(s) * 10.0 ** (s["tone_db"] / 20.0) * np.exp(2j * np.pi * (s["nu"] * n + s["tone_phase"]))


def scene_truth(s, delay_out, fs_out):
    """code phase (chips) at output sample 0 and Doppler of the present satellites: output q shows the input `delay_out` output
    samples after q's own time, so the code has advanced by delay_out * fc / fs_out chips"""
    return [(t + delay_out * FC / fs_out) % LC for t in s["tau0"]], list(s["dop"])
