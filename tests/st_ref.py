"""numpy FP64 restatement of space-time adaptive processing (include/gat.h, "space-time adaptive processing"), independent of
libgat: the snapshot z[t M + m] = x[m, n - t], the covariance over a block's N - T + 1 snapshots, the filter y = sum_q conj(w_q)
z_q and the bound the float32 kernels are held to -- and the scene the pipeline tests share: two antennas, two CW jammers, one
weak satellite, with a numpy search on the library's conventions.  Samples are complex arrays [M, ld] holding B blocks of N
samples block_stride apart, as tests/beam_ref.py and tests/array_ref.py take them."""
from __future__ import annotations

import ctypes
import math

import numpy as np

U = 2.0 ** -24  # unit roundoff of float32


def snapshots(x, N, B, T, block_stride=None):
    """x [M, ld] -> z [B, Q, N - T + 1] (x's dtype): z[b, t M + m, n'] = x[m, b S + n' + T - 1 - t]"""
    S = N if block_stride is None else block_stride
    M, No = x.shape[0], N - T + 1
    z = np.empty((B, T * M, No), dtype=x.dtype)
    for b in range(B):
        for t in range(T):
            z[b, t * M:(t + 1) * M] = x[:, b * S + T - 1 - t:b * S + T - 1 - t + No]
    return z


def covariance(x, N, B, T, bpe, block_stride=None, dtype=np.complex128):
    """R_e[q, q'] = sum_{b in e} sum_{n'} z_q conj(z_q') over every snapshot of the blocks of estimate e, [E, Q, Q]; in `dtype`
    (complex64: a float32 reference, one matrix product per block, whose own error against complex128 is what float32 summation
    costs on these samples)"""
    z = snapshots(np.asarray(x).astype(dtype), N, B, T, block_stride)
    R = z @ z.conj().transpose(0, 2, 1)
    return R if bpe == 1 else np.add.reduceat(R, np.arange(0, B, bpe), axis=0)


def narrow(w):
    """complex128 of the float32 values the library works with"""
    w = np.asarray(w).astype(np.complex128)
    return w.real.astype(np.float32).astype(np.float64) + 1j * w.imag.astype(np.float32).astype(np.float64)


def filt(x, w, N, B, T, block_stride=None):
    """x complex128 [M, ld], w complex [J, Q] (the kernels' float32 narrowing is NOT applied: the bound covers it).  complex128
    [B, J, N - T + 1]."""
    z = snapshots(np.asarray(x, dtype=np.complex128), N, B, T, block_stride)
    return np.einsum("jq,bqn->bjn", np.asarray(w, dtype=np.complex128).conj(), z)


def bound(x, w, N, B, T, block_stride=None):
    """Per-sample bound on |y - y64|, float64 [B, J, N - T + 1]: the beam bound with Q for M, (4 Q + 4) 2^-24 sum_q |w_q| |z_q| -- a
    complex dot product of length Q is two real FMA chains of length 2 Q on weights rounded once, held to twice first order."""
    z = np.abs(snapshots(np.asarray(x, dtype=np.complex128), N, B, T, block_stride))
    Q = z.shape[1]
    return (4 * Q + 4) * U * np.einsum("jq,bqn->bjn", np.abs(np.asarray(w, dtype=np.complex128)), z)


def steering(a, T, ref_tap):
    """a_st[t M + m] = a[m] [t == ref_tap], complex128 [Q]"""
    a = np.asarray(a, dtype=np.complex128)
    st = np.zeros((T, a.size), np.complex128)
    st[ref_tap] = a
    return st.reshape(-1)


def weights(R, a_st):
    """R^-1 a / (a^H R^-1 a) in FP64 (numpy.linalg.solve), [Q]"""
    z = np.linalg.solve(np.asarray(R, dtype=np.complex128), a_st)
    return z / np.vdot(a_st, z)


# ---- the scene (tests/test_spacetime_host.py, tests/test_spacetime_pipeline_gpu.py) ------------------------------------------------
# GPS L1 at 20 MHz, one code period a block: two antennas, two CW jammers each 40 dB over the noise power with different
# frequencies AND directions -- one more interferer than the array alone can null --, one satellite 22 dB under the noise on both
# antennas alike.  T taps give 2 T - 1 degrees of freedom.  The stream is N + T - 1 samples long, so that the filtered stream is
# one whole code period.
FC, LC = 1.023e6, 1023
SCENE = dict(fs=20e6, N=20000, M=2, T=5, ref_tap=2, col=11, dop=1000.0, tau0=417.3, phi0=0.2, sat_db=-22.0, jam_db=40.0,
             nu=(0.11, -0.23), step=(0.2, 0.37), jam_phase=(0.3, 0.85), max_doppler=2500.0, noise_seed=17)


def scene_sigma(s=SCENE):
    """noise sigma per component: the satellite (amplitude 1) is sat_db under the noise power 2 sigma^2"""
    return float(np.sqrt(10.0 ** (-s["sat_db"] / 10.0) / 2.0))


def scene_stream(s=SCENE, seed_offset=0, satellite=True, jammers=True):
    """complex128 [M, N + T - 1]: the satellite from the FP64 oracle's generator, numpy noise, the two tones; and the code table"""
    import oracle
    codes = oracle.codes("GPSL1", 32)
    n_tot, M = s["N"] + s["T"] - 1, s["M"]
    rng = np.random.default_rng(s["noise_seed"] + seed_offset)
    x = scene_sigma(s) * (rng.standard_normal((M, n_tot)) + 1j * rng.standard_normal((M, n_tot)))
    if satellite:
        fcode = FC * (1 + s["dop"] / 1575.42e6)
        re, im = oracle.gen_signal(codes, s["col"], fcode, s["fs"], s["dop"], s["tau0"], 2 * np.pi * s["phi0"], n_tot, 1)
        x += (re[0] + 1j * im[0])[None, :]
    if jammers:
        n = np.arange(n_tot, dtype=np.float64)
        amp = np.sqrt(2.0) * scene_sigma(s) * 10.0 ** (s["jam_db"] / 20.0)
        for nu, st, ph in zip(s["nu"], s["step"], s["jam_phase"]):
            x += amp * np.exp(2j * np.pi * (nu * n[None, :] + st * np.arange(M)[:, None] + ph))
    return x, codes


def scene_truth(s, delay):
    """code phase (chips) at sample 0 of a stream that is the input advanced by `delay` samples"""
    return (s["tau0"] + delay * FC * (1 + s["dop"] / 1575.42e6) / s["fs"]) % LC


def search(y, codes, col, s=SCENE):
    """The search of gpuacceleratedtracking_amd.acquire with its default grid on ONE block y [N] at baseband: per Doppler bin a
    circular FFT correlation with the code replica over the block, |R|^2 subsampled to the search's code bins, and
    gat_acq_stats_host on the grid (detected = peak / second >= min_peak_ratio, default 2.0).  Returns the record."""
    from gpuacceleratedtracking_amd import _lib
    from gpuacceleratedtracking_amd.acquisition import acquisition_stats_host
    fs, N = s["fs"], s["N"]
    assert y.shape == (N,)
    cs = max(1, int(round(0.5 * fs / FC)))
    J = int(math.ceil(LC * fs / (FC * cs)))
    step = fs / (2.0 * N)
    nd = int(math.floor(s["max_doppler"] / step + 1e-9))
    dop = np.arange(-nd, nd + 1) * step
    n = np.arange(N)
    rep = codes[col][np.floor(FC / fs * n).astype(np.int64) % LC].astype(np.float64)
    R = np.fft.fft(rep)
    grid = np.zeros((1, dop.size, J))
    for di, fd in enumerate(dop):
        a = y * np.exp(-2j * np.pi * fd / fs * n)  # sum_n a[n] rep[n + k]
        corr = np.fft.ifft(np.conj(np.fft.fft(np.conj(a))) * R)
        grid[0, di] = (np.abs(corr) ** 2)[np.arange(J) * cs]
    cfg = _lib.AcqConfig()
    cfg.struct_size = ctypes.sizeof(_lib.AcqConfig)
    cfg.num_doppler_bins, cfg.num_code_bins, cfg.code_step_samples = dop.size, J, cs
    cfg.if_hz, cfg.code_freq_hz, cfg.doppler_first_hz, cfg.doppler_step_hz = 0.0, FC, float(dop[0]), step
    cfg.first_shift, cfg.min_peak_ratio, cfg.code_length = 0, 2.0, LC
    return acquisition_stats_host(grid.astype(np.float32), cfg, fs, N)[0]
