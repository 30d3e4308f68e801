"""numpy FP64 restatement of the sample spectrum (include/gat.h, "sample spectrum"), independent of libgat: the windowed segments
in float64 (a float32 window times a float32 or integer sample is exact there), numpy's FFT in complex128, the squared magnitudes
and their sum over the segments, with the sum of absolute products A the error bound is stated in.  Samples are logical arrays
[B, M, N]; the layout helpers (tests/cond_ref.py's) put them into the four memory layouts with any strides.  The tone scenes of
tests/test_spectrum_host.py and the window forms are here too."""
from __future__ import annotations

import numpy as np

from tests.cond_ref import (CF32, DTYPE, I8, I16, LAYOUTS, LIMIT, PLANAR, get, index, make_buffers, put, random_samples,  # noqa: F401
                            same_bits)

VEC_SAMPLES = {PLANAR: 4, CF32: 2, I16: 4, I8: 8}  # samples of a 16-byte load
U = 2.0 ** -24


def num_segments(N, F, H):
    return (N - F) // H + 1


def window(name, F):
    """float32 [F]: the periodic form, computed in float64 and narrowed once"""
    x = 2.0 * np.pi * np.arange(F, dtype=np.float64) / F
    w = {"hann": 0.5 - 0.5 * np.cos(x), "hamming": 0.54 - 0.46 * np.cos(x), "blackman": 0.42 - 0.5 * np.cos(x) + 0.08 * np.cos(2.0 * x),
         "rect": np.ones(F)}[name]
    return w.astype(np.float32)


def segments(xr, xi, w, F, H):
    """complex128 [B, M, S, F]: w[n] x[s H + n], exact; and A [B, M, S] = sum_n |w[n]| (|x_re| + |x_im|)"""
    w64 = np.asarray(w, np.float32).astype(np.float64)
    x = np.asarray(xr, np.float64) + 1j * np.asarray(xi, np.float64)
    S = num_segments(x.shape[-1], F, H)
    seg = np.lib.stride_tricks.sliding_window_view(x, F, axis=-1)[:, :, ::H, :][:, :, :S, :]
    v = seg * w64
    with np.errstate(invalid="ignore"):
        A = ((np.abs(seg.real) + np.abs(seg.imag)) * np.abs(w64)).sum(axis=-1)
    return v, A


def spectrum(xr, xi, w, F, H):
    """(power64 [B, M, F], p64 [B, M, S, F], A [B, M, S]): the FP64 sums, the segments' own spectra and the bound's A"""
    v, A = segments(xr, xi, w, F, H)
    X = np.fft.fft(v, axis=-1)
    p = X.real * X.real + X.imag * X.imag
    return p.sum(axis=2), p, A


def bound_x(F, A):
    """|X - X64| per component (and in modulus): (11 log2 F + 1) u A -- one rounding of the windowed sample, and per stage the
    twiddle's error 5 sqrt(2) u, two roundings of the product and one of the sum, 5 sqrt(2) + 3 < 11"""
    return (11.0 * np.log2(F) + 1.0) * U * A


def bound_power(F, A):
    """|power - power64| [B, M] per bin: per segment (2 A + E) E + 2 u (1 + u) (A + E)^2 with E = bound_x -- |X| <= A, the two
    roundings of p --, summed, plus the sequential float32 sum's (S - 1) u / (1 - (S - 1) u) times the sum of the terms' bounds"""
    E = bound_x(F, A)
    big = (A + E) ** 2
    per = (2.0 * A + E) * E + 2.0 * U * (1.0 + U) * big
    S = A.shape[-1]
    g = (S - 1) * U / (1.0 - (S - 1) * U)
    return per.sum(axis=-1) + g * (big * (1.0 + 2.0 * U * (1.0 + U))).sum(axis=-1)


def host_spectrum(sp, layout, xr, xi, w, F, H, ant_stride=None, block_stride=None, offset=0):
    """the library's host twin over logical samples [B, M, N] put into `layout` with the given strides: float32 [B, M, F]
    (sp: the package's spectrum module)"""
    from gpuacceleratedtracking_amd.frontend import host_desc
    B, M, N = np.asarray(xr).shape
    bs = N if block_stride is None else block_stride
    a_s = (B - 1) * bs + N if ant_stride is None else ant_stride
    bufs = make_buffers(layout, B, M, N, a_s, bs, offset)
    put(bufs, layout, index(B, M, N, a_s, bs, offset), xr, xi)
    out = np.full((B, M, F), -3.25, np.float32)
    rc = sp.sample_spectrum_host(host_desc(bufs[0], bufs[1] if layout == PLANAR else None, layout, M, N, a_s, bs, offset), B,
                                 np.ascontiguousarray(w, np.float32), F, H, out)
    assert rc == 0, rc
    return out


# ---- the tone scenes (tests/test_spectrum_host.py) -------------------------------------------------------------------------------
# two antennas x 40000 samples of complex white noise, sigma = 14.13 per component (tests/fir_ref.py NOTCH's level), and one CW tone
TONE_SCENE = dict(M=2, N=40000, sigma=14.13, F=1024, H=512, seed=11)
TONE_NUS = (0.155, 0.1553, -0.31207, 0.0004883, 0.4999)
TONE_AMPS = (1997.6, 141.3, 44.7)


def tone_scene(tones, seed=None, s=TONE_SCENE):
    """float32 (re, im) [1, M, N]: noise plus the tones [(nu, amplitude, phase in cycles), ...], the same on every antenna"""
    rng = np.random.default_rng(s["seed"] if seed is None else seed)
    x = s["sigma"] * (rng.standard_normal((1, s["M"], s["N"])) + 1j * rng.standard_normal((1, s["M"], s["N"])))
    n = np.arange(s["N"], dtype=np.float64)
    for nu, amp, ph in tones:
        x = x + amp * np.exp(2j * np.pi * (nu * n + ph))[None, None, :]
    return x.real.astype(np.float32), x.imag.astype(np.float32)
