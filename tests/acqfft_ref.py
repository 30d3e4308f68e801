"""What the tests of the FFT acquisition search (gat_acquire_fft, gat_acquire_fft_host; csrc/gat_acq_fft.h) share: the shapes that
reach every instance, the scenes (satellites in noise, so that every Doppler row has a floor, in the four sample layouts), the
configuration record, the host twin's call and the bins to sample: the grid's ends, the first and last lag of every lag segment
(the seams), the peak and a few random ones.  The FP64 reference is tests/helpers.acq_power_oracle: the contract itself."""
from __future__ import annotations

import ctypes as C

import numpy as np

import oracle

FC, LC = 1.023e6, 1023
PLANAR, CF32, I16, I8 = 0, 1, 2, 3
PRNS = [3, 17, 30]
F_FIRST, F_STEP = -5000.0, 250.0

# name: layout, M, B, N, block_stride, fs, s, first_shift, J, D, if_hz, acq_fft_log2 (0: the plan's choice)
SHAPES = {
    "one-pass": (PLANAR, 1, 1, 2000, 2000, 2.0e6, 1, 0, 2000, 9, 0.0, 12),            # F = 4096, one segment
    "two-pass-two-segments": (CF32, 1, 1, 5000, 5000, 5.0e6, 1, 0, 5115, 5, 1.0e4, 13),  # F = 8192: Jseg = 3193, G = 2
    "odd-blocks": (PLANAR, 2, 3, 4001, 4100, 4.0e6, 3, -37, 700, 7, -2.5e3, 0),       # the plan takes F = 8192; s = 3
    "int16": (I16, 2, 2, 2000, 2011, 2.0e6, 2, 5, 900, 5, 0.0, 12),                   # F = 4096
    "int8": (I8, 1, 2, 3000, 3000, 3.0e6, 1, -3, 3069, 5, 500.0, 12),                 # F = 4096: Jseg = 1097, G = 3
}
SCALE = {PLANAR: 1.0, CF32: 1.0, I16: 1000.0, I8: 20.0}


def config(g, D, J, s, first_shift=0, f_first=F_FIRST, f_step=F_STEP, if_hz=0.0, lc=LC, fc=FC):
    cfg = g._lib.AcqConfig()
    cfg.struct_size = C.sizeof(g._lib.AcqConfig)
    cfg.num_doppler_bins, cfg.num_code_bins, cfg.code_step_samples = D, J, s
    cfg.if_hz, cfg.code_freq_hz, cfg.doppler_first_hz, cfg.doppler_step_hz = if_hz, fc, f_first, f_step
    cfg.first_shift, cfg.min_peak_ratio, cfg.code_length = first_shift, 2.0, lc
    return cfg


def scene(seed, layout, M, ld, fs, if_hz, prns=PRNS, noise=0.5):
    """The searched satellites (one on a Doppler bin, two between) in noise, as tests/test_acquisition_gpu.py builds them.  Returns
    (host arrays in `layout` [M, ld(, 2)], re, im float32 [M, ld]: the same values planar for the oracle)."""
    rng = np.random.default_rng(seed)
    codes = oracle.codes("GPSL1", 32)
    x = np.zeros(ld, dtype=np.complex128)
    for k, p in enumerate(prns):
        r1, i1 = oracle.gen_signal(codes, p, FC, fs, if_hz + 250.0 * (k - 1) + 100.0 * k, rng.uniform(0, LC), 0.3 * k, ld, 1)
        x += r1[0] + 1j * i1[0]
    x = x[None, :] * np.exp(2j * np.pi * rng.uniform(0, 1, (M, 1))) + noise * (rng.standard_normal((M, ld)) + 1j * rng.standard_normal((M, ld)))
    x = x * SCALE[layout]
    if layout in (I16, I8):
        dt = np.int16 if layout == I16 else np.int8
        lim = np.iinfo(dt).max
        pair = np.ascontiguousarray(np.clip(np.stack([np.rint(x.real), np.rint(x.imag)], axis=-1), -lim, lim).astype(dt))
        return (pair,), pair[..., 0].astype(np.float32), pair[..., 1].astype(np.float32)
    re, im = np.ascontiguousarray(x.real.astype(np.float32)), np.ascontiguousarray(x.imag.astype(np.float32))
    if layout == PLANAR:
        return (re, im), re, im
    return (np.ascontiguousarray(np.stack([re, im], axis=-1)),), re, im


def length(B, N, bstride):
    return (B - 1) * bstride + N + 7


def host_desc(g, arrays, layout, M, N, ld, bstride):
    from gpuacceleratedtracking_amd.frontend import host_desc as hd
    return hd(arrays[0], arrays[1] if layout == PLANAR else None, layout, M, N, ld, bstride)


def plan(g, desc, B, P, fs, cfg, log2=0, num_cus=256, dbatch=0, ubatch=0, own_power=False):
    from gpuacceleratedtracking_amd.acquisition import acquire_fft_plan
    return acquire_fft_plan(desc, B, P, fs, cfg, fft_log2=log2, doppler_batch=dbatch, unit_batch=ubatch, num_cus=num_cus, own_power=own_power)


def twin(g, desc, B, prns, fs, cfg, log2, groups=1):
    from gpuacceleratedtracking_amd.acquisition import acquire_fft_host
    return acquire_fft_host(desc, B, oracle.codes("GPSL1", 32), prns, fs, cfg, log2, groups)


def sample_bins(rng, J, s, N, log2, extra=(), n_random=24):
    """Code bins to compare: the ends, both sides of every seam between lag segments, `extra` (the peak) and random ones."""
    jseg = (1 << log2) - N + 1
    c = [0, J - 1, *extra, *rng.choice(J, min(J, n_random), replace=False)]
    o = jseg
    while o <= s * (J - 1):  # the last bin at a lag below the seam and the first at or above it
        c += [(o - 1) // s, -(-o // s)]
        o += jseg
    return np.unique([j for j in c if 0 <= j < J]).astype(np.int64)
