"""numpy restatements of the sample conditioner (include/gat.h, "sample conditioning"), independent of libgat: the rule in
float32 -- np.float32 subtract, multiply, np.rint (ties to even), clip -- and the level statistics in FP64 with the sums of
absolute values their bounds are stated in.  Samples are logical arrays [B, M, N]; the layout helpers put them into the four
memory layouts with any strides."""
from __future__ import annotations

import numpy as np

PLANAR, CF32, I16, I8 = 0, 1, 2, 3
LAYOUTS = (PLANAR, CF32, I16, I8)
DTYPE = {PLANAR: np.float32, CF32: np.float32, I16: np.int16, I8: np.int8}
LIMIT = {I16: 32767, I8: 127}


def condition(xr, xi, params, out_layout, blank_all=False):
    """xr, xi: float32 [B, M, N] (integer samples converted exactly); params: [M] records (scale, dc_re, dc_im, threshold).
    Returns (yr, yi, counts): the output components in the output's dtype and uint64 [M, 2] = (blanked, clipped)."""
    xr, xi = np.asarray(xr, np.float32), np.asarray(xi, np.float32)
    M = xr.shape[1]
    p = np.asarray(params)
    scale, dc_re, dc_im, T = (p[name].astype(np.float32).reshape(1, M, 1) for name in ("scale", "dc_re", "dc_im", "threshold"))
    with np.errstate(invalid="ignore", over="ignore"):
        keep = (np.abs(xr) <= T) & (np.abs(xi) <= T)  # a NaN component compares false
        if blank_all:
            keep = np.broadcast_to(keep.all(axis=1, keepdims=True), keep.shape)
        out, clipped = [], np.zeros(xr.shape, np.int64)
        for x, dc in ((xr, dc_re), (xi, dc_im)):
            t = np.subtract(x, dc, dtype=np.float32)
            y = np.multiply(t, scale, dtype=np.float32)
            if out_layout in LIMIT:
                lim = LIMIT[out_layout]
                r = np.rint(y)
                nan = np.isnan(y)
                clip = (nan | (np.abs(r) > lim)) & keep
                code = np.where(nan, np.float32(0), np.clip(r, -lim, lim))
                out.append(np.where(keep, code, np.float32(0)).astype(DTYPE[out_layout]))
                clipped += clip
            else:
                out.append(np.where(keep, y, np.float32(0)).astype(np.float32))  # a blanked sample is +0.0
    counts = np.stack([(~keep).sum(axis=(0, 2)), clipped.sum(axis=(0, 2))], axis=1).astype(np.uint64)
    return out[0], out[1], counts


def stats(xr, xi, thresholds=None, blank_all=False):
    """FP64 restatement over [B, M, N] (one estimate): a dict of [M] arrays -- kept, blanked, sum_re, sum_im, sum_pow, max_abs and
    abs_re, abs_im (sum |x| per component: what the 1e-5 bound of a signed sum is stated in)."""
    xr32, xi32 = np.asarray(xr, np.float32), np.asarray(xi, np.float32)
    M = xr32.shape[1]
    T = np.full(M, np.inf, np.float32) if thresholds is None else np.asarray(thresholds, np.float32)
    with np.errstate(invalid="ignore"):
        keep = (np.abs(xr32) <= T.reshape(1, M, 1)) & (np.abs(xi32) <= T.reshape(1, M, 1))
    if blank_all:
        keep = np.broadcast_to(keep.all(axis=1, keepdims=True), keep.shape)
    xr64, xi64 = np.where(keep, xr32, 0).astype(np.float64), np.where(keep, xi32, 0).astype(np.float64)
    ax = (0, 2)
    big = np.where(keep, np.maximum(np.abs(xr32), np.abs(xi32)), np.float32(0))
    return dict(kept=keep.sum(axis=ax), blanked=(~keep).sum(axis=ax), sum_re=xr64.sum(axis=ax), sum_im=xi64.sum(axis=ax),
                sum_pow=(xr64 * xr64 + xi64 * xi64).sum(axis=ax), max_abs=big.max(axis=ax).astype(np.float32),
                abs_re=np.abs(xr64).sum(axis=ax), abs_im=np.abs(xi64).sum(axis=ax))


def agc(st, target_rms, blank_factor=0.0, remove_dc=False):
    """FP64 formula of gat_agc_update for [M] statistics; returns float64 (scale, dc_re, dc_im, threshold) before narrowing."""
    kept = np.asarray(st["kept"], np.float64)
    out = np.zeros((kept.size, 4))
    out[:, 3] = np.inf
    with np.errstate(divide="ignore", invalid="ignore"):
        sigma = np.sqrt(np.asarray(st["sum_pow"], np.float64) / (2.0 * kept))
    ok = (kept > 0) & (sigma > 0) & np.isfinite(sigma)
    out[ok, 0] = target_rms / sigma[ok]
    if remove_dc:
        out[ok, 1] = np.asarray(st["sum_re"], np.float64)[ok] / kept[ok]
        out[ok, 2] = np.asarray(st["sum_im"], np.float64)[ok] / kept[ok]
    if blank_factor > 0:
        out[ok, 3] = blank_factor * sigma[ok]
    return out


def records(fe, M, scale=1.0, dc_re=0.0, dc_im=0.0, threshold=np.inf):
    """[M] gat_cond_params records (fe: the package's frontend module, for the record's dtype); scalars broadcast"""
    p = np.zeros(M, dtype=fe.COND_PARAMS_DTYPE)
    p["scale"], p["dc_re"], p["dc_im"], p["threshold"] = scale, dc_re, dc_im, threshold
    return p


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape
    return np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ---- memory layouts ------------------------------------------------------------------------------------------------------------
def elems(layout):
    """array elements per sample in the buffer(s) of a layout"""
    return 1 if layout == PLANAR else 2


def make_buffers(layout, B, M, N, ant_stride, block_stride, offset=0, fill=None):
    """Buffer(s) holding B blocks x M antennas x N samples at element n + m * ant_stride + b * block_stride + offset, with
    `offset` samples before and 3 after; fill: the sentinel value the rest holds."""
    total = offset + (B - 1) * block_stride + (M - 1) * ant_stride + N + 3
    dt = DTYPE[layout]
    sent = fill if fill is not None else (77 if layout in LIMIT else 7.5e8)
    if layout == PLANAR:
        return [np.full(total, sent, dt), np.full(total, sent, dt)]
    return [np.full((total, 2), sent, dt)]


def index(B, M, N, ant_stride, block_stride, offset=0):
    b, m, n = np.meshgrid(np.arange(B), np.arange(M), np.arange(N), indexing="ij")
    return offset + n + m * ant_stride + b * block_stride


def put(bufs, layout, idx, vr, vi):
    if layout == PLANAR:
        bufs[0][idx], bufs[1][idx] = vr, vi
    else:
        bufs[0][idx, 0], bufs[0][idx, 1] = vr, vi


def get(bufs, layout, idx):
    if layout == PLANAR:
        return bufs[0][idx], bufs[1][idx]
    return bufs[0][idx, 0], bufs[0][idx, 1]


def random_samples(rng, layout, shape, special=True):
    """Values of a layout's dtype with the rule's edge cases sprinkled in for the float layouts (NaN, +-inf, -0.0)."""
    if layout in LIMIT:
        lim = LIMIT[layout]
        return (rng.integers(-lim - 1, lim + 1, shape).astype(DTYPE[layout]), rng.integers(-lim - 1, lim + 1, shape).astype(DTYPE[layout]))
    vr, vi = (rng.standard_normal(shape).astype(np.float32) * np.float32(40.0) for _ in range(2))
    if special and vr.size >= 8:
        flat = vr.reshape(-1)
        pos = rng.choice(flat.size, size=min(6, flat.size), replace=False)
        flat[pos[:6]] = np.array([np.nan, np.inf, -np.inf, -0.0, 0.5, 1e30], np.float32)[:pos.size]
    return vr, vi


# ---- the pulsed-interference scene (tests/test_condition_pipeline_gpu.py and its CPU forecast, scripts/frontend_pulse_forecast.py) ----
# GPS L1 at 2.048 MHz: a 1 ms block is 2048 samples (a multiple of 8, so int8 blocks stay back to back: the search takes the
# code phase of block b from b * block_stride), the code bin is one sample (half a chip), the Doppler bin 500 Hz.
PULSED = dict(fs=2.048e6, N=2048, B=4, fc=1.023e6, cols=[6, 2, 18, 27], present=[6, 18], dop=[1100.0, -1400.0], tau0=[300.25, 811.6],
              phi0=[0.15, 0.7], sigma=4.0, max_doppler=2500.0, noise_seed=5, pulse_seed=17, duty=0.10, burst=16, pulse_db=40.0,
              blank_factor=4.0, iterations=4)


def pulsed_params():
    """[B, 2] channel values of the two present satellites, block b continuing block b - 1: (prn0, fcode, f, tau, phi in cycles)"""
    s = PULSED
    dop, b = np.array(s["dop"]), np.arange(s["B"], dtype=np.float64)[:, None]
    fcode = s["fc"] * (1 + dop / 1575.42e6)
    tau = np.mod(np.array(s["tau0"])[None, :] + fcode[None, :] * (s["N"] / s["fs"]) * b, 1023.0)
    phi = np.mod(np.array(s["phi0"])[None, :] + dop[None, :] * (s["N"] / s["fs"]) * b, 1.0)
    return np.array(s["present"]), fcode, dop, tau, phi


def pulses():
    """complex128 [B * N]: bursts of `burst` samples at random places covering about `duty` of the stream, each a tone of its own
    frequency and phase whose power is `pulse_db` over the noise power 2 sigma^2 (fixed seed)"""
    s = PULSED
    rng = np.random.default_rng(s["pulse_seed"])
    total = s["B"] * s["N"]
    amp = np.sqrt(2.0) * s["sigma"] * 10.0 ** (s["pulse_db"] / 20.0)
    out = np.zeros(total, np.complex128)
    n = np.arange(s["burst"])
    for start in rng.integers(0, total - s["burst"], int(s["duty"] * total / s["burst"])):
        out[start:start + s["burst"]] = amp * np.exp(2j * np.pi * (rng.uniform(-0.3, 0.3) * n + rng.uniform()))
    return out
