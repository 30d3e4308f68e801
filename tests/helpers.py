"""Shared helpers for the parity tests: build seeded inputs, run the HIP path through the C ABI
(via the Python host layer) and the FP64 oracle on the same inputs, compare."""
import numpy as np
import pytest

import oracle

# north star: "correlator outputs match the CPU reference within 1e-5 relative on ComplexF32
# accumulators".  Metric: per channel max|dR| / max|R_ref| over its [L, M]
# block, plus element-wise relative error on signal-bearing taps (|R| >= 0.1 max|R|).
RTOL = 1e-5


def system_tables(name):
    lc, fc, _ = oracle.SYSTEMS[name]
    return oracle.codes(name, 32), fc, lc


# ---- caller's code tables (gat_set_codes: any int8 chips, 1 .. 120 000 per row) -----------------------------------------
CHIP_KINDS = ("pm1", "pm1_zeros", "ternary", "int8")


def code_table(length, num_prns, seed, kind="pm1"):
    """A caller's chip table, int8 [num_prns, length] (the layout GNSSSystem(codes=...) takes).  kind: "pm1" random +-1;
    "pm1_zeros" +-1 with about 5 % of the chips 0 (the last row's last chip always, where the table has two chips or
    more); "ternary" {-1, 0, +1}; "int8" the whole range, -128 (first chip) and 127 (last chip) included.  A row of zeros only gets
    a +1 as its first chip."""
    rng = np.random.default_rng(seed)
    shape = (num_prns, length)
    if kind in ("pm1", "pm1_zeros"):
        t = np.where(rng.integers(0, 2, shape) == 1, 1, -1)
        if kind == "pm1_zeros":
            t[rng.random(shape) < 0.05] = 0
            if t.size > 1:
                t[-1, -1] = 0
    elif kind == "ternary":
        t = rng.integers(-1, 2, shape)
    elif kind == "int8":
        t = rng.integers(-128, 128, shape)
        t.flat[0], t.flat[-1] = -128, 127
    else:
        raise ValueError(kind)
    t[~t.any(axis=1), 0] = 1  # no row of zeros only (a channel without any signal has no relative error to judge)
    return np.ascontiguousarray(t, dtype=np.int8)


@pytest.fixture()
def standard_codes_after():
    """Tests share the default context, and the C-level users (resident correlator, acquisition) bind whatever table they
    are handed: bind the standard GPS L1 table again after the test, so that no caller's table leaks into later tests."""
    yield
    import gpuacceleratedtracking_amd as g
    g.get_context().set_codes(g.GPSL1().codes)


def make_case(seed, system="GPSL1", N=2500, M=1, L=3, K=1, B=1, fs=None, if_hz=0.0, noise=0.0, codes=None, fc=None,
              prns=None, tau=None):
    """Seeded scenario: K channels (distinct PRNs) summed into one antenna signal with
    per-antenna steering phases; per-(block, channel) Doppler / code phase / carrier phase.
    ``codes`` (int8 [P, Lc]) / ``fc``: a caller's table and code rate instead of the system's (default 1.023 MHz); ``prns``
    (K rows of it) and ``tau`` ([B, K] code phases) replace the drawn ones."""
    rng = np.random.default_rng(seed)
    if codes is None:
        codes, fc, lc = system_tables(system)
        num_prns = 32
    else:
        codes = np.ascontiguousarray(codes, dtype=np.int8)
        num_prns, lc = codes.shape
        fc = 1.023e6 if fc is None else fc
    if fs is None:
        fs = N / 1e-3
    # (every row of both ICD tables is pinned to its ICD, tests/test_oracle_golden.py; a caller's table of fewer rows than
    # channels repeats them)
    drawn = rng.permutation(num_prns)[:K] if K <= num_prns else rng.integers(0, num_prns, K)
    prns = drawn if prns is None else np.asarray(prns)
    f = if_hz + rng.uniform(-5e3, 5e3, size=(B, K))
    fcode = fc * (1.0 + (f - if_hz) / 1575.42e6)
    drawn_tau = rng.uniform(0, lc, size=(B, K))
    tau = drawn_tau if tau is None else np.broadcast_to(np.asarray(tau, dtype=np.float64), (B, K))
    phi = rng.uniform(0, 1, size=(B, K))
    prm = oracle.make_params(np.broadcast_to(prns, (B, K)), fcode, f, tau, phi)
    # signal: sum over channels, built with the oracle's gen_signal (phi in radians there)
    re = np.zeros((M, B * N), dtype=np.float32)
    im = np.zeros((M, B * N), dtype=np.float32)
    steer = np.exp(2j * np.pi * rng.uniform(0, 1, size=M)) if M > 1 else np.ones(1)
    for b in range(B):
        acc = np.zeros(N, dtype=np.complex128)
        for k in range(K):
            r1, i1 = oracle.gen_signal(codes, int(prns[k]), fcode[b, k], fs, f[b, k], tau[b, k],
                                       2 * np.pi * phi[b, k], N, 1)
            acc += r1[0].astype(np.float64) + 1j * i1[0].astype(np.float64)
        if noise > 0:
            acc += noise * (rng.standard_normal(N) + 1j * rng.standard_normal(N))
        x = steer[:, None] * acc[None, :]
        re[:, b * N:(b + 1) * N] = x.real.astype(np.float32)
        im[:, b * N:(b + 1) * N] = x.imag.astype(np.float32)
    shifts = oracle.sample_shifts(L, fs, fc)
    return dict(codes=codes, fc=fc, lc=lc, fs=fs, prm=prm, re=re, im=im, shifts=shifts, N=N, M=M, L=L,
                K=K, B=B, system=system)


def oracle_result(case):
    return oracle.correlate_f64(case["re"], case["im"], case["codes"], case["prm"], case["fs"],
                                case["shifts"], N=case["N"])


def check_close(got, ref, rtol=RTOL, what="", floor_frac=None, abs_floor=0.0):
    """got/ref complex [B, K, L, M].  ``floor_frac`` (default: env GAT_CHECK_FLOOR_FRAC, else 0 = strict): a channel
    whose own largest accumulator is below this fraction of the block's largest one (a short integration whose
    interferers happen to cancel its single tap) is scaled by that floor instead -- a relative error against a
    cancellation residue says nothing about the kernel (scripts/stress_matrix_sweep.py uses 0.01).  ``abs_floor``: the
    same as an absolute magnitude (callers that know the coherent scale N * rms|x| of the integration)."""
    import os
    if floor_frac is None:
        floor_frac = float(os.environ.get("GAT_CHECK_FLOOR_FRAC", "0"))
    got = np.asarray(got, dtype=np.complex128)
    ref = np.asarray(ref, dtype=np.complex128)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    B, K = ref.shape[:2]
    for b in range(B):
        for k in range(K):
            r, g = ref[b, k], got[b, k]
            scale = max(np.abs(r).max(), floor_frac * np.abs(ref[b]).max(), abs_floor)
            e_inf = np.abs(g - r).max() / scale
            assert e_inf <= rtol, f"{what} block {b} chan {k}: norm-wise error {e_inf:.3e} > {rtol}"
            if np.abs(r).max() < scale:  # only with a floor: the whole channel is a cancellation residue,
                continue               # there is no signal-bearing element to judge element-wise
            strong = np.abs(r) >= 0.1 * scale
            rel = (np.abs(g - r)[strong] / np.abs(r)[strong]).max()
            assert rel <= rtol, f"{what} block {b} chan {k}: element-wise error {rel:.3e} > {rtol}"


# ---- the acquisition search (include/gat.h gat_acquire) ----------------------------------------------------------------
def acq_power_oracle(re, im, codes, prn, fc, lc, fs, if_hz, f_first, f_step, rows, first_shift, s, cols, N, B,
                     block_stride):
    """The search's power P[i, j] for PRN ``prn`` (code-table row), Doppler rows ``rows`` and code bins ``cols``, built from
    the FP64 correlator exactly as gat_acquire's contract states it: the channel record {prn, fc, if + f_i, tau_b, 0} with
    f_i = f_first + i f_step and tau_b = fmod(fc / fs * b * block_stride, Lc), the tap first_shift + s j, |R|^2 summed over
    antennas and blocks.  re / im: float32 [M, ld] planar (the antenna stride is ld).  Returns float64 [len(rows), len(cols)]."""
    rows = np.asarray(rows, dtype=np.int64)
    cols = np.asarray(cols, dtype=np.int64)
    f = if_hz + (f_first + rows.astype(np.float64) * f_step)
    tau = np.fmod(fc / fs * (np.arange(B, dtype=np.int64) * block_stride).astype(np.float64), float(lc))
    shifts = (first_shift + s * cols).astype(np.int32)
    K = rows.size
    prm = oracle.make_params(np.full((B, K), prn), fc, np.broadcast_to(f, (B, K)), np.broadcast_to(tau[:, None], (B, K)), 0.0)
    R = oracle.correlate_f64(re, im, codes, prm, fs, shifts, N=N, blk_stride=block_stride)  # [B, K, L, M]
    return (R.real ** 2 + R.imag ** 2).sum(axis=(0, 3))


def acq_sample_bins(rng, D, J, n_rows=4, n_cols=12, rows=(), cols=()):
    """Sorted Doppler rows and code bins to compare: the grid's edges and tile seams (rows 0, D - 1, 31, 32; bins 0, J - 1,
    255, 256, where they exist), ``rows`` / ``cols`` (the peak), and a few random ones."""
    r = [0, D - 1, 31, 32, *rows, *rng.integers(0, D, n_rows)]
    c = [0, J - 1, 255, 256, *cols, *rng.integers(0, J, n_cols)]
    return (np.unique([i for i in r if 0 <= i < D]).astype(np.int64), np.unique([j for j in c if 0 <= j < J]).astype(np.int64))


def check_power_close(got, ref, rtol=RTOL, what=""):
    """got / ref [rows, cols] powers over the sampled bins, judged per Doppler row as check_close judges a channel: norm-wise
    max|dP| / max P_ref, and element-wise on the bins with P_ref >= 0.1 of the row's sampled maximum.  Returns the worst
    (norm-wise, element-wise) errors."""
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.isfinite(got).all(), f"{what}: non-finite power"
    worst_n = worst_e = 0.0
    for r in range(ref.shape[0]):
        scale = ref[r].max()
        assert scale > 0, f"{what} row {r}: zero reference"
        d = np.abs(got[r] - ref[r])
        e_inf = d.max() / scale
        strong = ref[r] >= 0.1 * scale
        rel = (d[strong] / ref[r][strong]).max()
        assert e_inf <= rtol, f"{what} row {r}: norm-wise error {e_inf:.3e} > {rtol}"
        assert rel <= rtol, f"{what} row {r}: element-wise error {rel:.3e} > {rtol}"
        worst_n, worst_e = max(worst_n, e_inf), max(worst_e, rel)
    return worst_n, worst_e


# ---- the channel record across its whole accepted domain (include/gat.h gat_channel_params) -------------------------------
SPAN_LIMIT = 1073741824.0  # 2^30: |code phase| bound of the kernels' int32 / float-reciprocal chip index


def span_bound_tau(ratio, reach, lc):
    """(inside, outside): the largest code phase tau >= 0 that the span rule |tau| + ratio * reach + 1 < min(2^30, 2^21 Lc)
    accepts, evaluated in the kernels' own double expression, and the next double above it (rejected)."""
    limit = min(SPAN_LIMIT, 2097152.0 * lc)
    ok = lambda t: abs(t) + abs(ratio) * reach + 1.0 < limit  # noqa: E731
    t = np.float64(limit - abs(ratio) * reach - 1.0)
    while not ok(t):
        t = np.nextafter(t, 0.0)
    while ok(np.nextafter(t, np.inf)):
        t = np.nextafter(t, np.inf)
    return float(t), float(np.nextafter(t, np.inf))


def floormod_hard_taus(lc, lo, hi, seed, count=3):
    """Integer code phases in [lo, hi) whose chip index floor(ip * (1/Lc)) the kernels' float-reciprocal modulo gets one
    quotient wrong (gat_phase.h floormod_fast, float32 arithmetic): up to `count` whose first remainder is negative and up to
    `count` whose first remainder is Lc + 1 or more (Lc itself reads the wrap chip, which hides a missing second correction).
    Which of the two occur depends on the rounding of 1 / Lc and on the sign of the range."""
    rng = np.random.default_rng(seed)
    ip = rng.integers(lo, hi, 400000, dtype=np.int64)
    inv = np.float32(1.0) / np.float32(lc)
    q = np.floor(ip.astype(np.float32) * inv).astype(np.int64)
    r = ip - q * lc
    low, high = ip[r < 0][:count], ip[r >= lc + 1][:count]
    return [float(x) for x in np.concatenate([low, high])]


def reduced_carrier(step, phi):
    """The carrier of a record reduced exactly: phase phi - floor(phi) in [0, 1], step s - rint(s) in [-1/2, 1/2].  Both
    subtractions are exact in binary64 (for |phi| >= 1, |s| >= 1/2), and n * rint(s) is a whole number of cycles."""
    step = np.asarray(step, dtype=np.float64)
    phi = np.asarray(phi, dtype=np.float64)
    return step - np.rint(step), phi - np.floor(phi)


def correlate_reduced(re, im, codes, prm, fs, shifts, N, blk_stride=None):
    """numpy reference of the correlator (as oracle.np_correlate) with the carrier phase n * s0 + phi0 built from the
    exactly reduced step s0 and phase phi0 of every record (reduced_carrier): exact wherever |phi| or |f / fs| is large,
    and the same as oracle.correlate_f64 where nothing needs reducing.  re / im float32 [M, ld] planar; prm: oracle records
    [B, K] (field prn0).  Returns complex128 [B, K, L, M]."""
    B, K = prm.shape
    M = re.shape[0]
    S = N if blk_stride is None else blk_stride
    lc = codes.shape[1]
    n = np.arange(N, dtype=np.float64)
    out = np.empty((B, K, len(shifts), M), dtype=np.complex128)
    for b in range(B):
        x = re[:, b * S:b * S + N].astype(np.float64) + 1j * im[:, b * S:b * S + N].astype(np.float64)
        for k in range(K):
            p = prm[b, k]
            s0, phi0 = reduced_carrier(p["carrier_freq_hz"] / fs, p["carrier_phase_cycles"])
            dw = x * np.exp(-2j * np.pi * (n * s0 + phi0))[None, :]
            ratio = np.float64(p["code_freq_hz"]) / np.float64(fs)
            row = codes[p["prn0"]].astype(np.float64)
            for li, s in enumerate(shifts):
                idx = np.mod(np.floor(ratio * (n + float(s)) + p["code_phase_chips"]).astype(np.int64), lc)
                out[b, k, li] = dw @ row[idx]
    return out


def channel_errors(got, ref):
    """Per (block, channel) errors as check_close judges them: norm-wise max|dR| / max|R_ref| and element-wise on the taps
    with |R_ref| >= 0.1 max|R_ref|.  Returns two float64 [B, K] arrays."""
    got = np.asarray(got, dtype=np.complex128)
    ref = np.asarray(ref, dtype=np.complex128)
    B, K = ref.shape[:2]
    e_n, e_e = np.zeros((B, K)), np.zeros((B, K))
    for b in range(B):
        for k in range(K):
            r, d = ref[b, k], np.abs(got[b, k] - ref[b, k])
            scale = np.abs(r).max()
            e_n[b, k] = d.max() / scale
            strong = np.abs(r) >= 0.1 * scale
            e_e[b, k] = (d[strong] / np.abs(r)[strong]).max()
    return e_n, e_e


# ---- the correlator's paths (shared by the domain tests: test_channel_domain_gpu.py, test_tap_domain_gpu.py) ------------------
SENTINEL = 7.0  # what correlate() pre-fills the outputs with by default


def reset(g, c):
    c.set_matrix_core(g.GAT_MC_AUTO)
    c.set_vector_tiling(4, 4, 16)
    for name, val in (("dc_bits", 1), ("dc_quads", -1), ("dc_aw2", -1), ("dc_one_wave_min", -1), ("dc_depth", 2)):
        c.set_option(name, val)


# ---- the paths ---------------------------------------------------------------------------------------------------------------
# mc: kernel selection; tiling / opts: forced vector-kernel settings; M, N: the call's antennas and block length (None: the
# test's own); offset: samples the signal's base is moved by (1: unaligned -> the scalar-load path); ragged: N - 1 samples
# (N mod 4 = 3 -> the tail kernel); want: what gat_last_launch_info must show.
PATHS = {
    "default-planar": dict(layout=0),
    "default-cf32": dict(layout=1),
    "default-i16": dict(layout=2),
    "default-i8": dict(layout=3),
    # (sixteen antennas: four antenna tiles, whose workgroups loop over channels -- 256 / KT replica entries per producer)
    "tiling-1-1-1": dict(mc=0, tiling=(1, 1, 1), M=16, want=lambda i: i["channels_per_wg"] == 1 and i["blocks_per_wg"] == 1),
    "tiling-2-2-4": dict(mc=0, tiling=(2, 2, 4), M=16, want=lambda i: i["channels_per_wg"] == 1),
    "tiling-4-2-4": dict(mc=0, tiling=(4, 2, 4), M=16, want=lambda i: i["channels_per_wg"] == 2),
    "tiling-4-4-16": dict(mc=0, tiling=(4, 4, 16), M=16, want=lambda i: i["channels_per_wg"] == 4),
    "one-wave": dict(mc=0, opts=dict(dc_one_wave_min=1), M=2, N=1000, want=lambda i: i["threads"] == 64),
    "2x2-quads": dict(mc=0, opts=dict(dc_aw2=1, dc_quads=1), want=lambda i: i["channels_per_wg"] == 2 and i["ant_tile"] == 4),
    "2x2-no-quads": dict(mc=0, opts=dict(dc_aw2=1, dc_quads=0), want=lambda i: i["channels_per_wg"] == 2 and i["ant_tile"] == 4),
    "scalar-load": dict(mc=0, offset=1, want=lambda i: i["vec"] != 4),
    "ragged-tail": dict(mc=0, ragged=True, want=lambda i: i["vec"] == 4),
    "split-finalize": dict(mc=0, B=1, N=16384, want=lambda i: i["splits"] > 1 and i["finalize_launched"] == 1),
    "mc-f32": dict(mc=2, M=16, want=lambda i: i["matrix_core"] == 1),
    "mc-bf16-f32": dict(mc=3, M=16, want=lambda i: i["matrix_core"] == 2),
    "mc-bf16-i16": dict(mc=3, M=16, layout=2, want=lambda i: i["matrix_core"] == 2),
    "mc-bf16-i8": dict(mc=3, M=16, layout=3, want=lambda i: i["matrix_core"] == 2),
}


def configure(g, ctx, path):
    reset(g, ctx)
    spec = PATHS[path]
    ctx.set_matrix_core(spec.get("mc", g.GAT_MC_AUTO))
    if "tiling" in spec:
        ctx.set_vector_tiling(*spec["tiling"])
    for name, val in spec.get("opts", {}).items():
        ctx.set_option(name, val)


def geometry(path, N, M, B):
    spec = PATHS[path]
    N = spec.get("N") or N
    if spec.get("ragged"):
        N -= 1
    return N, spec.get("M", M), spec.get("B", B)


def correlate(g, ctx, path, re, im, prm, N, fs, shifts, host=False, check_want=True, sentinel=SENTINEL, flags=0):
    """One call of the correlator on `path`: re / im float32 [M, B * S] planar (S = block stride, a multiple of 8), prm library
    records [B, K]; host: the records as host records (gat_downconvert_and_correlate) instead of device records; check_want:
    assert the path's launch info; sentinel: what the outputs are pre-filled with; flags: GAT_FLAG_*.  Returns the outputs
    complex128 [B, K, L, M] and the launch info."""
    import torch
    spec = PATHS[path]
    layout, off = spec.get("layout", 0), spec.get("offset", 0)
    B, K = prm.shape
    M, ld = re.shape
    S = ld // B
    dev = ctx.device
    if layout == 0:
        bufs = [torch.zeros((M, ld + 8), dtype=torch.float32, device=dev) for _ in range(2)]
        bufs[0][:, off:off + ld] = torch.from_numpy(re).to(dev)
        bufs[1][:, off:off + ld] = torch.from_numpy(im).to(dev)
        ptrs = (bufs[0].data_ptr() + 4 * off, bufs[1].data_ptr() + 4 * off)
    else:
        assert off == 0
        dt = {1: torch.float32, 2: torch.int16, 3: torch.int8}[layout]
        x = torch.stack([torch.from_numpy(re), torch.from_numpy(im)], dim=-1).to(dt).contiguous().to(dev)
        bufs = [x]
        ptrs = (x.data_ptr(), None)
    desc = g._lib.SignalDesc(ptrs[0], ptrs[1], layout, M, N, bufs[0].shape[1], S, 0)
    L = len(shifts)
    o_re = torch.full((B, K, L, M), sentinel, dtype=torch.float32, device=dev)
    o_im = torch.full((B, K, L, M), sentinel, dtype=torch.float32, device=dev)
    params = prm if host else ctx.params_to_device(prm)
    ctx.downconvert_and_correlate(desc, params, B, K, shifts, fs, o_re, o_im, flags)
    ctx.sync()
    got = o_re.cpu().numpy().astype(np.float64) + 1j * o_im.cpu().numpy().astype(np.float64)
    info = ctx.last_launch_info()
    if check_want and "want" in spec:
        assert spec["want"](info), (path, info)
    return got, info
