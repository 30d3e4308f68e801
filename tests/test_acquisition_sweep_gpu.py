"""The acquisition search (include/gat.h gat_acquire) at its edges: a seeded random sweep of the power grid against the FP64
oracle's correlator restated as the search's formula (tests/helpers.py acq_power_oracle) over systems, layouts, antennas,
blocks (padded, overlapping), ragged N, code steps 1..31, Doppler and code grids around the 32 x 256 tile, signed shifts
and repeated PRNs; fixed cases for the largest replica window, long coherent blocks and the split of (antenna, block) units
over workgroup groups; the device's statistics against gat_acq_stats_host where they can disagree (ties, peaks on the
grid's edges, too few noise bins); and the layout / alignment claims through the Python layer, bit for bit."""
import ctypes as C
import math

import numpy as np
import pytest

import oracle
from tests.helpers import acq_power_oracle, acq_sample_bins, check_power_close

pytestmark = pytest.mark.gpu

SYSTEMS = {"GPSL1": (1023, 1.023e6), "GPSL5": (10230, 10.23e6)}
ACQ_TILE_D, ACQ_TILE_J = 32, 256  # csrc/gat_acq_kernels.h kAcqDopTile, kAcqCodeTile
EXACT_FIELDS = ("prn", "detected", "doppler_bin", "code_bin", "peak_power", "num_noise_bins", "carrier_doppler_hz",
                "code_phase_chips")


@pytest.fixture(scope="module")
def g():
    import gpuacceleratedtracking_amd as g
    g.load_library()
    return g


def _codes(system):
    return oracle.codes(system, 32)


def _cfg(g, D, J, s, fc, lc, first_shift=0, f_first=0.0, f_step=0.0, if_hz=0.0):
    cfg = g._lib.AcqConfig()
    cfg.struct_size = C.sizeof(g._lib.AcqConfig)
    cfg.num_doppler_bins, cfg.num_code_bins, cfg.code_step_samples = D, J, s
    cfg.if_hz, cfg.code_freq_hz, cfg.doppler_first_hz, cfg.doppler_step_hz = if_hz, fc, f_first, f_step
    cfg.first_shift, cfg.min_peak_ratio, cfg.code_length = first_shift, 2.0, lc
    return cfg


def _quantize(x, layout, g):
    """complex128 [M, ld] -> host array in `layout` and the same values as float32 planes for the oracle.  int16 / int8 are
    scaled past full scale and clipped, so the extremes (-32768, -128 included) are in the signal."""
    if layout in (g.GAT_LAYOUT_INTERLEAVED_I16, g.GAT_LAYOUT_INTERLEAVED_I8):
        dt = np.int16 if layout == g.GAT_LAYOUT_INTERLEAVED_I16 else np.int8
        lo, hi = np.iinfo(dt).min, np.iinfo(dt).max
        peak = max(np.abs(x.real).max(), np.abs(x.imag).max(), 1e-30)
        y = x * (1.25 * hi / peak)
        pair = np.clip(np.stack([np.rint(y.real), np.rint(y.imag)], axis=-1), lo, hi).astype(dt)
        pair.reshape(-1)[:2] = (lo, hi)  # both extremes, whatever the draw
        return pair, pair[..., 0].astype(np.float32), pair[..., 1].astype(np.float32)
    re, im = x.real.astype(np.float32), x.imag.astype(np.float32)
    if layout == g.GAT_LAYOUT_PLANAR:
        return (re, im), re, im
    return np.ascontiguousarray(np.stack([re, im], axis=-1)), re, im


def _to_device(host):
    import torch
    if isinstance(host, tuple):
        return tuple(torch.from_numpy(np.ascontiguousarray(h)).cuda() for h in host)
    return (torch.from_numpy(np.ascontiguousarray(host)).cuda(),)


def _acquire(g, codes, sig, N, B, bstride, prns, fs, cfg, keep=True):
    """gat_acquire through the C ABI on the device signal `sig` (planar pair or one interleaved tensor); returns (rc, power
    [P, D, J] or None, results)."""
    import torch
    from gpuacceleratedtracking_amd.acquisition import _as_desc
    ctx = g.get_context()
    ctx.set_codes(codes)
    desc = _as_desc(sig if len(sig) == 2 else sig[0], N, B, bstride)
    P = len(prns)
    power = torch.full((P, cfg.num_doppler_bins, cfg.num_code_bins), float("nan"), dtype=torch.float32, device="cuda") if keep else None
    res = np.zeros(P, dtype=g._lib.ACQ_RESULT_DTYPE)
    pr = np.ascontiguousarray(prns, dtype=np.int32)
    rc = ctx.lib.gat_acquire(ctx._h, C.byref(desc), B, pr.ctypes.data_as(C.POINTER(C.c_int32)), P, fs, C.byref(cfg),
                             C.c_void_p(power.data_ptr() if keep else None), C.c_void_p(res.ctypes.data))
    return rc, (power.cpu().numpy() if keep else None), res


def _check_stats(g, res, power, cfg, fs, N, prns, exact_noise=False):
    """The device's results against gat_acq_stats_host on the device's grid: the peak, its neighbours' refinement and the
    noise set's size bit for bit; the noise sums (summed in another order) to 1e-12, or exactly on integer grids."""
    h = g.acquisition_stats_host(power, cfg, fs, N)
    assert np.array_equal(res["prn"], np.asarray(prns, dtype=np.int32))
    for f in EXACT_FIELDS[1:]:
        assert np.array_equal(h[f], res[f], equal_nan=True), (f, h[f], res[f])
    for f in ("noise_power", "second_power", "peak_to_second", "cn0_dbhz"):
        if exact_noise and f != "cn0_dbhz":
            assert np.array_equal(h[f], res[f], equal_nan=True), (f, h[f], res[f])
        else:
            assert np.allclose(h[f], res[f], rtol=1e-12, atol=1e-12 if f == "cn0_dbhz" else 0, equal_nan=True), (f, h[f], res[f])
    return h


def _constellation(rng, system, fs, ld, M, sats, noise):
    """Satellites (prn, carrier Hz, code phase chips at sample 0) over `ld` samples, steered over M antennas, in noise."""
    lc, fc = SYSTEMS[system]
    codes = _codes(system)
    x = np.zeros(ld, dtype=np.complex128)
    for p, f, tau in sats:
        r1, i1 = oracle.gen_signal(codes, int(p), fc, fs, f, tau, rng.uniform(0, 2 * np.pi), ld, 1)
        x += r1[0] + 1j * i1[0]
    steer = np.exp(2j * np.pi * rng.uniform(0, 1, (M, 1)))
    return steer * x[None, :] + noise * (rng.standard_normal((M, ld)) + 1j * rng.standard_normal((M, ld)))


def _bin_phase(fc, fs, lc, first_shift, s, j):
    """The code phase (chips at sample 0 of block 0) that lines a satellite up with code bin j."""
    return math.fmod(fc / fs * (first_shift + s * j), lc) % lc


# ---- the random sweep ---------------------------------------------------------------------------------------------------
def _draw(seed):
    rng = np.random.default_rng(7000 + seed)
    system = "GPSL5" if seed % 3 == 1 else "GPSL1"
    lc, fc = SYSTEMS[system]
    fs = float(rng.choice([4.0e6, 5.0e6, 20.46e6]) if system == "GPSL5" else rng.choice([1.5e6, 2.046e6, 4.0e6, 5.0e6, 16.368e6]))
    layout = seed % 4
    M = int(rng.choice([1, 2, 3, 4, 7]))
    kind = seed % 5
    N = [int(rng.integers(1, 128)), 128, 129, int(rng.integers(130, 60001)), int(rng.integers(130, 8000))][kind]
    B = int(rng.choice([1, 2, 3, 5]))
    while M * B * N > 250_000 and M * B > 1:  # the oracle's time, not the kernel's
        M, B = (M, B - 1) if B > 1 else (M - 1, B)
    stride_kind = seed % 3 if N > 1 else seed % 2
    bstride = [N, N + int(rng.integers(1, 40)), max(1, N - int(rng.integers(1, max(2, N))))][stride_kind] if B > 1 else N
    s = 31 if seed % 8 == 5 else int(rng.integers(1, 32))
    D = int(rng.choice([1, 2, 31, 32, 33, 40, 64, 65, int(rng.integers(1, 70))]))
    f_step = float(rng.choice([250.0, -333.25, 0.0, 500.0, -1000.0]))
    J = int(rng.choice([1, 2, 255, 256, 257, 300, 511, 513, int(rng.integers(1, 800))]))
    first_shift = int(rng.choice([-N - int(rng.integers(0, 600)), -int(rng.integers(0, N + 1)), 0, int(rng.integers(0, 40000))]))
    if_hz = float(rng.choice([0.0, rng.uniform(-0.25, 0.25) * fs]))
    P = int(rng.integers(1, 9))
    prns = [int(p) for p in rng.integers(0, 32, P)]
    if P > 1 and seed % 4 == 2:
        prns[-1] = prns[0]  # a repeated PRN
    keep = seed % 3 != 0
    return dict(rng=rng, system=system, lc=lc, fc=fc, fs=fs, layout=layout, M=M, N=N, B=B, bstride=bstride, s=s, D=D,
                f_step=f_step, J=J, first_shift=first_shift, if_hz=if_hz, prns=prns, keep=keep,
                ant_pad=int(rng.integers(0, 50)), f_first=float(-f_step * (D // 2)))


SWEEP_SEEDS = range(40)


@pytest.mark.parametrize("seed", SWEEP_SEEDS)
def test_random_sweep_matches_oracle(g, seed):
    c = _draw(seed)
    rng, N, B, M, bstride, s, D, J = c["rng"], c["N"], c["B"], c["M"], c["bstride"], c["s"], c["D"], c["J"]
    fs, fc, lc, prns = c["fs"], c["fc"], c["lc"], c["prns"]
    ld = (B - 1) * bstride + N + c["ant_pad"]
    # the first (up to) two distinct PRNs are present, each on a drawn grid bin (its Doppler a fraction of a bin off)
    planted = list(dict.fromkeys(prns))[:2]
    truth = {}
    sats = []
    for p in planted:
        i, j = int(rng.integers(0, D)), int(rng.integers(0, J))
        truth[p] = (i, j)
        f = c["if_hz"] + c["f_first"] + (i + rng.uniform(-0.2, 0.2)) * c["f_step"]
        sats.append((p, f, _bin_phase(fc, fs, lc, c["first_shift"], s, j)))
    x = _constellation(rng, c["system"], fs, ld, M, sats, noise=0.7)
    host, re, im = _quantize(x, c["layout"], g)
    sig = _to_device(host)
    codes = _codes(c["system"])
    cfg = _cfg(g, D, J, s, fc, lc, c["first_shift"], c["f_first"], c["f_step"], c["if_hz"])
    what = f"seed {seed} {c['system']} layout {c['layout']} M {M} B {B} N {N} stride {bstride} s {s} D {D} J {J} shift {c['first_shift']}"
    rc, power, res = _acquire(g, codes, sig, N, B, bstride, prns, fs, cfg, keep=c["keep"])
    assert rc == 0, what
    if not c["keep"]:  # no caller buffer: the results of that call against the host's statistics of a call that keeps it
        rc2, power, res2 = _acquire(g, codes, sig, N, B, bstride, prns, fs, cfg, keep=True)
        assert rc2 == 0, what
        assert res.tobytes() == res2.tobytes(), what
    assert np.isfinite(power).all(), what
    _check_stats(g, res, power, cfg, fs, N, prns)
    # a repeated PRN gets the same grid, bit for bit
    for k, p in enumerate(prns):
        first = prns.index(p)
        if first != k:
            assert power[k].tobytes() == power[first].tobytes(), what
    worst = [0.0, 0.0]
    for p in planted:
        k = prns.index(p)
        pk = np.unravel_index(np.argmax(power[k]), power[k].shape)
        rows, cols = acq_sample_bins(rng, D, J, n_rows=3, n_cols=10, rows=[pk[0], truth[p][0]], cols=[pk[1], truth[p][1]])
        ref = acq_power_oracle(re, im, codes, p, fc, lc, fs, c["if_hz"], c["f_first"], c["f_step"], rows, c["first_shift"],
                               s, cols, N, B, bstride)
        en, ee = check_power_close(power[k][np.ix_(rows, cols)], ref, what=f"{what} prn {p}")
        worst = [max(worst[0], en), max(worst[1], ee)]
    print(f"acq sweep {what}: norm-wise {worst[0]:.2e} element-wise {worst[1]:.2e}")


# ---- fixed cases --------------------------------------------------------------------------------------------------------
def _single_sat_case(g, layout, system, fs, N, M, B, bstride, s, D, J, first_shift, f_first, f_step, if_hz, prns, seed,
                     noise=0.5, peak=None):
    rng = np.random.default_rng(seed)
    lc, fc = SYSTEMS[system]
    i, j = peak if peak is not None else (D // 2, J // 2)
    ld = (B - 1) * bstride + N
    x = _constellation(rng, system, fs, ld, M, [(prns[0], if_hz + f_first + (i + 0.1) * f_step,
                                                  _bin_phase(fc, fs, lc, first_shift, s, j))], noise)
    host, re, im = _quantize(x, layout, g)
    codes = _codes(system)
    cfg = _cfg(g, D, J, s, fc, lc, first_shift, f_first, f_step, if_hz)
    rc, power, res = _acquire(g, codes, _to_device(host), N, B, bstride, prns, fs, cfg)
    assert rc == 0
    return rng, codes, re, im, cfg, power, res, (i, j)


def test_largest_code_step_over_two_code_tiles(g):
    """s = 31: the largest replica window (~ 97 KB of LDS, above the 64 KB default) with J over three code tiles."""
    fs, N, D, J, s = 16.368e6, 9000, 5, 600, 31
    rng, codes, re, im, cfg, power, res, (i, j) = _single_sat_case(
        g, g.GAT_LAYOUT_PLANAR, "GPSL1", fs, N, 2, 2, N + 3, s, D, J, -700, -500.0, 250.0, 1.0e5, [11, 4], seed=31, peak=(3, 300))
    _check_stats(g, res, power, cfg, fs, N, [11, 4])
    assert (res["doppler_bin"][0], res["code_bin"][0]) == (i, j)
    for k, p in enumerate([11, 4]):
        rows, cols = acq_sample_bins(rng, D, J, n_cols=16, rows=[i], cols=[j, 511, 512, j - 1, j + 1])
        ref = acq_power_oracle(re, im, codes, p, FC_L1, 1023, fs, 1.0e5, -500.0, 250.0, rows, -700, s, cols, N, 2, N + 3)
        check_power_close(power[k][np.ix_(rows, cols)], ref, what=f"s=31 prn {p}")


FC_L1 = SYSTEMS["GPSL1"][1]

LONG = [  # layout name, N, fs
    ("planar", 200_000, 20.0e6),
    ("int16", 1_000_000, 50.0e6),
    ("planar", 1 << 21, 50.0e6),
    ("int16", 1 << 21, 50.0e6),
]


@pytest.mark.parametrize("case", LONG, ids=[f"{c[0]}-{c[1]}" for c in LONG])
def test_long_coherent_blocks_match_oracle(g, case):
    """10 ms at 20 MHz, 20 ms at 50 MHz and 2^21 samples: the two-level sum's rounding at the coherent lengths a fine search
    uses, sampled at the peak, its neighbours and away from it."""
    name, N, fs = case
    layout = g.GAT_LAYOUT_PLANAR if name == "planar" else g.GAT_LAYOUT_INTERLEAVED_I16
    D, J, s = 9, 40, 3
    f_first, f_step = -40.0, 10.0
    first_shift = 1234
    rng, codes, re, im, cfg, power, res, (i, j) = _single_sat_case(
        g, layout, "GPSL1", fs, N, 1, 1, N, s, D, J, first_shift, f_first, f_step, 0.0, [6], seed=N, noise=2.0, peak=(4, 20))
    assert (res["doppler_bin"][0], res["code_bin"][0]) == (i, j)
    rows = np.array([0, i - 1, i, i + 1, D - 1])
    cols = np.unique([0, 3, j - 2, j - 1, j, j + 1, j + 2, 31, J - 1])
    ref = acq_power_oracle(re, im, codes, 6, FC_L1, 1023, fs, 0.0, f_first, f_step, rows, first_shift, s, cols, N, 1, N)
    en, ee = check_power_close(power[0][np.ix_(rows, cols)], ref, what=f"N {N} {name}")
    pk = abs(float(power[0][i, j]) - ref[2, list(cols).index(j)]) / ref[2, list(cols).index(j)]
    print(f"acq long N {N} {name}: norm-wise {en:.2e} element-wise {ee:.2e} peak bin {pk:.2e}")


def _groups(num_cus, P, D, J, units, cells):
    """The number of (antenna, block) groups gat_acquire chooses (csrc/gat_acq_api.cpp)."""
    wgs = P * -(-J // ACQ_TILE_J) * -(-D // ACQ_TILE_D)
    G = min(units, max(1, -(-2 * num_cus // wgs)))
    G = min(G, max(1, (1 << 30) // (cells * 4)))
    return min(G, 65535 // P)


@pytest.mark.parametrize("regime", ["uneven", "one_group"])
def test_unit_split_over_groups(g, regime):
    """(antenna, block) units over G workgroup groups: G > 1 with units % G != 0, and G == 1 with several units."""
    cus = g.get_context().device_info()["num_cus"]
    fs, s = 2.046e6, 1
    if regime == "uneven":
        P, D, J = 1, 8, 200
        units = 2 * cus + 7 if cus > 1 else 3  # G = min(units, 2 cus) = 2 cus, which does not divide units
        M, B, N = 1, units, 300
    else:
        P, D, J = 4, 3, ACQ_TILE_J * max(1, -(-2 * cus // 4))  # 2 cus workgroups already: G = 1
        M, B, N = 3, 2, 500
        units = M * B
    G = _groups(cus, P, D, J, units, P * D * J)
    assert (G > 1 and units % G != 0) if regime == "uneven" else (G == 1 and units > 1), (cus, G, units)
    prns = [9, 21, 9, 2][:P]
    rng, codes, re, im, cfg, power, res, (i, j) = _single_sat_case(
        g, g.GAT_LAYOUT_INTERLEAVED, "GPSL1", fs, N, M, B, N, s, D, J, 17, -1000.0, 500.0, 0.0, prns, seed=40 + G, noise=0.3)
    _check_stats(g, res, power, cfg, fs, N, prns)
    for k, p in enumerate(dict.fromkeys(prns)):
        rows, cols = acq_sample_bins(rng, D, J, n_cols=8, rows=[i], cols=[j, J - 2])
        ref = acq_power_oracle(re, im, codes, p, FC_L1, 1023, fs, 0.0, -1000.0, 500.0, rows, 17, s, cols, N, B, N)
        check_power_close(power[prns.index(p)][np.ix_(rows, cols)], ref, what=f"{regime} G {G} prn {p}")


# ---- device statistics against the host's where they can disagree -------------------------------------------------------
def _integer_signal(rng, M, ld, run):
    """Piecewise-constant integer samples in {-1, 0, 1} (runs of `run` samples): at zero Doppler every R is an integer and so
    is every power, exactly in float32 while |R|^2 summed stays below 2^24."""
    n = -(-ld // run)
    v = rng.integers(-1, 2, (M, n, 2)).astype(np.float32)
    v = np.repeat(v, run, axis=1)[:, :ld]
    return v[..., 0].copy(), v[..., 1].copy()


TIES = [  # name, signal, M, B, N, D, f_step, J, s
    ("all_ones_rows_identical", "ones", 2, 2, 1023, 40, 0.0, 1023, 1),
    ("piecewise_rows_identical", "piecewise", 2, 1, 1500, 40, 0.0, 700, 2),
    ("all_ones_one_row", "ones", 1, 3, 2046, 1, 0.0, 300, 1),
]


@pytest.mark.parametrize("case", TIES, ids=[t[0] for t in TIES])
def test_device_stats_equal_host_on_exact_grids_with_ties(g, case):
    """Integer grids, so the device and the host see the same numbers and every tie is a real tie: 'first on ties' (a strided
    per-thread scan + tree on the device, a linear scan on the host) must pick the same bin, and the rest must follow."""
    import torch
    name, kind, M, B, N, D, f_step, J, s = case
    fs = 1.023e6
    rng = np.random.default_rng(5)
    if kind == "ones":
        re = np.ones((M, B * N), dtype=np.float32)
        im = np.zeros_like(re)
    else:
        re, im = _integer_signal(rng, M, B * N, 37)
    codes = _codes("GPSL1")
    cfg = _cfg(g, D, J, s, FC_L1, 1023, 0, 0.0, f_step)
    prns = [0, 5, 5]
    rc, power, res = _acquire(g, codes, (torch.from_numpy(re).cuda(), torch.from_numpy(im).cuda()), N, B, N, prns, fs, cfg)
    assert rc == 0
    assert (power == np.rint(power)).all() and power.max() < 2 ** 24
    if f_step == 0.0 and D > 1:
        assert (power == power[:, :1]).all()  # identical rows: the peak's row must be 0
        assert (res["doppler_bin"] == 0).all()
    # ties are present: several bins share the grid's maximum, or the noise set's maximum
    assert any((power[k] == power[k].max()).sum() > 1 for k in range(len(prns)))
    _check_stats(g, res, power, cfg, fs, N, prns, exact_noise=True)
    cols = np.unique([0, 1, 255, 256, J - 1, *res["code_bin"]])
    for p in (0, 5):
        ref = acq_power_oracle(re, im, codes, p, FC_L1, 1023, fs, 0.0, 0.0, f_step, np.array([0, D - 1]), 0, s, cols, N, B, N)
        assert np.array_equal(power[prns.index(p)][np.ix_([0, D - 1], cols)].astype(np.float64), ref), p


@pytest.mark.parametrize("edge", ["first_code_bin", "last_code_bin", "last_doppler_row"])
def test_peak_on_the_grid_edge(g, edge):
    """A satellite whose peak is on the grid's edge: the missing neighbour is NaN, the refinement stays at the bin centre on
    that axis -- on the device as on the host."""
    fs, N, D, J, s = 4.0e6, 4000, 12, 300, 2
    f_first, f_step, first_shift = -3000.0, 500.0, 50
    i, j = {"first_code_bin": (5, 0), "last_code_bin": (6, J - 1), "last_doppler_row": (D - 1, 130)}[edge]
    rng = np.random.default_rng(77)
    lc = 1023
    x = _constellation(rng, "GPSL1", fs, N, 1, [(8, f_first + i * f_step, _bin_phase(FC_L1, fs, lc, first_shift, s, j))], 0.3)
    host, re, im = _quantize(x, g.GAT_LAYOUT_PLANAR, g)
    cfg = _cfg(g, D, J, s, FC_L1, lc, first_shift, f_first, f_step)
    rc, power, res = _acquire(g, _codes("GPSL1"), _to_device(host), N, 1, N, [8], fs, cfg)
    assert rc == 0
    _check_stats(g, res, power, cfg, fs, N, [8])
    r = res[0]
    assert (r["doppler_bin"], r["code_bin"], r["detected"]) == (i, j, 1)
    if edge == "last_doppler_row":
        assert r["carrier_doppler_hz"] == f_first + (D - 1) * f_step
    else:
        assert r["code_phase_chips"] == _bin_phase_exact(cfg, fs, j)


def _bin_phase_exact(cfg, fs, j):
    """csrc/gat_acq.h acq_code_phase at a whole bin."""
    lc = float(cfg.code_length)
    ph = cfg.code_freq_hz / fs * (float(cfg.first_shift) + float(cfg.code_step_samples) * float(j))
    ph -= math.floor(ph / lc) * lc
    return 0.0 if (ph >= lc or ph < 0.0) else ph


def test_too_few_noise_bins_gives_no_estimate(g):
    """Fewer than 64 bins outside the peak's +-1.5 chips: detected = -1 and NaN noise fields, on the device as on the host."""
    fs, N, D, J, s = 2.046e6, 2046, 5, 12, 1  # 6 chips of code bins: at most 5 x 9 noise bins
    rng = np.random.default_rng(3)
    x = _constellation(rng, "GPSL1", fs, N, 1, [(1, 0.0, _bin_phase(FC_L1, fs, 1023, 0, s, 6))], 0.3)
    host, re, im = _quantize(x, g.GAT_LAYOUT_PLANAR, g)
    cfg = _cfg(g, D, J, s, FC_L1, 1023, 0, -1000.0, 500.0)
    rc, power, res = _acquire(g, _codes("GPSL1"), _to_device(host), N, 1, N, [1, 2], fs, cfg)
    assert rc == 0
    _check_stats(g, res, power, cfg, fs, N, [1, 2])
    assert (res["detected"] == -1).all() and (res["num_noise_bins"] < 64).all()
    for f in ("noise_power", "second_power", "peak_to_second", "cn0_dbhz"):
        assert np.isnan(res[f]).all(), f


# ---- alignment and layout through the Python layer ---------------------------------------------------------------------
LAYOUT_IDS = ["planar", "interleaved", "int16", "int8"]


def _grids(g, system, sig, fs, N, **kw):
    res = g.acquire(system, sig, fs, [3, 14], num_samples=N, keep_power=True, **kw)
    return np.stack([r.power_bins.cpu().numpy() for r in res]), [(r.doppler_bin, r.code_bin, r.signal_power) for r in res]


@pytest.mark.parametrize("layout", range(4), ids=LAYOUT_IDS)
def test_odd_offset_view_equals_aligned_copy(g, layout):
    """A signal view starting at an odd sample offset (a sliced tensor) and the same samples in a fresh aligned tensor give
    the same grid bit for bit: the kernel reads samples with scalar loads."""
    system, fs, N, M, off = g.GPSL1(), 4.0e6, 4003, 3, 5
    rng = np.random.default_rng(50 + layout)
    x = _constellation(rng, "GPSL1", fs, N + 2 * off + 1, M, [(3, 1200.0, 321.7)], 0.5)
    host, _, _ = _quantize(x, layout, g)
    full = _to_device(host)
    view = tuple(t[:, off:off + N] for t in full)
    copy = tuple(v.clone() for v in view)
    assert all(v.data_ptr() % 16 != 0 for v in view) and all(c.data_ptr() % 16 == 0 for c in copy)
    kw = dict(max_doppler=3000.0, doppler_step=500.0, code_step_chips=0.5, num_code_bins=300, first_shift=-11)
    a, ra = _grids(g, system, view if layout == g.GAT_LAYOUT_PLANAR else view[0], fs, N, **kw)
    b, rb = _grids(g, system, copy if layout == g.GAT_LAYOUT_PLANAR else copy[0], fs, N, **kw)
    assert a.tobytes() == b.tobytes() and ra == rb


@pytest.mark.parametrize("layout", range(4), ids=LAYOUT_IDS)
def test_overlapping_blocks_equal_a_copy_laid_out_block_by_block(g, layout):
    """block_stride < N against the same blocks copied one after the other (block_stride = N).  fs = fc makes the blocks' code
    phases tau_b = fmod(b * stride, Lc) equal in both layouts (N - stride = Lc), so the grids must be equal bit for bit."""
    import torch
    system, fs, N, M, B = g.GPSL1(), FC_L1, 3000, 2, 3
    stride = N - 1023
    rng = np.random.default_rng(60 + layout)
    ld = (B - 1) * stride + N
    x = _constellation(rng, "GPSL1", fs, ld, M, [(14, -700.0, 100.25)], 0.5)
    host, _, _ = _quantize(x, layout, g)
    over = _to_device(host)
    blocks = tuple(torch.cat([t[:, b * stride:b * stride + N] for b in range(B)], dim=1).contiguous() for t in over)
    kw = dict(max_doppler=2000.0, doppler_step=250.0, code_step_chips=1.0, num_code_bins=1023, num_blocks=B)
    one = (lambda t: t if layout == g.GAT_LAYOUT_PLANAR else t[0])
    a, ra = _grids(g, system, one(over), fs, N, block_stride=stride, **kw)
    b, rb = _grids(g, system, one(blocks), fs, N, block_stride=N, **kw)
    assert a.tobytes() == b.tobytes() and ra == rb
