"""CPU tests of the acquisition search's statistics (include/gat.h gat_acq_stats_host; arithmetic in csrc/gat_acq.h, shared
with the device kernel) against a numpy restatement on seeded synthetic grids, the Julia shim's mirrors of the new structs,
and the Python layer's grid defaults.  No device needed."""
import ctypes as C
import math

import numpy as np
import pytest

FC, LC = 1.023e6, 1023


@pytest.fixture(scope="module")
def g():
    import gpuacceleratedtracking_amd as g
    g.load_library()
    return g


def _cfg(g, D, J, s, first_shift=0, f_first=-7000.0, f_step=500.0, lc=LC, ratio=2.0):
    cfg = g._lib.AcqConfig()
    cfg.struct_size = C.sizeof(g._lib.AcqConfig)
    cfg.num_doppler_bins, cfg.num_code_bins, cfg.code_step_samples = D, J, s
    cfg.code_freq_hz, cfg.doppler_first_hz, cfg.doppler_step_hz = FC, f_first, f_step
    cfg.first_shift, cfg.min_peak_ratio, cfg.code_length = first_shift, ratio, lc
    return cfg


def np_stats(power, D, J, s, first_shift, f_first, f_step, fs, N, lc=LC, ratio=2.0):
    """The statistics as include/gat.h states them."""
    def phase(j):
        ph = FC / fs * (first_shift + s * j)
        ph = ph - math.floor(ph / lc) * lc
        return 0.0 if (ph >= lc or ph < 0) else ph

    def parabola(a, b, c):
        den = a - 2 * b + c
        if not den < 0:
            return 0.0
        d = 0.5 * (a - c) / den
        return max(-0.5, min(0.5, d))

    out = []
    for g in power.astype(np.float64):
        pk = int(np.argmax(g))
        i, j = divmod(pk, J)
        peak = g[i, j]
        di = parabola(g[i - 1, j], peak, g[i + 1, j]) if 0 < i < D - 1 else 0.0
        dj = parabola(g[i, j - 1], peak, g[i, j + 1]) if 0 < j < J - 1 else 0.0
        ph = np.array([phase(k) for k in range(J)])
        d = np.abs(ph - phase(j))
        d = np.minimum(d, lc - d)
        sel = np.broadcast_to(d > 1.5, (D, J))
        r = dict(doppler_bin=i, code_bin=j, peak_power=peak, num_noise_bins=int(sel.sum()),
                 carrier_doppler_hz=f_first + (i + di) * f_step, code_phase_chips=phase(j + dj))
        if sel.sum() < 64:
            r.update(noise_power=np.nan, second_power=np.nan, peak_to_second=np.nan, cn0_dbhz=np.nan, detected=-1)
        else:
            noise = g[sel].mean()
            second = g[sel].max()
            r.update(noise_power=noise, second_power=second, peak_to_second=peak / second,
                     cn0_dbhz=10 * math.log10((peak - noise) / (noise * N / fs)), detected=int(peak / second >= ratio))
        out.append(r)
    return out


def _check(got, ref):
    for p, r in enumerate(ref):
        assert got["prn"][p] == p
        for k, v in r.items():
            if isinstance(v, int):
                assert got[k][p] == v, (p, k, got[k][p], v)
            elif np.isnan(v):
                assert np.isnan(got[k][p]), (p, k)
            else:
                assert got[k][p] == pytest.approx(v, rel=1e-9, abs=1e-9), (p, k, got[k][p], v)


def _grid(seed, P, D, J):
    return np.random.default_rng(seed).exponential(1.0, size=(P, D, J)).astype(np.float32)


def test_stats_match_restatement_on_random_grids(g):
    fs, N, D, J, s = 4e6, 4000, 29, 2000, 2
    pw = _grid(1, 4, D, J)
    pw[0, 10, 700] = 60.0  # a clear peak
    pw[0, 9, 700], pw[0, 11, 700], pw[0, 10, 699], pw[0, 10, 701] = 20.0, 35.0, 30.0, 12.0
    pw[1, 3, 5] = 4.0  # weak: no detection
    got = g.acquisition_stats_host(pw, _cfg(g, D, J, s), fs, N)
    ref = np_stats(pw, D, J, s, 0, -7000.0, 500.0, fs, N)
    _check(got, ref)
    assert got["detected"][0] == 1 and got["detected"][1] == 0


def test_peak_at_the_code_period_wrap(g):
    """A peak on the grid's last bins, whose phase sits just below Lc: the noise set's exclusion wraps to the first bins."""
    fs, N, D, J, s = 4e6, 4000, 9, 2000, 2
    pw = _grid(2, 1, D, J)
    jpk = 1998  # phase = 1998 * 2 * fc / fs = 1022.0 chips
    pw[0, 4, jpk] = 80.0
    pw[0, 4, 0] = 40.0  # 1.02 chip away across the wrap: inside the exclusion, so not the second peak
    got = g.acquisition_stats_host(pw, _cfg(g, D, J, s), fs, N)
    ref = np_stats(pw, D, J, s, 0, -7000.0, 500.0, fs, N)
    _check(got, ref)
    assert got["second_power"][0] < 40.0
    # the bins excluded: within 1.5 chips on both sides of the wrap
    ph = (FC / fs * s * np.arange(J)) % LC
    d = np.abs(ph - ph[jpk])
    assert got["num_noise_bins"][0] == D * int((np.minimum(d, LC - d) > 1.5).sum())
    assert np.minimum(d, LC - d)[0] <= 1.5 and np.minimum(d, LC - d)[1] > 1.5


def test_peak_on_the_grid_edge_keeps_the_bin_centre(g):
    fs, N, D, J, s = 4e6, 4000, 15, 300, 2
    pw = _grid(3, 2, D, J)
    pw[0, 0, 0] = 70.0  # Doppler and code edges: no parabola
    pw[0, 1, 0], pw[0, 0, 1] = 50.0, 60.0
    pw[1, 14, 149] = pw[1, 14, 150] = 70.0  # last Doppler row; a tie: the first bin is the peak, the vertex half a bin on
    pw[1, 13, 149], pw[1, 14, 148] = 10.0, 1.0
    got = g.acquisition_stats_host(pw, _cfg(g, D, J, s, first_shift=-40), fs, N)
    ref = np_stats(pw, D, J, s, -40, -7000.0, 500.0, fs, N)
    _check(got, ref)
    assert got["carrier_doppler_hz"][0] == -7000.0
    assert got["code_phase_chips"][0] == pytest.approx((FC / fs * -40) % LC)
    assert got["carrier_doppler_hz"][1] == -7000.0 + 14 * 500.0
    assert got["code_phase_chips"][1] == pytest.approx((FC / fs * (-40 + 2 * 149.5)) % LC)


def test_cn0_on_a_known_signal_to_noise_ratio(g):
    """Noise bins of mean 2 sigma^2 N, a peak of A^2 N^2 above it: C/N0 = A^2 fs / (2 sigma^2) = 45 dB-Hz."""
    fs, N, D, J, s = 20e6, 20000, 29, 2000, 10
    sigma2 = fs / (2 * 10 ** 4.5)
    noise = 2 * sigma2 * N
    pw = np.full((1, D, J), noise, dtype=np.float32)
    pw[0, 7, 321] = noise + N * N
    got = g.acquisition_stats_host(pw, _cfg(g, D, J, s), fs, N)
    assert got["cn0_dbhz"][0] == pytest.approx(45.0, abs=1e-4)
    assert got["noise_power"][0] == pytest.approx(noise, rel=1e-6)
    _check(got, np_stats(pw, D, J, s, 0, -7000.0, 500.0, fs, N))


def test_narrow_grid_has_no_noise_estimate(g):
    fs, N, D, J, s = 4e6, 40000, 3, 16, 1  # +-2 chips at a quarter chip: every bin within 1.5 chips of ... too few outside
    pw = _grid(4, 1, D, J)
    pw[0, 1, 8] = 50.0
    got = g.acquisition_stats_host(pw, _cfg(g, D, J, s, first_shift=400), fs, N)
    assert got["detected"][0] == -1 and got["num_noise_bins"][0] < 64
    for k in ("noise_power", "second_power", "peak_to_second", "cn0_dbhz"):
        assert np.isnan(got[k][0]), k
    _check(got, np_stats(pw, D, J, s, 400, -7000.0, 500.0, fs, N))


def test_stats_argument_errors(g):
    lib = g.load_library()
    pw = _grid(5, 1, 4, 100)
    res = np.zeros(1, dtype=g._lib.ACQ_RESULT_DTYPE)

    def call(cfg, P=1, D=4, J=100, fs=4e6, N=4000, power=pw):
        return lib.gat_acq_stats_host(C.c_void_p(power.ctypes.data) if power is not None else None, P, D, J,
                                      C.byref(cfg) if cfg is not None else None, fs, N, C.c_void_p(res.ctypes.data))
    ok = _cfg(g, 4, 100, 2)
    assert call(ok) == 0
    assert call(ok, power=None) == 1
    assert call(None) == 1
    assert call(ok, P=0) == 1
    assert call(_cfg(g, 0, 100, 2), D=0) == 1  # empty grid
    assert call(ok, D=5) == 1  # grid differs from the config
    assert call(_cfg(g, 4, 100, 0)) == 1  # s < 1
    assert call(_cfg(g, 4, 100, 64)) == 2  # s above the bound
    assert call(_cfg(g, 4, 100, 2, lc=0)) == 1
    assert call(ok, fs=0.0) == 1
    assert call(ok, N=0) == 1
    big = _cfg(g, 4096, 20000, 1)
    assert call(big, D=4096, J=20000) == 2  # grid above 2^26 bins
    bad = _cfg(g, 4, 100, 2)
    bad.struct_size = 8
    assert call(bad) == 1


def test_python_grid_defaults(g):
    """Half-chip code bins over one code period, Doppler +-7 kHz in steps of 1 / (2 N / fs), as the library receives them."""
    from gpuacceleratedtracking_amd import _lib
    assert C.sizeof(_lib.AcqConfig) == 72 and _lib.ACQ_RESULT_DTYPE.itemsize == 80
    fs, fc = 20e6, 1.023e6
    s = max(1, round(0.5 * fs / fc))
    assert s == 10 and math.ceil(LC * fs / (fc * s)) == 2000
    assert fs / (2 * 20000) == 500.0


def test_julia_mirrors_of_the_acquisition_structs():
    from tests.test_julia_shim_lint import c_class, c_layout, c_structs, jl_class, jl_ccalls, jl_layout, jl_structs
    cs, js = c_structs(), jl_structs()
    for cname, jname in (("gat_acq_config", "AcqConfig"), ("gat_acq_result", "AcqResult")):
        assert cname in cs and jname in js, (cname, jname)
        cf, jf = cs[cname], js[jname]
        assert [n for _, n in cf] == [n for _, n in jf]
        for (ct, n), (jt, _) in zip(cf, jf):
            assert c_class(ct) == jl_class(jt), (jname, n)
        assert c_layout(cname, [n for _, n in cf]) == jl_layout(jf)
    bound = {c["sym"] for c in jl_ccalls()}
    assert {"gat_acquire", "gat_acq_stats_host"} <= bound
