"""GPU tests of the acquisition search (include/gat.h gat_acquire, csrc/gat_acq.hip, gpuacceleratedtracking_amd.acquisition):
the power grid against the FP64 oracle's correlator restated as the search's formula, detection on a noisy multi-satellite
signal, a coarse -> fine search that seeds a tracking loop, determinism, and argument errors."""
import ctypes as C
import math

import numpy as np
import pytest

import oracle
from tests.helpers import acq_power_oracle, acq_sample_bins, check_power_close

pytestmark = pytest.mark.gpu

FC, LC = 1.023e6, 1023


@pytest.fixture(scope="module")
def g():
    import gpuacceleratedtracking_amd as g
    g.load_library()
    return g


def _cfg(g, D, J, s, first_shift=0, f_first=0.0, f_step=0.0, if_hz=0.0, lc=LC):
    cfg = g._lib.AcqConfig()
    cfg.struct_size = C.sizeof(g._lib.AcqConfig)
    cfg.num_doppler_bins, cfg.num_code_bins, cfg.code_step_samples = D, J, s
    cfg.if_hz, cfg.code_freq_hz, cfg.doppler_first_hz, cfg.doppler_step_hz = if_hz, FC, f_first, f_step
    cfg.first_shift, cfg.min_peak_ratio, cfg.code_length = first_shift, 2.0, lc
    return cfg


def _device_signal(g, x, layout):
    """x: complex128 [M, ld] -> (device signal in `layout`, the same values as float32 planar for the oracle)."""
    import torch
    if layout in (g.GAT_LAYOUT_INTERLEAVED_I16, g.GAT_LAYOUT_INTERLEAVED_I8):
        dt = np.int16 if layout == g.GAT_LAYOUT_INTERLEAVED_I16 else np.int8
        lim = np.iinfo(dt).max
        pair = np.clip(np.stack([np.rint(x.real), np.rint(x.imag)], axis=-1), -lim, lim).astype(dt)
        re, im = pair[..., 0].astype(np.float32), pair[..., 1].astype(np.float32)
        return (torch.from_numpy(np.ascontiguousarray(pair)).cuda(),), re, im
    re, im = x.real.astype(np.float32), x.imag.astype(np.float32)
    if layout == g.GAT_LAYOUT_PLANAR:
        return (torch.from_numpy(re).cuda(), torch.from_numpy(im).cuda()), re, im
    pair = np.ascontiguousarray(np.stack([re, im], axis=-1))
    return (torch.from_numpy(pair).cuda(),), re, im


def _acquire_raw(g, sig, N, B, bstride, prns, fs, cfg, keep=True):
    import torch
    from gpuacceleratedtracking_amd.acquisition import _as_desc
    ctx = g.get_context()
    ctx.set_codes(g.GPSL1().codes)
    desc = _as_desc(sig if len(sig) == 2 else sig[0], N, B, bstride)
    P = len(prns)
    power = torch.empty((P, cfg.num_doppler_bins, cfg.num_code_bins), dtype=torch.float32, device="cuda") if keep else None
    res = np.zeros(P, dtype=g._lib.ACQ_RESULT_DTYPE)
    pr = np.ascontiguousarray(prns, dtype=np.int32)
    rc = ctx.lib.gat_acquire(ctx._h, C.byref(desc), B, pr.ctypes.data_as(C.POINTER(C.c_int32)), P, fs, C.byref(cfg),
                             C.c_void_p(power.data_ptr() if keep else None), C.c_void_p(res.ctypes.data))
    return rc, (power.cpu().numpy() if keep else None), res


PARITY = [  # layout, M, B, N, block_stride, fs, s, first_shift, J, D, if_hz
    (0, 1, 1, 2000, 2000, 2.0e6, 1, 0, 600, 40, 0.0),
    (1, 4, 3, 20000, 20013, 20.0e6, 10, -37, 210, 29, 1.0e4),
    (2, 4, 1, 20000, 20000, 20.0e6, 10, 19000, 300, 33, 0.0),
    (3, 1, 3, 4001, 4100, 4.0e6, 1, 5, 700, 17, -2.5e3),
]


@pytest.mark.parametrize("case", PARITY, ids=["planar", "interleaved", "int16", "int8"])
def test_power_grid_matches_oracle(g, case):
    layout, M, B, N, bstride, fs, s, first_shift, J, D, if_hz = case
    rng = np.random.default_rng(100 + layout)
    codes = oracle.codes("GPSL1", 32)
    prns = [3, 17, 30]
    ld = (B - 1) * bstride + N + 7
    # the searched satellites (one on a Doppler bin, two between) in noise
    x = np.zeros(ld, dtype=np.complex128)
    for k, p in enumerate(prns):
        r1, i1 = oracle.gen_signal(codes, p, FC, fs, if_hz + 250.0 * (k - 1) + 100.0 * k, rng.uniform(0, LC), 0.3 * k, ld, 1)
        x += r1[0] + 1j * i1[0]
    x = x[None, :] * np.exp(2j * np.pi * rng.uniform(0, 1, (M, 1))) + 0.5 * (rng.standard_normal((M, ld)) + 1j * rng.standard_normal((M, ld)))
    scale = {0: 1.0, 1: 1.0, 2: 1000.0, 3: 20.0}[layout]
    sig, re, im = _device_signal(g, x * scale, layout)
    f_first, f_step = -5000.0, 250.0
    cfg = _cfg(g, D, J, s, first_shift, f_first, f_step, if_hz)
    rc, power, _ = _acquire_raw(g, sig, N, B, bstride, prns, fs, cfg)
    assert rc == 0
    rand = rng.choice(J, 40, replace=False)
    rows = np.arange(D)
    for pi, p in enumerate(prns):
        peak = np.unravel_index(np.argmax(power[pi]), power[pi].shape)
        _, jsel = acq_sample_bins(rng, D, J, n_cols=0, cols=[*rand, peak[1]])
        ref = acq_power_oracle(re, im, codes, p, FC, LC, fs, if_hz, f_first, f_step, rows, first_shift, s, jsel, N, B, bstride)
        check_power_close(power[pi][:, jsel], ref, what=f"prn {p}")


def test_all_ones_signal_is_exact(g):
    """All-ones samples at zero Doppler: every R is an integer, so is every power -- equal to the oracle's bit for bit."""
    import torch
    N, M, B, fs = 1024, 2, 2, 1.023e6
    codes = oracle.codes("GPSL1", 32)
    re = np.ones((M, B * N), dtype=np.float32)
    im = np.zeros_like(re)
    sig = (torch.from_numpy(re).cuda(), torch.from_numpy(im).cuda())
    J = 1023
    cfg = _cfg(g, 1, J, 1)
    prns = [0, 9]
    rc, power, _ = _acquire_raw(g, sig, N, B, N, prns, fs, cfg)
    assert rc == 0
    shifts = np.arange(J, dtype=np.int32)
    tau = np.fmod(FC / fs * (np.arange(B) * N).astype(np.float64), float(LC))
    for pi, p in enumerate(prns):
        prm = oracle.make_params(np.full((B, 1), p), FC, 0.0, np.broadcast_to(tau[:, None], (B, 1)), 0.0)
        R = oracle.correlate_f64(re, im, codes, prm, fs, shifts, N=N)
        ref = (np.abs(R) ** 2).sum(axis=(0, 3))
        assert np.array_equal(power[pi].astype(np.float64), ref)


def _noisy_constellation(g, fs, N, M, sats, seed):
    """sats: list of (prn0, doppler, code_phase); 45 dB-Hz each (sigma per component = sqrt(fs / (2 10^4.5)) in units of
    one satellite's amplitude), steered antennas, complex white noise; no satellites: the noise alone."""
    import torch
    sigma = math.sqrt(fs / (2 * 10 ** 4.5))
    if not sats:
        gen = torch.Generator(device="cuda").manual_seed(seed)
        re = torch.randn((M, N), generator=gen, device="cuda") * sigma
        return re, torch.randn((M, N), generator=gen, device="cuda") * sigma
    system = g.GPSL1()
    prm = g.make_params(np.array([p for p, _, _ in sats]), np.array([FC * (1 + d / 1575.42e6) for _, d, _ in sats]),
                        np.array([d for _, d, _ in sats]), np.array([t for _, _, t in sats]), 0.0, shape=(1, len(sats)))
    ctx = g.get_context()
    ctx.set_codes(system.codes)
    re = torch.empty((M, N), dtype=torch.float32, device="cuda")
    im = torch.empty_like(re)
    steer = torch.from_numpy(np.random.default_rng(seed).uniform(0, 1, M).astype(np.float32)).cuda()
    ctx.gen_signal(re, im, g.GAT_LAYOUT_PLANAR, N, M, N, N, 1, len(sats), ctx.params_to_device(prm), fs, amplitude=1.0,
                   steering_cycles=steer, noise_sigma=sigma, seed=seed)
    return re, im


# code phases 0.03 - 0.05 chip from a half-chip bin (0.5115 chip at 20 MHz, s = 10): the C/N0 read off the peak bin
SATS = [(2, 1500.0, 100.265), (7, -2000.0, 511.53), (12, 3000.0, 900.27), (19, -500.0, 33.27), (25, 4500.0, 700.78),
        (30, -4000.0, 250.66)]


def test_detects_six_satellites_among_32(g):
    fs, N, M = 20.0e6, 20000, 4
    re, im = _noisy_constellation(g, fs, N, M, SATS, seed=11)
    res = g.acquire(g.GPSL1(), (re, im), fs, range(32), num_samples=N, max_doppler=7000.0, doppler_step=500.0)
    truth = {p: (d, t) for p, d, t in SATS}
    for r in res:
        if r.prn in truth:
            d, t = truth[r.prn]
            assert r.detected == 1, r
            assert abs(r.carrier_doppler - d) <= 250.0, r
            dt = abs((r.code_phase - t + LC / 2) % LC - LC / 2)
            assert dt <= 0.25, (r, dt)
            assert abs(r.CN0 - 45.0) <= 2.0, r
        else:
            assert r.detected == 0, r


def test_noise_only_detects_nothing(g):
    fs, N, M = 20.0e6, 20000, 4
    re, im = _noisy_constellation(g, fs, N, M, [], seed=12)
    res = g.acquire(g.GPSL1(), (re, im), fs, range(32), num_samples=N, max_doppler=7000.0, doppler_step=500.0)
    assert all(r.detected == 0 for r in res), [r.peak_to_second for r in res]


def test_coarse_fine_then_track(g):
    """1 ms coarse search, 10 ms fine search (+-250 Hz in 10 Hz steps, +-2 chips), then the closed loop seeded from it
    converges as in test_closed_loop_single_satellite_converges."""
    system = g.GPSL1()
    N, M, fs, nblk = 4000, 2, 4e6, 1500
    prns, true_dop, true_tau0, true_phi0 = np.array([7]), np.array([-2210.0]), np.array([511.9]), np.array([0.6])
    fcode = FC * (1 + true_dop / 1575.42e6)
    b = np.arange(nblk, dtype=np.float64)[:, None]
    tau = np.mod(true_tau0[None, :] + fcode[None, :] * (N / fs) * b, 1023.0)
    phi = np.mod(true_phi0[None, :] + true_dop[None, :] * (N / fs) * b, 1.0)
    prm_sig = g.make_params(prns - 1, fcode, true_dop, tau, 2 * np.pi * phi, shape=(nblk, 1))
    re, im = g.gen_signal_stream(system, prm_sig, fs, N, M)
    coarse = g.acquire(system, (re, im), fs, prns - 1, num_samples=N)[0]
    assert coarse.detected == 1 and abs(coarse.carrier_doppler - true_dop[0]) < 250.0
    s = 1  # quarter-chip code bins for the fine search
    shift0 = int(math.floor((coarse.code_phase - 2.0) * fs / FC))
    fine = g.acquire(system, (re, im), fs, prns - 1, num_samples=10 * N, dopplers=coarse.carrier_doppler + np.arange(-250.0, 250.5, 10.0),
                     code_step_chips=0.25, first_shift=shift0, num_code_bins=int(math.ceil(4.0 * fs / FC / s)) + 1)[0]
    assert abs(fine.carrier_doppler - true_dop[0]) < 5.0, fine
    assert abs((fine.code_phase - true_tau0[0] + 511.5) % 1023.0 - 511.5) < 0.1, fine
    init = g.tracking_init([fine], system, detected_only=False)
    shifts = g.get_correlator_sample_shifts(system, g.EarlyPromptLateCorrelator(M, 3), fs, 0.5)
    loop = g.TrackingLoop(system, init["prns"], N, M, fs, shifts, init_carrier_doppler=init["init_carrier_doppler"],
                          init_code_phase=init["init_code_phase"], init_carrier_phase=0.0, dll_bandwidth_hz=4.0)
    for i in range(nblk):
        loop.step(re, im, start=i * N)
    st, p = loop.state(), loop.params().reshape(-1)
    tau_end = np.mod(true_tau0 + fcode * (N / fs) * nblk, 1023.0)
    dtau = np.abs(((p["code_phase_chips"] - tau_end + 511.5) % 1023.0) - 511.5)
    acc = loop.accumulators()
    assert abs(st["carrier_doppler_hz"][0] + 2210.0) < 0.2
    assert dtau[0] < 0.02
    assert abs(st["last_pll_error_cycles"][0]) < 5e-3 and abs(st["last_dll_error_chips"][0]) < 0.02
    assert (np.abs(acc[0, 1, :]) > 0.97 * N).all()
    assert (np.abs(acc[0, 1, :].imag) < 0.04 * N).all()


def test_deterministic_and_device_stats_equal_host(g):
    fs, N, M = 20.0e6, 20000, 4
    re, im = _noisy_constellation(g, fs, N, M, SATS[:3], seed=13)
    prns = list(range(8))
    D, J, s = 29, 2000, 10
    cfg = _cfg(g, D, J, s, 0, -7000.0, 500.0)
    rc1, p1, r1 = _acquire_raw(g, (re, im), N, 1, N, prns, fs, cfg)
    rc2, p2, r2 = _acquire_raw(g, (re, im), N, 1, N, prns, fs, cfg)
    assert rc1 == 0 and rc2 == 0
    assert p1.tobytes() == p2.tobytes() and r1.tobytes() == r2.tobytes()
    h = g.acquisition_stats_host(p1, cfg, fs, N)
    for f in ("detected", "doppler_bin", "code_bin", "num_noise_bins"):
        assert np.array_equal(h[f], r1[f]), f
    assert np.array_equal(r1["prn"], prns)
    for f in ("peak_power", "noise_power", "second_power", "peak_to_second", "carrier_doppler_hz", "code_phase_chips"):
        assert np.allclose(h[f], r1[f], rtol=1e-6, atol=0), f
    assert np.allclose(h["cn0_dbhz"], r1["cn0_dbhz"], rtol=0, atol=1e-5)


def test_argument_and_state_errors(g):
    import torch
    lib = g.load_library()
    fs, N = 4e6, 4000
    re = torch.zeros((1, N), dtype=torch.float32, device="cuda")
    im = torch.zeros_like(re)
    cfg = _cfg(g, 5, 100, 2)
    # before any code table: GAT_ERR_STATE
    h = C.c_void_p()
    assert lib.gat_create(0, None, C.byref(h)) == 0
    try:
        from gpuacceleratedtracking_amd.tracking import _signal_desc
        desc = _signal_desc(re, im, N)
        res = np.zeros(1, dtype=g._lib.ACQ_RESULT_DTYPE)
        pr = np.array([0], dtype=np.int32)
        call = lambda c, P=1: lib.gat_acquire(h, C.byref(desc), 1, pr.ctypes.data_as(C.POINTER(C.c_int32)), P, fs,  # noqa: E731
                                              C.byref(c), None, C.c_void_p(res.ctypes.data))
        assert call(cfg) == 3
        codes = np.ascontiguousarray(g.GPSL1().codes)
        assert lib.gat_set_codes(h, codes.ctypes.data_as(C.POINTER(C.c_int8)), codes.shape[1], codes.shape[0]) == 0
        assert call(cfg) == 0
        pr[0] = 99
        assert call(cfg) == 2  # PRN outside the table
        pr[0] = 0
        assert call(_cfg(g, 0, 100, 2)) == 1  # empty grid
        assert call(_cfg(g, 5, 0, 2)) == 1
        assert call(cfg, P=0) == 1
        assert call(_cfg(g, 5, 100, 0)) == 1  # s < 1
        assert call(_cfg(g, 5, 100, 40)) == 2  # s above the bound
        assert call(_cfg(g, 4096, 20000, 1)) == 2  # grid above 2^26 bins
        assert call(_cfg(g, 5, 100, 2, first_shift=1 << 30)) == 2
        bad = _cfg(g, 5, 100, 2)
        bad.struct_size = 8
        assert call(bad) == 1
    finally:
        lib.gat_destroy(h)
