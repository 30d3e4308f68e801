"""GPU tests of the FFT acquisition search (include/gat.h gat_acquire_fft, csrc/gat_acq_fft.hip, acquire(method="fft")): the device
grid against the FP64 contract in the four sample layouts at the shapes that reach every instance, device bits against the host
twin for every instance the plan can choose (one pass, two passes, one and several lag segments, unit groups, Doppler and unit
batches), the whole grid against the direct search, determinism and the device's statistics, detection on a noisy constellation,
a search that seeds a tracking loop, the beamformed search, and the refusals."""
import ctypes as C
import math

import numpy as np
import pytest

import oracle
from tests import acqfft_ref as ref
from tests.helpers import RTOL, acq_power_oracle, check_power_close

pytestmark = pytest.mark.gpu

FC, LC = ref.FC, ref.LC


@pytest.fixture(scope="module")
def g():
    import gpuacceleratedtracking_amd as g
    g.load_library()
    return g


@pytest.fixture()
def ctx(g):
    c = g.get_context()
    c.set_codes(g.GPSL1().codes)
    yield c
    for name in ("acq_fft_log2", "acq_fft_doppler_batch", "acq_fft_unit_batch"):
        c.set_option(name, 0)


def _to_device(arrays):
    import torch
    return tuple(torch.from_numpy(a).cuda() for a in arrays)


def _acquire(g, ctx, name, sig, N, B, bstride, prns, fs, cfg):
    """The raw call: (status, grid [P, D, J] on the host, results)."""
    import torch
    from gpuacceleratedtracking_amd.acquisition import _as_desc
    desc = _as_desc(sig if len(sig) == 2 else sig[0], N, B, bstride)
    P = len(prns)
    power = torch.full((P, cfg.num_doppler_bins, cfg.num_code_bins), -1.0, dtype=torch.float32, device="cuda")
    res = np.zeros(P, dtype=g._lib.ACQ_RESULT_DTYPE)
    pr = np.ascontiguousarray(prns, dtype=np.int32)
    rc = getattr(ctx.lib, name)(ctx._h, C.byref(desc), B, pr.ctypes.data_as(C.POINTER(C.c_int32)), P, fs, C.byref(cfg),
                                C.c_void_p(power.data_ptr()), C.c_void_p(res.ctypes.data))
    return rc, power.cpu().numpy(), res


SHAPES4 = ["one-pass", "two-pass-two-segments", "odd-blocks", "int8"]  # the fourth: three segments of one-pass transforms


@pytest.mark.parametrize("layout", [ref.PLANAR, ref.CF32, ref.I16, ref.I8], ids=["planar", "interleaved", "int16", "int8"])
@pytest.mark.parametrize("name", SHAPES4)
def test_power_grid_matches_oracle(g, ctx, name, layout):
    _, M, B, N, bstride, fs, s, first_shift, J, D, if_hz, lg = ref.SHAPES[name]
    ld = ref.length(B, N, bstride)
    arrays, re, im = ref.scene(100 + layout, layout, M, ld, fs, if_hz)
    cfg = ref.config(g, D, J, s, first_shift, ref.F_FIRST, ref.F_STEP, if_hz)
    ctx.set_option("acq_fft_log2", lg)
    rc, power, _ = _acquire(g, ctx, "gat_acquire_fft", _to_device(arrays), N, B, bstride, ref.PRNS, fs, cfg)
    assert rc == 0, ctx.lib.gat_last_error(ctx._h)
    log2 = lg if lg else 13
    rng = np.random.default_rng(7)
    codes = oracle.codes("GPSL1", 32)
    worst = [0.0, 0.0]
    for pi, p in enumerate(ref.PRNS):
        peak = np.unravel_index(np.argmax(power[pi]), power[pi].shape)
        jsel = ref.sample_bins(rng, J, s, N, log2, extra=[peak[1]])  # the seams between lag segments are among them
        want = acq_power_oracle(re, im, codes, p, FC, LC, fs, if_hz, ref.F_FIRST, ref.F_STEP, np.arange(D), first_shift, s, jsel, N, B, bstride)
        e = check_power_close(power[pi][:, jsel], want, what=f"{name} layout {layout} prn {p}")
        worst = [max(worst[0], e[0]), max(worst[1], e[1])]
    print(f"{name} layout {layout}: worst norm-wise {worst[0] / RTOL:.4f} RTOL, element-wise {worst[1] / RTOL:.4f} RTOL")


# name of the shape, PRNs, Doppler bins, forced log2 F, Doppler batch, unit batch -> what the plan must report (passes, segments, groups > 1, batched)
INSTANCES = {
    "one-pass-groups": ("int16", [3], 1, 12, 0, 0, (1, 1, True, False)),        # P = 1, D = 1: the four units go to four groups
    "one-pass-segments": ("int8", ref.PRNS, 5, 12, 0, 0, (1, 3, True, False)),
    "one-pass-2048": ("int16", ref.PRNS, 3, 11, 0, 0, (1, 37, True, False)),    # 49 lags a segment: seams everywhere
    "two-pass": ("two-pass-two-segments", ref.PRNS, 5, 13, 0, 0, (2, 2, False, False)),  # one unit: no groups
    "two-pass-groups": ("odd-blocks", [17], 1, 0, 0, 0, (2, 1, True, False)),   # six units in six groups
    "two-pass-2^14": ("odd-blocks", ref.PRNS, 7, 14, 0, 0, (2, 1, True, False)),
    "doppler-batches": ("odd-blocks", ref.PRNS, 7, 0, 2, 0, (2, 1, True, True)),
    "unit-batches": ("odd-blocks", ref.PRNS, 17, 14, 3, 3, (2, 1, True, True)),  # three groups, two batches of one step; a block lies in both
    "one-pass-batches": ("int16", ref.PRNS, 5, 12, 2, 0, (1, 1, True, True)),
}


@pytest.mark.parametrize("inst", list(INSTANCES))
def test_device_bits_equal_the_twin(g, ctx, inst):
    name, prns, D, lg, dbatch, ubatch, want = INSTANCES[inst]
    layout, M, B, N, bstride, fs, s, first_shift, J, _, if_hz, _ = ref.SHAPES[name]
    ld = ref.length(B, N, bstride)
    arrays, _, _ = ref.scene(100 + layout, layout, M, ld, fs, if_hz)
    cfg = ref.config(g, D, J, s, first_shift, ref.F_FIRST, ref.F_STEP, if_hz)
    cus = ctx.device_info()["num_cus"]
    pl = ref.plan(g, ref.host_desc(g, arrays, layout, M, N, ld, bstride), B, len(prns), fs, cfg, lg, cus, dbatch, ubatch)
    got = (pl["passes"], pl["num_segments"], pl["unit_groups"] > 1, pl["doppler_batch"] < D or pl["unit_batch"] < M * B)
    assert got == want, pl
    for opt, v in (("acq_fft_log2", lg), ("acq_fft_doppler_batch", dbatch), ("acq_fft_unit_batch", ubatch)):
        ctx.set_option(opt, v)
    rc, power, _ = _acquire(g, ctx, "gat_acquire_fft", _to_device(arrays), N, B, bstride, prns, fs, cfg)
    assert rc == 0, ctx.lib.gat_last_error(ctx._h)
    twin = ref.twin(g, ref.host_desc(g, arrays, layout, M, N, ld, bstride), B, prns, fs, cfg, pl["fft_log2"], pl["unit_groups"])
    assert power.tobytes() == twin.tobytes(), f"{inst}: {np.count_nonzero(power != twin)} of {power.size} bins differ, worst {np.abs(power - twin).max() / twin.max():.3e}"


@pytest.mark.parametrize("name", ["odd-blocks", "int8"])
def test_whole_grid_agrees_with_the_direct_search(g, ctx, name):
    """Each search is within RTOL of the contract, so they agree within 2 RTOL per Doppler row: norm-wise on every bin,
    element-wise on the bins at 0.1 of the row's maximum and above."""
    layout, M, B, N, bstride, fs, s, first_shift, J, D, if_hz, lg = ref.SHAPES[name]
    ld = ref.length(B, N, bstride)
    arrays, _, _ = ref.scene(100 + layout, layout, M, ld, fs, if_hz)
    sig = _to_device(arrays)
    cfg = ref.config(g, D, J, s, first_shift, ref.F_FIRST, ref.F_STEP, if_hz)
    ctx.set_option("acq_fft_log2", lg)
    rc1, fft, r1 = _acquire(g, ctx, "gat_acquire_fft", sig, N, B, bstride, ref.PRNS, fs, cfg)
    rc2, direct, r2 = _acquire(g, ctx, "gat_acquire", sig, N, B, bstride, ref.PRNS, fs, cfg)
    assert rc1 == 0 and rc2 == 0
    for pi in range(len(ref.PRNS)):
        check_power_close(fft[pi], direct[pi].astype(np.float64), rtol=2 * RTOL, what=f"{name} prn row {pi}")
    assert np.array_equal(r1["doppler_bin"], r2["doppler_bin"]) and np.array_equal(r1["code_bin"], r2["code_bin"])


def _noisy_constellation(g, fs, N, M, sats, seed):
    """sats: (prn0, doppler, code phase), 45 dB-Hz each on steered antennas in complex white noise (tests/test_acquisition_gpu.py's)."""
    import torch
    sigma = math.sqrt(fs / (2 * 10 ** 4.5))
    if not sats:
        gen = torch.Generator(device="cuda").manual_seed(seed)
        re = torch.randn((M, N), generator=gen, device="cuda") * sigma
        return re, torch.randn((M, N), generator=gen, device="cuda") * sigma
    prm = g.make_params(np.array([p for p, _, _ in sats]), np.array([FC * (1 + d / 1575.42e6) for _, d, _ in sats]),
                        np.array([d for _, d, _ in sats]), np.array([t for _, _, t in sats]), 0.0, shape=(1, len(sats)))
    ctx = g.get_context()
    ctx.set_codes(g.GPSL1().codes)
    re = torch.empty((M, N), dtype=torch.float32, device="cuda")
    im = torch.empty_like(re)
    steer = torch.from_numpy(np.random.default_rng(seed).uniform(0, 1, M).astype(np.float32)).cuda()
    ctx.gen_signal(re, im, g.GAT_LAYOUT_PLANAR, N, M, N, N, 1, len(sats), ctx.params_to_device(prm), fs, amplitude=1.0,
                   steering_cycles=steer, noise_sigma=sigma, seed=seed)
    return re, im


SATS = [(2, 1500.0, 100.265), (7, -2000.0, 511.53), (12, 3000.0, 900.27), (19, -500.0, 33.27), (25, 4500.0, 700.78), (30, -4000.0, 250.66)]


def test_deterministic_and_device_stats_equal_host(g, ctx):
    fs, N, M = 5.0e6, 5000, 4
    re, im = _noisy_constellation(g, fs, N, M, SATS[:3], seed=13)
    prns = list(range(8))
    cfg = ref.config(g, 29, 5000, 1, 0, -7000.0, 500.0)
    rc1, p1, r1 = _acquire(g, ctx, "gat_acquire_fft", (re, im), N, 1, N, prns, fs, cfg)
    rc2, p2, r2 = _acquire(g, ctx, "gat_acquire_fft", (re, im), N, 1, N, prns, fs, cfg)
    assert rc1 == 0 and rc2 == 0
    assert p1.tobytes() == p2.tobytes() and r1.tobytes() == r2.tobytes()
    h = g.acquisition_stats_host(p1, cfg, fs, N)
    for f in ("detected", "doppler_bin", "code_bin", "num_noise_bins"):
        assert np.array_equal(h[f], r1[f]), f
    assert np.array_equal(r1["prn"], prns)
    for f in ("peak_power", "noise_power", "second_power", "peak_to_second", "carrier_doppler_hz", "code_phase_chips"):
        assert np.allclose(h[f], r1[f], rtol=1e-6, atol=0), f
    assert np.allclose(h["cn0_dbhz"], r1["cn0_dbhz"], rtol=0, atol=1e-5)


def test_detects_six_satellites_among_32_at_sample_spacing(g):
    """32 PRNs, six satellites at 45 dB-Hz, 4 antennas, 5 MHz, 1 ms, s = 1 (5000 code bins): exactly those six, each within half a
    Doppler bin and one sample of the truth; their results make six tracking channels.  Noise alone: nothing."""
    fs, N, M = 5.0e6, 5000, 4
    re, im = _noisy_constellation(g, fs, N, M, SATS, seed=11)
    res = g.acquire(g.GPSL1(), (re, im), fs, range(32), num_samples=N, max_doppler=7000.0, doppler_step=500.0, code_step_chips=None, method="fft")
    truth = {p: (d, t) for p, d, t in SATS}
    assert {r.prn for r in res if r.detected == 1} == set(truth), [(r.prn, r.detected, r.peak_to_second) for r in res]
    for r in res:
        if r.prn in truth:
            d, t = truth[r.prn]
            assert abs(r.carrier_doppler - d) <= 250.0, r
            dt = abs((r.code_phase - t + LC / 2) % LC - LC / 2)
            assert dt <= FC / fs, (r, dt)
        else:
            assert r.detected == 0, r
    init = g.tracking_init(res, g.GPSL1())
    assert sorted(init["prns"] - 1) == sorted(truth) and init["params"].size == 6
    re, im = _noisy_constellation(g, fs, N, M, [], seed=12)
    res = g.acquire(g.GPSL1(), (re, im), fs, range(32), num_samples=N, max_doppler=7000.0, doppler_step=500.0, code_step_chips=None, method="fft")
    assert all(r.detected == 0 for r in res), [r.peak_to_second for r in res]


def test_fft_search_seeds_a_tracking_loop(g):
    """tests/test_acquisition_gpu.py's test_coarse_fine_then_track with both searches by FFT: 1 ms at sample spacing, then 10 ms
    (F = 65536) around it, then the closed loop from tracking_init converges under the same criteria.  The criteria are those of a
    noiseless stream (every prompt accumulator above 0.97 N): at 45 dB-Hz one millisecond's accumulator carries noise of
    sqrt(fs / (2 10^4.5 N)) = 0.13 of its own size, so the six-satellite scene above is held to detection, Doppler and code phase,
    and the loop is locked on this stream."""
    system = g.GPSL1()
    N, M, fs, nblk = 4000, 2, 4e6, 1500
    prns, true_dop, true_tau0, true_phi0 = np.array([7]), np.array([-2210.0]), np.array([511.9]), np.array([0.6])
    fcode = FC * (1 + true_dop / 1575.42e6)
    b = np.arange(nblk, dtype=np.float64)[:, None]
    tau = np.mod(true_tau0[None, :] + fcode[None, :] * (N / fs) * b, 1023.0)
    phi = np.mod(true_phi0[None, :] + true_dop[None, :] * (N / fs) * b, 1.0)
    prm_sig = g.make_params(prns - 1, fcode, true_dop, tau, 2 * np.pi * phi, shape=(nblk, 1))
    re, im = g.gen_signal_stream(system, prm_sig, fs, N, M)
    coarse = g.acquire(system, (re, im), fs, prns - 1, num_samples=N, code_step_chips=None, method="fft")[0]
    assert coarse.detected == 1 and abs(coarse.carrier_doppler - true_dop[0]) < 250.0
    assert abs((coarse.code_phase - true_tau0[0] + 511.5) % 1023.0 - 511.5) <= FC / fs
    shift0 = int(math.floor((coarse.code_phase - 2.0) * fs / FC))
    fine = g.acquire(system, (re, im), fs, prns - 1, num_samples=10 * N, dopplers=coarse.carrier_doppler + np.arange(-250.0, 250.5, 10.0),
                     code_step_chips=0.25, first_shift=shift0, num_code_bins=int(math.ceil(4.0 * fs / FC)) + 1, method="fft")[0]
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


def test_beamformed_search(g):
    """acquire(method="fft", weights=...) on a beamformed descriptor gives the grid of method="direct" within 2 RTOL per row."""
    import torch
    fs, N, M = 5.0e6, 5000, 4
    re, im = _noisy_constellation(g, fs, N, M, SATS[:2], seed=21)
    rng = np.random.default_rng(3)
    w = torch.from_numpy((rng.standard_normal((2, M)) + 1j * rng.standard_normal((2, M))).astype(np.complex64))
    kw = dict(num_samples=N, max_doppler=2000.0, doppler_step=500.0, code_step_chips=0.5, keep_power=True, weights=w)
    a = g.acquire(g.GPSL1(), (re, im), fs, [2, 7, 9], method="fft", **kw)
    b = g.acquire(g.GPSL1(), (re, im), fs, [2, 7, 9], method="direct", **kw)
    for ra, rb in zip(a, b):
        check_power_close(ra.power_bins.cpu().numpy(), rb.power_bins.cpu().numpy().astype(np.float64), rtol=2 * RTOL, what=f"beams, prn {ra.prn}")
        assert (ra.detected, ra.doppler_bin, ra.code_bin) == (rb.detected, rb.doppler_bin, rb.code_bin)
    with pytest.raises(ValueError):
        g.acquire(g.GPSL1(), (re, im), fs, [2], num_samples=N, method="fast")
    with pytest.raises(ValueError):
        g.acquire(g.GPSL1(), (re, im), fs, [2], num_samples=N, code_step_chips=None)  # sample spacing is the FFT search's default only


def test_argument_and_state_errors(g):
    import torch
    lib = g.load_library()
    fs, N = 4e6, 4000
    re = torch.zeros((1, N), dtype=torch.float32, device="cuda")
    im = torch.zeros_like(re)
    cfg = ref.config(g, 5, 100, 2)
    h = C.c_void_p()
    assert lib.gat_create(0, None, C.byref(h)) == 0
    try:
        from gpuacceleratedtracking_amd.tracking import _signal_desc
        desc = _signal_desc(re, im, N)
        res = np.zeros(1, dtype=g._lib.ACQ_RESULT_DTYPE)
        pr = np.array([0], dtype=np.int32)
        call = lambda c, P=1, d=desc: lib.gat_acquire_fft(h, C.byref(d), 1, pr.ctypes.data_as(C.POINTER(C.c_int32)), P, fs,  # noqa: E731
                                                          C.byref(c), None, C.c_void_p(res.ctypes.data))
        assert call(cfg) == 3  # before any code table: GAT_ERR_STATE
        codes = np.ascontiguousarray(g.GPSL1().codes)
        assert lib.gat_set_codes(h, codes.ctypes.data_as(C.POINTER(C.c_int8)), codes.shape[1], codes.shape[0]) == 0
        assert call(cfg) == 0
        pr[0] = 99
        assert call(cfg) == 2  # PRN outside the table
        pr[0] = 0
        assert call(ref.config(g, 0, 100, 2)) == 1 and call(ref.config(g, 5, 0, 2)) == 1 and call(cfg, P=0) == 1  # empty grid
        assert call(ref.config(g, 5, 100, 0)) == 1 and call(ref.config(g, 5, 100, 40)) == 2  # the code step
        assert call(ref.config(g, 4096, 20000, 1)) == 2  # grid above 2^26 bins
        bad = ref.config(g, 5, 100, 2, lc=511)
        assert call(bad) == 1  # code_length differs from the table's
        d2 = _signal_desc(re, im, N)
        d2.chan_stride = 8
        assert call(cfg, d=d2) == 1  # chan_stride, as gat_acquire answers it
        d2 = _signal_desc(re, im, N)
        d2.num_samples = 1 << 18
        assert call(cfg, d=d2) == 2  # N too long for the largest transform
        assert lib.gat_set_option(h, b"acq_fft_log2", 11) == 0
        assert call(cfg) == 2  # forced F = 2048 <= N
        assert lib.gat_set_option(h, b"acq_fft_log2", 5) == 0
        assert call(cfg) == 2  # a forced length below 2^10
        assert lib.gat_set_option(h, b"acq_fft_log2", 19) == 2
        assert lib.gat_set_option(h, b"acq_fft_log2", 0) == 0
        assert call(cfg) == 0
        assert lib.gat_acquire_fft(h, None, 1, pr.ctypes.data_as(C.POINTER(C.c_int32)), 1, fs, C.byref(cfg), None, C.c_void_p(res.ctypes.data)) == 1
    finally:
        lib.gat_destroy(h)
