"""End-to-end tests of the sample conditioner (gpuacceleratedtracking_amd/frontend.py): what blanking and requantising are for.

  * a pulsed interferer hides two satellites from the search on the raw stream; on the blanked int8 stream the search finds
    exactly those two (the verdicts were forecast on the CPU with the FP64 acquisition oracle: scripts/frontend_pulse_forecast.py);
  * requantising a clean stream to int8 moves no correlator output by more than the rounding errors' six sigma;
  * the conditioned int8 descriptor is a signal again: acquire, spatial_covariance, TrackingLoop.run and a resident correlator
    take it as it is (the loop in every block), each within the project's 1e-5 of the FP64 oracle on the same int8 values."""
import numpy as np
import pytest

import oracle
from tests import array_ref
from tests import cond_ref as ref
from tests.cond_ref import I8, PULSED, pulsed_params, pulses
from tests.helpers import acq_power_oracle, acq_sample_bins, check_close, check_power_close, make_case, oracle_result

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module")
def g():
    import gpuacceleratedtracking_amd as g
    g.load_library()
    return g


def test_blanking_uncovers_the_satellites_under_pulsed_interference(g):
    """Two satellites of 48 dB-Hz (amplitude 1 in noise of sigma = 4 per component), 4 blocks of 1 ms searched non-coherently for
    4 PRNs over +-2500 Hz, and bursts 40 dB over the noise on 10 % of the samples.  Forecast on the CPU beforehand
    (scripts/frontend_pulse_forecast.py: the FP64 oracle's generator, numpy noise of the same sigma, these pulses, the numpy
    restatement of statistics, AGC and conditioning, helpers.acq_power_oracle over the whole 11 x 2048 grid and
    gat_acq_stats_host on it), peak / second of PRN columns 6, 2, 18, 27:
        raw stream      1.002  1.039  1.128  1.015   -> nothing detected (the present PRNs' peaks sit in wrong bins)
        blanked int8   12.657  1.126  9.816  1.010   -> exactly the two present ones, at 1060.9 Hz / 300.214 chips and
                                                        -1421.8 Hz / 811.651 chips
    with 9.7 % of the samples blanked and none clipped.  The detection threshold is 2.0.  The pulses inflate the first sigma 30-fold:
    the blanking threshold of 4 sigma-hat is 124.6, 77.5, 4.14 and 4.14 true sigma in rounds 0 to 3 of {statistics under the last
    threshold, AGC}, so iterations = 4 has a round to spare.  The device draws another noise sequence than the forecast's: the
    verdicts are held, not the ratios; the blanked count is held exactly, against the numpy restatement on the device's samples."""
    import torch
    s = PULSED
    system = g.GPSL1()
    N, B, fs = s["N"], s["B"], s["fs"]
    prn0, fcode, dop, tau, phi = pulsed_params()
    prm = g.make_params(prn0, fcode, dop, tau, 2 * np.pi * phi, shape=(B, 2))
    re, im = g.gen_signal_stream(system, prm, fs, N, 1, noise_sigma=s["sigma"], seed=s["noise_seed"])
    p = pulses()
    re = (re + torch.from_numpy(p.real.astype(np.float32)).to(re.device)[None, :]).contiguous()
    im = (im + torch.from_numpy(p.imag.astype(np.float32)).to(im.device)[None, :]).contiguous()

    raw = g.acquire(system, (re, im), fs, s["cols"], num_samples=N, num_blocks=B, max_doppler=s["max_doppler"])
    print("raw:", [(r.prn, r.detected, round(r.peak_to_second, 3)) for r in raw])
    assert [r.detected for r in raw] == [0, 0, 0, 0]

    sig8, desc, counts, params = g.requantize((re, im), N, B, blank_factor=s["blank_factor"], iterations=s["iterations"])
    assert sig8.dtype == torch.int8 and desc.layout == I8 and desc.block_stride == N
    res = g.acquire(system, desc, fs, s["cols"], num_blocks=B, max_doppler=s["max_doppler"])
    print("blanked int8:", [(r.prn, r.detected, round(r.peak_to_second, 3), r.carrier_doppler, r.code_phase) for r in res])
    assert [r.prn for r in res] == s["cols"]
    assert [r.detected for r in res] == [1, 0, 1, 0]
    for r, f, t in ((res[0], s["dop"][0], s["tau0"][0]), (res[2], s["dop"][1], s["tau0"][1])):
        assert abs(r.carrier_doppler - f) <= 500.0
        assert abs(((r.code_phase - t + 511.5) % 1023.0) - 511.5) <= 0.5

    # the blanked count is the reference's, exactly (and so is every int8 code): the numpy restatement on the same samples and records
    vr, vi = (t.cpu().numpy().reshape(1, B, N).transpose(1, 0, 2) for t in (re, im))
    rec = params.cpu().numpy().copy().view(g.frontend.COND_PARAMS_DTYPE).reshape(1)
    er, ei, ecnt = ref.condition(vr, vi, rec, I8)
    got = counts.cpu().numpy()
    print("blanked", int(got[0, 0]), "of", B * N, "clipped", int(got[0, 1]), "threshold / sigma", float(rec["threshold"][0]) / s["sigma"])
    assert np.array_equal(got.astype(np.uint64), ecnt)
    assert 0.08 * B * N <= got[0, 0] <= 0.12 * B * N
    o = sig8.cpu().numpy().reshape(1, B, N, 2)
    assert np.array_equal(o[..., 0].transpose(1, 0, 2), er) and np.array_equal(o[..., 1].transpose(1, 0, 2), ei)


# ---- a clean stream and its int8 image ------------------------------------------------------------------------------------------
CLEAN = dict(seed=77, N=2048, M=2, L=3, K=2, B=4, fs=2.048e6, noise=2.0)


@pytest.fixture(scope="module")
def clean(g):
    """the float case, its requantize(target_rms = 16) image on the device, and the same case with the int8 values as samples"""
    import torch
    c = CLEAN
    case = make_case(c["seed"], N=c["N"], M=c["M"], L=c["L"], K=c["K"], B=c["B"], fs=c["fs"], noise=c["noise"])
    ctx = g.get_context()
    re, im = torch.from_numpy(case["re"]).to(ctx.device), torch.from_numpy(case["im"]).to(ctx.device)
    sig8, desc, counts, params = g.requantize((re, im), c["N"], c["B"], target_rms=16.0)
    ctx.sync()
    o = sig8.cpu().numpy()  # [M, B * N, 2]
    case8 = dict(case, re=np.ascontiguousarray(o[..., 0]).astype(np.float32), im=np.ascontiguousarray(o[..., 1]).astype(np.float32))
    p = case["prm"]
    lib_prm = g.make_params(p["prn0"], p["code_freq_hz"], p["carrier_freq_hz"], p["code_phase_chips"], p["carrier_phase_cycles"])
    return dict(case=case, case8=case8, re=re, im=im, sig8=sig8, desc=desc, counts=counts.cpu().numpy(), params=params.cpu().numpy(), prm=lib_prm)


def correlate(g, desc, case, prm):
    import torch
    ctx = g.get_context()
    ctx.set_codes(case["codes"])
    B, K, L, M = case["B"], case["K"], case["L"], case["M"]
    o_re = torch.empty((B, K, L, M), dtype=torch.float32, device=ctx.device)
    o_im = torch.empty_like(o_re)
    ctx.downconvert_and_correlate(desc, ctx.params_to_device(prm), B, K, case["shifts"], case["fs"], o_re, o_im)
    ctx.sync()
    return o_re.cpu().numpy().astype(np.float64) + 1j * o_im.cpu().numpy().astype(np.float64)


def test_requantisation_costs_nothing_measurable(g, clean):
    """|R_q / scale - R_f| <= 6 sqrt(N / 6) / scale for every accumulator: R_q - scale R_f is the sum of N rounding errors times
    unit phasors, each component uniform in +-1/2 (variance 1/12), so its squared magnitude has mean N / 6; six of those standard
    deviations.  Precondition: nothing clipped, for this seed, by the device's count and by the numpy restatement."""
    c, case = CLEAN, clean["case"]
    N, M, B = c["N"], c["M"], c["B"]
    assert clean["counts"].sum() == 0
    rec = clean["params"].copy().view(g.frontend.COND_PARAMS_DTYPE).reshape(M)
    vr, vi = (case[k].reshape(M, B, N).transpose(1, 0, 2) for k in ("re", "im"))
    _, _, ecnt = ref.condition(vr, vi, rec, I8)
    assert ecnt.sum() == 0  # the reference's precondition: clipped == 0 (and nothing blanked)
    fdesc = g._lib.SignalDesc(clean["re"].data_ptr(), clean["im"].data_ptr(), 0, M, N, B * N, N, 0)
    r_f = correlate(g, fdesc, case, clean["prm"])
    r_q = correlate(g, clean["desc"], case, clean["prm"])
    scale = rec["scale"].astype(np.float64)  # per antenna: the last axis of [B, K, L, M]
    err = np.abs(r_q / scale - r_f)
    bound = 6.0 * np.sqrt(N / 6.0) / scale
    print("worst |R_q / scale - R_f| over its bound:", float((err / bound).max()), "scale", scale, "|R_f| max", float(np.abs(r_f).max()))
    assert (err <= bound).all()
    assert np.abs(r_f).max() > 100 * bound.max()  # the bound is small next to the signal: the check says something


def test_the_conditioned_descriptor_is_a_signal_again(g, clean):
    """the int8 stream, unchanged, into acquire, spatial_covariance, TrackingLoop.run and a resident correlator: each against the
    FP64 oracle on the same int8 values at 1e-5"""
    import torch
    c, case8, desc, sig8 = CLEAN, clean["case8"], clean["desc"], clean["sig8"]
    N, M, B, K, fs = c["N"], c["M"], c["B"], c["K"], c["fs"]
    ctx = g.get_context()
    system = g.GPSL1()
    p0 = case8["prm"][0]

    # the correlator itself
    check_close(correlate(g, desc, case8, clean["prm"]), oracle_result(case8), what="correlator on the int8 image")

    # acquire: the whole grid kept, compared on sampled bins
    col = int(p0["prn0"][0])
    res = g.acquire(system, desc, fs, [col], num_blocks=B, max_doppler=5000.0, keep_power=True)[0]
    D, J = res.power_bins.shape
    rng = np.random.default_rng(3)
    rows, cols = acq_sample_bins(rng, D, J, rows=[res.doppler_bin], cols=[res.code_bin])
    want = acq_power_oracle(case8["re"], case8["im"], case8["codes"], col, case8["fc"], case8["lc"], fs, 0.0, float(res.dopplers[0]),
                            float(res.dopplers[1] - res.dopplers[0]), rows, 0, 1, cols, N, B, N)
    check_power_close(res.power_bins.cpu().numpy()[np.ix_(rows, cols)], want, what="acquire on the int8 image")

    # spatial covariance
    R = g.spatial_covariance(sig8, N, B).cpu().numpy()
    x = case8["re"].astype(np.float64) + 1j * case8["im"].astype(np.float64)
    check_close(R[:, None], array_ref.covariance(x, N, B, B)[:, None], what="covariance of the int8 image")

    # the tracking loop, every block: block b against the FP64 oracle on the records the loop's host twin (gat_tracking_update_host)
    # makes of the device's own accumulators of the blocks before it; block 0 runs on the start values
    import ctypes as C
    shifts = case8["shifts"]
    dop0 = p0["carrier_freq_hz"].astype(np.float64)
    loop = g.TrackingLoop(system, p0["prn0"] + 1, N, M, fs, shifts, init_carrier_doppler=dop0, init_code_phase=p0["code_phase_chips"],
                          init_carrier_phase=p0["carrier_phase_cycles"])
    cur = loop.params().reshape(K).copy()
    nxt = cur.copy()
    st = loop.state().copy()
    acc_re, acc_im = loop.run(sig8, None, B)
    loop.ctx.sync()
    a_re, a_im = acc_re.cpu().numpy(), acc_im.cpu().numpy()  # [B, K, L, M]
    got = a_re.astype(np.float64) + 1j * a_im.astype(np.float64)
    vp = C.c_void_p
    for b in range(B):
        oprm = oracle.make_params(cur["prn"], cur["code_freq_hz"], cur["carrier_freq_hz"], cur["code_phase_chips"], cur["carrier_phase_cycles"])
        want = oracle.correlate_f64(case8["re"][:, b * N:], case8["im"][:, b * N:], case8["codes"], oprm.reshape(1, K), fs, shifts, N=N)
        check_close(got[b:b + 1], want, what=f"TrackingLoop.run on the int8 image, block {b}")
        r, i = np.ascontiguousarray(a_re[b]), np.ascontiguousarray(a_im[b])
        assert loop.ctx.lib.gat_tracking_update_host(vp(r.ctypes.data), vp(i.ctypes.data), K, M, C.byref(loop.config), vp(st.ctypes.data),
                                                     vp(cur.ctypes.data), vp(nxt.ctypes.data)) == 0
        cur, nxt = nxt, cur
    end = loop.params().reshape(K)
    for f in ("code_freq_hz", "carrier_freq_hz", "code_phase_chips", "carrier_phase_cycles"):
        assert np.allclose(end[f], cur[f], rtol=1e-12, atol=1e-9), f  # (the tolerances of test_update_matches_oracle_restatement)

    # a resident correlator opened on the conditioned descriptor
    ctx.set_codes(case8["codes"])
    torch.cuda.synchronize()
    ref8 = oracle_result(case8)
    with ctx.open_resident(desc, K, shifts, fs, idle_us=200000) as resident:
        for b in (1, 0):
            r_re, r_im = resident.correlate(clean["prm"][b], block_offset=b * N)
            check_close((r_re + 1j * r_im)[None], ref8[b:b + 1], what=f"resident correlator on the int8 image, block {b}")
