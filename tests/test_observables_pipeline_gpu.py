"""The chain closes: history -> monitor -> decoder -> observables -> position fix with nothing read back before the fix, and a
real loop's history gives the code phase it tracked.

(a) The five channels and the site of fix_cases' ``short`` case, seen by one receiver at rest with a constant clock error, with
receptions on the loop's block grid (one every 1000 blocks of 1 ms; the transmit fractions are put on the grid of code phases, tau =
frac * fc and frac := tau / fc, a change below 2e-19 s).  ``obs_cases.history`` makes the parameter histories from the case's transmit times, ``obs_cases.prompt_signs`` the
accumulators whose bit edges sit at the histories' code-period boundaries (subframes 1 - 3 of every channel's ephemeris with the
TOW of the transmit time, noise, two channels negated).  ``monitor_accumulators`` -> ``decode_navigation`` -> ``observables`` ->
``position_fix`` run on device tensors only; the receiver comes back within 1e-3 m and 1e-3 / c s, the bounds of
test_position_pipeline_gpu.py, and tx_ms / tx_frac are the case's own.

(b) Two PRNs generated 150.4 chips apart, one antenna, 2.046 MHz, 200 blocks through ``run_history``; the sync records are written
by hand with one frame block and one TOW for both.  At record B the fraction is the loop's code phase over fc bit for bit, and
the difference of the two transmit times is the generated delay difference within 0.02 chips, the bound
test_tracking_loop_gpu.py holds this loop's code phase to."""
import numpy as np
import pytest

from tests import fix_cases as fc
from tests import obs_cases as oc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g():
    import gpuacceleratedtracking_amd as g
    g.load_library()
    return g


class Truth:
    pass


def truth_case(E, stride_ms, rx_ms_first):
    """The five satellites and the site of fix_cases' ``short`` case seen by one receiver at rest whose clock is 0.17 ms ahead, at E
    receptions stride_ms apart: a loop's block grid.  The fraction of the reception is chosen so that every channel's code phase
    stays outside [0.3, 0.7] of a period over the history -- the bit edges the monitor has to find lie well inside no block."""
    from tests import fix_ref as ref

    base = fc.case("short", 30, 5, 8)
    c = Truth()
    c.ephs, c.K, c.E = base.ephs, 5, E
    xyz, bias = fc.ground(*fc.RECEIVERS[0]) + np.array([12.0, -30.0, 7.0]), 1.7e-4
    margin = lambda f: np.abs((ref.transmit_times(c.ephs, xyz, rx_ms_first + 2 * stride_ms, f, bias)[1] * 1e3) % 1.0 - 0.5).min()  # noqa: E731
    frac = max((i * 5e-5 for i in range(20)), key=margin)
    assert margin(frac) > 0.2, margin(frac)
    rows = [ref.transmit_times(c.ephs, xyz, rx_ms_first + stride_ms * e, frac, bias) for e in range(E)]
    c.tx_ms = np.stack([r[0] for r in rows]).astype(np.int32)
    c.tx_frac = np.stack([r[1] for r in rows])
    c.rx_ms = np.array([rx_ms_first + stride_ms * e for e in range(E)], np.int32)
    c.rx_frac = np.full(E, frac)
    c.truth_xyz, c.truth_bias_s = np.tile(xyz, (E, 1)), np.full(E, bias)
    assert (np.stack([r[2] for r in rows]) > fc.SIN_5_DEG).all()
    return c


def test_history_to_position(g):
    import torch

    rng = np.random.default_rng(77)
    E, first, stride = 8, 200, 1000
    rx_ms_first = 244800000 + 600000 + 4321
    c = truth_case(E, stride, rx_ms_first)
    rx_frac0 = float(c.rx_frac[0])
    K = c.K
    assert (c.tx_ms >= 0).all()
    tau = c.tx_frac * oc.FC
    c.tx_frac = tau / oc.FC
    assert (tau < oc.LC).all()
    # every channel's frame 0: the first whole 6 s after the history's start; three subframes follow
    frame_ms = ((c.tx_ms[0].astype(np.int64) - first + 30) // 6000 + 1) * 6000
    B = int((frame_ms - (c.tx_ms[0] - first)).max()) + 18000 + 60
    h = oc.history(B, first + stride * np.arange(E), c.tx_ms, tau, carrier_hz=rng.uniform(-4000.0, 4000.0, K), carrier_phase0=rng.uniform(0, 1, K))
    sent = [g.Ephemeris.from_record(r) for r in c.ephs]
    bits = []
    for k, eph in enumerate(sent):
        payload = g.lnav_ephemeris_payloads(eph)
        bits.append(np.concatenate([g.lnav_subframe(int(frame_ms[k]) // 6000 + 1 + i, i + 1, payload=payload[i]) for i in range(3)]))
    negate = np.array([1.0, -1.0, 1.0, 1.0, -1.0])
    p = oc.prompt_signs(h, frame_ms, bits, rng) * np.exp(0.2j) * negate[None, :]
    p = p + 0.6 * (rng.standard_normal(p.shape) + 1j * rng.standard_normal(p.shape))
    acc_re = torch.from_numpy(np.ascontiguousarray(p.real[:, :, None, None], np.float32)).cuda()
    acc_im = torch.from_numpy(np.ascontiguousarray(p.imag[:, :, None, None], np.float32)).cuda()
    hist = torch.from_numpy(h.records.view(np.uint8).reshape(B + 1, K, 40).copy()).cuda()

    mon = g.monitor_accumulators(acc_re, acc_im, block_seconds=1e-3, prompt_index=0, overlay=g.overlay_for("GPSL1").astype(np.float64))
    nav = g.decode_navigation(mon)
    rx0_ms = (rx_ms_first - first) % 604800000
    obs = g.observables(hist, mon, nav, epoch_first=first, epoch_stride=stride, num_epochs=E, rx=(rx0_ms, rx_frac0), **oc.base_config())
    fix = g.position_fix(sent, obs.tx_ms, obs.tx_frac, obs.rx_ms, obs.rx_frac)
    assert mon._host is None and nav._host is None and obs._host is None and fix._host is None, "something was read back before the fix"

    print("status", obs.status, "frame block", obs.frame_block, "edge fraction", np.round(obs.edge_fraction, 3), "frame0_ms", obs.frame0_ms)
    assert (obs.status == 0).all()
    assert list(nav.inverted) == [0, 1, 0, 0, 1] and nav.ok[:, :3].all() and g.lnav_ephemerides(nav) == sent
    assert np.array_equal(obs.frame0_ms, frame_ms % 604800000)
    assert np.array_equal(obs.host("tx_ms"), c.tx_ms) and obs.host("tx_frac").tobytes() == np.ascontiguousarray(c.tx_frac).tobytes()
    assert np.array_equal(obs.host("rx_ms"), c.rx_ms) and np.abs(obs.host("rx_frac") - c.rx_frac).max() == 0.0
    err = np.linalg.norm(fix.xyz - c.truth_xyz, axis=1)
    print("fix status", np.unique(fix.status), "max error", err.max(), "m; clock", np.abs(fix.clock_bias_s - c.truth_bias_s).max(), "s")
    assert (fix.status == 0).all() and (fix.num_used == 5).all() and err.max() <= 1e-3
    assert np.abs(fix.clock_bias_s - c.truth_bias_s).max() <= 1e-3 / 299792458.0


def test_real_loop_history(g):
    import torch
    from gpuacceleratedtracking_amd import _lib

    system = g.GPSL1()
    N, M, fs, fcn, B = oc.N, 1, oc.FS, oc.FC, 200
    prns, dop = np.array([6, 21]), np.array([1000.0, -2000.0])
    tau0, phi0 = np.array([100.3, 250.7]), np.array([0.15, 0.7])
    fcode = fcn * (1 + dop / 1575.42e6)
    T = N / fs
    b = np.arange(B, dtype=np.float64)[:, None]
    prm = g.make_params(prns - 1, fcode, dop, np.mod(tau0[None, :] + fcode[None, :] * T * b, 1023.0), 2 * np.pi * np.mod(phi0[None, :] + dop[None, :] * T * b, 1.0),
                        shape=(B, 2))
    re, im = g.gen_signal_stream(system, prm, fs, N, M)
    shifts = g.get_correlator_sample_shifts(system, g.EarlyPromptLateCorrelator(M, 3), fs, 0.5)
    loop = g.TrackingLoop(system, prns, N, M, fs, shifts, init_carrier_doppler=dop, init_code_phase=tau0, init_carrier_phase=phi0)
    acc_re, acc_im, history = loop.run_history(re, im, B)
    # by hand: bit edges every 20 blocks from block 0, frame 0 at block 40 for both, one good frame whose TOW count is 40801
    gblk = 40
    mon, nav = np.zeros(2, _lib.MONITOR_CHANNEL_DTYPE), np.zeros(2, _lib.NAV_CHANNEL_DTYPE)
    frames = np.zeros((2, 1), _lib.NAV_FRAME_DTYPE)
    mon["num_symbols"], nav["frame_offset"], nav["num_frames"], nav["score"] = B // 20, gblk // 20, 1, 1
    frames["status"], frames["tow"], frames["id"] = 0x7FF, 40801, 1
    t = lambda a: torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda()  # noqa: E731
    obs = loop.observables(history, t(mon), (t(nav), t(frames)), symbol_blocks=20, epoch_first=B, num_epochs=1)
    assert obs._host is None
    p = loop.params().reshape(-1)
    tx_ms, tx_frac = obs.host("tx_ms")[0].astype(np.int64), obs.host("tx_frac")[0]
    assert (obs.status == 0).all() and (obs.frame_block == gblk).all() and (obs.frame0_ms == 244800000).all()
    assert tx_frac.tobytes() == (p["code_phase_chips"] / fcn).tobytes()
    assert obs.host("code_rate_hz")[0].tobytes() == p["code_freq_hz"].tobytes() and obs.host("carrier_frac")[0].tobytes() == p["carrier_phase_cycles"].tobytes()
    assert (tx_ms == 244800000 + (B - gblk)).all()  # one code period a block from the frame block on
    got = ((tx_ms[1] - tx_ms[0]) * 1e-3 + (tx_frac[1] - tx_frac[0])) * fcn
    want = (tau0[1] - tau0[0]) + (fcode[1] - fcode[0]) * T * B
    print(f"transmit-time difference {got:.5f} chips, generated {want:.5f} chips, error {got - want:+.5f} chips; carrier cycles",
          obs.host("carrier_cycles")[0], "doppler", obs.host("doppler_hz")[0])
    assert abs(got - want) < 0.02
    # the carrier: whole cycles plus the fraction advance by the Doppler over the history
    cyc = obs.host("carrier_cycles")[0] + obs.host("carrier_frac")[0] - phi0
    assert np.abs(cyc - dop * T * B).max() < 0.05
    host = g.observables_host(history.cpu().numpy(), mon, (nav, frames), loop=loop, symbol_blocks=20, epoch_first=B, num_epochs=1)
    assert host.host("tx_ms").tobytes() == obs.host("tx_ms").tobytes() and host.host("tx_frac").tobytes() == tx_frac.tobytes()
