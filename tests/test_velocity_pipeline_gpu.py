"""The chain reaches the velocity: history -> monitor -> decoder -> observables -> position fix -> velocity fix with nothing read
back before the end.

The five channels and the site of fix_cases' ``short`` case, as tests/test_observables_pipeline_gpu.py (a) has them, seen by one
receiver that moves at (30, -120, 55) m/s and whose clock, 0.17 ms ahead at the first reception, drifts by 2e-7 s/s; receptions on
the loop's block grid, one every 1000 blocks of 1 ms.  ``obs_cases.history`` makes the parameter histories from the transmit times
of the moving receiver; its carrier frequency is a row a block, and the rows at the epochs' blocks carry the Doppler of the
model-free truth (``vel_ref.range_rate_truth``: two light-time solutions in long double, differenced), which is what
``gat_observables`` hands on as ``doppler_hz``.  ``monitor_accumulators`` -> ``decode_navigation`` -> ``observables`` ->
``position_fix`` -> ``velocity_fix`` run on device tensors only.  The velocity comes back within 1e-6 m/s and the drift within
1e-14 s/s of the truth, the position within the 1e-3 m of the chain without the velocity."""
import numpy as np
import pytest

from tests import fix_cases as fc
from tests import fix_ref as ref
from tests import obs_cases as oc
from tests import vel_ref as vr

pytestmark = pytest.mark.gpu

V_ECEF = np.array([30.0, -120.0, 55.0])
DRIFT = 2e-7


@pytest.fixture(scope="module")
def g():
    import gpuacceleratedtracking_amd as g
    g.load_library()
    return g


class Truth:
    pass


def truth_case(E, stride_ms, rx_ms_first):
    """E receptions stride_ms apart by the receiver's clock.  Between two of them stride (1 - DRIFT) of GPS time pass, over which the
    receiver moves and its clock error grows.  The fraction of the reception is chosen so that every channel's code phase stays
    outside [0.3, 0.7] of a period over the history -- the bit edges the monitor has to find lie well inside no block."""
    base = fc.case("short", 30, 5, 8)
    c = Truth()
    c.ephs, c.K, c.E = base.ephs, 5, E
    xyz0, bias0 = fc.ground(*fc.RECEIVERS[0]) + np.array([12.0, -30.0, 7.0]), 1.7e-4
    elapsed = stride_ms * 1e-3 * np.arange(E) / (1.0 + DRIFT)  # GPS seconds since the first reception
    c.truth_xyz = xyz0[None, :] + elapsed[:, None] * V_ECEF[None, :]
    c.truth_bias_s = bias0 + DRIFT * elapsed
    margin = lambda f: min(np.abs((ref.transmit_times(c.ephs, c.truth_xyz[e], rx_ms_first + e * stride_ms, f, c.truth_bias_s[e])[1] * 1e3) % 1.0 - 0.5).min()  # noqa: E731
                           for e in (0, E - 1))
    frac = max((i * 5e-5 for i in range(20)), key=margin)
    assert margin(frac) > 0.2, margin(frac)
    rows = [ref.transmit_times(c.ephs, c.truth_xyz[e], rx_ms_first + stride_ms * e, frac, c.truth_bias_s[e]) for e in range(E)]
    c.tx_ms = np.stack([r[0] for r in rows]).astype(np.int32)
    c.tx_frac = np.stack([r[1] for r in rows])
    c.rx_ms = np.array([rx_ms_first + stride_ms * e for e in range(E)], np.int32)
    c.rx_frac = np.full(E, frac)
    assert (np.stack([r[2] for r in rows]) > fc.SIN_5_DEG).all()
    # the Doppler of the truth: the differenced light-time solutions' range rate, the drift and the satellites' clock rates
    c.doppler = np.zeros((E, c.K))
    for e in range(E):
        t_rx = np.longdouble(int(c.rx_ms[e])) / np.longdouble(1000) + np.longdouble(frac) - np.longdouble(c.truth_bias_s[e])
        rate = vr.range_rate_truth(c.ephs, c.truth_xyz[e], V_ECEF, t_rx)
        c.doppler[e] = vr.doppler(c.ephs, c.tx_ms[e], c.tx_frac[e], c.truth_xyz[e], V_ECEF, DRIFT, range_rate=rate)
    return c


def test_history_to_velocity(g):
    import torch

    rng = np.random.default_rng(78)
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
    blocks = first + stride * np.arange(E)
    carrier = np.tile(rng.uniform(-4000.0, 4000.0, K), (B + 1, 1))
    carrier[blocks] = c.doppler  # the loop's carrier frequency at an epoch's block is that epoch's Doppler (IF 0)
    h = oc.history(B, blocks, c.tx_ms, tau, carrier_hz=carrier, carrier_phase0=rng.uniform(0, 1, K))
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
    vel = g.velocity_fix(sent, obs.tx_ms, obs.tx_frac, obs.doppler_hz, fix)
    assert all(r._host is None for r in (mon, nav, obs, fix, vel)), "something was read back before the velocity"

    assert (obs.status == 0).all() and g.lnav_ephemerides(nav) == sent
    assert np.array_equal(obs.host("tx_ms"), c.tx_ms) and obs.host("tx_frac").tobytes() == np.ascontiguousarray(c.tx_frac).tobytes()
    assert obs.host("doppler_hz").tobytes() == c.doppler.tobytes()
    err = np.linalg.norm(fix.xyz - c.truth_xyz, axis=1)
    err_v = np.abs(vel.v_ecef - V_ECEF[None, :]).max()
    err_d = np.abs(vel.clock_drift - DRIFT).max()
    print(f"fix status {np.unique(fix.status)}, position {err.max():.3e} m (bound 1e-3); velocity status {np.unique(vel.status)}, velocity {err_v:.3e} m/s "
          f"(bound 1e-6), drift {err_d:.3e} s/s (bound 1e-14), rms residual {vel.rms_residual_mps.max():.3e} m/s, speed {vel.speed[0]:.6f} m/s")
    assert (fix.status == 0).all() and (fix.num_used == 5).all() and err.max() <= 1e-3
    assert (vel.status == 0).all() and (vel.num_used == 5).all() and err_v <= 1e-6 and err_d <= 1e-14
    # the twin on the observables read back: the same bytes
    host = g.velocity_fix_host(sent, obs.host("tx_ms"), obs.host("tx_frac"), obs.host("doppler_hz"), fix)
    assert host.velocities.tobytes() == vel.velocities.tobytes() and host.resid.tobytes() == vel.resid.tobytes()
