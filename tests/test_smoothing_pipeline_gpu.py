"""The chain through the carrier smoothing: history -> monitor -> decoder -> observables -> smooth_observables -> position fix with
nothing read back before the end.

The chain of tests/test_velocity_pipeline_gpu.py (five channels, a receiver that moves and whose clock drifts, receptions every 1000
blocks of 1 ms), with a carrier history that telescopes to the range: between two epochs the code of ``obs_cases.history`` advances by
the same amount every block, so the pseudorange P = rx - tx is linear there, and the carrier frequency of every block b of the span is
the Doppler of the range change over it, -carrier_hz (P_next - P_this) / (blocks * T).  The phase the observables hand on (whole
cycles plus fraction) then follows -carrier_hz P up to the rounding of a thousand additions, and code minus carrier does not grow:
status is MEASURED everywhere with GAP at epoch 0 alone.  This is the sign check of delta: with the carrier term subtracted instead
of added, delta would be twice the range change of an epoch -- up to 5e-6 s (1600 m) against a gate of 15 m -- and every epoch behind
the first would carry CMC.  The smoothed fix stays within the chain's 1e-3 m of the truth, and the device's bytes are the twin's on
the observables read back."""
import numpy as np
import pytest

from tests import obs_cases as oc
from tests.test_velocity_pipeline_gpu import truth_case

pytestmark = pytest.mark.gpu

FL = 1575.42e6
MEASURED, GAP = 1, 2


@pytest.fixture(scope="module")
def g():
    import gpuacceleratedtracking_amd as g
    g.load_library()
    return g


def test_history_to_smoothed_fix(g):
    import torch

    rng = np.random.default_rng(79)
    E, first, stride = 8, 200, 1000
    rx_ms_first = 244800000 + 600000 + 4321
    c = truth_case(E, stride, rx_ms_first)
    rx_frac0 = float(c.rx_frac[0])
    K = c.K
    tau = c.tx_frac * oc.FC
    c.tx_frac = tau / oc.FC
    assert (c.tx_ms >= 0).all() and (tau < oc.LC).all()
    frame_ms = ((c.tx_ms[0].astype(np.int64) - first + 30) // 6000 + 1) * 6000
    B = int((frame_ms - (c.tx_ms[0] - first)).max()) + 18000 + 60
    blocks = first + stride * np.arange(E)
    assert blocks[-1] < B
    # the carrier that telescopes to the range
    T = oc.N / oc.FS
    P = (c.rx_ms[:, None].astype(np.int64) - c.tx_ms).astype(np.longdouble) / 1000 + (c.rx_frac[:, None].astype(np.longdouble) - c.tx_frac)
    carrier = np.tile(rng.uniform(-4000.0, 4000.0, K), (B + 1, 1))
    for e in range(E - 1):
        carrier[blocks[e]:blocks[e + 1]] = (-np.longdouble(FL) * (P[e + 1] - P[e]) / (stride * np.longdouble(T))).astype(np.float64)[None, :]
    assert np.abs(carrier[blocks[0]:blocks[-1]]).max() < 6000.0  # a satellite's Doppler and the receiver's
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
    assert obs.if_hz == 0.0 and obs.epoch_seconds == stride * T
    sm = g.smooth_observables(obs, window=4)
    fix = g.position_fix(sent, obs.tx_ms, sm.tx_frac_dev, obs.rx_ms, obs.rx_frac)
    assert all(r._host is None for r in (mon, nav, obs, sm, fix)), "something was read back before the fix"

    assert (obs.status == 0).all()
    assert np.array_equal(obs.host("tx_ms"), c.tx_ms) and obs.host("tx_frac").tobytes() == np.ascontiguousarray(c.tx_frac).tobytes()
    want = np.full((E, K), MEASURED, np.uint8)
    want[0] |= GAP
    moved = np.abs(sm.tx_frac_out - obs.host("tx_frac")).max() * 299792458.0
    print(f"status {np.unique(sm.status)}, count {sm.count[:, 0]}, |cmc| {np.abs(sm.cmc_m).max():.3e} m, transmit times moved by {moved:.3e} m")
    assert np.array_equal(sm.status, want), sm.status
    assert np.array_equal(sm.count, np.minimum(np.arange(E) + 1, 4)[:, None].repeat(K, 1)) and (sm.measured == E).all() and (sm.arcs == 1).all()
    assert np.abs(sm.cmc_m).max() < 1e-5  # the phase's rounding is far below one unit u (1.07 um) an epoch: at most E units
    host = g.smooth_observables_host(obs, window=4)
    for name in ("tx_frac_out", "count", "cmc_s", "status", "channels"):
        assert getattr(host, name).tobytes() == getattr(sm, name).tobytes(), name
    err = np.linalg.norm(fix.xyz - c.truth_xyz, axis=1)
    print(f"fix status {np.unique(fix.status)}, position {err.max():.3e} m (bound 1e-3)")
    assert (fix.status == 0).all() and (fix.num_used == 5).all() and err.max() <= 1e-3
