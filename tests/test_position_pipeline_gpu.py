"""From accumulators to a position, on the device until the words are decoded: five channels' subframes 1 - 3 (``lnav_subframe``
over ``lnav_ephemeris_payloads``) become synthetic accumulators [B, K, 1, 1] (twenty blocks a bit, noise, one channel negated), go
through ``monitor_accumulators`` and ``decode_navigation`` -- which takes the monitor's device tensors as they are: nothing is read
back before the decoder ran --, then ``lnav_ephemerides`` (cold, on the host) and ``position_fix`` of 64 epochs whose transmit times
the reference's light-time iteration made for a receiver on the ground: the receiver comes back within 1e-3 m."""
import numpy as np
import pytest

from tests import fix_cases as fc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g():
    import gpuacceleratedtracking_amd as g
    g.load_library()
    return g


def accumulators(rng, bits, lead, sigma, negate):
    """float32 [B, K, 1, 1] planes: `lead` blocks of a 0 bit, then every bit of the channel over twenty blocks, then noise; unit
    amplitude at a phase of 0.2 rad, negated where the Costas loop locked to the negative"""
    K = len(bits)
    B = lead + 20 * max(len(b) for b in bits) + 5
    p = np.zeros((B, K), np.complex128)
    for k, b in enumerate(bits):
        series = np.concatenate([np.ones(lead), np.repeat(1.0 - 2.0 * np.asarray(b, np.float64), 20)])
        p[:len(series), k] = series * np.exp(0.2j) * (-1.0 if negate[k] else 1.0)
    p += sigma * (rng.standard_normal(p.shape) + 1j * rng.standard_normal(p.shape))
    return np.ascontiguousarray(p.real[:, :, None, None], np.float32), np.ascontiguousarray(p.imag[:, :, None, None], np.float32)


def test_accumulators_to_position(g):
    import torch

    rng = np.random.default_rng(31)
    c = fc.case("short", 30, 5, 64)
    K, negate, prefixes = c.K, [False, True, False, False, True], [13, 0, 250, 77, 5]
    sent = [g.Ephemeris.from_record(r) for r in c.ephs]
    bits = []
    for k, eph in enumerate(sent):
        payload = g.lnav_ephemeris_payloads(eph)
        frames = [g.lnav_subframe(40800 + i, i + 1, payload=payload[i]) for i in range(3)]
        bits.append(np.concatenate([rng.integers(0, 2, prefixes[k]).astype(np.uint8), *frames, rng.integers(0, 2, 9).astype(np.uint8)]))
    lead = 7
    acc_re, acc_im = accumulators(rng, bits, lead, 0.6, negate)
    mon = g.monitor_accumulators(torch.from_numpy(acc_re).cuda(), torch.from_numpy(acc_im).cuda(), block_seconds=1e-3, prompt_index=0,
                                 overlay=g.overlay_for("GPSL1").astype(np.float64))
    nav = g.decode_navigation(mon)
    assert mon._host is None, "the monitor was read back before the decoder ran"
    ephs = g.lnav_ephemerides(nav)
    print("frame offset", nav.frame_offset, "inverted", nav.inverted, "ids", nav.subframe_id[:, :3].tolist())
    assert list(nav.frame_offset) == prefixes and list(nav.inverted) == [int(v) for v in negate] and nav.ok[:, :3].all()
    assert all(e.valid == 1 for e in ephs) and ephs == sent
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    fix = g.position_fix(ephs, t(c.tx_ms), t(c.tx_frac), t(c.rx_ms), t(c.rx_frac))
    assert fix._host is None
    err = np.linalg.norm(fix.xyz - c.truth_xyz, axis=1)
    print("status", np.unique(fix.status), "max error", err.max(), "m; pdop", fix.pdop.max(), "iterations", fix.iterations.max())
    assert (fix.status == 0).all() and (fix.num_used == 5).all() and err.max() <= 1e-3
    assert np.abs(fix.clock_bias_s - c.truth_bias_s).max() <= 1e-3 / 299792458.0
    host = g.position_fix_host(ephs, c.tx_ms, c.tx_frac, c.rx_ms, c.rx_frac)
    assert host.fixes.tobytes() == fix.fixes.tobytes() and host.sat.tobytes() == fix.sat.tobytes()
