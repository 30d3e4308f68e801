"""From accumulators to a position that survives a bit edge taken a code period off, on the device until the words are decoded:
seven channels' subframes 1 - 3 become synthetic accumulators, go through ``monitor_accumulators`` and ``decode_navigation``, then
``lnav_ephemerides`` and the fix of 16 epochs whose transmit times the reference's light-time iteration made for a receiver on the
ground -- with one channel's transmit times moved by one code period in every epoch, what ``GAT_OBS_EDGE_AMBIGUOUS`` warns of.
``position_fix`` takes the measurement and returns status 0 kilometres away; ``position_fix_raim`` leaves exactly that channel out in
every epoch and the receiver comes back within 1e-3 m (the case carries no noise: the bound of tests/test_position_pipeline_gpu.py)."""
import numpy as np
import pytest

from tests import fix_cases as fc
from tests.test_position_pipeline_gpu import accumulators

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g():
    import gpuacceleratedtracking_amd as g
    g.load_library()
    return g


def test_accumulators_to_a_position_with_a_channel_a_code_period_off(g):
    import torch

    rng = np.random.default_rng(32)
    c = fc.case("short", 30, 7, 16)
    K, negate, prefixes = c.K, [False, True, False, False, True, False, True], [13, 0, 250, 77, 5, 140, 31]
    sent = [g.Ephemeris.from_record(r) for r in c.ephs]
    bits = []
    for k, eph in enumerate(sent):
        payload = g.lnav_ephemeris_payloads(eph)
        frames = [g.lnav_subframe(40800 + i, i + 1, payload=payload[i]) for i in range(3)]
        bits.append(np.concatenate([rng.integers(0, 2, prefixes[k]).astype(np.uint8), *frames, rng.integers(0, 2, 9).astype(np.uint8)]))
    acc_re, acc_im = accumulators(rng, bits, 7, 0.6, negate)
    mon = g.monitor_accumulators(torch.from_numpy(acc_re).cuda(), torch.from_numpy(acc_im).cuda(), block_seconds=1e-3, prompt_index=0,
                                 overlay=g.overlay_for("GPSL1").astype(np.float64))
    nav = g.decode_navigation(mon)
    ephs = g.lnav_ephemerides(nav)
    assert list(nav.frame_offset) == prefixes and all(e.valid == 1 for e in ephs) and ephs == sent

    bad = 3
    assert (c.tx_ms >= 0).all() and K == 7
    tx_ms = c.tx_ms.copy()
    tx_ms[:, bad] = (tx_ms[:, bad] + 1) % 604800000  # the bit edge taken one code period late
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    args = (ephs, t(tx_ms), t(c.tx_frac), t(c.rx_ms), t(c.rx_frac))
    fix = g.position_fix(*args)
    err = np.linalg.norm(fix.xyz - c.truth_xyz, axis=1)
    print("position_fix: status", np.unique(fix.status), "error", err.min(), "..", err.max(), "m")
    assert (fix.status == 0).all() and err.min() > 1e3  # a wrong answer marked good
    raim = g.position_fix_raim(*args, sigma_m=3.0, outputs=("used", "trial"))
    assert raim._host is None
    lb = g.positioning
    err = np.linalg.norm(raim.xyz - c.truth_xyz, axis=1)
    integ = raim.integrity
    print("position_fix_raim: status", np.unique(raim.status), "integrity", np.unique(integ["status"]), "excluded", np.unique(raim.excluded[:, 0]),
          "max error", err.max(), "m; T", integ["stat0"].min(), "->", integ["stat"].max())
    assert (integ["status"] == lb.RAIM_DETECTED | lb.RAIM_EXCLUDED).all() and raim.detected.all()
    assert (integ["num_excluded"] == 1).all() and (raim.excluded[:, 0] == bad).all() and (raim.excluded[:, 1:] == -1).all()
    assert (raim.status == lb.EXCLUDED).all() and (raim.num_used == K - 1).all() and not raim.used[:, bad].any() and raim.used.sum() == c.E * (K - 1)
    assert err.max() <= 1e-3 and np.abs(raim.clock_bias_s - c.truth_bias_s).max() <= 1e-3 / 299792458.0
    assert (np.argmin(np.where(raim.trial >= 0, raim.trial, np.inf), axis=1) == bad).all()
    host = g.position_fix_raim_host(ephs, tx_ms, c.tx_frac, c.rx_ms, c.rx_frac, sigma_m=3.0, outputs=("used", "trial"))
    assert host.fixes.tobytes() == raim.fixes.tobytes() and host.integrity.tobytes() == raim.integrity.tobytes()
    assert host.trial.tobytes() == raim.trial.tobytes() and host.used.tobytes() == raim.used.tobytes()
