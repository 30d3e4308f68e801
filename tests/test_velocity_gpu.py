"""gat_velocity_fix on the device against its host twin, byte for byte on the records, sat_vel and resid, at the shapes where a kernel
that gives a wave to an epoch and a lane to a channel can go wrong: K = 1, 3, 4, 5, 12, 63 and 64 with E = 1, 4, 5 and 9 (whole and
partial workgroups of four epochs); every subset of the optional outputs, with and without ``used`` and weights; epochs of every
kind inside one workgroup -- clean, without a fix, with three channels, singular (two identical satellites among four), one channel
with a NaN Doppler, a fix at the Earth's centre -- where each clean epoch keeps the bytes it has without the others; the same call
twice; and a fix that came from position_fix_raim on the device with a channel left out.  The twin itself is compared with the
independent restatement in tests/test_velocity_host.py."""
import itertools

import numpy as np
import pytest

from tests import fix_cases as fc
from tests import raim_cases as rcs
from tests import vel_cases as vc

pytestmark = pytest.mark.gpu

OUTPUTS = ("sat_vel", "resid")


@pytest.fixture(scope="module")
def g():
    import gpuacceleratedtracking_amd as g
    g.load_library()
    return g


def cuda(a):
    import torch

    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def fix_records(fix):
    """the gat_fix records of a host PositionFix or of a structured array, as the device call takes them"""
    rec = fix if isinstance(fix, np.ndarray) else fix.fixes
    return cuda(np.ascontiguousarray(rec).view(np.uint8).reshape(rec.shape[0], -1))


def both(g, c, doppler, fix, used=None, weights=None, **kw):
    """(device, twin) of one call; ``used``: an array or None"""
    host = g.velocity_fix_host(c.ephs, c.tx_ms, c.tx_frac, doppler, fix if isinstance(fix, np.ndarray) else fix.fixes, weights, used=used, **kw)
    dev = g.velocity_fix(c.ephs, cuda(c.tx_ms), cuda(c.tx_frac), cuda(doppler), fix_records(fix), cuda(weights), used=cuda(used), **kw)
    assert dev._host is None  # nothing read back by the call
    return dev, host


def same_bits(dev, host, outputs=OUTPUTS, what=""):
    differ = np.flatnonzero([a.tobytes() != b.tobytes() for a, b in zip(dev.velocities, host.velocities)])
    assert differ.size == 0, (what, "epochs", differ[:10], dev.velocities[differ[:3]], host.velocities[differ[:3]])
    for name in outputs:
        a, b = getattr(dev, name), getattr(host, name)
        assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), (what, name)


def case_of(K: int, E: int) -> vc.VelCase:
    base = fc.case("short", 30, K, 8) if K < 30 else fc.case("mid", K)
    c = base.tiled(E) if E != base.E else base
    return vc.moving(c, fix=vc.records(c.truth_xyz, c.truth_bias_s) if K < 4 else None)


@pytest.mark.parametrize("K", [1, 3, 4, 5, 12, 63, 64])
def test_device_equals_twin_at_the_edges_of_the_work_split(g, K):
    per_group = g.velocity_plan(1, K)["waves_per_workgroup"]
    assert per_group == 4 and g.velocity_plan(5, K)["workgroups"] == 2 and g.velocity_plan(9, K)["workgroups"] == 3
    rng = np.random.default_rng(K)
    for E in (1, 4, 5, 9):
        case = case_of(K, E)
        used = (rng.uniform(size=case.doppler.shape) < 0.9).astype(np.uint8)
        weights = rng.uniform(0.5, 2.0, case.doppler.shape)
        for u, w in ((None, None), (used, weights)):
            dev, host = both(g, case.case, case.doppler, case.fix, u, w)
            same_bits(dev, host, what=(K, E, u is not None))
        if K < 4:
            assert (host.status == g.velocity.FEW_SATS).all() and (host.num_valid == K).all() and not host.resid.any() and host.sat_vel.all()
        elif K >= 12:  # all channels: the receivers' velocities come back
            dev, host = both(g, case.case, case.doppler, case.fix)
            assert (dev.status == 0).all() and np.abs(dev.v_ecef - case.v_ecef).max() < 1e-7 and np.abs(dev.clock_drift - case.drift).max() < 1e-15


def test_every_subset_of_the_optional_outputs_and_inputs(g):
    case = case_of(12, 5)
    rng = np.random.default_rng(4)
    used = (rng.uniform(size=case.doppler.shape) < 0.8).astype(np.uint8)
    weights = rng.uniform(0.5, 2.0, case.doppler.shape)
    for u, w in itertools.product((None, used), (None, weights)):
        for n in range(len(OUTPUTS) + 1):
            for outs in itertools.combinations(OUTPUTS, n):
                dev, host = both(g, case.case, case.doppler, case.fix, u, w, outputs=outs)
                same_bits(dev, host, outs, (u is not None, w is not None, outs))
                assert set(dev._raw) == {"velocities", *outs}
        assert (host.num_used == (case.seen & (True if u is None else u != 0)).sum(axis=1)).all()


@pytest.fixture(scope="module")
def kinds(g):
    """nine epochs of twelve channels, three workgroups: clean, no fix, three channels, singular | NaN Doppler, the Earth's centre,
    clean, clean | clean.  Returns (case, doppler, fix records, used) of the tile and of the calm tile (every epoch clean)."""
    e_twin = 3
    base = fc.twinned(fc.case("short", 30, 12, 8).tiled(9), e_twin)
    case = vc.moving(base)
    c = case.case
    assert case.seen.all()
    calm = (c, case.doppler.copy(), case.fix.fixes.copy(), np.ones(c.tx_ms.shape, np.uint8))
    rec, dop, used = calm[2].copy(), calm[1].copy(), calm[3].copy()
    rec["status"][1] = g.positioning.FEW_SATS
    used[2, 3:] = 0
    order = np.argsort(-c.sin_el[e_twin])
    assert np.array_equal(c.ephs[order[0]], c.ephs[order[1]]) and c.tx_ms[e_twin, order[0]] == c.tx_ms[e_twin, order[1]]
    used[e_twin] = 0
    used[e_twin, order[:4]] = 1
    dop[4, 7] = np.nan
    rec["x"][5], rec["y"][5], rec["z"][5] = 0.0, 0.0, 0.0
    return calm, (c, dop, rec, used)


def test_epochs_of_every_kind_inside_one_workgroup(g, kinds):
    v = g.velocity
    calm, (c, dop, rec, used) = kinds
    dev, host = both(g, c, dop, rec, used)
    same_bits(dev, host, what="kinds")
    again, _ = both(g, c, dop, rec, used)  # the same call twice: the same bytes
    same_bits(again, dev, what="twice")
    quiet, quiet_host = both(g, *calm[:3], calm[3])
    same_bits(quiet, quiet_host, what="calm")
    assert list(dev.status) == [0, v.NO_FIX, v.FEW_SATS, v.SINGULAR, 0, v.NO_GEODETIC, 0, 0, 0], dev.status
    for e in (0, 6, 7, 8):  # a clean epoch keeps the bytes it has without the others
        assert dev.velocities[e].tobytes() == quiet.velocities[e].tobytes() and dev.resid[e].tobytes() == quiet.resid[e].tobytes()
        assert dev.sat_vel[e].tobytes() == quiet.sat_vel[e].tobytes()
    zero = np.zeros((), dtype=dev.velocities.dtype)
    want = zero.copy()
    want["status"] = v.NO_FIX
    assert dev.velocities[1].tobytes() == want.tobytes() and not dev.sat_vel[1].any() and not dev.resid[1].any()
    for e, status, n in ((2, v.FEW_SATS, 3), (3, v.SINGULAR, 4)):
        want = zero.copy()
        want["status"], want["num_valid"], want["num_used"] = status, 12, n
        assert dev.velocities[e].tobytes() == want.tobytes() and not dev.resid[e].any() and dev.sat_vel[e].all()
    assert dev.num_valid[4] == 11 and dev.num_used[4] == 11 and not dev.sat_vel[4, 7].any() and dev.resid[4, 7] == 0.0
    assert np.abs(dev.v_ecef[4] - quiet.v_ecef[4]).max() < 1e-8
    assert dev.vx[5] != 0.0 and dev.rms_residual_mps[5] > 0.0 and not any(dev.velocities[5][n] for n in ("ve", "vn", "vu", "sin_lat", "cos_lat", "sin_lon",
                                                                                                         "cos_lon", "height_m"))


def test_a_fix_from_the_integrity_test_with_a_channel_left_out(g):
    """position_fix_raim on the device leaves out the channel that is a code period off; velocity_fix takes that fix as it is -- the
    records and its ``used`` output, both still on the device -- and the channel is not in the velocity's set"""
    base = fc.case("short", 30, 12, 8)
    case = vc.moving(base)
    c = base.copy()
    e, k = 2, int(np.argsort(-base.sin_el[2])[2])
    rcs.shift_period(c, e, k, 1)
    fix = g.position_fix_raim(c.ephs, cuda(c.tx_ms), cuda(c.tx_frac), cuda(c.rx_ms), cuda(c.rx_frac), sigma_m=rcs.SIGMA_M)
    dev = g.velocity_fix(c.ephs, cuda(c.tx_ms), cuda(c.tx_frac), cuda(case.doppler), fix)
    assert fix._host is None and dev._host is None
    fix_host = g.position_fix_raim_host(*c.args(), sigma_m=rcs.SIGMA_M)
    host = g.velocity_fix_host(c.ephs, c.tx_ms, c.tx_frac, case.doppler, fix_host)
    same_bits(dev, host, what="raim")
    assert fix.excluded[e, 0] == k and fix.status[e] == g.positioning.EXCLUDED and fix.used[e, k] == 0
    assert (dev.status == 0).all() and dev.num_used[e] == 11 and dev.num_valid[e] == 12 and (np.delete(dev.num_used, e) == 12).all()
    assert np.abs(dev.v_ecef - case.v_ecef).max() < 1e-6  # the transmit time a millisecond off moves the satellite by 4 m and 0.6 mm/s
    every = g.velocity_fix(c.ephs, cuda(c.tx_ms), cuda(c.tx_frac), cuda(case.doppler), fix, used=None)
    assert (every.num_used == 12).all()


def test_refusals_of_the_device_entry_point(g):
    import torch

    case = case_of(12, 3)
    c = case.case
    args = (cuda(c.tx_ms), cuda(c.tx_frac), cuda(case.doppler), fix_records(case.fix))
    for kw in (dict(carrier_hz=0.0), dict(carrier_hz=float("nan")), dict(flags=1)):
        with pytest.raises(g.GatError):
            g.velocity_fix(c.ephs, *args, **kw)
    with pytest.raises(ValueError):
        g.velocity_fix(c.ephs, args[0], args[1].float(), args[2], args[3])
    with pytest.raises(ValueError):
        g.velocity_fix(c.ephs[:5], *args)
    with pytest.raises(ValueError):
        g.velocity_fix(c.ephs, *args[:3], args[3][:2])
    for host_one in range(4):  # a tensor that is not on the device never reaches the kernel
        with pytest.raises(ValueError):
            g.velocity_fix(c.ephs, *[a if i != host_one else a.cpu() for i, a in enumerate(args)])
    with pytest.raises(ValueError):
        g.velocity_fix(c.ephs, *args, used=torch.ones(c.tx_ms.shape, dtype=torch.uint8))
    with pytest.raises(ValueError):
        g.velocity_fix(c.ephs, *args, used="all")
    dev, host = both(g, c, case.doppler, case.fix)  # the context still works
    same_bits(dev, host)
