"""gat_velocity_fix on the device against its host twin, byte for byte on the records, sat_vel and resid, over the hostile entries of
tests/velplan/velplan_main.cpp on designated channels of hostile epochs among clean ones, in the tiles of tests/fix_domain.py (nine
epochs: two workgroups and one, a hostile epoch among the clean ones of each full workgroup and one alone in the last), K = 64 and 12:
every real field of the ephemeris NaN and the infinities, eccentricities and semi-axes at and beyond the fence (sqrt_a = 5e-324,
0.004 and 1e200 among them), transmit times and weights at their edges; then, on the calm tile, doppler_hz and weights that are NaN
and the infinities, a fix whose x, y, z or clock bias is, a fix at the Earth's centre and one exactly on a satellite.  The fix is a
given state (the receivers' true one): what gat_position_fix makes of such epochs is tests/test_position_domain_gpu.py's.  Every
clean epoch must keep the bytes it has in the calm tile."""
import numpy as np
import pytest

from tests import fix_domain as fd
from tests import vel_cases as vc

pytestmark = pytest.mark.gpu

BAD = (np.nan, np.inf, -np.inf)


@pytest.fixture(scope="module")
def g():
    import gpuacceleratedtracking_amd as g
    g.load_library()
    return g


def cuda(a):
    import torch

    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def both(g, c, doppler, rec, weights=None):
    host = g.velocity_fix_host(c.ephs, c.tx_ms, c.tx_frac, doppler, rec, weights)
    dev = g.velocity_fix(c.ephs, cuda(c.tx_ms), cuda(c.tx_frac), cuda(doppler), cuda(rec.view(np.uint8).reshape(rec.shape[0], -1)), cuda(weights))
    return dev, host


def same_bits(dev, host, what):
    differ = np.flatnonzero([a.tobytes() != b.tobytes() for a, b in zip(dev.velocities, host.velocities)])
    assert differ.size == 0, (what, "epochs", differ[:10], dev.velocities[differ[:3]], host.velocities[differ[:3]])
    for name in ("sat_vel", "resid"):
        a, b = getattr(dev, name), getattr(host, name)
        if a.tobytes() != b.tobytes():
            at = np.argwhere(a.view(np.uint64) != b.view(np.uint64))
            raise AssertionError((what, name, "differs at", at[:10].tolist(), a[tuple(at[0])], b[tuple(at[0])]))


def clean_epochs_keep_their_bytes(dev, quiet, clean, what):
    for e in clean:
        assert dev.velocities[e].tobytes() == quiet.velocities[e].tobytes(), (what, e)
        assert dev.resid[e].tobytes() == quiet.resid[e].tobytes() and dev.sat_vel[e].tobytes() == quiet.sat_vel[e].tobytes(), (what, e)


@pytest.fixture(scope="module", params=[64, 12])
def scene(request):
    """the tiles of K channels, the calm tile moving (its Doppler serves every tile: a designated channel's is 0) and the fix records"""
    K = request.param
    tiles = fd.hostile(K, 4)
    calm = vc.moving(tiles[0].calm, fix=vc.records(tiles[0].calm.truth_xyz, tiles[0].calm.truth_bias_s))
    return K, tiles, calm


def test_device_equals_twin_on_every_hostile_entry(g, scene):
    K, tiles, calm = scene
    assert g.velocity_plan(tiles[0].E, K)["workgroups"] == 3 and tiles[0].E == 9
    quiet, quiet_host = both(g, calm.case, calm.doppler, calm.fix)
    same_bits(quiet, quiet_host, (K, "calm"))
    assert (quiet.status[list(tiles[0].clean)] == 0).all() and np.abs(quiet.v_ecef - calm.v_ecef)[list(tiles[0].clean)].max() < 1e-7
    for n, t in enumerate(tiles):
        labels = sorted({label for label, _, _ in t.entries})
        for weights in (t.weights, None):
            dev, host = both(g, t.case, calm.doppler, calm.fix, weights)
            same_bits(dev, host, (K, n, labels))
            clean_epochs_keep_their_bytes(dev, quiet, t.clean, (K, n, labels))
        for label, e, k in t.entries:
            if label.split("=")[-1] in ("nan", "+inf", "-inf") and not label.startswith(("rx_frac", "weight")):
                assert not dev.sat_vel[e, k].any() and dev.resid[e, k] == 0.0, label  # a field that is not finite: the channel does not count
            if label in ("sqrt_a=subnormal", "sqrt_a=0.004", "sqrt_a=1e200"):
                print(f"K = {K}: {label} at epoch {e}, channel {k}: device sat_vel {dev.sat_vel[e, k].tolist()}, the twin's bits; status {dev.status[e]}")


def test_hostile_doppler_weights_and_fix_states(g, scene):
    K, tiles, calm = scene
    v = g.velocity
    c, hostile, clean = calm.case, tiles[0].hostile, tiles[0].clean
    quiet, _ = both(g, c, calm.doppler, calm.fix)
    chan = [int(np.flatnonzero(calm.seen[e])[0]) for e in hostile]
    zero = np.zeros((), dtype=quiet.velocities.dtype)
    for bad in BAD:
        dop, w = calm.doppler.copy(), np.ones(calm.doppler.shape)
        for e, k in zip(hostile, chan):
            dop[e, k], w[e, k] = bad, bad
        dev, host = both(g, c, dop, calm.fix)
        same_bits(dev, host, (K, "doppler", bad))
        clean_epochs_keep_their_bytes(dev, quiet, clean, ("doppler", bad))
        for e, k in zip(hostile, chan):
            assert dev.num_valid[e] == quiet.num_valid[e] - 1 and not dev.sat_vel[e, k].any() and dev.resid[e, k] == 0.0 and dev.status[e] == 0
        dev, host = both(g, c, calm.doppler, calm.fix, w)
        same_bits(dev, host, (K, "weight", bad))
        clean_epochs_keep_their_bytes(dev, quiet, clean, ("weight", bad))
        for e, k in zip(hostile, chan):
            assert dev.num_valid[e] == quiet.num_valid[e] and dev.num_used[e] == quiet.num_used[e] - 1 and dev.sat_vel[e, k].any()
        for field in ("x", "y", "z", "clock_bias_s"):
            rec = calm.fix.copy()
            rec[field][list(hostile)] = bad
            dev, host = both(g, c, calm.doppler, rec)
            same_bits(dev, host, (K, field, bad))
            clean_epochs_keep_their_bytes(dev, quiet, clean, (field, bad))
            want = zero.copy()
            want["status"] = v.NO_FIX
            for e in hostile:
                assert dev.velocities[e].tobytes() == want.tobytes() and not dev.sat_vel[e].any() and not dev.resid[e].any()
    # the Earth's centre, and exactly on a satellite (the last range is zero or a rounding of the coordinates: defined either way)
    from tests import fix_ref as ref

    rec = calm.fix.copy()
    e0, e1 = hostile[0], hostile[1]
    rec["x"][e0], rec["y"][e0], rec["z"][e0] = 0.0, 0.0, 0.0
    pos, _ = ref.satellite(c.ephs[chan[1]], c.tx_ms[e1, chan[1]], c.tx_frac[e1, chan[1]])
    rec["x"][e1], rec["y"][e1], rec["z"][e1] = pos
    dev, host = both(g, c, calm.doppler, rec)
    same_bits(dev, host, (K, "centre and satellite"))
    clean_epochs_keep_their_bytes(dev, quiet, clean, "centre and satellite")
    assert dev.status[e0] == v.NO_GEODETIC and dev.vx[e0] != 0.0 and dev.ve[e0] == 0.0 and dev.height_m[e0] == 0.0
    assert dev.num_valid[e1] == quiet.num_valid[e1]
    print(f"K = {K}: a fix on a satellite: status {dev.status[e1]}, velocity {dev.v_ecef[e1].tolist()}")
