"""gat_range_corrections on the device against its host twin, byte for byte on every output, at the shapes where a kernel that gives a
thread to an (epoch, channel) can go wrong: one thread, one partial wave, exactly one workgroup, one thread more, 258 threads, a K
that divides nothing; every subset of the optional outputs with the zenith delays as an array and as the config's pair; ionosphere
only, troposphere only, both and neither; epochs of every kind inside one workgroup -- clean, without a fix, a fix at the Earth's
centre, a channel without a measurement, a channel below the floor -- where each clean epoch keeps the bytes it has without the
others; the same call twice; and fix records left on the device by position_fix_raim with a channel excluded.  The twin itself is
compared with the independent restatement in tests/test_atmosphere_host.py."""
import itertools

import numpy as np
import pytest

from tests import atm_cases as ac
from tests import fix_cases as fc
from tests import raim_cases as rcs
from tests import vel_cases as vc

pytestmark = pytest.mark.gpu

OUTPUTS = ("delay", "geom", "channel_status", "epoch_status")
SHAPES = [(1, 1), (1, 64), (4, 64), (5, 64), (9, 12), (43, 6), (3, 5), (64, 4)]


@pytest.fixture(scope="module")
def g():
    import gpuacceleratedtracking_amd as g
    g.load_library()
    return g


def cuda(a):
    import torch

    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def fix_records(rec):
    return cuda(np.ascontiguousarray(rec).view(np.uint8).reshape(rec.shape[0], -1))


def both(g, c, rec, zenith=None, **kw):
    """(device, twin) of one call on the case's times at the fix records ``rec``; ``zenith``: an array [E, 2], a pair or None"""
    host = g.range_corrections_host(*c.args(), rec, zenith=zenith, **kw)
    dev = g.range_corrections(c.ephs, cuda(c.tx_ms), cuda(c.tx_frac), cuda(c.rx_ms), cuda(c.rx_frac), fix_records(rec),
                              zenith=cuda(zenith) if isinstance(zenith, np.ndarray) else zenith, **kw)
    assert dev._host is None  # nothing read back by the call
    return dev, host


def same_bits(dev, host, outputs=OUTPUTS, what=""):
    for name in ("tx_frac_out",) + tuple(outputs):
        a, b = getattr(dev, name), getattr(host, name)
        assert a.shape == b.shape and a.dtype == b.dtype, (what, name)
        assert a.tobytes() == b.tobytes(), (what, name, np.argwhere(a.view(np.uint8).reshape(a.shape + (-1,)) != b.view(np.uint8).reshape(b.shape + (-1,)))[:5])


def case_of(E: int, K: int):
    """(case, fix records at the true states, zenith [E, 2])"""
    base = fc.case("short", 30, K, 8) if K < 30 else fc.case("mid", K)
    c = base.tiled(E) if E != base.E else base
    rng = np.random.default_rng(E * 100 + K)
    return c, vc.records(c.truth_xyz, c.truth_bias_s), np.stack([rng.uniform(2.0, 2.4, E), rng.uniform(0.02, 0.3, E)], axis=1)


@pytest.mark.parametrize("E,K", SHAPES)
def test_device_equals_twin_at_the_edges_of_the_work_split(g, E, K):
    plan = g.atmosphere_plan(E, K)
    assert plan["threads"] == 256 and plan["workgroups"] == -(-E * K // 256) and plan["lds_bytes"] == 0 and plan["scratch_bytes"] == 0
    c, rec, zen = case_of(E, K)
    dev, host = both(g, c, rec, zen, iono=ac.broadcast_iono())
    same_bits(dev, host, what=(E, K))
    seen = c.tx_ms >= 0
    assert (host.epoch_status == 0).all() and (host.channel_status[~seen] == 0).all() and (host.channel_status[seen] != 0).all()
    up = seen & (host.sin_el >= 0.0)
    assert (host.channel_status[up] == g.atmosphere.CH_CORRECTED).all() and (host.iono[up] > 1.0).all() and (host.tropo[up] > 2.0).all()


def test_every_subset_of_the_optional_outputs_with_and_without_zenith(g):
    c, rec, zen = case_of(9, 12)
    for z in (zen, (2.3, 0.1)):
        for n in range(len(OUTPUTS) + 1):
            for outs in itertools.combinations(OUTPUTS, n):
                dev, host = both(g, c, rec, z, iono=ac.broadcast_iono(), outputs=outs)
                same_bits(dev, host, outs, (isinstance(z, tuple), outs))
                assert set(dev._raw) - {"zenith"} == {"tx_frac_out", *outs}


def test_each_switch(g):
    c, rec, zen = case_of(5, 64)
    k = ac.broadcast_iono()
    full, _ = both(g, c, rec, zen, iono=k)
    for iono, z in ((k, None), (None, zen), (k, zen), (None, None)):
        dev, host = both(g, c, rec, z, iono=iono)
        same_bits(dev, host, what=(iono is not None, z is not None))
        assert np.array_equal(dev.iono, full.iono if iono is not None else np.zeros_like(full.iono))
        assert np.array_equal(dev.tropo, full.tropo if z is not None else np.zeros_like(full.tropo))
        assert np.array_equal(dev.geom, full.geom)
    assert dev.tx_frac.tobytes() == np.ascontiguousarray(c.tx_frac).tobytes()  # neither: byte for byte


def test_epochs_of_every_kind_inside_one_workgroup(g):
    a = g.atmosphere
    c, calm_rec, zen = case_of(9, 12)
    assert g.atmosphere_plan(9, 12)["workgroups"] == 1 and (c.tx_ms >= 0).all()
    k = ac.broadcast_iono()
    quiet, quiet_host = both(g, c, calm_rec, zen, iono=k)
    same_bits(quiet, quiet_host, what="calm")
    floor = float(np.sort(quiet.sin_el[6])[2:4].mean())  # three channels of epoch 6 lie below it
    floor_all = float(quiet.sin_el.min()) - 1e-3         # a floor below every channel
    assert floor_all > -1.0
    t = c.copy()
    rec = calm_rec.copy()
    rec["status"][1] = g.positioning.SINGULAR
    rec["x"][2], rec["y"][2], rec["z"][2] = 0.0, 0.0, 0.0
    t.tx_ms[4, 7] = -1
    dev, host = both(g, t, rec, zen, iono=k, floor_sin=floor_all)
    same_bits(dev, host, what="kinds")
    again, _ = both(g, t, rec, zen, iono=k, floor_sin=floor_all)
    same_bits(again, dev, what="twice")
    quiet_f, _ = both(g, c, calm_rec, zen, iono=k, floor_sin=floor_all)
    assert list(dev.epoch_status) == [0, a.NO_FIX, a.NO_GEODETIC, 0, 0, 0, 0, 0, 0]
    for e in (0, 3, 5, 6, 7, 8):  # a clean epoch keeps the bytes it has without the others
        for name in ("tx_frac_out", "delay", "geom", "channel_status"):
            assert getattr(dev, name)[e].tobytes() == getattr(quiet_f, name)[e].tobytes(), (e, name)
    for e in (1, 2):  # no frame: every fraction passes through, the rest is zero
        assert dev.tx_frac[e].tobytes() == t.tx_frac[e].tobytes() and not dev.delay[e].any() and not dev.geom[e].any() and not dev.channel_status[e].any()
    others = np.arange(12) != 7
    assert dev.channel_status[4, 7] == 0 and dev.tx_frac[4, 7] == t.tx_frac[4, 7] and not dev.delay[4, 7].any() and not dev.geom[4, 7].any()
    assert dev.delay[4][others].tobytes() == quiet_f.delay[4][others].tobytes()
    # a floor that three channels of epoch 6 lie below
    low, low_host = both(g, c, calm_rec, zen, iono=k, floor_sin=floor)
    same_bits(low, low_host, what="floor")
    under = quiet.sin_el < floor
    assert under[6].sum() == 3 and (low.channel_status[under] == a.CH_LOW).all() and (low.channel_status[~under] == a.CH_CORRECTED).all()
    assert not low.delay[under].any() and np.array_equal(low.tx_frac[under], c.tx_frac[under]) and np.array_equal(low.geom, quiet.geom)
    assert np.array_equal(low.tx_frac[~under], quiet.tx_frac[~under])


def test_fix_records_left_on_the_device_by_the_integrity_test(g):
    """position_fix_raim on the device leaves out the channel that is a code period off; range_corrections takes its records as they
    are, still on the device"""
    base = fc.case("short", 30, 12, 8)
    c = base.copy()
    e, ch = 2, int(np.argsort(-base.sin_el[2])[2])
    rcs.shift_period(c, e, ch, 1)
    k = ac.broadcast_iono()
    args = (cuda(c.tx_ms), cuda(c.tx_frac), cuda(c.rx_ms), cuda(c.rx_frac))
    fix = g.position_fix_raim(c.ephs, *args, sigma_m=rcs.SIGMA_M)
    dev = g.range_corrections(c.ephs, *args, fix, iono=k, zenith=(2.3, 0.1))
    assert fix._host is None and dev._host is None
    fix_host = g.position_fix_raim_host(*c.args(), sigma_m=rcs.SIGMA_M)
    host = g.range_corrections_host(*c.args(), fix_host, iono=k, zenith=(2.3, 0.1))
    same_bits(dev, host, what="raim")
    assert fix.excluded[e, 0] == ch and fix.status[e] == g.positioning.EXCLUDED
    assert (dev.epoch_status == 0).all() and (dev.channel_status == g.atmosphere.CH_CORRECTED).all()  # the left-out channel is corrected too


def test_refusals_of_the_device_entry_point(g):
    c, rec, zen = case_of(3, 5)
    args = (cuda(c.tx_ms), cuda(c.tx_frac), cuda(c.rx_ms), cuda(c.rx_frac), fix_records(rec))
    for kw in (dict(carrier_hz=0.0), dict(carrier_hz=float("nan")), dict(floor_sin=float("inf")), dict(flags=8)):
        with pytest.raises(g.GatError):
            g.range_corrections(c.ephs, *args, **kw)
    with pytest.raises(ValueError):
        g.range_corrections(c.ephs, *args[:4], args[4][:2])
    with pytest.raises(ValueError):
        g.range_corrections(c.ephs, *args, zenith=cuda(zen).cpu())
    with pytest.raises(ValueError):
        g.range_corrections(c.ephs, *args, zenith=cuda(zen[:2]))
    with pytest.raises(ValueError):
        g.range_corrections(c.ephs, *args, outputs=("resid",))
    dev, host = both(g, c, rec, zen, iono=ac.broadcast_iono())  # the context still works
    same_bits(dev, host)
