"""gat_range_corrections over its input domain: the device and the host twin agree on the bytes of every output (no restatement
here, but to show that a condition is really met) for NaN, the infinities and the zeros in each Klobuchar coefficient, each zenith
delay and each field of the fix; floor_sin at -1, 0, 1 - ulp and exactly a channel's sin el; a receiver on the axis and at the pole;
phi_i beyond the clip both ways; PER below 72000 and AMP below 0; t on both sides of both wraps; |xx| on both sides of 1.57, found by
bisection on rx_frac in the twin; and sin el = 1."""
import numpy as np
import pytest

from tests import atm_cases as ac
from tests import atm_ref as ar
from tests import fix_cases as fc
from tests import vel_cases as vc
from tests.test_atmosphere_gpu import both, same_bits

pytestmark = pytest.mark.gpu

VALUES = (np.nan, np.inf, -np.inf, 0.0, -0.0)


@pytest.fixture(scope="module")
def g():
    import gpuacceleratedtracking_amd as g
    g.load_library()
    return g


@pytest.fixture(scope="module")
def scene():
    """eight epochs of twelve channels at one site, the fixes at the true states, zenith delays, the broadcast coefficients"""
    c = fc.case("short", 30, 12, 8)
    assert (c.tx_ms >= 0).all()
    rng = np.random.default_rng(5)
    return c, vc.records(c.truth_xyz, c.truth_bias_s), np.stack([rng.uniform(2.0, 2.4, 8), rng.uniform(0.02, 0.3, 8)], axis=1), ac.broadcast_iono()


def test_values_that_are_not_finite_and_zeros_in_every_coefficient(g, scene):
    c, rec, zen, k = scene
    a = g.atmosphere
    for which in ("alpha", "beta"):
        for i in range(4):
            for v in VALUES:
                coeff = {"alpha": list(k.alpha), "beta": list(k.beta)}
                coeff[which][i] = v
                dev, host = both(g, c, rec, zen, iono=g.Klobuchar(**coeff))
                same_bits(dev, host, what=(which, i, v))
                if not np.isfinite(v):  # a coefficient that is not finite: no delay, for every channel, and the fraction as it came
                    assert (host.channel_status == a.CH_NONFINITE).all() and not host.delay.any() and host.tx_frac.tobytes() == c.tx_frac.tobytes()
                    assert host.geom.any()
                else:
                    assert (host.channel_status == a.CH_CORRECTED).all() and np.isfinite(host.delay).all()


def test_values_that_are_not_finite_and_zeros_in_the_zenith_delays(g, scene):
    c, rec, zen, k = scene
    a = g.atmosphere
    calm, _ = both(g, c, rec, zen, iono=k)
    for col in (0, 1):
        for v in VALUES:
            z = zen.copy()
            z[3, col] = v
            dev, host = both(g, c, rec, z, iono=k)
            same_bits(dev, host, what=("zenith", col, v))
            others = np.arange(8) != 3
            assert dev.delay[others].tobytes() == calm.delay[others].tobytes() and dev.tx_frac[others].tobytes() == calm.tx_frac[others].tobytes()
            assert (dev.channel_status[3] == (a.CH_CORRECTED if np.isfinite(v) else a.CH_NONFINITE)).all()
            pair, pair_host = both(g, c, rec, tuple(z[3]), iono=k)  # the same through the config's scalars
            same_bits(pair, pair_host, what=("pair", col, v))
            assert pair.delay[3].tobytes() == dev.delay[3].tobytes()


def test_values_that_are_not_finite_and_zeros_in_every_field_of_the_fix(g, scene):
    c, rec, zen, k = scene
    a = g.atmosphere
    calm, _ = both(g, c, rec, zen, iono=k)
    for name in ("x", "y", "z", "clock_bias_s"):
        for v in VALUES:
            r = rec.copy()
            r[name][[1, 6]] = v
            dev, host = both(g, c, r, zen, iono=k)
            same_bits(dev, host, what=(name, v))
            clean = [0, 2, 3, 4, 5, 7]
            for out in ("tx_frac_out", "delay", "geom", "channel_status", "epoch_status"):
                assert getattr(dev, out)[clean].tobytes() == getattr(calm, out)[clean].tobytes(), (name, v, out)
            assert (dev.epoch_status[[1, 6]] == (0 if np.isfinite(v) else a.NO_FIX)).all()
    for status in (g.positioning.FEW_SATS, g.positioning.SINGULAR, g.positioning.NONFINITE, g.positioning.NOT_CONVERGED | g.positioning.MASKED):
        r = rec.copy()
        r["status"][2] = status
        dev, host = both(g, c, r, zen, iono=k)
        same_bits(dev, host, what=("status", status))
        assert dev.epoch_status[2] == (a.NO_FIX if status & 7 else 0)


def test_floors(g, scene):
    c, rec, zen, k = scene
    a = g.atmosphere
    calm, _ = both(g, c, rec, zen, iono=k, floor_sin=-1.0)
    assert (calm.channel_status == a.CH_CORRECTED).all()
    exact = float(calm.sin_el[2, 5])
    for floor in (-1.0, 0.0, float(np.nextafter(1.0, 0.0)), exact, float(np.nextafter(exact, 2.0))):
        dev, host = both(g, c, rec, zen, iono=k, floor_sin=floor)
        same_bits(dev, host, what=("floor", floor))
        assert np.array_equal(dev.channel_status == a.CH_CORRECTED, calm.sin_el >= floor) and np.array_equal(dev.channel_status == a.CH_LOW, calm.sin_el < floor)
    assert dev.channel_status[2, 5] == a.CH_LOW  # a floor one ulp above a channel's sine leaves it out; the sine itself keeps it


def test_on_the_axis_and_at_the_pole(g, scene):
    c, rec, zen, k = scene
    a = g.atmosphere
    r = rec.copy()
    r["x"][:], r["y"][:] = 0.0, 0.0
    r["z"][:] = [6356752.3, -6356752.3, 7.0e6, 1.0e6, 999999.0, 6356752.3, 6356752.3, 6356752.3]
    r["x"][5], r["y"][6], r["x"][7], r["y"][7] = 1e-9, -1e-300, -0.0, -0.0
    dev, host = both(g, c, r, zen, iono=k, floor_sin=-1.0)
    same_bits(dev, host, what="axis")
    assert list(dev.epoch_status) == [0, 0, 0, 0, a.NO_GEODETIC, 0, 0, 0]
    assert np.isfinite(dev.delay).all() and np.isfinite(dev.geom).all() and np.isfinite(dev.tx_frac).all()
    assert ((dev.channel_status & (a.CH_CORRECTED | a.CH_NONFINITE)) != 0)[[0, 1, 2, 3, 5, 6, 7]].all()
    # on the axis the longitude is 0 by the frame's rule: the azimuth is measured from the x axis's meridian
    assert np.abs(dev.geom[0, :, 1] ** 2 + dev.geom[0, :, 2] ** 2 - 1.0).max() < 1e-15


def _restated(c, rec, zen, k, e):
    return ar.corrections(c.ephs, np.where(c.tx_ms[e] >= 0, c.tx_ms[e], 0), np.where(c.tx_ms[e] >= 0, c.tx_frac[e], 0.0), c.rx_ms[e], c.rx_frac[e],
                          np.array([rec["x"][e], rec["y"][e], rec["z"][e]]), rec["clock_bias_s"][e], k.alpha, k.beta, *zen[e])


def test_the_clip_the_raised_values_and_the_wraps(g):
    """the sites of fix_cases reach from 89 N to 78 S and from 166 E to 78 W: phi_i passes the clip both ways; the mid-week afternoon
    wraps t down and the first minutes of the week wrap it up"""
    k = ac.broadcast_iono()
    met = {"clip+": 0, "clip-": 0, "inside": 0, "t>=day": 0, "t<0": 0, "t in": 0}
    for name in ("mid", "week_start"):
        c = fc.case(name)
        rec = vc.records(c.truth_xyz, c.truth_bias_s)
        zen = np.tile([2.3, 0.1], (c.E, 1))
        dev, host = both(g, c, rec, zen, iono=k)
        same_bits(dev, host, what=name)
        for e in range(c.E):
            r, s = _restated(c, rec, zen, k, e), (c.tx_ms[e] >= 0) & (host.channel_status[e] == g.atmosphere.CH_CORRECTED)
            met["clip+"] += int((r["phi_i"][s] > 0.417).sum()); met["clip-"] += int((r["phi_i"][s] < -0.417).sum()); met["inside"] += int((np.abs(r["phi_i"][s]) < 0.415).sum())
            met["t>=day"] += int((r["t"][s] >= 86401.0).sum()); met["t<0"] += int((r["t"][s] < -1.0).sum()); met["t in"] += int(((r["t"][s] > 1.0) & (r["t"][s] < 86399.0)).sum())
    print(met)
    assert all(v > 0 for v in met.values()), met
    # PER below 72000 and AMP below 0, each of them everywhere
    c = fc.case("mid")
    rec = vc.records(c.truth_xyz, c.truth_bias_s)
    zen = np.tile([2.3, 0.1], (c.E, 1))
    for coeff in (dict(alpha=k.alpha, beta=(5e4, 0.0, 0.0, 0.0)), dict(alpha=(-1e-8, 0.0, 0.0, 0.0), beta=k.beta), dict(alpha=(0.0, 0.0, 0.0, 0.0), beta=(72000.0, 0.0, 0.0, 0.0))):
        dev, host = both(g, c, rec, zen, iono=g.Klobuchar(**coeff))
        same_bits(dev, host, what=coeff)
        assert np.isfinite(host.delay).all()
    up = host.channel_status == g.atmosphere.CH_CORRECTED
    night = host.iono.copy()  # AMP = 0: F 5e-9 c everywhere
    dev, host = both(g, c, rec, zen, iono=g.Klobuchar(alpha=(-1e-8, 0.0, 0.0, 0.0), beta=k.beta))
    assert np.array_equal(host.iono[up], night[up])  # AMP below 0 is raised to 0


def test_both_sides_of_the_daytime_threshold(g, scene):
    """|xx| = 1.57 lies between two neighbouring doubles of rx_frac, found in the twin: a channel is on the day side exactly when its
    delay differs from the one AMP = 0 gives"""
    c, rec, zen, k = scene
    flat = g.Klobuchar(alpha=(0.0, 0.0, 0.0, 0.0), beta=k.beta)
    e, ch = 0, 4
    one = c.copy()
    for name in ("tx_ms", "tx_frac", "sin_el"):
        setattr(one, name, np.ascontiguousarray(getattr(c, name)[e:e + 1, ch:ch + 1]))
    one.ephs, one.E, one.K = c.ephs[ch:ch + 1], 1, 1
    r1 = rec[e:e + 1].copy()
    base_ms = int(c.rx_ms[e])

    def day(ms, frac):
        one.rx_ms, one.rx_frac = np.array([ms], dtype=np.int32), np.array([frac])
        with_amp = g.range_corrections_host(*one.args(), r1, iono=k).iono[0, 0]
        return with_amp != g.range_corrections_host(*one.args(), r1, iono=flat).iono[0, 0]

    hours = [base_ms + h * 3600000 for h in range(-12, 12)]
    sides = [day(ms, 0.0) for ms in hours]
    i = next(i for i in range(len(sides) - 1) if sides[i] and not sides[i + 1])  # dusk
    lo, hi = hours[i], hours[i + 1]
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if day(mid, 0.0) else (lo, mid)
    assert day(lo, 0.0) and not day(lo, 1e-3)
    flo, fhi = 0.0, 1e-3
    while np.nextafter(flo, 1.0) < fhi:
        mid = 0.5 * (flo + fhi)
        flo, fhi = (mid, fhi) if day(lo, mid) else (flo, mid)
    assert day(lo, flo) and not day(lo, fhi) and np.nextafter(flo, 1.0) == fhi
    two = c.copy()
    two.rx_ms[0:2], two.rx_frac[0], two.rx_frac[1] = lo, flo, fhi
    for name in ("tx_ms", "tx_frac"):
        getattr(two, name)[1] = getattr(two, name)[0]
    r2 = rec.copy()
    r2[1] = r2[0]
    dev, host = both(g, two, r2, zen, iono=k)
    same_bits(dev, host, what="threshold")
    dev0, _ = both(g, two, r2, zen, iono=flat)
    assert dev.iono[0, ch] != dev0.iono[0, ch] and dev.iono[1, ch] == dev0.iono[1, ch]


def test_a_satellite_overhead(g):
    ephs, tx_ms, tx_frac, rx_ms, rx_frac, fixes = ac.overhead()

    class One:
        def args(self):
            return ephs, tx_ms, tx_frac, rx_ms, rx_frac

    one = One()
    one.ephs, one.tx_ms, one.tx_frac, one.rx_ms, one.rx_frac = ephs, tx_ms, tx_frac, rx_ms, rx_frac
    dev, host = both(g, one, fixes, (2.3012, 0.1234), iono=ac.broadcast_iono())
    same_bits(dev, host, what="overhead")
    assert dev.sin_el[0, 0] == 1.0 and dev.channel_status[0, 0] == g.atmosphere.CH_CORRECTED and abs(dev.tropo[0, 0] - 2.4246) <= 1e-12
