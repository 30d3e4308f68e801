"""Receivers under an atmosphere for the range-correction tests, on top of tests/fix_cases.py: a case of fix_cases (its sites, clock
errors and reception times) whose transmit times are solved again with the delay of tests/atm_ref.py -- Klobuchar with non-zero
coefficients, quantised through the library's page-18 encoder, and the standard atmosphere's zenith delays of the site -- added to
the light time at the true position.  A satellite below two degrees over the ellipsoid is a channel without a measurement.  Two
things are asserted here, on the CPU, when a case is built: every epoch keeps at least six satellites above five degrees (the
fix_cases condition), and in every (epoch, channel) the tests compare with the restatement, the restatement's own values -- at the
true position and at the twin's first fix -- stay farther than 1e-6 (relative) from every discontinuity of the model: |xx| = 1.57,
|phi_i| = 0.416, PER = 72000, AMP = 0, the day's wraps and floor_sin.  Pure numpy and the host library; needs no device."""
import functools

import numpy as np

from tests import atm_ref as ar
from tests import fix_cases as fc
from tests import fix_ref as ref

ALPHA = (1.1e-8, 1.5e-8, -6e-8, -6e-8)
BETA = (9e4, 1.3e5, -6.5e4, -3.9e5)
MIN_EL = np.radians(2.0)
FLOOR_SIN = 0.0


def lib():
    import gpuacceleratedtracking_amd as g

    return g


@functools.lru_cache(maxsize=None)
def broadcast_iono():
    """ALPHA and BETA on the message's grid: through the page's encoder, a subframe 4 of the decoder and back"""
    g = lib()
    payload = g.lnav_page18_payload(g.Klobuchar(ALPHA, BETA), a0=1e-7, a1=-2e-14, tot=405504.0, wnt=33, dt_ls=18, wnlsf=137, dn=7, dt_lsf=18)
    sym = 1.0 - 2.0 * np.concatenate([g.lnav_subframe(100 + i, 4, payload=payload) for i in range(3)]).astype(np.float64)
    page = g.lnav_page18(g.decode_navigation_host(sym[None, :], "LNAV"), 0)
    assert page.valid == 1 and page.sv_id == 56
    k = page.klobuchar
    assert all(v != 0.0 for v in k.alpha + k.beta)
    return k


def delayed_times(ephs, xyz, rx_ms, rx_frac, clock_bias_s, iono, zd, zw):
    """fix_ref.transmit_times with the restatement's delay at the true position added to the light time: (tx_ms, tx_frac, delay [m],
    elevation over the ellipsoid [rad]) of every satellite"""
    k = len(ephs)
    xyz = np.asarray(xyz, dtype=np.float64)
    t_rx = float(rx_ms) * 1e-3 + rx_frac - clock_bias_s
    lat, lon, _ = ar.geodetic(xyz)
    east = np.array([-np.sin(lon), np.cos(lon), 0.0])
    north = np.array([-np.sin(lat) * np.cos(lon), -np.sin(lat) * np.sin(lon), np.cos(lat)])
    up = np.array([np.cos(lat) * np.cos(lon), np.cos(lat) * np.sin(lon), np.sin(lat)])
    tau, delay = np.full(k, 0.075), np.zeros(k)
    for _ in range(10):
        pos = ref.orbit(ephs, ref.wrap_week(t_rx - tau) % ref.WEEK)
        d = ref.rotated(pos, tau) - xyz
        rng = np.linalg.norm(d, axis=-1)
        los = d / rng[:, None]
        el, az = np.arcsin(np.clip(los @ up, -1.0, 1.0)), np.arctan2(los @ east, los @ north)
        safe = np.maximum(el, MIN_EL)  # below it the channel is dropped; the model need not be evaluated there
        delay = ar.klobuchar(iono.alpha, iono.beta, lat, lon, safe, az, t_rx % ar.DAY)["iono"] + ar.tropo(safe, zd, zw)
        tau = (rng + delay) / ref.C_LIGHT
    dts = np.zeros(k)
    for _ in range(4):
        dts = ref.clock_correction(ephs, (t_rx - tau + dts) % ref.WEEK)
    off = rx_frac - clock_bias_s - tau + dts
    m = np.floor(off * 1e3)
    tx_frac = off - m * 1e-3
    m, tx_frac = np.where(tx_frac >= 1e-3, m + 1, m), np.where(tx_frac >= 1e-3, tx_frac - 1e-3, tx_frac)
    m, tx_frac = np.where(tx_frac < 0, m - 1, m), np.where(tx_frac < 0, tx_frac + 1e-3, tx_frac)
    tx_ms = (int(rx_ms) + m.astype(np.int64)) % 604800000
    return tx_ms.astype(np.int32), tx_frac, delay, el


class AtmCase:
    """case: a copy of the fix_cases.Case with the delayed transmit times; clean: the Case it came from; iono: the Klobuchar; zenith
    [E, 2]; delay [E, K]: what was added [m]; seen [E, K]; fix0: the twin's fix on the delayed times (every output); at_truth, at_fix0:
    the restatement's dicts per epoch at the true state and at fix0's"""

    def __init__(self, clean: fc.Case):
        g = lib()
        self.clean, self.iono = clean, broadcast_iono()
        c = clean.copy()
        E, K = c.E, c.K
        self.zenith, self.delay = np.zeros((E, 2)), np.zeros((E, K))
        el = np.zeros((E, K))
        for e in range(E):
            lat, _, h = ar.geodetic(c.truth_xyz[e])
            self.zenith[e] = ar.tropo_zenith(h, np.sin(lat))
            ms, frac, self.delay[e], el[e] = delayed_times(c.ephs, c.truth_xyz[e], c.rx_ms[e], c.rx_frac[e], c.truth_bias_s[e], self.iono, *self.zenith[e])
            seen = (clean.tx_ms[e] >= 0) & (el[e] > MIN_EL)
            c.tx_ms[e], c.tx_frac[e] = np.where(seen, ms, -1), np.where(seen, frac, 0.0)
        self.case, self.E, self.K = c, E, K
        self.seen = c.tx_ms >= 0
        self.delay = np.where(self.seen, self.delay, 0.0)
        assert (((el > np.radians(5.0)) & self.seen).sum(axis=1) >= min(6, K)).all()
        self.fix0 = g.position_fix_host(*c.args())
        assert (self.fix0.status == 0).all()
        self.at_truth = [self.restated(e, c.truth_xyz[e], c.truth_bias_s[e]) for e in range(E)]
        self.at_fix0 = [self.restated(e, self.fix0.xyz[e], self.fix0.clock_bias_s[e]) for e in range(E)]
        for e in range(E):
            for r in (self.at_truth[e], self.at_fix0[e]):
                ok = ar.margins_ok(r, FLOOR_SIN, self.iono.alpha)
                assert ok[self.seen[e]].all(), (e, np.flatnonzero(~ok & self.seen[e]))

    def restated(self, e, xyz, bias):
        c = self.case
        ms, frac = np.where(self.seen[e], c.tx_ms[e], 0), np.where(self.seen[e], c.tx_frac[e], 0.0)
        return ar.corrections(c.ephs, ms, frac, c.rx_ms[e], c.rx_frac[e], xyz, bias, self.iono.alpha, self.iono.beta, *self.zenith[e])

    def args(self):
        return self.case.args()


@functools.lru_cache(maxsize=None)
def case(name: str, count: int = 30, channels=None, epochs: int = 8) -> AtmCase:
    return AtmCase(fc.case(name, count, channels, epochs))


def overhead():
    """a polar orbit's satellite over the pole and a fix on the axis below it: cos of the latitude is 0 and the line of sight is the
    axis, so sin el is 1 exactly.  (ephemerides, tx_ms, tx_frac, rx_ms, rx_frac, fix records) of one epoch and one channel"""
    from gpuacceleratedtracking_amd import _lib

    eph = lib().Ephemeris(wn=801, toe=244800.0, toc=244800.0, sqrt_a=5153.6, e=0.0, m0=np.pi / 2, i0=np.pi / 2, omega0=0.3)
    fixes = np.zeros(1, dtype=_lib.FIX_DTYPE)
    fixes["z"] = 6356752.3
    tx_ms = np.array([[244800000]], dtype=np.int32)
    return np.array([eph.record]), tx_ms, np.zeros((1, 1)), np.array([244800067], dtype=np.int32), np.array([0.0002]), fixes
