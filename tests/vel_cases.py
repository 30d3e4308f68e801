"""Moving receivers for the velocity-fix tests, on top of tests/fix_cases.py: a case of fix_cases (its sites, clock errors and
transmit times) whose receivers move and whose clocks drift, with the Doppler observable that tests/vel_ref.py's model -- or its
model-free truth -- gives every seen channel.  Pure numpy and the host library; needs no device."""
import functools

import numpy as np

from tests import fix_cases as fc
from tests import fix_ref as ref
from tests import vel_ref as vr

DRIFTS = (0.0, 2e-7, -2e-7)


def lib():
    import gpuacceleratedtracking_amd as g

    return g


class VelCase:
    """case: the fix_cases.Case; v_ecef [E, 3], drift [E]: what the receivers do; doppler [E, K] (0 where nothing is seen); fix: the
    twin's position fix of the case (every output)"""

    def __init__(self, case, v_ecef, drift, doppler, fix=None):
        self.case, self.v_ecef, self.drift, self.doppler = case, v_ecef, drift, doppler
        self.E, self.K = case.E, case.K
        self.seen = case.tx_ms >= 0
        self.fix = lib().position_fix_host(*case.args()) if fix is None else fix
        assert fix is not None or (self.fix.status == 0).all()

    def args(self):
        c = self.case
        return c.ephs, c.tx_ms, c.tx_frac, self.doppler, self.fix


def motions(E: int, seed: int, top_speed: float = 300.0):
    """per epoch a velocity (the first at rest, the second at the top speed, the rest anywhere below it) and a drift of DRIFTS"""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(E, 3))
    v = d / np.linalg.norm(d, axis=1)[:, None] * rng.uniform(0.0, top_speed, E)[:, None]
    v[0] = 0.0
    if E > 1:
        v[1] *= top_speed / np.linalg.norm(v[1])
    return v, np.array([DRIFTS[e % len(DRIFTS)] for e in range(E)])


def reception_time(c: fc.Case, e: int):
    """the GPS time of epoch e's reception in long double: what the receiver's clock reads less its error"""
    return np.longdouble(int(c.rx_ms[e])) / np.longdouble(1000) + np.longdouble(c.rx_frac[e]) - np.longdouble(c.truth_bias_s[e])


def moving(c: fc.Case, seed: int = 11, truth: bool = False, v_ecef=None, drift=None, fix=None) -> VelCase:
    """the case with moving receivers; ``truth``: the range rates from ``vel_ref.range_rate_truth`` instead of the model"""
    v, d = motions(c.E, seed)
    v = v if v_ecef is None else np.asarray(v_ecef, dtype=np.float64)
    d = d if drift is None else np.asarray(drift, dtype=np.float64)
    seen = c.tx_ms >= 0
    dop = np.zeros(c.tx_ms.shape)
    for e in range(c.E):
        ms, frac = np.where(seen[e], c.tx_ms[e], 0), np.where(seen[e], c.tx_frac[e], 0.0)
        rr = vr.range_rate_truth(c.ephs, c.truth_xyz[e], v[e], reception_time(c, e)) if truth else None
        dop[e] = np.where(seen[e], vr.doppler(c.ephs, ms, frac, c.truth_xyz[e], v[e], d[e], range_rate=rr), 0.0)
    return VelCase(c, v, d, dop, fix)


@functools.lru_cache(maxsize=None)
def case(name: str, count: int = 30, channels=None, epochs: int = 8, truth: bool = False) -> VelCase:
    return moving(fc.case(name, count, channels, epochs), truth=truth)


def records(xyz, bias_s=0.0, status=0):
    """gat_fix records [E] that say nothing but a state: what the velocity fix reads of a fix"""
    from gpuacceleratedtracking_amd import _lib

    xyz = np.atleast_2d(np.asarray(xyz, dtype=np.float64))
    f = np.zeros(xyz.shape[0], dtype=_lib.FIX_DTYPE)
    f["x"], f["y"], f["z"], f["clock_bias_s"], f["status"] = xyz[:, 0], xyz[:, 1], xyz[:, 2], bias_s, status
    return f


def restated(vc: VelCase, e: int, use=None, weights=None, doppler=None):
    """the restatement's velocity of epoch e at the twin's fix"""
    c = vc.case
    use = vc.seen[e] if use is None else use
    ms, frac = np.where(vc.seen[e], c.tx_ms[e], 0), np.where(vc.seen[e], c.tx_frac[e], 0.0)
    return vr.velocity(c.ephs, ms, frac, vc.doppler[e] if doppler is None else doppler, vc.fix.xyz[e], use, weights)
