"""Synthetic constellations and receivers for the position-fix tests.  A constellation is six planes of near-circular orbits
(sqrtA about 5153.6, e in 0.001 .. 0.02, i0 about 0.96 rad) with spread mean anomalies and small harmonic and clock terms, every
value quantised by the library's encoder so that words -> ephemeris is exact.  A case holds receivers on the ground with clock
errors and the transmit times the reference's light-time iteration gives them; a satellite below the horizon is a channel without
a measurement.  Every epoch of every case keeps at least six satellites above five degrees: asserted here, on the CPU, when the
case is built."""
import functools

import numpy as np

from tests import fix_ref as ref

SIN_5_DEG = float(np.sin(np.radians(5.0)))
EARTH_RADIUS = 6371.0e3


def lib():
    import gpuacceleratedtracking_amd as g

    return g


def quantise(ephs: list) -> list:
    """every field on the message's grid: through the encoder and back (the host decoder, no device)"""
    g = lib()
    sym = []
    for e in ephs:
        bits = g.lnav_ephemeris_payloads(e)
        sym.append(1.0 - 2.0 * np.concatenate([g.lnav_subframe(100 + i, i + 1, payload=bits[i]) for i in range(3)]).astype(np.float64))
    nav = g.decode_navigation_host(np.stack(sym), "LNAV")
    out = g.lnav_ephemerides(nav)
    assert all(e.valid == 1 for e in out)
    return out


@functools.lru_cache(maxsize=None)
def constellation(count: int, toe: float, toc: float, seed: int = 1):
    """``count`` quantised ephemerides as a structured array [count]"""
    g = lib()
    rng = np.random.default_rng(seed)
    slots = -(-count // 6)
    ephs = []
    for i in range(count):
        plane, slot = i % 6, i // 6
        u = lambda lo, hi: float(rng.uniform(lo, hi))  # noqa: E731
        ephs.append(g.Ephemeris(
            wn=801, iodc=256 + (i % 200), iode=(i % 200), health=0, ura=1, fit=0, toe=toe, toc=toc,
            af0=u(-3e-4, 3e-4), af1=u(-4e-12, 4e-12), af2=0.0 if i % 3 else u(-2e-17, 2e-17), tgd=u(-1e-8, 1e-8),
            sqrt_a=5153.6 + u(-0.4, 0.4), e=u(0.001, 0.02), m0=float(np.mod(2 * np.pi * (slot / slots + plane / 11.0) + np.pi, 2 * np.pi) - np.pi) * 0.999,
            delta_n=u(3.5e-9, 5.5e-9), omega0=float(np.mod(np.radians(60.0 * plane + 17.0) + np.pi, 2 * np.pi) - np.pi), i0=0.96 + u(-0.02, 0.02),
            omega=u(-3.0, 3.0), omega_dot=u(-8.8e-9, -7.6e-9), idot=u(-5e-10, 5e-10),
            cuc=u(-4e-6, 4e-6), cus=u(-4e-6, 9e-6), crc=u(150.0, 350.0), crs=u(-120.0, 120.0), cic=u(-2e-7, 2e-7), cis=u(-2e-7, 2e-7)))
    return np.array([e.record for e in quantise(ephs)])


def ground(lat_deg, lon_deg, height=0.0):
    lat, lon = np.radians(lat_deg), np.radians(lon_deg)
    r = EARTH_RADIUS + height
    return np.array([r * np.cos(lat) * np.cos(lon), r * np.cos(lat) * np.sin(lon), r * np.sin(lat)])


RECEIVERS = [(48.1, 11.6, 520.0), (-33.9, 151.2, 30.0), (0.0, -78.5, 2850.0), (89.0, 10.0, 0.0), (-77.8, 166.7, 10.0), (35.7, 139.7, 40.0),
             (64.1, -21.9, 15.0), (-15.8, -47.9, 1100.0)]


class Case:
    """ephs [K]; tx_ms, tx_frac [E, K]; rx_ms, rx_frac [E]; truth_xyz [E, 3], truth_bias_s [E]; sin_el [E, K] (geometric, of every
    satellite, seen or not)"""

    def __init__(self, ephs, rx_times, seed=5, channels=None, site=None):
        rng = np.random.default_rng(seed)
        E = len(rx_times)
        rows = []
        for e, (ms, frac) in enumerate(rx_times):
            xyz = ground(*RECEIVERS[(e if site is None else site) % len(RECEIVERS)]) + rng.uniform(-50.0, 50.0, 3)
            bias = float(rng.uniform(-3e-4, 3e-4))
            tx_ms, tx_frac, sin_el = ref.transmit_times(ephs, xyz, ms, frac, bias)
            rows.append((xyz, bias, tx_ms, tx_frac, sin_el))
        sin_el = np.stack([r[4] for r in rows])
        if channels is not None:  # the `channels` satellites that stand highest over the case
            pick = np.sort(np.argsort(-sin_el.min(axis=0))[:channels])
            ephs, sin_el = ephs[pick], sin_el[:, pick]
            rows = [(r[0], r[1], r[2][pick], r[3][pick], r[4][pick]) for r in rows]
        seen = sin_el > 0.0
        self.ephs = ephs
        self.tx_ms = np.where(seen, np.stack([r[2] for r in rows]), -1).astype(np.int32)
        self.tx_frac = np.where(seen, np.stack([r[3] for r in rows]), 0.0)
        self.rx_ms = np.array([t[0] for t in rx_times], dtype=np.int32)
        self.rx_frac = np.array([t[1] for t in rx_times], dtype=np.float64)
        self.truth_xyz = np.stack([r[0] for r in rows])
        self.truth_bias_s = np.array([r[1] for r in rows])
        self.sin_el = sin_el
        self.E, self.K = E, len(ephs)
        assert ((sin_el > SIN_5_DEG).sum(axis=1) >= min(6, self.K)).all(), (sin_el > SIN_5_DEG).sum(axis=1)
        assert (self.tx_frac >= 0).all() and (self.tx_frac < 1e-3).all()

    def args(self):
        return self.ephs, self.tx_ms, self.tx_frac, self.rx_ms, self.rx_frac

    def copy(self):
        import copy

        return copy.deepcopy(self)

    def tiled(self, epochs: int):
        """the case's epochs repeated to `epochs` of them"""
        c = self.copy()
        idx = np.arange(epochs) % self.E
        for name in ("tx_ms", "tx_frac", "rx_ms", "rx_frac", "truth_xyz", "truth_bias_s", "sin_el"):
            setattr(c, name, np.ascontiguousarray(getattr(self, name)[idx]))
        c.E = epochs
        return c


def times(first_ms: int, step_ms: int, count: int, frac: float = 0.000123456):
    return [((first_ms + i * step_ms) % 604800000, frac * ((i % 5) + 1) / 5.0) for i in range(count)]


@functools.lru_cache(maxsize=None)
def case(name: str, count: int = 30, channels=None, epochs: int = 8) -> Case:
    """mid: toe in mid-week, receptions an hour before to an hour after it (t_k of both signs).  week_start: toe and toc at the end of
    the week before, receptions in the first minutes of the week, the first so early that its transmissions lie in the week
    before.  week_end: toe and toc at the start of the next week, receptions in the last minutes of this one.  short: one site over
    a few minutes, so that `channels` satellites can stand high in every epoch."""
    if name == "mid":
        return Case(constellation(count, 244800.0, 244800.0 - 16 * 5), times(244800000 - 3600000, 7200000 // (epochs - 1), epochs), channels=channels)
    if name == "week_start":
        return Case(constellation(count, 604784.0, 604784.0), [(30, 0.0004)] + times(50000, 240000, epochs - 1), channels=channels)
    if name == "week_end":
        return Case(constellation(count, 16.0, 0.0), times(604800000 - 1800000, 1800000 // epochs - 3, epochs), channels=channels)
    if name == "short":
        return Case(constellation(count, 244800.0, 244800.0 - 16 * 5), times(244800000 + 600000, 480000 // epochs, epochs), channels=channels, site=0)
    raise KeyError(name)


ALL = ("mid", "week_start", "week_end")


def twinned(c: Case, e: int) -> Case:
    """a copy in which the channel that stands lowest in epoch e carries the satellite that stands highest there, in every epoch"""
    t = c.copy()
    a, b = int(np.argmax(c.sin_el[e])), int(np.argmin(c.sin_el[e]))
    t.ephs = c.ephs.copy()
    t.ephs[b] = t.ephs[a]
    for name in ("tx_ms", "tx_frac", "sin_el"):
        getattr(t, name)[:, b] = getattr(t, name)[:, a]
    return t


# ---- special epochs -------------------------------------------------------------------------------------------------------------------
def starvable(c: Case, e: int, mask_sin: float, margin: float = 0.02):
    """(three satellites of epoch e well above the mask, two seen ones well below it), every one a different satellite; None where
    the epoch has no such five"""
    seen = np.flatnonzero(c.tx_ms[e] >= 0)
    _, first = np.unique(np.stack([c.tx_ms[e, seen], c.tx_frac[e, seen]]), axis=1, return_index=True)  # one channel a satellite
    seen = seen[np.sort(first)]
    order = seen[np.argsort(-c.sin_el[e, seen])]
    high = order[c.sin_el[e, order] > mask_sin + margin][:3]
    low = order[(c.sin_el[e, order] < mask_sin - margin) & (c.sin_el[e, order] > margin)][-2:]
    return (high, low) if len(high) == 3 and len(low) == 2 else None


def special(c: Case, e: int, kind: str, weights: np.ndarray, mask_sin: float = -1.0):
    """turn epoch e of the case (in place) into the special case `kind`; returns the status bits it must show"""
    lb = lib().positioning
    seen = np.flatnonzero(c.tx_ms[e] >= 0)
    order = seen[np.argsort(-c.sin_el[e, seen])]  # highest first
    if kind == "mask_starved":  # five measurements, three of them above the mask: the first pass stands (under that mask)
        high, low = starvable(c, e, mask_sin)
        keep = np.zeros(c.K, bool)
        keep[high], keep[low] = True, True
        c.tx_ms[e, ~keep] = -1
        return lb.MASK_STARVED
    if kind == "three":
        c.tx_ms[e, order[3:]] = -1
        return lb.FEW_SATS
    if kind == "weights_three":  # enough measurements, too few weights
        weights[e, order[3:]] = 0.0
        weights[e, order[4]] = np.nan
        return lb.FEW_SATS
    if kind == "nan":
        c.tx_frac[e, :] = np.nan
        return lb.FEW_SATS
    if kind == "nan_rx":
        c.rx_frac[e] = np.inf
        return lb.FEW_SATS
    if kind == "twins":  # four measurements, two of them one satellite (a case made by `twinned` for this epoch): a singular system
        assert np.array_equal(c.ephs[order[0]], c.ephs[order[1]]) and c.tx_ms[e, order[0]] == c.tx_ms[e, order[1]]
        c.tx_ms[e, order[4:]] = -1
        return lb.SINGULAR
    raise KeyError(kind)
