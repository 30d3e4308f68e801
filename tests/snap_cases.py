"""Snapshot receivers for the snapshot-fix tests, on top of tests/fix_cases.py: a case of fix_cases (its sites, clock errors and
transmit times) of which the receiver keeps the fractions of the transmit times alone, knows its position to within 30 km (the
prior: the truth displaced that far at most in a random direction) and its clock to within 20 s (whole milliseconds added to the
reading; the case's own clock error of up to 0.3 ms is the fractional part).

These bounds are a condition, not a measurement: the worst relative error of two predicted ranges is 2 x 30 km + 2 x 0.93 km/s x
20 s = 97 km, under (0.5 - 0.1) x 299.8 km = 119.9 km.  Asserted here, on the CPU, when a case is built: every epoch keeps at least
six satellites above five degrees (fix_cases.Case asserts it) and the restatement (tests/snap_ref.py) alone resolves every integer
with |q - n| < 0.4.  Pure numpy; needs no device."""
import functools

import numpy as np

from tests import fix_cases as fc
from tests import snap_ref as sr

WEEK_MS = 604800000
MAX_PRIOR_M = 30.0e3
MAX_CLOCK_MS = 20000


class SnapCase:
    """case: the fix_cases.Case; code_frac [E, K] (NaN where nothing is seen); rx_ms [E] (the case's plus offset_ms), rx_frac [E];
    prior [E, 3]; offset_ms [E]; ref: the restatement's result per epoch (a list of dicts, computed once, never changed)"""

    def __init__(self, case: fc.Case, seed: int = 21, prior_m: float = MAX_PRIOR_M, clock_ms: int = MAX_CLOCK_MS, check: bool = True):
        rng = np.random.default_rng(seed)
        self.case, self.E, self.K = case, case.E, case.K
        self.ephs = case.ephs
        self.seen = case.tx_ms >= 0
        self.code_frac = np.where(self.seen, case.tx_frac, np.nan)
        self.offset_ms = rng.integers(-clock_ms, clock_ms + 1, case.E)
        if case.E > 1:
            self.offset_ms[0], self.offset_ms[1] = clock_ms, -clock_ms
        self.rx_ms = ((case.rx_ms.astype(np.int64) + self.offset_ms) % WEEK_MS).astype(np.int32)
        self.rx_frac = case.rx_frac.copy()
        d = rng.normal(size=(case.E, 3))
        length = rng.uniform(0.0, prior_m, case.E)
        length[0] = prior_m
        self.prior = case.truth_xyz + d / np.linalg.norm(d, axis=1)[:, None] * length[:, None]
        self.truth_xyz, self.truth_bias_s = case.truth_xyz, case.truth_bias_s
        self.ref = None
        if check:
            self.ref = [sr.snapshot(self.ephs, self.code_frac[e], self.rx_ms[e], self.rx_frac[e], self.prior[e]) for e in range(self.E)]
            assert all(r["worst"] < 0.4 and not r["reresolved"] for r in self.ref), [r["worst"] for r in self.ref]

    def args(self):
        return self.ephs, self.code_frac, self.rx_ms, self.rx_frac, self.prior

    def tiled(self, epochs: int):
        """the case's epochs repeated to `epochs` of them (the restatement's results with them)"""
        import copy

        c = copy.copy(self)
        idx = np.arange(epochs) % self.E
        c.case = self.case.tiled(epochs)
        for name in ("seen", "code_frac", "offset_ms", "rx_ms", "rx_frac", "prior", "truth_xyz", "truth_bias_s"):
            setattr(c, name, np.ascontiguousarray(getattr(self, name)[idx]))
        c.ref = None if self.ref is None else [self.ref[i] for i in idx]
        c.E = epochs
        return c


@functools.lru_cache(maxsize=None)
def case(name: str, count: int = 30, channels=None, epochs: int = 8, check: bool = True) -> SnapCase:
    return SnapCase(fc.case(name, count, channels, epochs), check=check)


ALL = fc.ALL


def whole_ms_of(bias_s, truth_bias_s):
    """j: the whole milliseconds by which a solved clock bias stands off the case's -- a reference integer one off moves the bias by
    a millisecond and the coarse time by one the other way, and is no error"""
    return np.rint((np.asarray(bias_s) - np.asarray(truth_bias_s)) * 1e3)
