"""Cases for the fix-integrity tests on top of tests/fix_cases.py: copies of its cases with seeded pseudorange noise of 3 m and
faults injected into chosen epochs.

  period   one channel a code period off: +-1 in tx_ms (what GAT_OBS_EDGE_AMBIGUOUS warns of), 300 km of pseudorange
  bias60   one channel 60 m off
  two      a code period on one channel and 500 m on another, in an epoch with at least nine measurements
  n5       a code period on one channel of an epoch cut to five measurements: detected, nothing to exclude with
  n4       the same in an epoch cut to four: no redundancy, no test

When a case is built, the REFERENCE alone (tests/raim_ref.py, on the CPU) must agree with what the case is meant to show, at
p_fa = 1e-3: every clean epoch passes, every faulted epoch meant to be repaired is detected, the reference's winner is the faulted
channel with the runner-up's T at least ten times the winner's, and the two-fault epochs resolve greedily in two rounds.  The
seeds and channels below were chosen so that this holds; a change that breaks it fails here, nothing is skipped at test time."""
import functools

import numpy as np

from tests import fix_cases as fc
from tests import raim_ref as rr

SIGMA_M = 3.0
P_FA = 1e-3
C_LIGHT = 299792458.0
WEEK_MS = 604800000


@functools.lru_cache(maxsize=None)
def thresholds():
    import gpuacceleratedtracking_amd as g

    return g.raim_thresholds(P_FA, SIGMA_M)


def shift_tx(c, e, k, metres):
    """move channel k's pseudorange in epoch e by `metres` (a later reception is an earlier transmission), the fraction kept in
    [0, 1e-3) by a carry into the milliseconds"""
    frac = c.tx_frac[e, k] - metres / C_LIGHT
    carry = int(np.floor(frac / 1e-3))
    frac -= carry * 1e-3
    if frac >= 1e-3:
        frac, carry = frac - 1e-3, carry + 1
    if frac < 0.0:
        frac, carry = frac + 1e-3, carry - 1
    c.tx_frac[e, k] = frac
    c.tx_ms[e, k] = (int(c.tx_ms[e, k]) + carry) % WEEK_MS


def shift_period(c, e, k, periods):
    c.tx_ms[e, k] = (int(c.tx_ms[e, k]) + periods) % WEEK_MS


def noisy(base, seed):
    c = base.copy()
    rng = np.random.default_rng(seed)
    noise = rng.normal(0.0, SIGMA_M, c.tx_ms.shape)
    for e in range(c.E):
        for k in np.flatnonzero(c.tx_ms[e] >= 0):
            shift_tx(c, e, k, noise[e, k])
    return c


def cut(c, e, keep):
    """keep `keep` satellites of epoch e, spread from the highest to the lowest so that the geometry stays good"""
    seen = np.flatnonzero(c.tx_ms[e] >= 0)
    order = seen[np.argsort(-c.sin_el[e, seen])]
    kept = order[np.unique(np.rint(np.linspace(0, len(order) - 1, keep)).astype(int))]
    assert len(kept) == keep, (len(order), keep)
    c.tx_ms[e, np.setdiff1d(seen, kept)] = -1
    return kept


def reference(c, e, max_exclude=1, weights=None):
    return rr.raim(c.ephs, c.tx_ms[e], c.tx_frac[e], c.rx_ms[e], c.rx_frac[e], thresholds(), None if weights is None else weights[e], max_exclude)


class RaimCase:
    """case: the fix_cases.Case with noise and faults; plan[e] = (kind, faulted channels in the order the reference excludes them)"""

    def __init__(self, case, plan):
        self.case, self.plan = case, plan
        self.E, self.K = case.E, case.K

    def args(self):
        return self.case.args()

    def epochs(self, *kinds):
        return [e for e, (kind, _) in sorted(self.plan.items()) if kind in kinds]


def inject(c, e, kind, pick):
    """turn epoch e into `kind`; `pick` chooses among the epoch's measured channels, highest first.  Returns the faulted channels."""
    seen = np.flatnonzero(c.tx_ms[e] >= 0)
    order = seen[np.argsort(-c.sin_el[e, seen])]
    if kind == "clean":
        return ()
    if kind == "period":
        k = int(order[pick % len(order)])
        shift_period(c, e, k, 1 if pick % 2 else -1)
        return (k,)
    if kind == "bias60":
        k = int(order[pick % len(order)])
        shift_tx(c, e, k, 60.0 if pick % 2 else -60.0)
        return (k,)
    if kind == "two":
        assert len(order) >= 9, len(order)
        a, b = int(order[pick % len(order)]), int(order[(pick + 3) % len(order)])
        shift_period(c, e, a, 1)
        shift_tx(c, e, b, 500.0)
        return (a, b)
    if kind in ("n5", "n4"):
        kept = cut(c, e, 5 if kind == "n5" else 4)
        k = int(kept[pick % len(kept)])
        shift_period(c, e, k, 1)
        return (k,)
    raise KeyError(kind)


def check(rc: RaimCase):
    """the reference alone must show what the case means to show"""
    c = rc.case
    for e in range(c.E):
        kind, faulted = rc.plan.get(e, ("clean", ()))
        if kind == "failed":
            continue
        r = reference(c, e, 2 if kind == "two" else 1)
        if kind == "clean":
            assert r["status"] in (0, rr.NO_REDUNDANCY), (e, kind, r["status"], r["stat0"])
        elif kind in ("period", "bias60"):
            assert r["status"] == rr.DETECTED | rr.EXCLUDED and r["excluded"] == list(faulted), (e, kind, r["status"], r["excluded"], faulted)
            assert r["ratio"] >= 10.0, (e, kind, r["ratio"])
        elif kind == "two":
            assert r["status"] == rr.DETECTED | rr.EXCLUDED and r["excluded"] == list(faulted), (e, kind, r["status"], r["excluded"], faulted)
            one = reference(c, e, 1)
            assert one["status"] == rr.DETECTED | rr.UNRESOLVED and one["ratio"] >= 10.0, (e, one["status"], one["ratio"])
        elif kind == "n5":
            assert r["status"] == rr.DETECTED | rr.UNRESOLVED and r["dof"] == 1, (e, r["status"], r["dof"])
        elif kind == "n4":
            assert r["status"] == rr.NO_REDUNDANCY, (e, r["status"])
    return rc


# epoch -> (kind, pick) of the three host cases: 8 epochs each
PLANS = {
    "mid": {1: ("period", 0), 2: ("bias60", 0), 3: ("two", 1), 5: ("period", 3), 6: ("n5", 1), 7: ("n4", 0)},
    "week_start": {0: ("period", 2), 2: ("bias60", 1), 4: ("two", 0), 5: ("n5", 2), 7: ("bias60", 3)},
    "week_end": {0: ("bias60", 2), 1: ("period", 5), 3: ("n4", 1), 4: ("period", 1), 6: ("two", 2)},
}
SEEDS = {"mid": 7, "week_start": 8, "week_end": 9}


def build(base, plan, seed):
    c = noisy(base, seed)
    done = {}
    for e, (kind, pick) in plan.items():
        done[e] = (kind, inject(c, e, kind, pick))
    return check(RaimCase(c, done))


@functools.lru_cache(maxsize=None)
def case(name: str) -> RaimCase:
    return build(fc.case(name), PLANS[name], SEEDS[name])


ALL = tuple(PLANS)

# what an epoch of each kind must show from the library, with max_exclude >= the faults of the epoch
EXPECT = {"clean": 0, "period": rr.DETECTED | rr.EXCLUDED, "bias60": rr.DETECTED | rr.EXCLUDED, "two": rr.DETECTED | rr.EXCLUDED,
          "n5": rr.DETECTED | rr.UNRESOLVED, "n4": rr.NO_REDUNDANCY, "failed": rr.NOT_CHECKED}


@functools.lru_cache(maxsize=None)
def mixed(K: int, E: int, seed: int = 11) -> RaimCase:
    """E epochs of K channels for the device tests with every kind of epoch the count allows, in the order clean, period, two (K >= 9),
    n5, n4, failed (three measurements), bias60, clean ..: the kinds of one workgroup differ.  With fewer than six measurements nothing can be
    repaired: a period fault there is an n5 epoch; with fewer than eight the 60 m fault gives way to a period."""
    base = fc.case("short", 30, K, 8) if K < 30 else fc.case("mid", K)
    base = base.tiled(E) if E != base.E else base
    c = noisy(base, seed + K)
    kinds = ["clean", "period", "two", "n5", "n4", "failed", "bias60"]
    done = {}
    for e in range(E):
        kind = kinds[e % len(kinds)]
        n = int((c.tx_ms[e] >= 0).sum())
        if kind == "two" and n < 9:
            kind = "period"
        if kind == "bias60" and n < 8:  # 60 m among fewer satellites do not single their channel out by a factor of ten
            kind = "period"
        if kind == "period" and n < 6:
            kind = "n5"
        if kind == "failed":
            fc.special(c, e, "three", None)
            done[e] = ("failed", ())
        elif kind != "clean":
            done[e] = (kind, inject(c, e, kind, e + 1))
    return check(RaimCase(c, done))
