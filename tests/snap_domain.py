"""The snapshot fix's whole input domain (include/gat.h, "snapshot fix": fraction, usable, integers, solver, mask), for the tests of
the host twin and of the device: pure numpy and the host library on top of tests/fix_domain.py and tests/snap_cases.py.

``hostile(K)``     the tiles of fix_domain.hostile(K, 4) (nine epochs, three workgroups, a hostile epoch among the clean ones of each
                   full workgroup and one alone in the last) as snapshot receivers, made as snap_cases.SnapCase makes them: the
                   ephemeris, rx_frac and weight entries carry over, a tx_frac entry is a code_frac entry (a tx_ms entry leaves a
                   plain channel: the snapshot fix reads no tx_ms); then tiles with the code_frac and rx_ms entries of their own.
                   Every entry is labelled and has the ``ok`` and ``used`` that ``usable`` below, restated from gat.h, gives it.
``prior_entries``  hostile priors on the calm tile, as prior_xyz and, where the call does not refuse them, as init_xyz.
``full_width()``   one site's twelve satellites repeated over 64 channels: every lane used, the highest satellite five or six times.
``status_paths()`` the inputs of every status bit's path, each found on the CPU from the restatement or the twin.
Asserted here, on the CPU, when a case is built: every clean epoch keeps at least six satellites above five degrees (fix_cases and
fix_domain assert it) and the restatement (tests/snap_ref.py) alone resolves every integer of it with |q - n| < 0.4; the two sin el
that bracket a mask are at least 1e-3 apart."""
import functools
import math

import numpy as np

from tests import fix_cases as fc
from tests import fix_domain as fd
from tests import snap_cases as sc
from tests import snap_ref as sr

INT32_MIN, INT32_MAX = fd.INT32_MIN, fd.INT32_MAX
OUTPUTS = ("tx_ms", "rx_ms_out", "n_ms", "resid", "sin_el", "used")
CONVERGED = dict(tol_m=1e-6, max_iter=12)
E_RANGE_M = 5e-7  # what the twin and the restatement disagree on per range: tests/test_snapshot_host.py
MARGIN = 4.0
FAILED = 1 | 2 | 4  # FEW_SATS, SINGULAR, NONFINITE: every output zero


def lib():
    import gpuacceleratedtracking_amd as g

    return g


# ---- usable, restated from gat.h ------------------------------------------------------------------------------------------------------
def usable(eph, code_frac, rx_ms, rx_frac, state_finite=True) -> bool:
    """gat.h: "a channel counts (num_valid) when its ephemeris is usable as in gat_position_fix [valid != 0, 0 <= e < 0.5 and sqrt_a >
    0], its fraction [finite and in [0, 1e-3)] and the reception [rx_ms >= 0, rx_frac finite] are given and its first predicted state
    is finite".  The last condition is the rule's own arithmetic: ``state_finite`` is what the entry's label says of it."""
    fence = int(eph["valid"]) != 0 and 0.0 <= float(eph["e"]) < 0.5 and float(eph["sqrt_a"]) > 0.0
    f = float(code_frac)
    given = math.isfinite(f) and 0.0 <= f < 1e-3 and int(rx_ms) >= 0 and math.isfinite(float(rx_frac))
    return bool(fence and given and state_finite)


# ---- the entries ------------------------------------------------------------------------------------------------------------------------
def carried_over():
    """{label: state_finite} of fix_domain's entries.  The snapshot fix evaluates a satellite at R - 0.075 s where the fix evaluates
    it at its transmit time, some milliseconds apart: an ephemeris whose state is not finite there is not finite here; the garbage
    orbits that count there (sqrt_a = 0.004, 0.0086, 1.0) have a finite velocity as well (A n < 1e10 m/s).  A code_frac of 1e300 is
    outside [0, 1e-3) before any range is formed.  rx_frac = 1e300 is finite and given, but the satellite's time is 1e300 s and its
    mean anomaly 1e296, far beyond the sine's range (fix_domain: 1e28 already overflows): no predicted state is finite.  At 1e19 s
    the clock's af2 term is 1e21 s and M up to 1e17, beyond the range in which gat_fix.h's sine is one ("of any magnitude, or not
    finite"): the text of gat.h does not say which channels count (GARBAGE: the test asserts an upper bound and the epoch's end
    alone); those that do have z = c 1e19 and a reference range of 1e22 ms: NONFINITE by kSnapMaxMs."""
    out = {en[0]: en[3] for en in fd.ephemeris_entries()}
    out.update({en[0]: True for en in fd.cell_entries()})
    out.update({en[0]: en[2] for en in fd.epoch_entries()})
    assert GARBAGE <= set(out)
    return out


GARBAGE = {"rx_frac=1e+19"}


def code_frac_entries(rx_frac: float):
    """(label, value) of one (epoch, channel): the ends of [0, 1e-3), phi = 0 without a borrow, and a borrow whose phi + 1e-3 rounds to
    the whole period"""
    return [("code_frac=0.0", 0.0), ("code_frac=-0.0", -0.0), ("code_frac=1e-3-ulp", float(np.nextafter(1e-3, 0.0))),
            ("code_frac=rx_frac", float(rx_frac)), ("code_frac=rx_frac+ulp", float(np.nextafter(rx_frac, 1.0)))]


RX_MS_ENTRIES = [(f"rx_ms={v}", v) for v in (0, 604799999, 604800000, INT32_MAX, -1, INT32_MIN)]  # the epoch's; every finite time counts


class Tile:
    """ephs [K]; code_frac, weights [E, K]; rx_ms, rx_frac [E]; prior [E, 3]; clean, hostile: the epochs of each kind; want_ok,
    want_used [E, K] (used: with the weights; in an epoch of ``garbage`` an upper bound); entries: (label, epoch, channel)"""

    def __init__(self, snap: sc.SnapCase, weights, clean, hostile, finite, entries):
        self.ephs, self.code_frac, self.rx_ms, self.rx_frac, self.prior = snap.ephs, snap.code_frac, snap.rx_ms, snap.rx_frac, snap.prior
        self.weights, self.clean, self.hostile, self.entries = weights, clean, hostile, entries
        self.E, self.K = snap.E, snap.K
        self.want_ok = np.array([[usable(self.ephs[k], self.code_frac[e, k], self.rx_ms[e], self.rx_frac[e], finite[e, k]) for k in range(self.K)]
                                 for e in range(self.E)])
        self.want_used = self.want_ok & np.vectorize(fd.weight_counts)(weights)
        self.garbage = sorted({e for label, e, _ in entries if label in GARBAGE})  # epochs whose count the text leaves open

    def args(self, weights=True):
        return self.ephs, self.code_frac, self.rx_ms, self.rx_frac, self.prior, (self.weights if weights else None)


class Scene:
    """K; calm: the snapshot receivers of the calm tile (the designated channels measure nothing); tiles; clean, hostile; ref: the
    restatement's result of every clean epoch of the calm tile {epoch: dict}, computed once, never changed; chans: the designated
    channels; truth_xyz, truth_bias_s, offset_ms of the calm tile"""


def _snap(case: fc.Case) -> sc.SnapCase:
    return sc.SnapCase(case, check=False)


@functools.lru_cache(maxsize=None)
def hostile(K: int) -> Scene:
    fix_tiles = fd.hostile(K, 4)
    s = Scene()
    s.K, s.clean, s.hostile = K, fix_tiles[0].clean, fix_tiles[0].hostile
    calm_case = fix_tiles[0].calm
    s.calm = _snap(calm_case)
    s.ref = {e: sr.snapshot(s.calm.ephs, s.calm.code_frac[e], s.calm.rx_ms[e], s.calm.rx_frac[e], s.calm.prior[e]) for e in s.clean}
    assert all(r["worst"] < 0.4 and not r["reresolved"] for r in s.ref.values()), [r["worst"] for r in s.ref.values()]
    finite_of = carried_over()
    tiles = []
    for t in fix_tiles:
        assert t.calm is calm_case
        finite = np.ones((t.E, t.K), bool)
        for label, e, k in t.entries:
            finite[e, k] = finite_of[label]
        tiles.append(Tile(_snap(t.case), t.weights, t.clean, t.hostile, finite, list(t.entries)))
    base = fd.base_case(K).tiled(calm_case.E)
    s.chans = fd.designated(base, s.clean, 16 if K == 64 else K // 3)  # fix_domain's: they measure nothing in the calm tile
    assert (calm_case.tx_ms[:, s.chans] < 0).all()
    good_frac = fd.all_transmit_times(base)[1]
    ones, every = np.ones((s.calm.E, K)), np.ones((s.calm.E, K), bool)
    # code_frac: a designated channel an entry, in every hostile epoch
    per_epoch = [code_frac_entries(s.calm.rx_frac[e]) for e in s.hostile]
    for first in range(0, len(per_epoch[0]), len(s.chans)):
        c = _snap(calm_case)
        entries = []
        for k, i in zip(s.chans, range(first, len(per_epoch[0]))):
            for e, ens in zip(s.hostile, per_epoch):
                c.code_frac[e, k] = ens[i][1]
                entries.append((ens[i][0], e, int(k)))
        tiles.append(Tile(c, ones, s.clean, s.hostile, every, entries))
    # rx_ms is the epoch's: tiles of their own, the designated channels good ones
    for first in range(0, len(RX_MS_ENTRIES), len(s.hostile)):
        c = _snap(calm_case)
        entries = []
        for e, (label, value) in zip(s.hostile, RX_MS_ENTRIES[first:first + len(s.hostile)]):
            c.code_frac[e, s.chans] = good_frac[e, s.chans]
            c.rx_ms[e] = value
            entries += [(label, e, k) for k in range(K)]
        tiles.append(Tile(c, ones, s.clean, s.hostile, every, entries))
    for t in tiles:  # a clean epoch is the calm tile's, to the byte
        for e in s.clean:
            for name in ("code_frac", "rx_ms", "rx_frac", "prior"):
                assert getattr(t, name)[e].tobytes() == getattr(s.calm, name)[e].tobytes(), name
            assert (t.weights[e] == 1.0).all()
    covered = {label for t in tiles for label, _, _ in t.entries}
    assert covered == set(finite_of) | {en[0] for en in code_frac_entries(0.5e-3)} | {en[0] for en in RX_MS_ENTRIES}
    s.tiles = tuple(tiles)
    s.truth_xyz, s.truth_bias_s, s.offset_ms = s.calm.truth_xyz, s.calm.truth_bias_s, s.calm.offset_ms
    return s


# ---- hostile priors ---------------------------------------------------------------------------------------------------------------------
def prior_entries(s: Scene):
    """(label, value of the coordinate or the whole prior, refused as init_xyz).  1e200: the squared distance overflows, no predicted
    range is finite, no channel counts (gat.h, usable): FEW_SATS, before any whole millisecond is formed.  1e12: a travel time of
    3336 s, every satellite a finite state that long before the reception, every channel counts, and the reference's range is 3.3e6
    whole milliseconds, beyond kSnapMaxMs in snap_reference: NONFINITE.  The centre: every sin el is 0, the reference is the lowest
    used channel."""
    out = [(f"{'xyz'[i]}={name}", (i, v), True) for i in range(3) for name, v in (("nan", np.nan), ("+inf", np.inf), ("-inf", -np.inf))]
    out += [("x=1e200", (0, 1e200), False), ("x=1e12", (0, 1e12), False), ("centre", (0.0, 0.0, 0.0), False)]
    return out


def on_a_satellite(s: Scene, e: int):
    """(channel, xyz): the position of the highest satellite of epoch e of the calm tile at the reception's reading R, as the fix's
    rule evaluates it (the twin's ``sat`` output for a transmission at R): the snapshot fix's third evaluation is at R - r / c with r
    / c below the reading's resolution.  The last range is zero or a rounding of the coordinates: defined either way."""
    g = lib()
    k = int(np.argmax(np.where(np.isfinite(s.calm.code_frac[e]), s.calm.case.sin_el[e], -1.0)))
    one = g.position_fix_host(s.calm.ephs, np.broadcast_to(s.calm.rx_ms[e], (1, s.K)).copy(), np.broadcast_to(s.calm.rx_frac[e], (1, s.K)).copy(),
                              s.calm.rx_ms[e:e + 1], s.calm.rx_frac[e:e + 1])
    return k, tuple(float(v) for v in one.sat[0, k, :3])


# ---- what gat.h gives a result: asserted on the twin's and on the device's alike -------------------------------------------------------------
RECORD_ONLY = ("status", "num_valid", "num_used", "iterations")


def check_classification(S, f, t, weighted: bool):
    """num_valid, num_used, used and tx_ms == -1 of one tile's result are what ``usable`` says, entry by entry"""
    want_used = t.want_used if weighted else t.want_ok
    failed = (f.status & FAILED) != 0
    for e in t.garbage:  # times beyond the sine's range: the text leaves open which channels count; the epoch ends at kSnapMaxMs
        assert f.status[e] in (S.NONFINITE, S.FEW_SATS) and f.num_valid[e] <= t.want_ok[e].sum() and f.num_used[e] <= want_used[e].sum()
        assert (f.status[e] == S.FEW_SATS) == (f.num_used[e] < 5)
    told = np.setdiff1d(np.arange(t.E), t.garbage)
    for label, e, k in t.entries:
        assert (f.tx_ms[e, k] != -1) == (t.want_ok[e, k] and not failed[e]), (label, e, k)
        assert (f.used[e, k] != 0) == (want_used[e, k] and not failed[e]), (label, e, k)
    assert (f.num_valid == t.want_ok.sum(axis=1))[told].all(), (f.num_valid, t.want_ok.sum(axis=1))
    assert (f.num_used == want_used.sum(axis=1))[told].all(), (f.num_used, want_used.sum(axis=1))
    assert np.array_equal(f.tx_ms[~failed] != -1, t.want_ok[~failed]) and (f.tx_ms[failed] == -1).all() and (f.rx_ms_out[failed] == -1).all()
    assert np.array_equal(f.used[~failed] != 0, want_used[~failed]) and not f.used[failed].any()
    assert ((f.status & S.FEW_SATS) != 0)[told].tolist() == (want_used.sum(axis=1) < 5)[told].tolist()  # gat.h: fewer than 5 used channels
    for name in ("resid", "sin_el"):
        assert np.isfinite(getattr(f, name)).all(), name
    for e in np.flatnonzero(failed):  # every output zero but status, num_valid, num_used and iterations
        assert all(f.fixes[e][n] == 0 for n in f.fixes.dtype.names if n not in RECORD_ONLY) and not f.n_ms[e].any() and not f.resid[e].any()


def check_prior(S, f, calm, epochs, label, on_k):
    """the result of epochs whose prior is the entry `label`"""
    for e in epochs:
        if label.endswith(("nan", "inf")) or label == "x=1e200":  # no predicted range is finite: no channel counts
            assert f.status[e] == S.FEW_SATS and f.num_valid[e] == 0 and (f.tx_ms[e] == -1).all() and not f.xyz[e].any(), (label, e, f.fixes[e])
        elif label == "x=1e12":  # every channel counts; the reference's range is no number of milliseconds (kSnapMaxMs)
            assert f.status[e] == S.NONFINITE and f.num_valid[e] == calm.num_valid[e] and f.iterations[e] == 0, (label, e, f.fixes[e])
            assert (f.tx_ms[e] == -1).all() and f.rx_ms_out[e] == -1 and not f.xyz[e].any()
        elif label == "centre":  # every channel counts, every sin el of the resolution is 0; whatever the solve makes of 6371 km
            assert f.num_valid[e] == calm.num_valid[e], (label, e)
        else:  # the satellite's own channel has a range of zero or of a rounding: it counts or it does not, no other is touched
            assert f.num_valid[e] in (calm.num_valid[e], calm.num_valid[e] - 1), (label, e, f.num_valid[e], calm.num_valid[e])


# ---- all 64 lanes ---------------------------------------------------------------------------------------------------------------------
class Wide:
    """snap: the SnapCase (E = 5, K = 64: channel k carries satellite k mod 12); ref: the restatement per epoch; k0: its reference
    channel per epoch"""


@functools.lru_cache(maxsize=None)
def full_width() -> Wide:
    base = fc.case("short", 30, 12, 8).tiled(5)
    assert (base.tx_ms >= 0).all()
    idx = np.arange(64) % 12
    c = base.copy()
    c.ephs = base.ephs[idx]
    for name in ("tx_ms", "tx_frac", "sin_el"):
        setattr(c, name, np.ascontiguousarray(getattr(base, name)[:, idx]))
    c.K = 64
    w = Wide()
    w.snap = _snap(c)
    w.ref = [sr.snapshot(c.ephs, w.snap.code_frac[e], w.snap.rx_ms[e], w.snap.rx_frac[e], w.snap.prior[e]) for e in range(c.E)]
    assert all(r["worst"] < 0.4 and not r["reresolved"] and r["use"].all() for r in w.ref)
    # the restatement's reference: argmax takes the lowest channel of the tie
    w.k0 = []
    for e in range(c.E):
        _, sin_el = sr.predicted(c.ephs, w.snap.prior[e], 0.0, 0.0, int(w.snap.rx_ms[e]) * sr.MS + w.snap.rx_frac[e])
        k0 = int(np.argmax(sin_el))
        assert k0 < 12 and (sin_el[k0::12] == sin_el[k0]).all() and (np.delete(sin_el[:12], k0) < sin_el[k0]).all()  # a tie of five or six
        w.k0.append(k0)
        # the case solves to the truth, by the restatement alone
        r = w.ref[e]
        assert np.linalg.norm(r["xyz"] - c.truth_xyz[e]) < 1e-4 and np.array_equal(r["tx_ms"], c.tx_ms[e])
    return w


# ---- every status bit's path --------------------------------------------------------------------------------------------------------------
class Paths:
    """snap: nine epochs of twelve channels at one site, all seen; prior, weights: the call's (epoch `again` has a prior that is
    resolved again, `five` and `four` weights that leave so many used); plain: the twin's result of the default call; e_c, mask_c,
    e_d, mask_d: an epoch and the mask half-way between its 5th and 6th (4th and 5th) highest sin el; mask_e: the mask between the
    lowest and the second lowest sin el of epoch `again`; tol_first: a tol_m the first step of every epoch passes"""

    def args(self):
        return self.snap.ephs, self.snap.code_frac, self.snap.rx_ms, self.snap.rx_frac, self.prior, self.weights


def _between(sin_el, used, n: int) -> float:
    """half-way between the n-th and the (n + 1)-th highest sin el of the used channels, at least 1e-3 apart"""
    v = np.sort(sin_el[used != 0])[::-1]
    assert v[n - 1] - v[n] >= 1e-3, (v[n - 1], v[n])
    return float((v[n - 1] + v[n]) / 2)


@functools.lru_cache(maxsize=None)
def status_paths() -> Paths:
    g = lib()
    S = g.snapshot
    p = Paths()
    p.snap = _snap(fc.case("short", 30, 12, 8).tiled(9))
    c = p.snap
    assert c.seen.all() and c.K == 12 and c.E == 9
    p.again, p.five, p.four = 5, 6, 3  # inside the full workgroups (epochs 0 .. 3 and 4 .. 7)
    p.prior, p.weights = c.prior.copy(), np.ones((c.E, c.K))
    # (e) the nearest prior along the case's own direction whose integers the twin resolves again
    e = p.again
    d = (c.prior[e] - c.truth_xyz[e]) / np.linalg.norm(c.prior[e] - c.truth_xyz[e])
    for km in range(100, 400, 5):
        p.prior[e] = c.truth_xyz[e] + d * km * 1e3
        one = g.snapshot_fix_host(c.ephs, c.code_frac[e:e + 1], c.rx_ms[e:e + 1], c.rx_frac[e:e + 1], p.prior[e:e + 1])
        if one.status[0] & S.RERESOLVED and not one.status[0] & FAILED:
            break
    else:
        raise AssertionError("no prior along the direction is resolved again")
    assert sr.snapshot(c.ephs, c.code_frac[e], c.rx_ms[e], c.rx_frac[e], p.prior[e])["reresolved"]  # the restatement agrees
    # (f) five and four used of twelve valid: spread over the sky, the highest and the lowest among them
    order = np.argsort(-c.case.sin_el, axis=1)
    p.weights[p.five] = 0.0
    p.weights[p.five, order[p.five, [0, 3, 6, 9, 11]]] = 1.0
    p.weights[p.four] = 0.0
    p.weights[p.four, order[p.four, [0, 3, 6, 11]]] = 1.0
    p.plain = g.snapshot_fix_host(*p.args())
    ordinary = [e for e in range(c.E) if e not in (p.again, p.five, p.four)]
    assert (p.plain.status[ordinary] == 0).all() and (p.plain.num_used[ordinary] == 12).all()
    # (c), (d): masks from the twin's sin el at the solved state of two ordinary epochs
    p.e_c, p.e_d = ordinary[1], ordinary[2]
    p.mask_c = _between(p.plain.sin_el[p.e_c], p.plain.used[p.e_c], 5)
    p.mask_d = _between(p.plain.sin_el[p.e_d], p.plain.used[p.e_d], 4)
    p.mask_e = _between(p.plain.sin_el[p.again], p.plain.used[p.again], 11)
    # (b) a tol_m the first step passes: the prior is 30 km off at most (epoch `again` some hundred), the first step that long
    p.tol_first = 1e7
    return p
