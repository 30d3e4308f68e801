"""The host twin gat_snapshot_fix_host over the whole domain gat.h admits (tests/snap_domain.py): every hostile entry classified as
``usable`` -- restated from the text of gat.h -- says, with no clean epoch disturbed; hostile priors; all 64 channels used with the
reference on a tie; and every status bit's path with exactly the result its paragraph of gat.h gives.  Needs no device.

Bounds.  The derivation is that of tests/test_snapshot_host.py with its fixed dilution replaced by each epoch's
own: the twin and the restatement disagree by under e_v = 5e-7 m per range; a disagreement of e_v per range moves the solution by
at most e_v times the dilution of the five-unknown system, so with the margin of 4 position and clock bias are held to 5e-7 m x the
restatement's gdop of that epoch x 4 (the bias over c) and the coarse time to 5e-7 m x the restatement's tdop x 4; n_ms, tx_ms and
rx_ms_out are exact.  Measured over the clean epochs of both scenes and the full-width case (printed by the tests): position at most
4.4e-8 m against bounds from 1.3e-6 m, bias 1.3e-16 s against 4.2e-15 s, coarse time 9.2e-11 s against 7.4e-10 s."""
import numpy as np
import pytest

from tests import snap_domain as sd
from tests import snap_ref as sr

RECORD_ONLY, check_classification, check_prior = sd.RECORD_ONLY, sd.check_classification, sd.check_prior


@pytest.fixture(scope="module")
def g():
    import gpuacceleratedtracking_amd as g
    return g


def keeps_its_bytes(f, calm, epochs, what):
    for e in epochs:
        assert f.fixes[e].tobytes() == calm.fixes[e].tobytes(), (what, e)
        for name in sd.OUTPUTS:
            assert getattr(f, name)[e].tobytes() == getattr(calm, name)[e].tobytes(), (what, e, name)


@pytest.mark.parametrize("K", [64, 12])
def test_hostile_entries_are_classified_and_disturb_no_clean_epoch(g, K):
    S, s = g.snapshot, sd.hostile(K)
    calm = g.snapshot_fix_host(*s.calm.args())
    clean = list(s.clean)
    assert (calm.status[clean] == 0).all() and np.linalg.norm(calm.xyz[clean] - s.truth_xyz[clean], axis=1).max() < 1e-3  # not vacuous
    labels = set()
    for t in s.tiles:
        for weighted in (True, False):
            f = g.snapshot_fix_host(*t.args(weighted))
            check_classification(S, f, t, weighted)
            keeps_its_bytes(f, calm, clean, sorted({en[0] for en in t.entries}))
        labels |= {label for label, _, _ in t.entries}
        print(f"K = {K}: hostile epochs {t.hostile}: status {f.status[list(t.hostile)].tolist()}, valid {f.num_valid[list(t.hostile)].tolist()}: "
              + ", ".join(sorted({label for label, _, _ in t.entries}))[:150])
    assert len(labels) == 78 + 24 + 7 + 5 + 6


def compare_with_restatement(s, r):
    """one epoch of a result against the restatement's: (position, bias, coarse time) differences over their bounds"""
    bound_m, bound_tc = sd.E_RANGE_M * r["gdop"] * sd.MARGIN, sd.E_RANGE_M * r["tdop"] * sd.MARGIN
    pos = float(np.linalg.norm(s["xyz"] - r["xyz"]))
    bias, tc = abs(s["clock_bias_s"] - r["clock_bias_s"]), abs(s["coarse_time_s"] - r["coarse_time_s"])
    assert pos < bound_m and bias < bound_m / sr.C and tc < bound_tc, (pos, bound_m, bias, bound_m / sr.C, tc, bound_tc)
    assert np.array_equal(s["n_ms"], r["n"]) and np.array_equal(s["tx_ms"], r["tx_ms"]) and s["rx_ms_out"] == r["rx_ms_out"]
    assert np.array_equal(s["used"] != 0, r["use"])
    return (pos, bound_m), (bias, bound_m / sr.C), (tc, bound_tc)


def epoch_of(f, e):
    return {"xyz": f.xyz[e], "clock_bias_s": f.clock_bias_s[e], "coarse_time_s": f.coarse_time_s[e], "n_ms": f.n_ms[e], "tx_ms": f.tx_ms[e],
            "rx_ms_out": f.rx_ms_out[e], "used": f.used[e]}


def report(what, rows):
    worst = [max(r[i][0] for r in rows) for i in range(3)]
    least = [min(r[i][1] for r in rows) for i in range(3)]
    print(f"{what}: twin - restatement at most {worst[0]:.3g} m, {worst[1]:.3g} s, t_c {worst[2]:.3g} s; the smallest bounds {least[0]:.3g} m, "
          f"{least[1]:.3g} s, {least[2]:.3g} s")


@pytest.mark.parametrize("K", [64, 12])
def test_clean_epochs_equal_the_restatement_within_their_own_bound(g, K):
    s = sd.hostile(K)
    f = g.snapshot_fix_host(*s.calm.args(), **sd.CONVERGED)
    assert (f.status[list(s.clean)] == 0).all()
    report(f"K = {K}, clean epochs", [compare_with_restatement(epoch_of(f, e), s.ref[e]) for e in s.clean])
    # every tile's clean epochs have these bytes: the tiles under this configuration as well
    for t in s.tiles[::5]:
        keeps_its_bytes(g.snapshot_fix_host(*t.args(), **sd.CONVERGED), f, s.clean, "converged")


def test_hostile_priors(g):
    S = g.snapshot
    for K in (64, 12):
        s = sd.hostile(K)
        calm = g.snapshot_fix_host(*s.calm.args())
        on_k, on_xyz = sd.on_a_satellite(s, s.hostile[0])
        entries = sd.prior_entries(s) + [("on a satellite", on_xyz, False)]
        for label, value, refused in entries:
            prior = s.calm.prior.copy()
            for e in s.hostile:
                if len(value) == 2:
                    prior[e, value[0]] = value[1]
                else:
                    prior[e] = value
            f = g.snapshot_fix_host(s.calm.ephs, s.calm.code_frac, s.calm.rx_ms, s.calm.rx_frac, prior)
            keeps_its_bytes(f, calm, s.clean, label)
            check_prior(S, f, calm, s.hostile[:1] if label == "on a satellite" else s.hostile, label, on_k)
            if refused:
                continue
            xyz = tuple(s.calm.prior[0]) if len(value) == 2 else value
            if len(value) == 2:
                xyz = xyz[:value[0]] + (value[1],) + xyz[value[0] + 1:]
            whole = g.snapshot_fix_host(s.calm.ephs, s.calm.code_frac, s.calm.rx_ms, s.calm.rx_frac, init_xyz=xyz)
            same = g.snapshot_fix_host(s.calm.ephs, s.calm.code_frac, s.calm.rx_ms, s.calm.rx_frac, np.tile(np.array(xyz), (s.calm.E, 1)))
            assert whole.fixes.tobytes() == same.fixes.tobytes(), label
            if label != "on a satellite":
                check_prior(S, whole, calm, range(s.calm.E), label, on_k)


def test_all_64_channels_used_and_the_reference_on_a_tie(g):
    w = sd.full_width()
    c = w.snap
    f = g.snapshot_fix_host(*c.args(), **sd.CONVERGED)
    assert (f.status == 0).all() and (f.num_used == 64).all() and (f.num_valid == 64).all() and f.used.all()
    report("full width", [compare_with_restatement(epoch_of(f, e), w.ref[e]) for e in range(c.E)])
    assert np.linalg.norm(f.xyz - c.truth_xyz, axis=1).max() < sd.CONVERGED["tol_m"] + 1e-5 and np.array_equal(f.tx_ms, c.case.tx_ms)
    assert all(k0 < 12 for k0 in w.k0)  # the restatement's reference: the lowest channel of the tie (asserted where the case is built)


def test_status_paths(g):
    S, p = g.snapshot, sd.status_paths()
    c, plain = p.snap, p.plain
    ok = [e for e in range(c.E) if e != p.four]
    # (f) five used of twelve valid: a fix; four: FEW_SATS with a zero record and no time
    assert plain.status[p.five] == 0 and plain.num_used[p.five] == 5 and plain.num_valid[p.five] == 12 and plain.used[p.five].sum() == 5
    assert plain.status[p.four] == S.FEW_SATS and plain.num_used[p.four] == 4 and plain.num_valid[p.four] == 12
    zero = plain.fixes[p.four]
    assert all(zero[n] == 0 for n in zero.dtype.names if n not in RECORD_ONLY) and (plain.tx_ms[p.four] == -1).all() and plain.rx_ms_out[p.four] == -1
    assert plain.status[p.again] & S.RERESOLVED and not plain.status[p.again] & (S.MASKED | sd.FAILED)
    # (a) one iteration at a tolerance no first step passes: with and without a mask
    for mask in (-1.0, p.mask_c):  # a mask that would leave five of twelve
        a = g.snapshot_fix_host(*p.args(), max_iter=1, tol_m=1e-6, mask_sin=mask)
        assert (a.status[ok] & ~S.AMBIGUOUS == S.NOT_CONVERGED).all() and (a.iterations[ok] == 1).all() and a.status[p.four] == S.FEW_SATS  # the far prior's margin
        assert a.xyz[ok].all() and (a.last_step_m[ok] > 1e-6).all() and (a.gdop[ok] > 0).all()  # a written record
        assert (a.tx_ms[ok] >= 0).all() and (a.rx_ms_out[ok] >= 0).all() and (a.num_used[ok] == plain.num_used[ok]).all()  # times, no mask
    # (b) one iteration at a tolerance the first step passes: converged, the integers looked at again
    b = g.snapshot_fix_host(*p.args(), max_iter=1, tol_m=p.tol_first)
    assert (b.status[ok] & ~(S.AMBIGUOUS | S.RERESOLVED) == 0).all() and (b.last_step_m[ok] < p.tol_first).all()
    assert (b.iterations[ok] == np.where(b.status[ok] & S.RERESOLVED, 2, 1)).all()
    # (c) five kept
    m = g.snapshot_fix_host(*p.args(), mask_sin=p.mask_c)
    assert m.status[p.e_c] == S.MASKED and m.num_used[p.e_c] == 5 and m.used[p.e_c].sum() == 5 and m.num_valid[p.e_c] == 12
    assert ((m.used[p.e_c] != 0) == (plain.sin_el[p.e_c] >= p.mask_c)).all()
    # (d) four would be kept: the record of the unmasked call with the one bit added
    m = g.snapshot_fix_host(*p.args(), mask_sin=p.mask_d)
    want = plain.fixes[p.e_d].copy()
    want["status"] |= S.MASK_STARVED
    assert m.fixes[p.e_d].tobytes() == want.tobytes() and m.used[p.e_d].tobytes() == plain.used[p.e_d].tobytes() and m.status[p.e_d] == S.MASK_STARVED
    for name in sd.OUTPUTS:
        assert getattr(m, name)[p.e_d].tobytes() == getattr(plain, name)[p.e_d].tobytes(), name
    # (e) resolved again and masked in one epoch
    m = g.snapshot_fix_host(*p.args(), mask_sin=p.mask_e)
    assert m.status[p.again] & S.RERESOLVED and m.status[p.again] & S.MASKED and m.num_used[p.again] == 11
    # (g) the margins
    assert (g.snapshot_fix_host(*p.args(), ambiguity_margin=0.0).status[ok] & S.AMBIGUOUS == 0).all()
    assert (g.snapshot_fix_host(*p.args(), ambiguity_margin=0.5).status[ok] & S.AMBIGUOUS != 0).all()  # every |q - n| > 0
