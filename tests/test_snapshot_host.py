"""The snapshot fix on the host: the host twin gat_snapshot_fix_host against the independent numpy restatement (tests/snap_ref.py),
against the truth the cases (tests/snap_cases.py) were built from, its integers and the times it hands on, the far prior, the special
epochs, every refusal and a tracked channel without a time of week.  Needs no device.

Bounds.  What the twin and the restatement disagree on per range, e_v: the satellite's state, under 3e-7 m
(tests/test_position_host.py); the satellite's own time held in seconds of the week, half an ulp of 6e5 s = 5.8e-11 s in each of
the two, at a range rate under 930 m/s: 1.1e-7 m; the rounding of rho, r and their difference near 2.5e7 m, 3 x 3.7e-9 m: together
under 5e-7 m.  A disagreement of e_v per range moves the solution by at most e_v times the dilution of the five-unknown system, which
over the cases is gdop <= 2.6 (x, y, z, b) and tdop <= 2.5e-3 s/m; with a margin of 4 the tolerances are 5e-7 x 2.6 x 4 < 1e-5 m,
5e-7 x 2.6 x 4 / c < 2e-14 s and 5e-7 x 2.5e-3 x 4 = 5e-9 s for t_c.  Measured: 4.3e-8 m, 8.7e-17 s, 7.7e-11 s.  Against the truth
(tol_m = 1e-6): tol_m more; measured 7.9e-8 m, 1.8e-16 s, 5.2e-11 s."""
import ctypes as C

import numpy as np
import pytest

from tests import fix_cases as fc
from tests import snap_cases as sc
from tests import snap_ref as sr

CONVERGED = dict(tol_m=1e-6, max_iter=12)
TOL_M, TOL_BIAS_S, TOL_TC_S = 1e-5, 2e-14, 5e-9
MAX_GDOP, MAX_TDOP = 2.6, 2.5e-3


@pytest.fixture(scope="module")
def g():
    import gpuacceleratedtracking_amd as g
    return g


@pytest.fixture(scope="module", params=sc.ALL)
def solved(request, g):
    c = sc.case(request.param)
    return c, g.snapshot_fix_host(*c.args(), **CONVERGED)


def test_twin_equals_the_restatement_within_the_derived_bound(solved):
    c, s = solved
    assert (s.status == 0).all() and (s.num_used == c.seen.sum(axis=1)).all() and (s.num_valid == s.num_used).all()
    assert s.gdop.max() <= MAX_GDOP and s.tdop.max() <= MAX_TDOP  # the conditioning the tolerances were derived for
    pos = max(np.linalg.norm(s.xyz[e] - c.ref[e]["xyz"]) for e in range(c.E))
    bias = max(abs(s.clock_bias_s[e] - c.ref[e]["clock_bias_s"]) for e in range(c.E))
    tc = max(abs(s.coarse_time_s[e] - c.ref[e]["coarse_time_s"]) for e in range(c.E))
    print(f"twin - restatement: {pos:.3g} m, {bias:.3g} s, t_c {tc:.3g} s")
    assert pos < TOL_M and bias < TOL_BIAS_S and tc < TOL_TC_S
    for e in range(c.E):
        r = c.ref[e]
        assert np.abs(s.resid[e] - r["resid"])[c.seen[e]].max() < TOL_M
        # the dilutions: the restatement's coarse-time column is a difference quotient (1e-6 m/s of 1e3)
        assert abs(s.pdop[e] / r["pdop"] - 1) < 1e-5 and abs(s.gdop[e] / r["gdop"] - 1) < 1e-5 and abs(s.tdop[e] / r["tdop"] - 1) < 1e-5


def test_twin_finds_the_truth(solved):
    c, s = solved
    j = sc.whole_ms_of(s.clock_bias_s, c.truth_bias_s)
    pos = np.linalg.norm(s.xyz - c.truth_xyz, axis=1).max()
    bias = np.abs(s.clock_bias_s - c.truth_bias_s - j * 1e-3).max()
    tc = np.abs(s.coarse_time_s - (c.offset_ms - j) * 1e-3).max()
    print(f"twin - truth: {pos:.3g} m, {bias:.3g} s, t_c {tc:.3g} s")
    assert pos < CONVERGED["tol_m"] + TOL_M and bias < CONVERGED["tol_m"] / sr.C + TOL_BIAS_S and tc < TOL_TC_S
    assert (np.abs(j) <= 1).all()
    assert s.rms_residual_m.max() < TOL_M and (s.last_step_m < CONVERGED["tol_m"]).all()


def test_integers_and_times_are_the_restatements_exactly(solved):
    c, s = solved
    for e in range(c.E):
        r = c.ref[e]
        assert np.array_equal(s.n_ms[e], r["n"]) and np.array_equal(s.tx_ms[e], r["tx_ms"]) and s.rx_ms_out[e] == r["rx_ms_out"]
        assert np.array_equal(s.used[e] != 0, r["use"])
    # and the case's own: the transmit times gat_observables would have written with a decoded time of week
    assert np.array_equal(s.tx_ms, c.case.tx_ms) and np.array_equal(s.rx_ms_out, c.case.rx_ms)
    assert np.array_equal(s.n_ms != 0, c.seen) and (s.sin_el[c.seen] > 0).all() and not s.sin_el[~c.seen].any()


def test_position_fix_takes_the_times_as_they_are(g, solved):
    c, s = solved
    frac = np.where(c.seen, c.code_frac, 0.0)
    fix = g.position_fix_host(c.ephs, s.tx_ms, frac, s.rx_ms_out, c.rx_frac, init_xyz=tuple(c.prior[0]), **CONVERGED)
    assert (fix.status == 0).all() and (fix.num_used == s.num_used).all()
    assert np.linalg.norm(fix.xyz - s.xyz, axis=1).max() < TOL_M
    j = sc.whole_ms_of(s.clock_bias_s, fix.clock_bias_s)  # the fix's clock error is the snapshot's modulo the milliseconds it gave to m
    assert np.abs(s.clock_bias_s - fix.clock_bias_s - j * 1e-3).max() < TOL_BIAS_S


def test_without_prior_xyz_every_epoch_starts_at_init_xyz(g):
    c = sc.case("short", 30, 12, 8)
    a = g.snapshot_fix_host(c.ephs, c.code_frac, c.rx_ms, c.rx_frac, np.tile(c.prior[0], (c.E, 1)))
    b = g.snapshot_fix_host(c.ephs, c.code_frac, c.rx_ms, c.rx_frac, init_xyz=tuple(c.prior[0]))
    assert a.fixes.tobytes() == b.fixes.tobytes() and (a.status == 0).all()


def test_a_prior_200_km_off_is_never_silently_wrong(g):
    """Beyond the condition of tests/snap_cases.py the integers may be wrong; then the fix is off by tens of kilometres, and the
    status says so: judged against the restatement's own margins of each epoch."""
    far = sc.SnapCase(fc.case("mid"), seed=33, prior_m=200.0e3, check=False)
    d = far.prior - far.truth_xyz
    far.prior = far.truth_xyz + d / np.linalg.norm(d, axis=1)[:, None] * 200.0e3
    s = g.snapshot_fix_host(*far.args(), **CONVERGED)
    flagged = 0
    for e in range(far.E):
        r = sr.snapshot(far.ephs, far.code_frac[e], far.rx_ms[e], far.rx_frac[e], far.prior[e])
        if abs(r["worst"] - 0.4) > 1e-9:  # not on the margin itself
            assert bool(s.status[e] & g.snapshot.AMBIGUOUS) == r["ambiguous"], (e, r["worst"], s.status[e])
        wrong = np.linalg.norm(s.xyz[e] - far.truth_xyz[e]) > 1.0
        assert not wrong or s.status[e] & (g.snapshot.AMBIGUOUS | g.snapshot.RERESOLVED), (e, s.status[e])
        assert wrong or np.array_equal(s.tx_ms[e], far.case.tx_ms[e])
        flagged += bool(s.status[e] & (g.snapshot.AMBIGUOUS | g.snapshot.RERESOLVED))
    assert flagged > 0


def test_a_wrong_integer_is_resolved_again(g):
    """a prior far enough for one channel's integer to come out wrong by one, near enough for the solve to land where the second
    resolution sees it: found by walking the prior away from the truth"""
    c = sc.case("mid")
    e = 0
    d = c.prior[e] - c.truth_xyz[e]
    d /= np.linalg.norm(d)
    seen = 0
    for km in range(100, 200, 5):
        prior = c.truth_xyz[e] + d * km * 1e3
        s = g.snapshot_fix_host(c.ephs, c.code_frac[e:e + 1], c.rx_ms[e:e + 1], c.rx_frac[e:e + 1], prior[None], **CONVERGED)
        r = sr.snapshot(c.ephs, c.code_frac[e], c.rx_ms[e], c.rx_frac[e], prior)
        if s.status[0] & g.snapshot.RERESOLVED:
            seen += 1
            assert r["reresolved"] and np.array_equal(s.n_ms[0], r["n"])
            if np.array_equal(s.tx_ms[0], c.case.tx_ms[e]):
                assert np.linalg.norm(s.xyz[0] - c.truth_xyz[e]) < CONVERGED["tol_m"] + TOL_M
    print("re-resolved priors:", seen)
    assert seen > 0


def test_special_epochs(g):
    c = sc.case("short", 30, 12, 8)
    S = g.snapshot
    order = np.argsort(-c.case.sin_el, axis=1)
    frac, w = c.code_frac.copy(), np.ones(c.code_frac.shape)
    frac[1, order[1, 4:]] = np.nan          # four measurements
    w[2, order[2, 4:]] = 0.0                # enough measurements, four weights
    w[2, order[2, 5]] = np.nan
    frac[3, 5] = np.nan                     # costs one channel only
    frac[4, 6] = 1e-3                       # outside [0, 1e-3)
    frac[5, 7] = -1e-9
    s = g.snapshot_fix_host(c.ephs, frac, c.rx_ms, c.rx_frac, c.prior, w, **CONVERGED)
    clean = g.snapshot_fix_host(*c.args(), **CONVERGED)
    assert s.status.tolist() == [0, S.FEW_SATS, S.FEW_SATS, 0, 0, 0, 0, 0]
    assert s.num_valid.tolist() == [12, 4, 12, 11, 11, 11, 12, 12] and s.num_used.tolist() == [12, 4, 4, 11, 11, 11, 12, 12]
    for e in (1, 2):
        f = s.fixes[e]
        assert all(f[n] == 0 for n in f.dtype.names if n not in ("status", "num_valid", "num_used", "iterations"))
        assert (s.tx_ms[e] == -1).all() and s.rx_ms_out[e] == -1 and not s.n_ms[e].any() and not s.resid[e].any() and not s.used[e].any()
    for e, k in ((3, 5), (4, 6), (5, 7)):
        assert s.tx_ms[e, k] == -1 and s.used[e, k] == 0 and s.n_ms[e, k] == 0
        keep = np.arange(c.K) != k
        assert np.array_equal(s.tx_ms[e, keep], c.case.tx_ms[e, keep])
        assert np.linalg.norm(s.xyz[e] - c.truth_xyz[e]) < CONVERGED["tol_m"] + TOL_M
    for e in (0, 6, 7):  # one epoch never touches another
        assert s.fixes[e].tobytes() == clean.fixes[e].tobytes()


def test_two_identical_satellites_among_five_are_singular(g):
    e = 3
    base = fc.twinned(fc.case("short", 30, 12, 8), e)
    c = sc.SnapCase(base, check=False)
    order = np.argsort(-base.sin_el[e])
    assert np.array_equal(c.ephs[order[0]], c.ephs[order[1]])
    frac = c.code_frac.copy()
    frac[e, order[5:]] = np.nan
    s = g.snapshot_fix_host(c.ephs, frac, c.rx_ms, c.rx_frac, c.prior, **CONVERGED)
    assert s.status[e] == g.snapshot.SINGULAR and s.num_used[e] == 5 and not s.xyz[e].any() and (s.tx_ms[e] == -1).all()
    assert (np.delete(s.status, e) == 0).all()


def test_mask_and_weights(g):
    c = sc.case("mid")
    mask = float(np.sin(np.radians(15.0)))
    s = g.snapshot_fix_host(*c.args(), mask_sin=mask, **CONVERGED)
    low = c.seen & (c.case.sin_el < mask - 1e-3)
    assert low.any() and ((s.status & g.snapshot.MASKED) != 0).tolist() == low.any(axis=1).tolist()
    assert not (s.used != 0)[low].any() and (s.num_used == (c.seen & ~low).sum(axis=1)).all()
    assert np.linalg.norm(s.xyz - c.truth_xyz, axis=1).max() < CONVERGED["tol_m"] + TOL_M
    assert np.array_equal(s.tx_ms, c.case.tx_ms)  # a masked channel keeps its time
    rng = np.random.default_rng(2)
    w = rng.uniform(0.5, 2.0, c.code_frac.shape)
    sw = g.snapshot_fix_host(*c.args(), w, **CONVERGED)
    assert (sw.status == 0).all() and np.linalg.norm(sw.xyz - c.truth_xyz, axis=1).max() < CONVERGED["tol_m"] + TOL_M


def test_code_noise_moves_the_fix_by_its_dilution(g):
    """one metre of noise on a fraction stays far from the margin: the integers stand, the position moves by metres"""
    c = sc.case("mid")
    rng = np.random.default_rng(8)
    frac = np.mod(c.code_frac + rng.normal(0.0, 1.0, c.code_frac.shape) / sr.C, 1e-3)
    s = g.snapshot_fix_host(c.ephs, frac, c.rx_ms, c.rx_frac, c.prior)
    err = np.linalg.norm(s.xyz - c.truth_xyz, axis=1)
    assert (s.status == 0).all() and (err < 5.0 * s.pdop).all() and err.max() > 0.01
    assert np.abs(s.coarse_time_s - c.offset_ms * 1e-3).max() < 5.0 * s.tdop.max() + 1e-3


def test_every_refusal(g):
    from gpuacceleratedtracking_amd import _lib

    c = sc.case("short", 30, 12, 8)
    lib, S = _lib.load(), g.snapshot
    fixes = np.full(c.E, 7, dtype=np.uint8).repeat(_lib.SNAP_FIX_DTYPE.itemsize)
    before = fixes.copy()
    a = lambda x: None if x is None else x.ctypes.data  # noqa: E731
    ephs = np.ascontiguousarray(c.ephs)
    frac, rx_ms, rx_frac = np.ascontiguousarray(c.code_frac), np.ascontiguousarray(c.rx_ms), np.ascontiguousarray(c.rx_frac)

    def call(cfg, E=c.E, K=c.K, eph=ephs, fr=frac, ms=rx_ms, rf=rx_frac, out=fixes, byref=True):
        return lib.gat_snapshot_fix_host(a(eph), a(fr), a(ms), a(rf), None, None, E, K, C.byref(cfg) if byref else None, a(out), *[None] * 6)

    assert call(S.snap_config()) == 0 and not np.array_equal(fixes, before)
    fixes[:] = before
    ARG, RANGE = 1, 2  # GAT_ERR_ARG, GAT_ERR_RANGE
    good = S.snap_config()
    for kw in (dict(eph=None), dict(fr=None), dict(ms=None), dict(rf=None), dict(out=None), dict(byref=False), dict(E=0), dict(K=0), dict(E=-1)):
        assert call(good, **kw) == ARG, kw
    bad_size = S.snap_config()
    bad_size.struct_size -= 8
    assert call(bad_size) == ARG
    for kw in (dict(max_iter=0), dict(tol_m=0.0), dict(tol_m=float("nan")), dict(mask_sin=float("inf")), dict(init_xyz=(0.0, float("nan"), 0.0)),
               dict(ambiguity_margin=-1e-9), dict(ambiguity_margin=0.5000001), dict(ambiguity_margin=float("nan")), dict(flags=1)):
        assert call(S.snap_config(**kw)) == ARG, kw
    reserved = S.snap_config()
    reserved.reserved = 1
    assert call(reserved) == ARG
    assert call(good, K=_lib.GAT_MAX_FIX_CHANNELS + 1) == RANGE and call(good, E=_lib.GAT_MAX_FIX_EPOCHS + 1) == RANGE
    assert np.array_equal(fixes, before)  # nothing was written
    for margin in (0.0, 0.5):
        assert call(S.snap_config(ambiguity_margin=margin)) == 0
    # the plan refuses what the call refuses, but for the pointers
    assert g.snapshot_plan(9, 12) == {"workgroups": 3, "waves_per_workgroup": 4, "threads": 256, "lds_bytes": 4 * (20 * 65 + 32) * 8, "scratch_bytes": 0}
    for kw in (dict(max_iter=0), dict(ambiguity_margin=0.6), dict(flags=2)):
        with pytest.raises(_lib.GatError):
            g.snapshot_plan(9, 12, **kw)
    with pytest.raises(_lib.GatError):
        g.snapshot_plan(9, 65)
    with pytest.raises(ValueError):
        g.snapshot_fix_host(*c.args(), outputs=("sat",))


def test_margin_zero_and_half(g):
    c = sc.case("mid")
    assert (g.snapshot_fix_host(*c.args(), ambiguity_margin=0.0).status == 0).all()
    assert ((g.snapshot_fix_host(*c.args(), ambiguity_margin=0.5).status & g.snapshot.AMBIGUOUS) != 0).all()  # every |q - n| > 0


def test_tracked_channels_without_a_time_of_week_still_fix(g):
    """An ``Observables`` as a tracking session without a decoded time of week leaves it: every channel GAT_OBS_NO_TOW, tx_ms = -1,
    and the fraction of the transmit time as the loop's code phase gives it.  The position fix has nothing; the snapshot fix takes
    the fractions and the coarse clock, and its times make the position fix work."""
    from gpuacceleratedtracking_amd import _lib
    from gpuacceleratedtracking_amd.observables import NO_TOW, Observables

    c = sc.case("short", 30, 12, 8)
    channels = np.zeros(c.K, dtype=_lib.OBS_CHANNEL_DTYPE)
    channels["status"] = NO_TOW
    obs = Observables({"tx_ms": np.full((c.E, c.K), -1, np.int32), "tx_frac": c.code_frac.copy(), "rx_ms": c.rx_ms, "rx_frac": c.rx_frac,
                       "channels": channels})
    assert not obs.measured.any()
    nothing = g.position_fix_host(c.ephs, obs.tx_ms, obs.tx_frac, obs.rx_ms, obs.rx_frac)
    assert (nothing.status == g.positioning.FEW_SATS).all()
    s = g.snapshot_fix_host(c.ephs, obs.tx_frac, obs.rx_ms, obs.rx_frac, c.prior, **CONVERGED)
    assert (s.status == 0).all() and np.linalg.norm(s.xyz - c.truth_xyz, axis=1).max() < CONVERGED["tol_m"] + TOL_M
    fix = g.position_fix_host(c.ephs, s.tx_ms, obs.tx_frac, s.rx_ms_out, obs.rx_frac, init_xyz=tuple(c.prior[0]), **CONVERGED)
    assert (fix.status == 0).all() and np.linalg.norm(fix.xyz - c.truth_xyz, axis=1).max() < CONVERGED["tol_m"] + TOL_M


def test_code_fractions_of_acquisition_results(g):
    from gpuacceleratedtracking_amd.acquisition import AcquisitionResult

    def result(prn, phase, detected=1):
        return AcquisitionResult(prn=prn, sampling_frequency=20e6, carrier_doppler=0.0, code_phase=phase, CN0=45.0, noise_power=1.0,
                                 signal_power=2.0, peak_to_second=3.0, second_power=1.0, detected=detected, doppler_bin=0, code_bin=0)

    prns, frac = g.code_fractions([result(3, 0.0), result(7, 511.5), result(9, 1022.99), result(11, 100.0, detected=0), result(12, 1023.0)], g.GPSL1())
    assert prns.tolist() == [3, 7, 9, 11, 12] and prns.dtype == np.int32
    assert frac[0] == 0.0 and frac[1] == 511.5 / 1.023e6 and frac[2] == 1022.99 / 1.023e6 and np.isnan(frac[3]) and frac[4] == 0.0
    assert (frac[[0, 1, 2, 4]] >= 0).all() and (frac[[0, 1, 2, 4]] < 1e-3).all()
