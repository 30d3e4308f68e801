"""gat_position_fix_raim_host (the host twin of the fix integrity call, csrc/gat_raim_plan.h) against the independent restatement of
tests/raim_ref.py on the cases of tests/raim_cases.py, the rule's properties (where nothing is left out the bytes are
gat_position_fix_host's), every refusal, and ``raim_thresholds`` against tabulated chi-square quantiles.  Bounds: the position within
1e-5 m (the bound of the fix against its restatement, tests/test_position_host.py); T = sum w v^2 then within 2 sqrt(n T) 2e-5 sqrt(w)
-- each of n residuals moves by at most about 2e-5 m (the position's 1e-5 and as much of clock), and d(sum w v^2) <= 2 sum w |v| dv <=
2 sqrt(n sum w v^2) max sqrt(w) dv by Cauchy-Schwarz."""
import numpy as np
import pytest

from tests import fix_cases as fc
from tests import raim_cases as rc
from tests import raim_ref as rr

FIX_OUTPUTS = ("sat", "resid", "sin_el", "used")


@pytest.fixture(scope="module")
def g():
    import gpuacceleratedtracking_amd as g
    return g


def twin(g, c, **kw):
    kw.setdefault("thresholds", rc.thresholds())
    kw.setdefault("outputs", FIX_OUTPUTS + ("trial",))
    return g.position_fix_raim_host(*c.args(), **kw)


def same_fix_bytes(a, b, epochs=None):
    """fixes, sat, resid, sin_el and used of the epochs (None: all) have the same bytes"""
    idx = slice(None) if epochs is None else np.asarray(epochs, dtype=np.int64)
    assert a.fixes[idx].tobytes() == b.fixes[idx].tobytes()
    for name in FIX_OUTPUTS:
        assert np.ascontiguousarray(getattr(a, name)[idx]).tobytes() == np.ascontiguousarray(getattr(b, name)[idx]).tobytes(), name


@pytest.mark.parametrize("name", rc.ALL)
def test_twin_against_the_restatement(g, name):
    lb = g.positioning
    case = rc.case(name)
    c = case.case
    r = twin(g, c, max_exclude=2)
    plain = g.position_fix_host(*c.args())
    integ = r.integrity
    worst_trial = 0.0
    for e in range(c.E):
        kind, faulted = case.plan.get(e, ("clean", ()))
        want = rr.raim(c.ephs, c.tx_ms[e], c.tx_frac[e], c.rx_ms[e], c.rx_frac[e], rc.thresholds(), None, 2)
        assert integ["status"][e] == want["status"] == rc.EXPECT[kind], (e, kind, integ["status"][e], want["status"])
        n_ex = int(integ["num_excluded"][e])
        assert list(integ["excluded"][e][:n_ex]) == want["excluded"] == (list(faulted) if kind in ("period", "bias60", "two") else [])
        assert (integ["excluded"][e][n_ex:] == -1).all() and integ["dof"][e] == want["dof"]
        assert np.array_equal(r.used[e] != 0, want["used"])
        assert np.linalg.norm(r.xyz[e] - want["xyz"]) <= 1e-5, (e, kind, np.linalg.norm(r.xyz[e] - want["xyz"]))
        n = int(r.num_used[e])
        for mine, theirs in ((integ["stat"][e], want["stat"]), (integ["stat0"][e], want["stat0"])):
            assert abs(mine - theirs) <= 2.0 * np.sqrt(n * max(mine, theirs)) * 2e-5, (e, kind, mine, theirs)
        assert bool(r.status[e] & lb.EXCLUDED) == (n_ex > 0) and r.detected[e] == bool(want["status"] & rr.DETECTED)
        if integ["status"][e] & rr.DETECTED and plain.num_used[e] >= 6:
            # the first round's trials, solved from the contaminated state with frozen satellites, against the from-scratch solves
            cand = want["trial"] >= 0
            assert np.array_equal(r.trial[e] >= 0, cand)
            assert int(np.argmin(np.where(cand, r.trial[e], np.inf))) == int(np.argmin(np.where(cand, want["trial"], np.inf))) == want["excluded"][0]
            worst_trial = max(worst_trial, float(np.abs(r.trial[e][cand] / want["trial"][cand] - 1.0).max()))
        else:
            assert (r.trial[e] == -1.0).all()
        if n_ex:
            # as good as a fix that never saw the faulted channels, and far better than the fix that did
            w = np.ones(c.tx_ms.shape)
            w[e, list(integ["excluded"][e][:n_ex])] = 0.0
            without = g.position_fix_host(*c.args(), weights=w)
            assert np.linalg.norm(r.xyz[e] - without.xyz[e]) <= 2e-4, (e, np.linalg.norm(r.xyz[e] - without.xyz[e]))  # 2 tol_m
            before, after = np.linalg.norm(plain.xyz[e] - c.truth_xyz[e]), np.linalg.norm(r.xyz[e] - c.truth_xyz[e])
            print(f"{name} epoch {e} {kind}: error {before:.3f} m with the fault, {after:.3f} m repaired; T {integ['stat0'][e]:.4g} -> {integ['stat'][e]:.4g}")
            assert after < 30.0 and after < 0.5 * before, (e, kind, before, after)
    print(f"{name}: largest relative difference of a first-round trial T_j to the from-scratch solve {worst_trial:.3e}")
    same_fix_bytes(r, plain, np.flatnonzero(integ["num_excluded"] == 0))


@pytest.mark.parametrize("name", rc.ALL)
def test_infinite_thresholds_give_the_fix_itself(g, name):
    c = rc.case(name).case
    thr = np.full(61, np.inf)
    for kw in ({}, dict(mask_sin=fc.SIN_5_DEG * 3.0, tol_m=1e-6, max_iter=12)):
        for weights in (None, np.random.default_rng(3).uniform(0.5, 2.0, c.tx_ms.shape)):
            r = twin(g, c, thresholds=thr, weights=weights, max_exclude=4, **kw)
            same_fix_bytes(r, g.position_fix_host(*c.args(), weights=weights, **kw))
            assert not (r.integrity["status"] & rr.DETECTED).any() and not r.detected.any() and (r.integrity["num_excluded"] == 0).all()
            assert (r.trial == -1.0).all() and (r.excluded == -1).all()


def test_unresolved_no_redundancy_and_failed_epochs(g):
    lb = g.positioning
    c = rc.case("mid").case.copy()
    w = np.ones(c.tx_ms.shape)
    assert fc.special(c, 0, "three", w) == lb.FEW_SATS and fc.special(c, 4, "nan", w) == lb.FEW_SATS
    plain = g.position_fix_host(*c.args())
    r = twin(g, c)
    assert r.integrity["status"][0] == r.integrity["status"][4] == rr.NOT_CHECKED
    assert r.integrity["status"][6] == rr.DETECTED | rr.UNRESOLVED and r.num_used[6] == 5 and r.integrity["dof"][6] == 1  # n = 5
    assert r.integrity["status"][7] == rr.NO_REDUNDANCY and r.num_used[7] == 4 and r.integrity["dof"][7] == 0  # n = 4
    same_fix_bytes(r, plain, [0, 4, 6, 7])
    # a fix that did not converge is not checked either
    short = twin(g, c, max_iter=1)
    assert (short.status[[1, 2, 3]] == lb.NOT_CONVERGED).all() and (short.integrity["status"][[1, 2, 3]] == rr.NOT_CHECKED).all()
    same_fix_bytes(short, g.position_fix_host(*c.args(), max_iter=1))
    # detection alone: every detected epoch stands as the full set gave it
    det = twin(g, c, max_exclude=0)
    faulted = [1, 2, 3, 5, 6]
    assert (det.integrity["status"][faulted] == rr.DETECTED | rr.UNRESOLVED).all() and (det.integrity["num_excluded"] == 0).all()
    assert (det.trial == -1.0).all() and (det.integrity["stat"] == det.integrity["stat0"]).all()
    same_fix_bytes(det, plain)
    # two faults and one round: unresolved, the full set's bytes; a trial that cannot converge in one iteration: unresolved too
    assert r.integrity["status"][3] == rr.DETECTED | rr.UNRESOLVED and r.integrity["num_excluded"][3] == 0 and (r.trial[3] >= 0).any()
    same_fix_bytes(r, plain, [3])
    one = twin(g, c, trial_iter=1)
    assert (one.integrity["status"][[1, 5]] == rr.DETECTED | rr.UNRESOLVED).all() and (one.trial[[1, 5]] == -1.0).all()
    same_fix_bytes(one, plain, [1, 5])


def test_one_faulted_epoch_leaves_the_others_alone(g):
    base = rc.noisy(fc.case("mid"), 21)
    clean = twin(g, base)
    assert (clean.integrity["status"] == 0).all()
    c = base.copy()
    k = rc.inject(c, 3, "period", 2)[0]
    r = twin(g, c)
    assert r.integrity["status"][3] == rr.DETECTED | rr.EXCLUDED and r.excluded[3, 0] == k and r.used[3, k] == 0
    others = [e for e in range(c.E) if e != 3]
    same_fix_bytes(r, clean, others)
    assert r.integrity[others].tobytes() == clean.integrity[others].tobytes() and r.trial[others].tobytes() == clean.trial[others].tobytes()


def test_weights_as_inverse_variances(g):
    """weights 1 / sigma^2 with the thresholds of sigma_m = 1 decide as unit weights with the thresholds of sigma_m do"""
    case = rc.case("week_end")
    c = case.case
    w = np.full(c.tx_ms.shape, 1.0 / rc.SIGMA_M ** 2)
    a = g.position_fix_raim_host(*c.args(), weights=w, max_exclude=2)
    b = g.position_fix_raim_host(*c.args(), sigma_m=rc.SIGMA_M, max_exclude=2)
    assert np.array_equal(a.integrity["status"], b.integrity["status"]) and np.array_equal(a.excluded, b.excluded)
    assert np.abs(a.xyz - b.xyz).max() < 1e-4
    with pytest.raises(ValueError):
        g.position_fix_raim_host(*c.args())  # no weights and no sigma_m: no scale for the thresholds


def test_every_refusal(g):
    import ctypes as C

    from gpuacceleratedtracking_amd import _lib
    from gpuacceleratedtracking_amd.positioning import fix_config, raim_config
    from gpuacceleratedtracking_amd.streams import addr

    c = rc.case("mid").case
    thr = rc.thresholds()
    for kw in (dict(max_exclude=-1), dict(max_exclude=5), dict(trial_iter=0), dict(raim_flags=1), dict(max_iter=0), dict(tol_m=0.0), dict(flags=1),
               dict(mask_sin=float("nan"))):
        with pytest.raises(_lib.GatError) as err:
            twin(g, c, **kw)
        assert err.value.status == 1, kw
    for d, bad in ((1, np.nan), (60, 0.0), (17, -1.0), (5, -np.inf)):
        t = thr.copy()
        t[d] = bad
        with pytest.raises(_lib.GatError):
            twin(g, c, thresholds=t)
    t = thr.copy()
    t[0] = np.nan  # entry 0 is not read
    assert twin(g, c, thresholds=t).integrity.tobytes() == twin(g, c).integrity.tobytes()
    with pytest.raises(ValueError):
        twin(g, c, thresholds=thr[:60])
    with pytest.raises(ValueError):
        twin(g, c, outputs=("nothing",))
    with pytest.raises(_lib.GatError):
        g.raim_plan(0, 5)
    with pytest.raises(_lib.GatError):
        g.raim_plan(5, 65)
    # the raw entry point: null pointers and a wrong struct_size, with nothing written
    lib = g.load_library()
    cfg, rcfg = fix_config(), raim_config(thr)
    E, K = c.tx_ms.shape
    fixes, integ = np.full(E, 0x5a, np.uint8).repeat(80), np.full(E, 0x5a, np.uint8).repeat(64)
    ephs = np.ascontiguousarray(c.ephs)

    def call(rcfg_ref, fixes_ptr, integ_ptr):
        return lib.gat_position_fix_raim_host(addr(ephs), addr(c.tx_ms), addr(c.tx_frac), addr(c.rx_ms), addr(c.rx_frac), None, E, K, C.byref(cfg),
                                              rcfg_ref, fixes_ptr, integ_ptr, None, None, None, None, None)

    assert call(None, addr(fixes), addr(integ)) == 1 and call(C.byref(rcfg), addr(fixes), None) == 1 and call(C.byref(rcfg), None, addr(integ)) == 1
    rcfg.struct_size -= 8
    assert call(C.byref(rcfg), addr(fixes), addr(integ)) == 1
    assert (fixes == 0x5a).all() and (integ == 0x5a).all()
    rcfg.struct_size += 8
    assert call(C.byref(rcfg), addr(fixes), addr(integ)) == 0 and integ.view(_lib.INTEGRITY_DTYPE)["status"].tolist() == twin(g, c).integrity["status"].tolist()


def test_plan_report(g):
    fix, raim = g.position_plan(9, 12), g.raim_plan(9, 12)
    assert {k: v for k, v in raim.items() if k != "lds_bytes"} == {k: v for k, v in fix.items() if k != "lds_bytes"}
    assert raim["lds_bytes"] == fix["lds_bytes"] + raim["waves_per_workgroup"] * 64 * 6 * 8 and raim["scratch_bytes"] == 0


def test_thresholds_against_tabulated_quantiles(g):
    t = g.raim_thresholds(1e-3)
    assert t.shape == (61,) and t.dtype == np.float64 and t[0] == 0.0 and (np.diff(t[1:]) > 0).all()
    for d, q in ((1, 10.828), (2, 13.816), (5, 20.515), (10, 29.588), (20, 45.315), (60, 99.607)):
        assert abs(t[d] / q - 1.0) <= 1e-4, (d, t[d], q)
    assert np.allclose(g.raim_thresholds(1e-3, 3.0), 9.0 * t, rtol=1e-15)
    # the median of two degrees of freedom is 2 ln 2: the series branch of the incomplete gamma function
    assert abs(g.raim_thresholds(0.5)[2] - 2.0 * np.log(2.0)) <= 1e-12
    try:
        from scipy.stats import chi2
    except ImportError:
        return
    for p in (1e-3, 1e-6, 0.05, 0.5):
        mine = g.raim_thresholds(p)[1:]
        assert np.abs(mine / chi2.isf(p, np.arange(1, 61)) - 1.0).max() <= 1e-9, p
