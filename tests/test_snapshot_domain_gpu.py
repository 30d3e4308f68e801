"""gat_snapshot_fix on the device over the whole domain of tests/snap_domain.py, byte for byte against its host twin on the records
and on all six optional outputs: every hostile entry of the tiles (nine epochs: two workgroups and one, a hostile epoch among the
clean ones of each full workgroup and one alone in the last; K = 64 and 12) -- every real field of the ephemeris not finite,
eccentricities and semi-axes at and beyond the fence, code fractions at the ends of [0, 1e-3) and either side of rx_frac, rx_frac
and rx_ms at their edges, weights -- hostile priors as prior_xyz and as init_xyz, all 64 lanes used with the reference on a tie
(E = 5), and every status bit's path (E = 9, the special epochs inside full workgroups).  Every clean epoch keeps the bytes it has
in the calm run on the device, and the status assertions of tests/test_snapshot_domain_host.py are repeated on the device's own
result.  The kernel's lanes evaluate an orbit inside the iteration and branch wave-wide on ballots of per-lane results: these are
the inputs under which those ballots differ from lane to lane.  The twin against the restatement is the host test's."""
import numpy as np
import pytest

from tests import fix_domain as fd
from tests import snap_domain as sd
from tests import snap_ref as sr
from tests.snap_domain import RECORD_ONLY, check_classification, check_prior

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g():
    import gpuacceleratedtracking_amd as g
    g.load_library()
    return g


def cuda(a):
    import torch

    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def both(g, ephs, frac, rx_ms, rx_frac, prior=None, weights=None, **kw):
    """(device, twin) of one call"""
    host = g.snapshot_fix_host(ephs, frac, rx_ms, rx_frac, prior, weights, **kw)
    dev = g.snapshot_fix(ephs, cuda(frac), cuda(rx_ms), cuda(rx_frac), cuda(prior), cuda(weights), **kw)
    assert dev._host is None  # nothing read back by the call
    return dev, host


def same_bits(dev, host, what):
    differ = np.flatnonzero([a.tobytes() != b.tobytes() for a, b in zip(dev.fixes, host.fixes)])
    assert differ.size == 0, (what, "epochs", differ[:10], dev.fixes[differ[:3]], host.fixes[differ[:3]])
    for name in sd.OUTPUTS:
        a, b = getattr(dev, name), getattr(host, name)
        assert a.shape == b.shape and a.dtype == b.dtype, (what, name)
        if a.tobytes() != b.tobytes():
            at = np.argwhere(a.view(np.uint8).reshape(a.shape + (-1,)) != b.view(np.uint8).reshape(b.shape + (-1,)))
            raise AssertionError((what, name, "differs at", at[:5].tolist()))


def keeps_its_bytes(dev, quiet, epochs, what):
    for e in epochs:
        assert dev.fixes[e].tobytes() == quiet.fixes[e].tobytes(), (what, e)
        for name in sd.OUTPUTS:
            assert getattr(dev, name)[e].tobytes() == getattr(quiet, name)[e].tobytes(), (what, e, name)


@pytest.fixture(scope="module", params=[64, 12])
def scene(request, g):
    """the tiles of K channels and the calm run on the device"""
    s = sd.hostile(request.param)
    assert g.snapshot_plan(s.calm.E, s.K)["workgroups"] == 3 and s.calm.E == 9
    quiet, quiet_host = both(g, *s.calm.args())
    same_bits(quiet, quiet_host, (s.K, "calm"))
    clean = list(s.clean)
    assert (quiet.status[clean] == 0).all() and np.linalg.norm(quiet.xyz[clean] - s.truth_xyz[clean], axis=1).max() < 1e-3
    return s, quiet


def test_device_equals_twin_on_every_hostile_entry(g, scene):
    S = g.snapshot
    s, quiet = scene
    seen, labels = 0, set()
    for n, t in enumerate(s.tiles):
        what = (s.K, n, sorted({label for label, _, _ in t.entries}))
        for weighted in (True, False):
            dev, host = both(g, *t.args(weighted))
            same_bits(dev, host, what)
            keeps_its_bytes(dev, quiet, s.clean, what)
            check_classification(S, dev, t, weighted)
            seen |= int(np.bitwise_or.reduce(dev.status))
        labels |= {label for label, _, _ in t.entries}
        print(f"K = {s.K}: hostile epochs {t.hostile}: device status {dev.status[list(t.hostile)].tolist()}, valid {dev.num_valid[list(t.hostile)].tolist()}: "
              + ", ".join(what[2])[:150])
    assert len(labels) == 78 + 24 + 7 + 5 + 6
    assert seen & S.FEW_SATS and seen & S.NONFINITE and seen & S.AMBIGUOUS  # no used channel (rx_ms = -1); the fence (rx_frac = 1e19)


def test_hostile_priors(g, scene):
    S = g.snapshot
    s, quiet = scene
    on_k, on_xyz = sd.on_a_satellite(s, s.hostile[0])
    c = s.calm
    for label, value, refused in sd.prior_entries(s) + [("on a satellite", on_xyz, False)]:
        prior = c.prior.copy()
        for e in s.hostile:
            if len(value) == 2:
                prior[e, value[0]] = value[1]
            else:
                prior[e] = value
        dev, host = both(g, c.ephs, c.code_frac, c.rx_ms, c.rx_frac, prior)
        same_bits(dev, host, (s.K, label))
        keeps_its_bytes(dev, quiet, s.clean, label)
        check_prior(S, dev, quiet, s.hostile[:1] if label == "on a satellite" else s.hostile, label, on_k)
        if label in ("centre", "on a satellite"):
            print(f"K = {s.K}: prior {label}: device status {dev.status[list(s.hostile)].tolist()}, valid {dev.num_valid[list(s.hostile)].tolist()}")
        if refused:
            with pytest.raises(g._lib.GatError):
                g.snapshot_fix(c.ephs, cuda(c.code_frac), cuda(c.rx_ms), cuda(c.rx_frac), init_xyz=tuple(prior[s.hostile[0]]))
            continue
        dev, host = both(g, c.ephs, c.code_frac, c.rx_ms, c.rx_frac, init_xyz=tuple(prior[s.hostile[0]]))
        same_bits(dev, host, (s.K, label, "init_xyz"))
        if label != "on a satellite":
            check_prior(S, dev, quiet, range(c.E), label, on_k)


def test_all_64_lanes_used_and_the_reference_on_a_tie(g):
    w = sd.full_width()
    c = w.snap
    assert g.snapshot_plan(c.E, 64)["workgroups"] == 2 and c.E == 5 and c.K == 64
    rng = np.random.default_rng(64)
    for weights, kw in ((None, {}), (None, sd.CONVERGED), (rng.uniform(0.5, 2.0, c.code_frac.shape), {}), (None, dict(mask_sin=fd.MASK_15))):
        dev, host = both(g, *c.args(), weights, **kw)
        same_bits(dev, host, ("full width", weights is not None, kw))
        assert (dev.num_valid == 64).all() and (dev.status & ~g.snapshot.MASKED == 0).all()
        if "mask_sin" not in kw:
            assert (dev.num_used == 64).all() and dev.used.all()
        assert np.linalg.norm(dev.xyz - c.truth_xyz, axis=1).max() < 1e-3 and np.array_equal(dev.tx_ms, c.case.tx_ms)
        for e in range(c.E):
            assert np.array_equal(dev.n_ms[e], w.ref[e]["n"])  # the restatement's, with its reference the lowest channel of the tie


def test_status_paths(g):
    S, p = g.snapshot, sd.status_paths()
    c = p.snap
    assert g.snapshot_plan(c.E, c.K)["workgroups"] == 3 and max(p.again, p.five, p.four, p.e_c, p.e_d) < 8  # inside the full workgroups
    ok = [e for e in range(c.E) if e != p.four]
    plain, host = both(g, *p.args())
    same_bits(plain, host, "plain")
    same_bits(plain, p.plain, "the call the masks were found with")
    assert plain.status[p.five] == 0 and plain.num_used[p.five] == 5 and plain.num_valid[p.five] == 12 and plain.used[p.five].sum() == 5
    assert plain.status[p.four] == S.FEW_SATS and plain.num_used[p.four] == 4 and plain.num_valid[p.four] == 12
    zero = plain.fixes[p.four]
    assert all(zero[n] == 0 for n in zero.dtype.names if n not in RECORD_ONLY) and (plain.tx_ms[p.four] == -1).all() and plain.rx_ms_out[p.four] == -1
    assert plain.status[p.again] & S.RERESOLVED and not plain.status[p.again] & (S.MASKED | sd.FAILED)
    for mask in (-1.0, p.mask_c):  # a mask that would leave five of twelve  # (a)
        a, host = both(g, *p.args(), max_iter=1, tol_m=1e-6, mask_sin=mask)
        same_bits(a, host, ("a", mask))
        assert (a.status[ok] & ~S.AMBIGUOUS == S.NOT_CONVERGED).all() and (a.iterations[ok] == 1).all() and a.status[p.four] == S.FEW_SATS
        assert a.xyz[ok].all() and (a.last_step_m[ok] > 1e-6).all() and (a.gdop[ok] > 0).all()
        assert (a.tx_ms[ok] >= 0).all() and (a.rx_ms_out[ok] >= 0).all() and (a.num_used[ok] == plain.num_used[ok]).all()
    b, host = both(g, *p.args(), max_iter=1, tol_m=p.tol_first)  # (b)
    same_bits(b, host, "b")
    assert (b.status[ok] & ~(S.AMBIGUOUS | S.RERESOLVED) == 0).all() and (b.iterations[ok] == np.where(b.status[ok] & S.RERESOLVED, 2, 1)).all()
    m, host = both(g, *p.args(), mask_sin=p.mask_c)  # (c)
    same_bits(m, host, "c")
    assert m.status[p.e_c] == S.MASKED and m.num_used[p.e_c] == 5 and m.used[p.e_c].sum() == 5 and m.num_valid[p.e_c] == 12
    assert ((m.used[p.e_c] != 0) == (plain.sin_el[p.e_c] >= p.mask_c)).all()
    m, host = both(g, *p.args(), mask_sin=p.mask_d)  # (d)
    same_bits(m, host, "d")
    want = plain.fixes[p.e_d].copy()
    want["status"] |= S.MASK_STARVED
    assert m.fixes[p.e_d].tobytes() == want.tobytes() and m.status[p.e_d] == S.MASK_STARVED
    for name in sd.OUTPUTS:
        assert getattr(m, name)[p.e_d].tobytes() == getattr(plain, name)[p.e_d].tobytes(), name
    m, host = both(g, *p.args(), mask_sin=p.mask_e)  # (e)
    same_bits(m, host, "e")
    assert m.status[p.again] & S.RERESOLVED and m.status[p.again] & S.MASKED and m.num_used[p.again] == 11
    for margin in (0.0, 0.5):  # (g)
        m, host = both(g, *p.args(), ambiguity_margin=margin)
        same_bits(m, host, ("g", margin))
        assert ((m.status[ok] & S.AMBIGUOUS != 0) == (margin == 0.5)).all()


def test_a_singular_epoch_and_a_range_beyond_the_fence_among_clean_ones(g, scene):
    """the two status bits the tiles do not promise: two identical satellites among five used (SINGULAR), and a channel whose clock
    is 1e4 s off, its range 1e7 whole milliseconds from the reference's (NONFINITE through snap_integer, not snap_reference)"""
    S = g.snapshot
    s, quiet = scene
    c = s.calm
    e = s.hostile[0]
    order = np.argsort(-np.where(np.isfinite(c.code_frac[e]), c.case.sin_el[e], -2.0))
    twin_of, k = int(order[0]), int(s.chans[0])
    ephs, frac = c.ephs.copy(), c.code_frac.copy()
    ephs[k] = ephs[twin_of]  # the designated channel measures nothing in any other epoch
    frac[e, order[4:]] = np.nan
    frac[e, k] = c.code_frac[e, twin_of]
    dev, host = both(g, ephs, frac, c.rx_ms, c.rx_frac, c.prior)
    same_bits(dev, host, (s.K, "singular"))
    keeps_its_bytes(dev, quiet, s.clean, "singular")
    assert dev.status[e] == S.SINGULAR and dev.num_used[e] == 5 and not dev.xyz[e].any() and (dev.tx_ms[e] == -1).all()
    ephs, frac = c.ephs.copy(), c.code_frac.copy()
    ephs["af0"][k] = 1e4
    frac[e, k] = 0.5e-3
    _, sin_el = sr.predicted(ephs, c.prior[e], 0.0, 0.0, int(c.rx_ms[e]) * sr.MS + c.rx_frac[e])
    assert int(np.argmax(np.where(np.isfinite(frac[e]), sin_el, -2.0))) != k  # not the reference: the fence is snap_integer's
    dev, host = both(g, ephs, frac, c.rx_ms, c.rx_frac, c.prior)
    same_bits(dev, host, (s.K, "af0"))
    keeps_its_bytes(dev, quiet, s.clean, "af0")
    assert dev.status[e] == S.NONFINITE and dev.num_valid[e] == quiet.num_valid[e] + 1 and dev.iterations[e] == 0 and (dev.tx_ms[e] == -1).all()
