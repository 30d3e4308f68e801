"""gat_position_fix_raim on the device against its host twin, bit for bit on fixes, integrity, trial, sat, resid, sin_el and used, at the
shapes where a kernel that gives a wave to an epoch and a lane to a candidate can go wrong: K = 5 (no round possible), 6 (the
smallest round), 7, 12, 33 and 64 (every lane a channel); E = 1, 3, 4, 5 and 9 (a partial workgroup, a full one, the first wave of a
second, more than two); clean, repaired, two-fault, unresolved, no-redundancy and failed epochs side by side in one workgroup
(tests/raim_cases.py ``mixed``); with and without weights, with the elevation mask, max_exclude 0, 1, 2 and 4, every subset of the
optional outputs, the same call twice, and infinite thresholds against ``position_fix`` on the device.  The twin itself is compared
with the independent restatement in tests/test_raim_host.py."""
import itertools

import numpy as np
import pytest

from tests import fix_cases as fc
from tests import raim_cases as rc
from tests import raim_ref as rr

pytestmark = pytest.mark.gpu

OUTPUTS = ("sat", "resid", "sin_el", "used", "trial")


@pytest.fixture(scope="module")
def g():
    import gpuacceleratedtracking_amd as g
    g.load_library()
    return g


def device(g, c, weights=None, **kw):
    import torch

    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    kw.setdefault("thresholds", rc.thresholds())
    kw.setdefault("outputs", OUTPUTS)
    return g.position_fix_raim(c.ephs, t(c.tx_ms), t(c.tx_frac), t(c.rx_ms), t(c.rx_frac), t(weights), **kw)


def twin(g, c, weights=None, **kw):
    kw.setdefault("thresholds", rc.thresholds())
    kw.setdefault("outputs", OUTPUTS)
    return g.position_fix_raim_host(*c.args(), weights=weights, **kw)


def same_bits(dev, host, outputs=OUTPUTS, integrity=True):
    assert dev.fixes.tobytes() == host.fixes.tobytes(), np.flatnonzero([a.tobytes() != b.tobytes() for a, b in zip(dev.fixes, host.fixes)])[:10]
    if integrity:
        assert dev.integrity.tobytes() == host.integrity.tobytes(), (dev.integrity, host.integrity)
    for name in outputs:
        a, b = getattr(dev, name), getattr(host, name)
        assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), name


@pytest.mark.parametrize("K", [5, 6, 7, 12, 33, 64])
def test_device_equals_twin_at_the_edges_of_the_work_split(g, K):
    per_group = g.raim_plan(1, K)["waves_per_workgroup"]
    assert per_group == 4 and g.raim_plan(per_group + 1, K)["workgroups"] == 2
    rng = np.random.default_rng(K)
    for E in (1, 3, 4, 5, 9):
        case = rc.mixed(K, E)
        c = case.case
        for weights in (None, rng.uniform(0.8, 1.25, c.tx_ms.shape)):
            host = twin(g, c, weights, max_exclude=2)
            dev = device(g, c, weights, max_exclude=2)
            assert dev._host is None  # nothing read back by the call
            same_bits(dev, host)
            if weights is None:  # what the case means to show, on the device (its bits are the twin's)
                for e in range(E):
                    kind, faulted = case.plan.get(e, ("clean", ()))
                    assert dev.integrity["status"][e] == rc.EXPECT[kind], (K, E, e, kind, dev.integrity["status"][e])
                    n_ex = int(dev.integrity["num_excluded"][e])
                    assert list(dev.excluded[e][:n_ex]) == (list(faulted) if kind in ("period", "bias60", "two") else []), (K, E, e, kind)
                    assert not dev.used[e][list(dev.excluded[e][:n_ex])].any()


@pytest.mark.parametrize("max_exclude", [0, 1, 2, 4])
def test_rounds_weights_and_the_mask(g, max_exclude):
    lb = g.positioning
    case = rc.mixed(64, 9)
    c = case.case
    w = np.random.default_rng(5).uniform(0.8, 1.25, c.tx_ms.shape)
    kw = dict(mask_sin=float(np.sin(np.radians(12.0))), tol_m=1e-6, max_iter=12, max_exclude=max_exclude)
    host = twin(g, c, w, **kw)
    dev = device(g, c, w, **kw)
    same_bits(dev, host)
    same_bits(device(g, c, w, **kw), dev)  # the same call twice: the same bits
    assert (dev.status & lb.MASKED).any()
    plain = twin(g, c, None, max_exclude=max_exclude)
    same_bits(device(g, c, None, max_exclude=max_exclude), plain)
    excluded = plain.integrity["num_excluded"]
    two = case.epochs("two")
    if max_exclude == 0:
        assert (excluded == 0).all() and (plain.trial == -1.0).all()
    else:
        assert (excluded[case.epochs("period", "bias60")] == 1).all() and (excluded[two] == (2 if max_exclude >= 2 else 0)).all()
    print("max_exclude", max_exclude, "integrity status", dev.integrity["status"].tolist(), "excluded", dev.integrity["num_excluded"].tolist())


def test_every_subset_of_the_optional_outputs(g):
    c = rc.mixed(12, 5).case
    host = twin(g, c, max_exclude=2)
    for n in range(len(OUTPUTS) + 1):
        for outs in itertools.combinations(OUTPUTS, n):
            dev = device(g, c, outputs=outs, max_exclude=2)
            same_bits(dev, host, outs)
            assert set(dev._raw) == {"fixes", "integrity", *outs}


def test_infinite_thresholds_give_position_fix_on_the_device(g):
    import torch

    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    c = rc.mixed(64, 9).case
    for kw in ({}, dict(mask_sin=fc.SIN_5_DEG * 3.0)):
        dev = device(g, c, thresholds=np.full(61, np.inf), max_exclude=4, **kw)
        fix = g.position_fix(c.ephs, t(c.tx_ms), t(c.tx_frac), t(c.rx_ms), t(c.rx_frac), **kw)
        same_bits(dev, fix, ("sat", "resid", "sin_el", "used"), integrity=False)
        assert not dev.detected.any() and (dev.trial == -1.0).all() and (dev.integrity["num_excluded"] == 0).all()
    # and with finite thresholds wherever nothing is left out
    dev = device(g, c)
    fix = g.position_fix(c.ephs, t(c.tx_ms), t(c.tx_frac), t(c.rx_ms), t(c.rx_frac))
    keep = np.flatnonzero(dev.integrity["num_excluded"] == 0)
    assert 0 < len(keep) < c.E and dev.fixes[keep].tobytes() == fix.fixes[keep].tobytes()
    for name in ("sat", "resid", "sin_el", "used"):
        assert np.ascontiguousarray(getattr(dev, name)[keep]).tobytes() == np.ascontiguousarray(getattr(fix, name)[keep]).tobytes(), name


def test_refusals_of_the_device_entry_point(g):
    import torch

    from gpuacceleratedtracking_amd import _lib

    c = rc.mixed(12, 3).case
    for kw in (dict(max_exclude=5), dict(max_exclude=-1), dict(trial_iter=0), dict(raim_flags=1), dict(max_iter=0), dict(thresholds=np.full(61, np.nan))):
        with pytest.raises(_lib.GatError):
            device(g, c, **kw)
    with pytest.raises(ValueError):
        g.position_fix_raim(c.ephs, torch.from_numpy(c.tx_ms).cuda(), torch.from_numpy(c.tx_frac), torch.from_numpy(c.rx_ms).cuda(),
                            torch.from_numpy(c.rx_frac).cuda(), sigma_m=3.0)
    same_bits(device(g, c), twin(g, c))  # the context still works
    assert rr.DETECTED == g.positioning.RAIM_DETECTED
