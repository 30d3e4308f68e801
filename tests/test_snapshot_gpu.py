"""gat_snapshot_fix on the device against its host twin, byte for byte on the records and on every optional output, at the shapes
where a kernel that gives a wave to an epoch and a lane to a channel can go wrong: K = 1, 4, 5, 6, 12, 63 and 64 with E = 1, 4, 5 and
9 (whole and partial workgroups of four epochs, the 4 / 5 boundary of FEW_SATS); with and without ``prior_xyz``, weights and the
mask; every subset of the optional outputs; epochs of every kind inside one workgroup -- clean, four measurements, singular (two
identical satellites among five), one NaN fraction, a prior at the Earth's centre, one whose integers are resolved again -- where
each clean epoch keeps the bytes it has without the others; and the same call twice.  The twin itself is compared with the
independent restatement in tests/test_snapshot_host.py."""
import itertools

import numpy as np
import pytest

from tests import fix_cases as fc
from tests import snap_cases as sc

pytestmark = pytest.mark.gpu

OUTPUTS = ("tx_ms", "rx_ms_out", "n_ms", "resid", "sin_el", "used")
MASK = float(np.sin(np.radians(15.0)))


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


def same_bits(dev, host, outputs=OUTPUTS, what=""):
    differ = np.flatnonzero([a.tobytes() != b.tobytes() for a, b in zip(dev.fixes, host.fixes)])
    assert differ.size == 0, (what, "epochs", differ[:10], dev.fixes[differ[:3]], host.fixes[differ[:3]])
    for name in outputs:
        a, b = getattr(dev, name), getattr(host, name)
        assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), (what, name)


def case_of(K: int, E: int) -> sc.SnapCase:
    base = sc.case("short", 30, K, 8, check=False) if K < 30 else sc.case("mid", K, None, 8, check=False)
    return base.tiled(E) if E != base.E else base


@pytest.mark.parametrize("K", [1, 4, 5, 6, 12, 63, 64])
def test_device_equals_twin_at_the_edges_of_the_work_split(g, K):
    plan = g.snapshot_plan(1, K)
    assert plan["waves_per_workgroup"] == 4 and g.snapshot_plan(5, K)["workgroups"] == 2 and g.snapshot_plan(9, K)["workgroups"] == 3
    rng = np.random.default_rng(K)
    for E in (1, 4, 5, 9):
        c = case_of(K, E)
        weights = rng.uniform(0.5, 2.0, c.code_frac.shape)
        for prior, w, mask in ((c.prior, None, -1.0), (None, weights, -1.0), (c.prior, weights, MASK)):
            dev, host = both(g, c.ephs, c.code_frac, c.rx_ms, c.rx_frac, prior, w, mask_sin=mask, init_xyz=tuple(c.prior[0]))
            same_bits(dev, host, what=(K, E, prior is not None, w is not None, mask))
            if K < 5:
                assert (host.status == g.snapshot.FEW_SATS).all() and (host.num_valid == c.seen.sum(axis=1)).all() and (host.tx_ms == -1).all()
            elif prior is not None and mask < 0:  # the receivers come back, and the transmit times a decoded time of week would give
                assert (dev.status == 0).all() and np.linalg.norm(dev.xyz - c.truth_xyz, axis=1).max() < 1e-3
                assert np.array_equal(dev.tx_ms, c.case.tx_ms) and np.array_equal(dev.rx_ms_out, c.case.rx_ms)
            if mask > 0 and K >= 12:
                assert (dev.status & g.snapshot.MASKED).any()


def test_every_subset_of_the_optional_outputs(g):
    c = case_of(12, 5)
    for n in range(len(OUTPUTS) + 1):
        for outs in itertools.combinations(OUTPUTS, n):
            dev, host = both(g, *c.args(), outputs=outs)
            same_bits(dev, host, outs, outs)
            assert set(dev._raw) == {"fixes", *outs}


@pytest.fixture(scope="module")
def kinds(g):
    """nine epochs of twelve channels, three workgroups: clean, four measurements, singular, NaN fraction | the Earth's centre, resolved
    again, clean, clean | clean.  Returns (ephs, frac, rx_ms, rx_frac, prior) of the calm tile (every epoch clean) and of the tile."""
    e_twin = 2
    base = fc.twinned(fc.case("short", 30, 12, 8).tiled(9), e_twin)
    c = sc.SnapCase(base, check=False)
    assert c.seen.all()
    calm = (c.ephs, c.code_frac.copy(), c.rx_ms, c.rx_frac, c.prior.copy())
    frac, prior = c.code_frac.copy(), c.prior.copy()
    order = np.argsort(-base.sin_el, axis=1)
    frac[1, order[1, 4:]] = np.nan
    assert np.array_equal(c.ephs[order[e_twin, 0]], c.ephs[order[e_twin, 1]])
    frac[e_twin, order[e_twin, 5:]] = np.nan
    frac[3, 7] = np.nan
    prior[4] = 0.0
    d = (c.prior[5] - c.truth_xyz[5]) / np.linalg.norm(c.prior[5] - c.truth_xyz[5])
    for km in range(100, 400, 5):  # the nearest prior along the case's own direction whose integers are resolved again
        prior[5] = c.truth_xyz[5] + d * km * 1e3
        s = g.snapshot_fix_host(c.ephs, frac[5:6], c.rx_ms[5:6], c.rx_frac[5:6], prior[5:6])
        if s.status[0] & g.snapshot.RERESOLVED:
            break
    else:
        raise AssertionError("no prior along the direction is resolved again")
    return calm, (c.ephs, frac, c.rx_ms, c.rx_frac, prior)


def test_epochs_of_every_kind_inside_one_workgroup(g, kinds):
    S = g.snapshot
    calm, mixed = kinds
    dev0, host0 = both(g, *calm)
    same_bits(dev0, host0, what="calm")
    dev, host = both(g, *mixed)
    same_bits(dev, host, what="mixed")
    assert dev.status[0] == 0 and dev.status[1] == S.FEW_SATS and dev.status[2] == S.SINGULAR and dev.status[3] == 0 and dev.num_used[3] == 11
    assert dev.status[5] & S.RERESOLVED and not S.RERESOLVED & dev.status[[0, 3, 6, 7, 8]].max()
    assert (dev.tx_ms[[1, 2]] == -1).all() and (dev.rx_ms_out[[1, 2]] == -1).all() and not dev.xyz[[1, 2]].any()
    for e in (0, 6, 7, 8):  # one epoch never touches another
        assert dev.fixes[e].tobytes() == dev0.fixes[e].tobytes()
        for name in ("tx_ms", "n_ms", "resid", "sin_el", "used"):
            assert getattr(dev, name)[e].tobytes() == getattr(dev0, name)[e].tobytes(), (e, name)


def test_the_same_call_twice(g, kinds):
    _, mixed = kinds
    a, _ = both(g, *mixed, mask_sin=MASK)
    b, host = both(g, *mixed, mask_sin=MASK)
    same_bits(a, host)
    same_bits(b, host)


def test_refusals_come_before_any_launch(g):
    import torch

    c = case_of(12, 4)
    args = (c.ephs, cuda(c.code_frac), cuda(c.rx_ms), cuda(c.rx_frac), cuda(c.prior))
    for kw in (dict(max_iter=0), dict(tol_m=0.0), dict(ambiguity_margin=0.6), dict(flags=1), dict(mask_sin=float("nan"))):
        with pytest.raises(g._lib.GatError):
            g.snapshot_fix(*args, **kw)
    with pytest.raises(ValueError):
        g.snapshot_fix(c.ephs, cuda(c.code_frac).float(), *args[2:])
    with pytest.raises(ValueError):
        g.snapshot_fix(c.ephs, args[1], args[2], args[3], torch.zeros((3, 3), dtype=torch.float64, device="cuda"))
    torch.cuda.synchronize()
