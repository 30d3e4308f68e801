"""gat_position_fix_raim on the device against its host twin, byte for byte on fixes, integrity, trial, sat, resid, sin_el and used,
over the whole domain gat.h admits (tests/fix_domain.py): the hostile tiles of the position fix with max_exclude 0 and 4 under
thresholds that detect every checked epoch (the smallest positive double: 0 is refused), that never detect (+inf) and that are +inf
at odd d only; and the extra epochs -- exactly five used channels after the mask (detected, no round possible), a satellite that
counts with a meaningless state (sqrt_a = 0.0086) as one of seven, a channel a code period off, and with trial_iter = 1 epochs
whose every trial fails.  Only bits are asserted, and the one class gat.h fixes whatever the numbers: GAT_RAIM_NOT_CHECKED exactly
where the fix failed or did not converge.  What the garbage satellite's epoch gets is printed, not asserted."""
import numpy as np
import pytest

from tests import fix_domain as fd
from tests import raim_cases as rc

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
    return g.position_fix_raim(c.ephs, t(c.tx_ms), t(c.tx_frac), t(c.rx_ms), t(c.rx_frac), t(weights), outputs=OUTPUTS, **kw)


def twin(g, c, weights=None, **kw):
    return g.position_fix_raim_host(*c.args(), weights=weights, outputs=OUTPUTS, **kw)


def same_bits(dev, host, what=""):
    differ = np.flatnonzero([a.tobytes() != b.tobytes() for a, b in zip(dev.fixes, host.fixes)])
    assert differ.size == 0, (what, "fixes of epochs", differ[:10], dev.fixes[differ[:3]], host.fixes[differ[:3]])
    differ = np.flatnonzero([a.tobytes() != b.tobytes() for a, b in zip(dev.integrity, host.integrity)])
    assert differ.size == 0, (what, "integrity of epochs", differ[:10], dev.integrity[differ[:3]], host.integrity[differ[:3]])
    for name in OUTPUTS:
        a, b = getattr(dev, name), getattr(host, name)
        assert a.shape == b.shape and a.dtype == b.dtype
        assert a.tobytes() == b.tobytes(), (what, name, np.argwhere(a != b)[:10].tolist())


def classes(g, r):
    """gat.h, "fix": a fix that failed or carries GAT_FIX_NOT_CONVERGED is GAT_RAIM_NOT_CHECKED -- and no other is"""
    lb = g.positioning
    unfit = (r.status & (lb.FEW_SATS | lb.SINGULAR | lb.NONFINITE | lb.NOT_CONVERGED)) != 0
    assert np.array_equal(r.integrity["status"] == lb.RAIM_NOT_CHECKED, unfit), (r.status, r.integrity["status"])
    assert (r.integrity["num_excluded"][unfit] == 0).all() and (r.trial[unfit] == -1.0).all()


@pytest.mark.parametrize("K", [64, 12])
@pytest.mark.parametrize("max_exclude", [0, 4])
def test_device_equals_twin_on_every_hostile_entry(g, K, max_exclude):
    per_group = g.raim_plan(1, K)["waves_per_workgroup"]
    tiles = fd.hostile(K, per_group)
    seen = set()
    for table, thresholds in fd.threshold_tables().items():
        for n, t in enumerate(tiles):
            kw = dict(thresholds=thresholds, max_exclude=max_exclude)
            dev = device(g, t.case, t.weights, **kw)
            same_bits(dev, twin(g, t.case, t.weights, **kw), (K, max_exclude, table, n, sorted({label for label, _, _ in t.entries})))
            classes(g, dev)
            if table == "inf":
                assert not dev.detected.any() and (dev.trial == -1.0).all()
            seen |= set(np.unique(dev.integrity["status"]).tolist())
    print(f"K = {K}, max_exclude = {max_exclude}: integrity statuses met {sorted(seen)}")


@pytest.mark.parametrize("table", ["tiny", "inf", "inf_at_odd", "p_fa"])
def test_device_equals_twin_on_the_extra_epochs(g, table):
    lb = g.positioning
    x = fd.raim_extras()
    thresholds = rc.thresholds() if table == "p_fa" else fd.threshold_tables()[table]
    for max_exclude in (0, 4):
        for trial_iter in (8, 1):
            kw = dict(thresholds=thresholds, max_exclude=max_exclude, trial_iter=trial_iter, mask_sin=x.mask_sin, tol_m=1e-6, max_iter=64)
            dev = device(g, x.case, **kw)
            same_bits(dev, twin(g, x.case, **kw), (table, max_exclude, trial_iter))
            classes(g, dev)
            integ = dev.integrity
            five = integ[x.five]
            assert dev.status[x.five] == lb.MASKED and dev.num_used[x.five] == 5 and dev.num_valid[x.five] == 7 and five["dof"] == 1
            assert five["num_excluded"] == 0 and (dev.trial[x.five] == -1.0).all()  # no round with fewer than six
            if table == "tiny":
                assert five["status"] == lb.RAIM_DETECTED | lb.RAIM_UNRESOLVED
                ran = np.flatnonzero((dev.num_used >= 6) & (integ["status"] != lb.RAIM_NOT_CHECKED))
                assert ran.size >= 6 and (integ["status"][ran] & lb.RAIM_DETECTED).all()
                if max_exclude and trial_iter == 1:
                    # from a state that a code period has moved by kilometres, one iteration brings no leave-one-out solve within
                    # tol_m: every trial of that epoch fails, none counts and the rounds end
                    assert x.period in ran and (dev.trial[x.period] == -1.0).all() and integ["num_excluded"][x.period] == 0
                    assert integ["status"][x.period] == lb.RAIM_DETECTED | lb.RAIM_UNRESOLVED
                if max_exclude and trial_iter == 8:
                    assert ((dev.trial[ran] >= 0.0).sum(axis=1) == dev.num_used[ran]).all()
            if table == "p_fa" and trial_iter == 8:
                moved = integ[x.period]
                assert moved["status"] == lb.RAIM_DETECTED | (lb.RAIM_EXCLUDED if max_exclude else lb.RAIM_UNRESOLVED)
                assert moved["excluded"][0] == (x.moved if max_exclude else -1)
            seven = integ[x.seven]
            if max_exclude and trial_iter == 8:
                print(f"{table}, max_exclude {max_exclude}: the epoch with the garbage satellite (channel {x.garbage}) as one of seven: fix status "
                      f"{dev.status[x.seven]}, {dev.iterations[x.seven]} iterations, used {dev.num_used[x.seven]}, integrity status {seven['status']}, "
                      f"excluded {seven['excluded'].tolist()}, T {seven['stat0']:.4g}")
    if table == "p_fa":  # and without the mask, which takes the garbage satellite (it lies at the Earth's centre: below every horizon) out
        kw = dict(thresholds=thresholds, max_exclude=4, tol_m=1e-6, max_iter=64)
        dev = device(g, x.case, **kw)
        same_bits(dev, twin(g, x.case, **kw), (table, "no mask"))
        classes(g, dev)
        seven = dev.integrity[x.seven]
        print(f"without the mask: fix status {dev.status[x.seven]}, integrity status {seven['status']}, excluded {seven['excluded'].tolist()}, T {seven['stat0']:.4g} -> "
              f"{seven['stat']:.4g}, {np.linalg.norm(dev.xyz[x.seven] - x.case.truth_xyz[x.seven]):.3g} m from the truth")
