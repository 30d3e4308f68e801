"""gat_position_fix on the device against its host twin, bit for bit on every output, at the shapes where a kernel that gives a
wave to an epoch and a lane to a channel can go wrong: K = 4, 5, 63 and 64; E = 1, 3 and one more than a workgroup's epochs (from
``position_plan``); E = 1000 with every special epoch scattered in (three satellites, too few weights, NaN observables, two identical
satellites among four, five satellites of which three stand above the mask, an unusable ephemeris), with weights and an elevation
mask and without, with max_iter = 1, which does not converge, and from a start so far away that the sums are not finite; every
subset of the optional outputs; the same call twice; tensors that are not on the device.  The twin itself is compared with the independent restatement in
tests/test_position_host.py."""
import itertools

import numpy as np
import pytest

from tests import fix_cases as fc

pytestmark = pytest.mark.gpu

OUTPUTS = ("sat", "resid", "sin_el", "used")


@pytest.fixture(scope="module")
def g():
    import gpuacceleratedtracking_amd as g
    g.load_library()
    return g


def device(g, c, weights=None, **kw):
    import torch

    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    return g.position_fix(c.ephs, t(c.tx_ms), t(c.tx_frac), t(c.rx_ms), t(c.rx_frac), t(weights), **kw)


def same_bits(dev, host, outputs=OUTPUTS):
    assert dev.fixes.tobytes() == host.fixes.tobytes(), np.flatnonzero([a.tobytes() != b.tobytes() for a, b in zip(dev.fixes, host.fixes)])[:10]
    for name in outputs:
        a, b = getattr(dev, name), getattr(host, name)
        assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), name


def case_of(K: int, E: int):
    base = fc.case("short", 30, K, 8) if K < 30 else fc.case("mid", K)
    return base.tiled(E) if E != base.E else base


@pytest.mark.parametrize("K", [4, 5, 63, 64])
def test_device_equals_twin_at_the_edges_of_the_work_split(g, K):
    per_group = g.position_plan(1, K)["waves_per_workgroup"]
    assert g.position_plan(per_group + 1, K)["workgroups"] == 2
    rng = np.random.default_rng(K)
    for E in (1, 3, per_group + 1):
        c = case_of(K, E)
        for weights in (None, rng.uniform(0.5, 2.0, c.tx_ms.shape)):
            host = g.position_fix_host(*c.args(), weights=weights)
            dev = device(g, c, weights)
            assert dev._host is None  # nothing read back by the call
            same_bits(dev, host)
            assert (host.status == 0).all() and np.linalg.norm(host.xyz - c.truth_xyz, axis=1).max() < 1e-3


MASK_SIN = float(np.sin(np.radians(12.0)))


@pytest.fixture(scope="module")
def scattered(g):
    """1000 epochs of 30 channels, a special epoch every 37 and more, one channel's ephemeris unusable; want[e] = (kind, status)"""
    lb = g.positioning
    e0 = 5
    base = fc.case("mid")
    twins = (int(np.argmax(base.sin_el[e0])), int(np.argmin(base.sin_el[e0])))
    c = fc.twinned(base, e0).tiled(1000)
    c.ephs = c.ephs.copy()
    dead = [int(k) for k in np.argsort(-base.sin_el[0]) if k not in twins][2]  # seen in epoch 0, neither of the twins
    c.ephs["valid"][dead] = 0
    w = np.random.default_rng(2).uniform(0.5, 2.0, c.tx_ms.shape)
    want = {}
    kinds = ("three", "weights_three", "nan", "nan_rx")
    for i, e in enumerate(range(11, 1000, 37)):
        want[e] = (kinds[i % 4], fc.special(c, e, kinds[i % 4], w))
    for e in range(e0 + 8, 1000, 8 * 17):
        c.sin_el[e, dead] = -1.0  # not among the four the special epoch keeps
        want[e] = ("twins", fc.special(c, e, "twins", w))
    starved = 0
    for e in range(200, 1000, 29):
        c.tx_ms[e, dead] = -1  # the unusable channel is no candidate
        if e in want or fc.starvable(c, e, MASK_SIN) is None:
            continue
        want[e] = ("mask_starved", fc.special(c, e, "mask_starved", w, MASK_SIN))
        starved += 1
    assert starved >= 8, starved
    return c, w, want, dead, lb


CONFIGS = {"weights_mask": dict(mask_sin=MASK_SIN, tol_m=1e-6, max_iter=12), "plain": {}, "max_iter_1": dict(max_iter=1),
           "far_start": dict(init_xyz=(1e200, 0.0, 0.0))}


@pytest.mark.parametrize("config", list(CONFIGS))
def test_device_equals_twin_with_special_epochs_scattered_in(g, scattered, config):
    c, w, want, dead, lb = scattered
    kw = CONFIGS[config]
    weights = w if config == "weights_mask" else None
    host = g.position_fix_host(*c.args(), weights=weights, **kw)
    dev = device(g, c, weights, **kw)
    same_bits(dev, host)
    again = device(g, c, weights, **kw)  # the same call twice: the same bits
    same_bits(again, dev)
    assert not host.used[:, dead].any() and not host.sat[:, dead].any()
    # what every epoch must show under this configuration, on the device (its bits are the twin's)
    few = {e for e, (kind, _) in want.items() if kind in ("three", "nan", "nan_rx") or (kind == "weights_three" and weights is not None)}
    twin_epochs = {e for e, (kind, _) in want.items() if kind == "twins"}
    starved = {e for e, (kind, _) in want.items() if kind == "mask_starved"}
    status = dev.status
    for e in range(c.E):
        if e in few:
            expect = lb.FEW_SATS
        elif config == "far_start":  # the sums are not finite, whatever the geometry: tested before the pivots
            expect = lb.NONFINITE
        elif e in twin_epochs:
            expect = lb.SINGULAR
        elif config == "max_iter_1":
            expect = lb.NOT_CONVERGED
        elif e in starved and config == "weights_mask":
            expect = lb.MASK_STARVED
        else:
            expect = None
        if expect is not None:
            assert status[e] == expect, (e, want.get(e), status[e], expect)
        else:
            assert status[e] & ~(lb.MASKED | lb.MASK_STARVED) == 0, (e, status[e])
        if expect in (lb.FEW_SATS, lb.NONFINITE, lb.SINGULAR):
            assert dev.x[e] == 0.0 and dev.gdop[e] == 0.0 and not dev.used[e].any() and not dev.resid[e].any()
    if config == "max_iter_1":
        assert (dev.iterations[status == lb.NOT_CONVERGED] == 1).all() and dev.xyz[status == lb.NOT_CONVERGED].all()
    if config in ("weights_mask", "plain"):
        good = np.array([e not in few and e not in twin_epochs for e in range(c.E)])
        assert np.linalg.norm(dev.xyz[good] - c.truth_xyz[good], axis=1).max() < 1e-3
    if config == "weights_mask":
        idx = sorted(starved)
        assert (status & lb.MASKED).any() and (dev.num_used[idx] == 5).all() and (dev.used[idx].sum(axis=1) == 5).all()
        assert ((dev.sin_el[idx] >= MASK_SIN) & (dev.used[idx] != 0)).sum(axis=1).tolist() == [3] * len(idx)
    print(config, "status counts", {int(s): int((status == s).sum()) for s in np.unique(status)})


def test_every_subset_of_the_optional_outputs(g):
    c = case_of(30, 5)
    host = g.position_fix_host(*c.args(), mask_sin=0.2)
    for n in range(len(OUTPUTS) + 1):
        for outs in itertools.combinations(OUTPUTS, n):
            dev = device(g, c, outputs=outs, mask_sin=0.2)
            same_bits(dev, host, outs)
            assert set(dev._raw) == {"fixes", *outs}


def test_refusals_of_the_device_entry_point(g):
    import torch

    from gpuacceleratedtracking_amd import _lib

    c = case_of(30, 3)
    for kw in (dict(max_iter=0), dict(tol_m=0.0), dict(flags=1), dict(mask_sin=float("nan"))):
        with pytest.raises(_lib.GatError):
            device(g, c, **kw)
    with pytest.raises(ValueError):
        g.position_fix(c.ephs, torch.from_numpy(c.tx_ms).cuda(), torch.from_numpy(c.tx_frac).cuda().float(), torch.from_numpy(c.rx_ms).cuda(),
                       torch.from_numpy(c.rx_frac).cuda())
    with pytest.raises(ValueError):
        g.position_fix(c.ephs[:5], torch.from_numpy(c.tx_ms).cuda(), torch.from_numpy(c.tx_frac).cuda(), torch.from_numpy(c.rx_ms).cuda(),
                       torch.from_numpy(c.rx_frac).cuda())
    # a tensor that is not on the device never reaches the kernel
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
    for host_one in range(4):
        args = [t(a).cuda() if i != host_one else t(a) for i, a in enumerate((c.tx_ms, c.tx_frac, c.rx_ms, c.rx_frac))]
        with pytest.raises(ValueError):
            g.position_fix(c.ephs, *args)
    with pytest.raises(ValueError):
        g.position_fix(c.ephs, t(c.tx_ms).cuda(), t(c.tx_frac).cuda(), t(c.rx_ms).cuda(), t(c.rx_frac).cuda(), t(np.ones(c.tx_ms.shape)))
    same_bits(device(g, c), g.position_fix_host(*c.args()))  # the context still works
