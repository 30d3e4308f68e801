"""gat_position_fix on the device against its host twin, byte for byte on fixes, sat, resid, sin_el and used, over the whole domain
gat.h admits (tests/fix_domain.py): every hostile entry -- fields of the ephemeris that are not finite, eccentricities and
semi-axes at and beyond the fence of ``usable``, orbits that are usable by the letter and garbage by their numbers (sqrt_a = 0.004
and 0.0086 and a transmit time of 1e19 s put the sine's argument at 1e18 rad, where its quadrant was once taken by a conversion
that is undefined from 2^63 on and differs between the builds), times and weights at their edges -- in tiles of two workgroups and
one epoch, a hostile epoch among the clean ones of each workgroup and one alone in the last; the configurations at the edges of
gat_fix_config; a start on a satellite; orbits far from GPS-nominal; and K = 1, 2, 3, which can only be GAT_FIX_FEW_SATS.  What
the twin computes there is compared with gat.h in tests/test_position_domain_host.py; here the device must give the twin's bits,
and the classes are asserted on the device's own outputs once more.  No launch has more than a few hundred epochs."""
import numpy as np
import pytest

from tests import fix_cases as fc
from tests import fix_domain as fd

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g():
    import gpuacceleratedtracking_amd as g
    g.load_library()
    return g


def device(g, c, weights=None, **kw):
    import torch

    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    return g.position_fix(c.ephs, t(c.tx_ms), t(c.tx_frac), t(c.rx_ms), t(c.rx_frac), t(weights), **kw)


def same_bits(dev, host, what=""):
    differ = np.flatnonzero([a.tobytes() != b.tobytes() for a, b in zip(dev.fixes, host.fixes)])
    assert differ.size == 0, (what, "fixes of epochs", differ[:10], dev.fixes[differ[:3]], host.fixes[differ[:3]])
    for name in fd.OUTPUTS:
        a, b = getattr(dev, name), getattr(host, name)
        assert a.shape == b.shape and a.dtype == b.dtype
        if a.tobytes() != b.tobytes():
            at = np.argwhere(a.view(np.uint64 if a.dtype == np.float64 else np.uint8) != b.view(np.uint64 if b.dtype == np.float64 else np.uint8))
            raise AssertionError((what, name, "differs at", at[:10].tolist(), a[tuple(at[0])], b[tuple(at[0])]))


@pytest.mark.parametrize("K", [64, 12])
def test_device_equals_twin_on_every_hostile_entry(g, K):
    per_group = g.position_plan(1, K)["waves_per_workgroup"]
    tiles = fd.hostile(K, per_group)
    assert g.position_plan(tiles[0].E, K)["workgroups"] == 3 and tiles[0].E == 2 * per_group + 1 and tiles[0].hostile[-1] == tiles[0].E - 1
    assert all(t.hostile[i] // per_group == i and any(e // per_group == i for e in t.clean) for t in tiles for i in (0, 1))
    for n, t in enumerate(tiles):
        for weights in (t.weights, None):
            host = g.position_fix_host(*t.args(), weights=weights)
            dev = device(g, t.case, weights)
            labels = sorted({label for label, _, _ in t.entries})
            same_bits(dev, host, (K, n, labels))
            # the classes, on the device's own outputs
            want_used = t.want_used if weights is not None else t.want_ok
            assert np.array_equal(dev.sat.any(axis=2), t.want_ok) and (dev.num_valid == t.want_ok.sum(axis=1)).all(), labels
            assert (dev.num_used == want_used.sum(axis=1)).all(), labels
        decisive = [label for label in labels if label in ("sqrt_a=0.004", "sqrt_a=0.0086", "tx_frac=1e+19")]
        if decisive:
            for label, e, k in t.entries:
                if label in decisive:
                    print(f"K = {K}: {label} at epoch {e}, channel {k}: device sat {dev.sat[e, k].tolist()}, the twin's bits; fix status {dev.status[e]}")


@pytest.mark.parametrize("name", list(fd.CONFIGS))
def test_device_equals_twin_under_every_configuration(g, name):
    c = fd.config_case()
    kw = fd.CONFIGS[name]
    dev = device(g, c, **kw)
    same_bits(dev, g.position_fix_host(*c.args(), **kw), name)
    fd.check_config(name, dev, c, g.position_fix_host(*c.args()))


def test_a_start_on_a_satellite_is_nonfinite_on_the_device(g):
    lb = g.positioning
    c = fd.config_case()
    e = 2
    k, xyz = fd.on_a_satellite(c, e, g.position_fix_host(*c.args()).sat)
    dev = device(g, c, init_xyz=xyz)
    same_bits(dev, g.position_fix_host(*c.args(), init_xyz=xyz), "start on a satellite")
    assert dev.status[e] == lb.NONFINITE and dev.iterations[e] == 0 and not dev.xyz[e].any() and not dev.used[e].any()
    assert (dev.status[np.arange(c.E) != e] & lb.NONFINITE == 0).all()


def test_device_equals_twin_on_the_wide_orbits(g):
    w = fd.wide()
    host = g.position_fix_host(*w.args())
    dev = device(g, w)
    same_bits(dev, host, "wide orbits")
    assert dev.sat.all() and (dev.num_valid == w.K).all()


@pytest.mark.parametrize("K", [1, 2, 3])
def test_fewer_than_four_channels_are_few_sats(g, K):
    """every epoch is GAT_FIX_FEW_SATS and every output of it zero but status, num_valid, num_used and iterations -- and ``sat``, which
    gat.h keeps for every channel that counts, whatever became of the fix"""
    lb = g.positioning
    per_group = g.position_plan(1, K)["waves_per_workgroup"]
    c = fc.case("short", 30, K, 8).tiled(2 * per_group + 1)
    assert (c.tx_ms >= 0).all()
    dev = device(g, c)
    same_bits(dev, g.position_fix_host(*c.args()), K)
    assert (dev.status == lb.FEW_SATS).all() and (dev.num_valid == K).all() and (dev.num_used == K).all() and (dev.iterations == 0).all()
    for name in ("x", "y", "z", "clock_bias_s", "rms_residual_m", "last_step_m", "gdop", "pdop"):
        assert not getattr(dev, name).any(), name
    assert not dev.resid.any() and not dev.sin_el.any() and not dev.used.any() and dev.sat.all()
