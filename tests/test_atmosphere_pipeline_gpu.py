"""position_fix_corrected on the device: fix -> range corrections -> fix (or RAIM) with nothing read back before the caller looks,
the bytes of the three host twins chained on the same inputs, and the host pipeline's bound against the truth
(tests/test_atmosphere_pipeline_host.py) met on the device.  The standard atmosphere's zenith delays are made on the device by torch
operations, outside the rule: the twins are given the array the device made."""
import numpy as np
import pytest

from tests import atm_cases as ac
from tests import fix_cases as fc
from tests.test_atmosphere_pipeline_host import P_FA, SIGMA_M, bound

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g():
    import gpuacceleratedtracking_amd as g
    g.load_library()
    return g


def cuda(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def twins(g, a, zenith, raim):
    c = a.case
    first = g.position_fix_host(*c.args(), outputs=())
    corr = g.range_corrections_host(*c.args(), first, iono=a.iono, zenith=zenith)
    second = g.position_fix_raim_host if raim else g.position_fix_host
    return corr, second(c.ephs, c.tx_ms, corr.tx_frac, c.rx_ms, c.rx_frac, **({"sigma_m": SIGMA_M, "p_fa": P_FA} if raim else {}))


@pytest.mark.parametrize("raim", [False, True])
@pytest.mark.parametrize("name", fc.ALL)
def test_the_chain_on_the_device_has_the_twins_bytes(g, name, raim):
    a = ac.case(name)
    c = a.case
    args = (c.ephs, cuda(c.tx_ms), cuda(c.tx_frac), cuda(c.rx_ms), cuda(c.rx_frac))
    fix, corr = g.position_fix_corrected(*args, iono=a.iono, tropo=cuda(a.zenith), raim=raim, **({"sigma_m": SIGMA_M, "p_fa": P_FA} if raim else {}))
    assert fix._host is None and corr._host is None, "something was read back before the caller looked"
    corr_host, fix_host = twins(g, a, a.zenith, raim)
    for name_ in ("tx_frac_out", "delay", "geom", "channel_status", "epoch_status"):
        assert getattr(corr, name_).tobytes() == getattr(corr_host, name_).tobytes(), name_
    assert fix.fixes.tobytes() == fix_host.fixes.tobytes() and fix.resid.tobytes() == fix_host.resid.tobytes() and fix.used.tobytes() == fix_host.used.tobytes()
    if raim:
        assert fix.integrity.tobytes() == fix_host.integrity.tobytes() and not fix.detected.any()
    err = np.linalg.norm(fix.xyz - c.truth_xyz, axis=1)
    b = np.array([bound(a, e) for e in range(a.E)])
    print(f"{name}, raim {raim}: corrected on the device, per epoch (error / B) " + ", ".join(f"{x:.2e}/{y:.2e}" for x, y in zip(err, b)))
    assert (fix.status == 0).all() and (err <= b).all()


def test_the_standard_atmosphere_on_the_device(g):
    """tropo="standard": the zenith delays come from the first fix's records by torch operations and stay on the device; they are
    the restatement's at the first fix's own position within 1e-9 m (a few roundings of 1e-16 on 2.4 m, and of the height), and the
    twins given that array have the device's bytes.  (Against the true site they differ by what the first fix's 5 to 70 m of height
    are: 29 mm at most here.)"""
    from tests import atm_ref as ar

    a = ac.case("mid")
    c = a.case
    fix, corr = g.position_fix_corrected(c.ephs, cuda(c.tx_ms), cuda(c.tx_frac), cuda(c.rx_ms), cuda(c.rx_frac), iono=a.iono, tropo="standard")
    assert fix._host is None and corr._host is None
    zen = corr.zenith
    at_fix0 = np.array([ar.tropo_zenith(h, np.sin(lat)) for lat, _, h in (ar.geodetic(a.fix0.xyz[e]) for e in range(a.E))])
    print(f"zenith delays on the device against the restatement's at the first fix: {np.abs(zen - at_fix0).max():.3e} m; at the true site: "
          f"{np.abs(zen - a.zenith).max():.3e} m")
    assert zen.shape == (a.E, 2) and np.abs(zen - at_fix0).max() <= 1e-9
    corr_host, fix_host = twins(g, a, zen, False)
    assert corr.tx_frac.tobytes() == corr_host.tx_frac.tobytes() and corr.delay.tobytes() == corr_host.delay.tobytes()
    assert fix.fixes.tobytes() == fix_host.fixes.tobytes()
    assert (fix.status == 0).all()
