"""fix -> corrections -> fix (or RAIM) -> velocity through the host twins, on the receivers of tests/atm_cases.py that see a real sky.

The uncorrected fix is more than a metre from the truth in every epoch (4.9 to 71 m over the cases).  The corrected one is within
a per-epoch bound B of it that the restatement alone gives: B = GDOP sqrt(n) (930 d_max / c + max_k |d_k at the first fix - d_k at the
truth|) + 1e-3 m -- the time-shift form moves a satellite by at most 930 m/s d / c along the line of sight, the delays are formed at
the first fix and not at the truth, a least-squares solution moves by at most GDOP times the norm of what its n ranges move by, and
1e-3 m is the cases' own bound against the truth.  With thresholds at sigma = 3 m and p_fa = 1e-3 the integrity test detects no
corrected epoch; of the 24 uncorrected ones it detects 8 -- those whose lowest satellites carry tens of metres of troposphere --,
leaves a channel out of 3 of them and hands on fixes that are all still metres off, some with a status that says excluded and 16
with a status that says tested and passed: the long fault the corrections remove.  The velocity fix moves by less than its own bound of 1e-6 m/s when its transmit times are
the corrected ones."""
import numpy as np
import pytest

import gpuacceleratedtracking_amd as g
from tests import atm_cases as ac
from tests import fix_cases as fc
from tests import fix_ref as ref
from tests import vel_cases as vc

SIGMA_M, P_FA = 3.0, 1e-3
SAT_SPEED_LOS = 930.0  # m/s: a GPS satellite's largest speed along a line of sight from the ground


def bound(a: ac.AtmCase, e: int) -> float:
    """B of epoch e, from the restatement alone"""
    s = a.seen[e]
    c = a.case
    pos, _ = ref.satellite(c.ephs[s], c.tx_ms[e][s], c.tx_frac[e][s])
    _, los = ref.geometry(pos, c.truth_xyz[e])
    rows = np.concatenate([-los, np.ones((los.shape[0], 1))], axis=1)
    gdop = float(np.sqrt(np.trace(np.linalg.inv(rows.T @ rows))))
    d0 = (a.at_fix0[e]["iono"] + a.at_fix0[e]["tropo"])[s]
    dt = (a.at_truth[e]["iono"] + a.at_truth[e]["tropo"])[s]
    return gdop * np.sqrt(s.sum()) * (SAT_SPEED_LOS * d0.max() / ref.C_LIGHT + np.abs(d0 - dt).max()) + 1e-3


def chain(a: ac.AtmCase, raim: bool = False):
    """(corrections at the first fix, the second fix) by the twins"""
    c = a.case
    corr = g.range_corrections_host(*c.args(), a.fix0, iono=a.iono, zenith=a.zenith)
    fix = g.position_fix_raim_host if raim else g.position_fix_host
    return corr, fix(c.ephs, c.tx_ms, corr.tx_frac, c.rx_ms, c.rx_frac, **({"sigma_m": SIGMA_M, "p_fa": P_FA} if raim else {}))


@pytest.mark.parametrize("name", fc.ALL)
def test_the_corrected_fix_finds_the_truth(name):
    a = ac.case(name)
    c = a.case
    before = np.linalg.norm(a.fix0.xyz - c.truth_xyz, axis=1)
    assert (a.fix0.status == 0).all() and (before > 1.0).all(), before
    corr, fix = chain(a)
    after = np.linalg.norm(fix.xyz - c.truth_xyz, axis=1)
    b = np.array([bound(a, e) for e in range(a.E)])
    print(f"{name}: uncorrected {before.min():.2f} .. {before.max():.2f} m from the truth; corrected per epoch (error / B) "
          + ", ".join(f"{x:.2e}/{y:.2e}" for x, y in zip(after, b)))
    assert (fix.status == 0).all() and (after <= b).all()
    assert (np.abs(fix.clock_bias_s - c.truth_bias_s) * ref.C_LIGHT <= b).all()
    # what was added at the truth is what the corrections find at the first fix, within the same term of B
    d = corr.iono + corr.tropo
    assert (np.abs(d - a.delay)[a.seen] <= b.max()).all() and (d[a.seen] > 2.0).all()


def test_the_integrity_test_on_a_real_sky():
    detected_clean, detected_raw, excluded_raw, total = 0, 0, 0, 0
    for name in fc.ALL:
        a = ac.case(name)
        c = a.case
        _, fix = chain(a, raim=True)
        raw = g.position_fix_raim_host(*c.args(), sigma_m=SIGMA_M, p_fa=P_FA)
        detected_clean += int(fix.detected.sum())
        detected_raw += int(raw.detected.sum())
        excluded_raw += int(((raw.status & g.positioning.EXCLUDED) != 0).sum())
        total += a.E
        assert (fix.status == 0).all() and (fix.integrity["status"] == 0).all()
        off = np.linalg.norm(raw.xyz - c.truth_xyz, axis=1)
        assert (off > 1.0).all()  # excluded or not, the uncorrected fix stays metres off
    print(f"sigma {SIGMA_M} m, p_fa {P_FA}: corrected epochs detected {detected_clean} of {total}; uncorrected detected {detected_raw}, with a channel left out {excluded_raw}")
    assert detected_clean == 0 and detected_raw > 0


@pytest.mark.parametrize("name", fc.ALL)
def test_the_velocity_fix_takes_the_corrected_times(name):
    a = ac.case(name)
    c = a.case
    corr, fix = chain(a)
    m = vc.moving(c, fix=fix)
    plain = g.velocity_fix_host(c.ephs, c.tx_ms, c.tx_frac, m.doppler, fix)
    moved = g.velocity_fix_host(c.ephs, c.tx_ms, corr.tx_frac, m.doppler, fix)
    step = np.abs(moved.v_ecef - plain.v_ecef).max()
    err = np.abs(moved.v_ecef - m.v_ecef).max()
    print(f"{name}: the velocity moves by {step:.3e} m/s with the corrected times (its bound 1e-6), {err:.3e} m/s from the truth")
    assert (moved.status == 0).all() and step < 1e-6 and err < 1e-6
