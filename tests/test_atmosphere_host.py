"""The range corrections' rule on the host: the arctangent against mpmath over its whole domain, the twin
(gat_range_corrections_host) against the numpy restatement of tests/atm_ref.py over the cases of tests/atm_cases.py, the model's
night side and zenith, and subframe 4, page 18 through the encoder, the decoder and back.  No device."""
import numpy as np
import pytest

import gpuacceleratedtracking_amd as g
from gpuacceleratedtracking_amd import _lib, atmosphere
from tests import atm_cases as ac
from tests import atm_ref as ar
from tests import fix_cases as fc

ATAN_BOUND = 1e-15  # rad: the bound fix_sincos carries


def _exact(y, x):
    """mpmath's angle of every pair as (the nearest double, what is left of it)"""
    import mpmath as mp

    mp.mp.prec = 120
    hi, lo = np.empty(len(y)), np.empty(len(y))
    for i, (a, b) in enumerate(zip(y, x)):
        m = mp.atan2(mp.mpf(float(a)), mp.mpf(float(b))) if (a != 0.0 or b != 0.0) else mp.mpf(0)
        hi[i] = float(m)
        lo[i] = float(m - mp.mpf(hi[i]))
    return hi, lo


def _error(got, hi, lo):
    return np.abs((got - hi) - lo)


def test_atan2_powers_of_two():
    """both arguments in +-2^k, k = -1074 .. 1023: the exact angle depends on the difference of the exponents and the signs alone"""
    ks = np.arange(-1074, 1024)
    mag = np.ldexp(1.0, ks)
    assert mag[0] == 5e-324 and np.isfinite(mag[-1])
    d = np.arange(-2097, 2098)
    worst = 0.0
    import mpmath as mp

    mp.mp.prec = 120
    for sy in (1.0, -1.0):
        for sx in (1.0, -1.0):
            ref = [mp.atan2(sy * mp.ldexp(1, int(v)), mp.mpf(sx)) for v in d]  # the angle of (sx, sy 2^d)
            hi = np.array([float(m) for m in ref])
            lo = np.array([float(m - mp.mpf(h)) for m, h in zip(ref, hi)])
            idx = (ks[:, None] - ks[None, :]) + 2097  # ky - kx
            got = atmosphere.atan2_host(sy * mag[:, None], sx * mag[None, :])
            worst = max(worst, float(_error(got, hi[idx], lo[idx]).max()))
    print(f"atan2 over +-2^k x +-2^k: max error {worst:.3e} rad")
    assert worst <= ATAN_BOUND


def test_atan2_octant_edges_and_zeros():
    """every octant edge with four neighbours a side, at several magnitudes, and the signed zeros"""
    ys, xs = [], []
    for m in (1.0, 3.7, 2.0 ** -1000, 2.0 ** 1000, 5e-324 * 64):
        for ex, ey in ((1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1)):
            x0, y0 = ex * m, ey * m
            for which in (0, 1):  # step y about the edge, then x
                for n in range(-4, 5):
                    a, b = x0, y0
                    tgt = np.inf if n > 0 else -np.inf
                    for _ in range(abs(n)):
                        if which == 0:
                            b = np.nextafter(b, tgt)
                        else:
                            a = np.nextafter(a, tgt)
                    ys.append(b), xs.append(a)
    ys, xs = np.array(ys), np.array(xs)
    hi, lo = _exact(ys, xs)
    got = atmosphere.atan2_host(ys, xs)
    worst = float(_error(got, hi, lo).max())
    print(f"atan2 at the octant edges ({len(ys)} points): max error {worst:.3e} rad")
    assert worst <= ATAN_BOUND
    z = atmosphere.atan2_host([0.0, -0.0, 0.0, -0.0, 0.0, -0.0, 0.0, -0.0], [1.0, 1.0, -1.0, -1.0, 0.0, 0.0, -0.0, -0.0])
    assert z[0] == 0.0 and not np.signbit(z[0]) and z[1] == 0.0 and np.signbit(z[1])
    assert z[2] == np.pi and z[3] == -np.pi
    assert (z[4:] == 0.0).all() and not np.signbit(z[4:]).any()  # x = y = 0: +0
    bad = atmosphere.atan2_host([np.nan, 1.0, np.inf, -np.inf, np.inf], [1.0, np.nan, np.inf, np.inf, -np.inf])
    assert np.isnan(bad).all()  # what the caller's finiteness test catches
    one = atmosphere.atan2_host([1.0, -1.0, np.inf, 1.0], [np.inf, -np.inf, 1.0, 0.0])
    assert one[0] == 0.0 and one[1] == -np.pi and one[2] == np.pi / 2 and one[3] == np.pi / 2


def test_atan2_unit_circle():
    rng = np.random.default_rng(20261021)
    th = rng.uniform(-np.pi, np.pi, 400000)
    ys, xs = np.sin(th), np.cos(th)
    hi, lo = _exact(ys, xs)
    worst = float(_error(atmosphere.atan2_host(ys, xs), hi, lo).max())
    print(f"atan2 on the unit circle (400000 points): max error {worst:.3e} rad")
    assert worst <= ATAN_BOUND


def _twin(a, **kw):
    return g.range_corrections_host(*a.args(), a.fix0, iono=a.iono, zenith=a.zenith, **kw)


@pytest.mark.parametrize("name", fc.ALL)
def test_twin_against_restatement(name):
    """delays within 1e-9 m and geometry within 1e-12: roundings of 1e-16 on at most 150 m through about 40 operations stay under
    1e-11 m"""
    a = ac.case(name)
    assert (a.E, a.K) == (8, 30)
    corr = _twin(a)
    assert (corr.epoch_status == 0).all()
    assert (corr.channel_status[a.seen] == atmosphere.CH_CORRECTED).all() and (corr.channel_status[~a.seen] == 0).all()
    worst = {"iono": 0.0, "tropo": 0.0, "geom": 0.0}
    nights = 0
    for e in range(a.E):
        r, s = a.at_fix0[e], a.seen[e]
        worst["iono"] = max(worst["iono"], np.abs(corr.iono[e] - r["iono"])[s].max())
        worst["tropo"] = max(worst["tropo"], np.abs(corr.tropo[e] - r["tropo"])[s].max())
        for i, n in enumerate(("sin_el", "cos_a", "sin_a")):
            worst["geom"] = max(worst["geom"], np.abs(corr.geom[e, :, i] - r[n])[s].max())
        # the night side is exactly F 5e-9 c in the restatement, and the twin has it
        night = s & (np.abs(r["xx"]) >= 1.57)
        nights += int(night.sum())
        assert np.array_equal(r["iono"][night], r["night"][night])
        assert (np.abs(corr.iono[e] - r["night"])[night] <= 1e-9).all()
        # the corrected fraction is the fraction plus the delay over c; a channel without a measurement passes through
        want = a.case.tx_frac[e] + (r["iono"] + r["tropo"]) / ar.C_LIGHT
        assert (np.abs(corr.tx_frac[e] - want)[s] <= 1e-17).all()
        assert np.array_equal(corr.tx_frac[e][~s], a.case.tx_frac[e][~s]) and (corr.delay[e][~s] == 0.0).all() and (corr.geom[e][~s] == 0.0).all()
    print(f"{name}: twin - restatement: iono {worst['iono']:.3e} m, tropo {worst['tropo']:.3e} m, geometry {worst['geom']:.3e}; {nights} night-side channels")
    assert worst["iono"] <= 1e-9 and worst["tropo"] <= 1e-9 and worst["geom"] <= 1e-12
    assert nights > 0 and nights < a.seen.sum()


def test_switches_and_floor():
    a = ac.case("mid")
    both = _twin(a)
    io = g.range_corrections_host(*a.args(), a.fix0, iono=a.iono)
    tr = g.range_corrections_host(*a.args(), a.fix0, zenith=a.zenith)
    none = g.range_corrections_host(*a.args(), a.fix0)
    assert np.array_equal(io.iono, both.iono) and (io.tropo == 0.0).all() and np.array_equal(tr.tropo, both.tropo) and (tr.iono == 0.0).all()
    assert none.tx_frac.tobytes() == a.case.tx_frac.tobytes() and (none.delay == 0.0).all()
    assert np.array_equal(none.geom, both.geom) and np.array_equal(none.channel_status, both.channel_status)
    # the config's scalars are the array's values
    e = 3
    pair = g.range_corrections_host(*a.args(), a.fix0, iono=a.iono, zenith=tuple(a.zenith[e]))
    assert pair.delay[e].tobytes() == both.delay[e].tobytes()
    # a floor: the channels below it keep their fraction and their geometry, and say so
    floor = float(np.median(both.sin_el[a.seen]))
    fl = _twin(a, floor_sin=floor)
    low = a.seen & (both.sin_el < floor)
    assert low.any() and (fl.channel_status[low] == atmosphere.CH_LOW).all() and (fl.delay[low] == 0.0).all()
    assert np.array_equal(fl.tx_frac[low], a.case.tx_frac[low]) and np.array_equal(fl.geom, both.geom)
    assert np.array_equal(fl.tx_frac[~low], both.tx_frac[~low])
    # the carrier scales the ionosphere alone
    l2 = _twin(a, carrier_hz=1227.6e6)
    assert np.allclose(l2.iono, both.iono * (1575.42 / 1227.6) ** 2, rtol=1e-14) and np.array_equal(l2.tropo, both.tropo)


def test_zenith_is_the_sum():
    zd, zw = 2.3012, 0.1234
    corr = g.range_corrections_host(*ac.overhead(), zenith=(zd, zw))
    assert corr.channel_status[0, 0] == atmosphere.CH_CORRECTED and corr.sin_el[0, 0] == 1.0
    print(f"zenith: tropo - (z_d + z_w) = {corr.tropo[0, 0] - (zd + zw):.3e} m")
    assert abs(corr.tropo[0, 0] - (zd + zw)) <= 1e-12
    assert corr.geom[0, 0, 1] ** 2 + corr.geom[0, 0, 2] ** 2 == pytest.approx(1.0, abs=1e-15)


def test_tropo_zenith_is_saastamoinen():
    h, s = np.array([0.0, 520.0, 2850.0]), np.sin(np.radians([0.0, 48.1, -33.9]))
    z = g.tropo_zenith(h, s)
    zd, zw = ar.tropo_zenith(h, s)
    assert z.shape == (3, 2) and np.allclose(z[:, 0], zd, rtol=1e-14) and np.allclose(z[:, 1], zw, rtol=1e-14)
    assert 2.25 < z[0, 0] < 2.35 and 0.05 < z[0, 1] < 0.2
    import torch

    zt = g.tropo_zenith(torch.from_numpy(h), torch.from_numpy(s))
    assert np.allclose(zt.numpy(), z, rtol=1e-13)
    dry = g.tropo_zenith(h, s, humidity=0.0)
    assert (dry[:, 1] == 0.0).all() and np.array_equal(dry[:, 0], z[:, 0])


def test_refusals_and_plan():
    a = ac.case("mid")
    for kw in ({"carrier_hz": 0.0}, {"carrier_hz": np.nan}, {"carrier_hz": -1.0}, {"floor_sin": np.inf}, {"floor_sin": np.nan}, {"flags": 4}):
        with pytest.raises(g.GatError):
            _twin(a, **kw)
    p = g.atmosphere_plan(43, 6)
    assert p == {"workgroups": 2, "waves_per_workgroup": 4, "threads": 256, "lds_bytes": 0, "scratch_bytes": 0}
    assert g.atmosphere_plan(4, 64)["workgroups"] == 1 and g.atmosphere_plan(5, 64)["workgroups"] == 2
    with pytest.raises(g.GatError):
        g.atmosphere_plan(1, 65)


# ---- subframe 4, page 18 ------------------------------------------------------------------------------------------------------------------
_P18 = (("data_id", 2, False, 0), ("sv_id", 6, False, 0), ("wnt", 8, False, 0), ("dt_ls", 8, True, 0), ("wnlsf", 8, False, 0), ("dn", 8, False, 0),
        ("dt_lsf", 8, True, 0), ("a0", 32, True, -30), ("a1", 24, True, -50), ("tot", 8, False, 12))
_P18_IONO = ((-30, -27, -24, -24), (11, 14, 16, 16))


def _page(raw: dict) -> atmosphere.Page18:
    rec = np.zeros((), dtype=_lib.PAGE18_DTYPE)
    for name, _, _, ex in _P18:
        rec[name] = raw[name] * (2.0 ** ex if rec.dtype[name].kind == "f" else 1)
    for i in range(4):
        rec["alpha"][i], rec["beta"][i] = raw["alpha"][i] * 2.0 ** _P18_IONO[0][i], raw["beta"][i] * 2.0 ** _P18_IONO[1][i]
    return atmosphere.Page18(rec)


def _decode(payload):
    sym = 1.0 - 2.0 * np.concatenate([g.lnav_subframe(200 + i, 4, payload=payload) for i in range(3)]).astype(np.float64)
    return g.lnav_page18(g.decode_navigation_host(sym[None, :], "LNAV"), 0)


def _span(bits, signed):
    return (-(1 << (bits - 1)), (1 << (bits - 1)) - 1) if signed else (0, (1 << bits) - 1)


def test_page18_round_trip():
    """words -> fields -> words is the identity on every bit, for random fields and each field's extremes, and the decoder gives the
    fields back through a subframe"""
    rng = np.random.default_rng(18)
    raws = []
    for _ in range(40):
        raw = {n: int(rng.integers(*_span(b, s), endpoint=True)) for n, b, s, _ in _P18}
        raw["alpha"], raw["beta"] = [int(v) for v in rng.integers(-128, 128, 4)], [int(v) for v in rng.integers(-128, 128, 4)]
        raws.append(raw)
    base = dict(raws[0])
    for n, b, s, _ in _P18:
        for v in _span(b, s):
            raws.append({**base, n: v})
    for i in range(4):
        for v in (-128, 127):
            for which in ("alpha", "beta"):
                r = {**base, which: list(base[which])}
                r[which][i] = v
                raws.append(r)
    seen = set()
    for raw in raws:
        raw["sv_id"] = 56  # the page the decoder looks for
        page = _page(raw)
        payload = g.lnav_page18_payload(page)
        assert payload.shape == (190,) and (payload[176:] == 0).all()
        back = _decode(payload)
        assert back.valid == 1
        rec, got = page.record.copy(), back.record.copy()
        rec["valid"] = 1
        assert got.tobytes() == rec.tobytes(), (raw, got, rec)
        assert np.array_equal(g.lnav_page18_payload(back), payload)  # every bit
        seen.add(payload.tobytes())
    assert len(seen) > 60
    # another page of subframe 4, a bad frame and no frame at all give no page
    other = g.lnav_page18_payload(_page({**base, "sv_id": 63}))
    assert _decode(other).valid == 0
    k = ac.broadcast_iono()
    assert k.alpha == (12 * 2.0 ** -30, 2 * 2.0 ** -27, -1 * 2.0 ** -24, -1 * 2.0 ** -24) and k.beta == (44 * 2.0 ** 11, 8 * 2.0 ** 14, -1 * 2.0 ** 16, -6 * 2.0 ** 16)
