"""The position fix on the host: the ephemeris decoder and encoder, and the host twin gat_position_fix_host against the independent
numpy restatement (tests/fix_ref.py), against the truth the cases (tests/fix_cases.py) were built from, in every special epoch and
in every refusal.  Needs no device.

Bounds.  Satellite state against the restatement: about ten operations at 2.7e7 m x 1.1e-16 each and six angles at 3e-8 m are
under 3e-7 m; the tolerance is 1e-6 m and 1e-12 s (measured: 1.2e-7 m, 9e-22 s).  Fix against the restatement, both converged
(tol_m = 1e-6, max_iter = 12): the residuals' rounding, 2e7 m x 1e-16, times GDOP is under 1e-7 m; the tolerance is 1e-5 m and
1e-13 s (measured: 1.9e-8 m, 3.1e-17 s).  Against the truth: 1e-3 m (measured: 9e-8 m)."""
import numpy as np
import pytest

from tests import fix_cases as fc
from tests import fix_ref as ref

CONVERGED = dict(tol_m=1e-6, max_iter=12)
PI = 3.1415926535898
# name: (bits, signed, log2 of the scale, semicircles) -- IS-GPS-200 table 20-I and 20-III, restated
FIELDS = {"tgd": (8, True, -31, False), "toc": (16, False, 4, False), "af2": (8, True, -55, False), "af1": (16, True, -43, False),
          "af0": (22, True, -31, False), "crs": (16, True, -5, False), "delta_n": (16, True, -43, True), "m0": (32, True, -31, True),
          "cuc": (16, True, -29, False), "e": (32, False, -33, False), "cus": (16, True, -29, False), "sqrt_a": (32, False, -19, False),
          "toe": (16, False, 4, False), "cic": (16, True, -29, False), "omega0": (32, True, -31, True), "cis": (16, True, -29, False),
          "i0": (32, True, -31, True), "crc": (16, True, -5, False), "omega": (32, True, -31, True), "omega_dot": (24, True, -43, True),
          "idot": (14, True, -43, True)}
INTS = {"wn": 10, "ura": 4, "health": 6, "iodc": 10, "fit": 1}


@pytest.fixture(scope="module")
def g():
    import gpuacceleratedtracking_amd as g
    return g


def eph_from_raw(g, raw: dict):
    vals = {}
    for name, (bits, signed, exp, semi) in FIELDS.items():
        vals[name] = float(raw[name]) * 2.0 ** exp * (PI if semi else 1.0)
    for name in INTS:
        vals[name] = int(raw[name])
    return g.Ephemeris(iode=int(raw["iodc"]) & 0xff, **vals)


def raw_extreme(which: str, rng=None) -> dict:
    raw = {}
    for name, (bits, signed, _, _) in FIELDS.items():
        lo, hi = (-(1 << (bits - 1)), (1 << (bits - 1)) - 1) if signed else (0, (1 << bits) - 1)
        raw[name] = {"min": lo, "max": hi, "minus_one": -1 if signed else 1}.get(which, None)
        if raw[name] is None:
            raw[name] = int(rng.integers(lo, hi + 1))
    for name, bits in INTS.items():
        raw[name] = {"min": 0, "max": (1 << bits) - 1, "minus_one": 1}.get(which, None)
        if raw[name] is None:
            raw[name] = int(rng.integers(0, 1 << bits))
    return raw


def symbols_of(g, eph, tows=(200, 201, 202), order=(1, 2, 3)):
    bits = g.lnav_ephemeris_payloads(eph)
    return 1.0 - 2.0 * np.concatenate([g.lnav_subframe(t, sf, payload=bits[sf - 1]) for t, sf in zip(tows, order)]).astype(np.float64)


@pytest.mark.parametrize("which", ["min", "max", "minus_one", "random0", "random1", "random2"])
def test_ephemeris_round_trip(g, which):
    """Ephemeris -> payload bits -> subframes with parity -> +-1 symbols -> the decoder's words -> Ephemeris: every field equal, at the
    extremes of every field (the most negative values, IODC = 1023 above 255) and at random ones"""
    rng = np.random.default_rng(40 + int(which[-1])) if which.startswith("random") else None
    raw = raw_extreme(which, rng)
    eph = eph_from_raw(g, raw)
    nav = g.decode_navigation_host(symbols_of(g, eph)[None, :], "LNAV")
    assert nav.ok[0, :3].all() and nav.subframe_id[0, :3].tolist() == [1, 2, 3]
    back = g.lnav_ephemeris(nav, 0)
    assert back.valid == 1 and back.reason == 0
    for name in g.Ephemeris.FIELDS:
        assert getattr(back, name) == getattr(eph, name), (name, getattr(back, name), getattr(eph, name))
    if which == "max":
        assert back.iodc == 1023 and back.iode == 255 and back.e == (2 ** 32 - 1) * 2.0 ** -33
    if which == "min":
        assert back.m0 == -PI and back.af0 == -(2.0 ** 21) * 2.0 ** -31 and back.idot == -(2.0 ** 13) * 2.0 ** -43 * PI
    assert g.lnav_ephemerides(nav)[0] == back


def test_ephemeris_takes_the_newest_matching_set(g):
    rng = np.random.default_rng(3)
    old, new = eph_from_raw(g, raw_extreme("r", rng)), eph_from_raw(g, raw_extreme("r", rng))
    assert (old.iodc & 0xff) != (new.iodc & 0xff)
    sym = np.concatenate([symbols_of(g, old, (10, 11, 12)), symbols_of(g, new, (13, 14, 15))])
    nav = g.decode_navigation_host(sym[None, :], "LNAV")
    assert nav.ok[0, :6].all()
    assert g.lnav_ephemeris(nav, 0) == g.lnav_ephemeris(g.decode_navigation_host(symbols_of(g, new)[None, :], "LNAV"), 0)
    # the new issue's subframe 1 only: the old issue is the newest complete set and stands until the new one is complete
    fresh = symbols_of(g, new, (13, 14, 15))
    sym = np.concatenate([symbols_of(g, old, (10, 11, 12)), fresh[:300]])
    kept = g.lnav_ephemeris(g.decode_navigation_host(sym[None, :], "LNAV"), 0)
    assert kept.valid == 1 and kept == g.lnav_ephemeris(g.decode_navigation_host(symbols_of(g, old)[None, :], "LNAV"), 0)
    sym = np.concatenate([symbols_of(g, old, (10, 11, 12)), fresh[:600]])  # and its subframe 2: still the old one
    assert g.lnav_ephemeris(g.decode_navigation_host(sym[None, :], "LNAV"), 0) == kept
    # subframe 1 of the new issue with subframes 2 and 3 of the old one, and nothing else: no set of one issue
    sym = np.concatenate([fresh[:300], symbols_of(g, old, (11, 12, 13))[300:]])
    bad = g.lnav_ephemeris(g.decode_navigation_host(sym[None, :], "LNAV"), 0)
    assert bad.valid == 0 and bad.reason == 2 and bad.sqrt_a == 0.0


# where every field lies: subframe, then (first payload bit, bits) of each part, the payload's bit 0 being d1 of word 3 -- restated
# from the interface specification's figures 20-1 (word w, data bit d: 24 (w - 3) + d - 1), not read from the library's table
LAYOUT = {"wn": (1, [(0, 10)]), "ura": (1, [(12, 4)]), "health": (1, [(16, 6)]), "iodc": (1, [(22, 2), (120, 8)]), "tgd": (1, [(112, 8)]),
          "toc": (1, [(128, 16)]), "af2": (1, [(144, 8)]), "af1": (1, [(152, 16)]), "af0": (1, [(168, 22)]),
          "crs": (2, [(8, 16)]), "delta_n": (2, [(24, 16)]), "m0": (2, [(40, 32)]), "cuc": (2, [(72, 16)]), "e": (2, [(88, 32)]),
          "cus": (2, [(120, 16)]), "sqrt_a": (2, [(136, 32)]), "toe": (2, [(168, 16)]), "fit": (2, [(184, 1)]),
          "cic": (3, [(0, 16)]), "omega0": (3, [(16, 32)]), "cis": (3, [(48, 16)]), "i0": (3, [(64, 32)]), "crc": (3, [(96, 16)]),
          "omega": (3, [(112, 32)]), "omega_dot": (3, [(144, 24)]), "idot": (3, [(176, 14)])}
IODE_AT = ((2, 0), (3, 168))  # IODE, 8 bits, in subframes 2 and 3


@pytest.mark.parametrize("name", sorted(LAYOUT))
def test_every_field_lies_where_the_specification_puts_it(g, name):
    """One field set to a pattern with a clear first and last bit, everything else zero: the encoder puts exactly those bits at the
    restated offsets, and a payload built by hand from the offsets decodes to the value -- each direction against the test's own
    layout, so that a field at the wrong offset or two swapped fields of one width cannot pass."""
    sf, parts = LAYOUT[name]
    width = sum(n for _, n in parts)
    pattern = (1 << (width - 1)) | 1 if width > 1 else 1  # the first and the last bit: negative where the field is signed
    if name in FIELDS:
        _, signed, exp, semi = FIELDS[name]
        value = float(pattern - (1 << width) if signed else pattern) * 2.0 ** exp * (PI if semi else 1.0)
    else:
        value = pattern
    want = np.zeros((3, 190), np.uint8)
    at = 0
    for first, n in parts:
        for i in range(n):
            want[sf - 1, first + i] = (pattern >> (width - 1 - at)) & 1
            at += 1
    iode = (pattern & 0xff) if name == "iodc" else 0  # the issue of data goes with IODC: its low 8 bits, in subframes 2 and 3
    for s, first in IODE_AT:
        for i in range(8):
            want[s - 1, first + i] = (iode >> (7 - i)) & 1
    eph = g.Ephemeris(**{name: value}, **({"iode": iode} if name == "iodc" else {}))
    assert np.array_equal(g.lnav_ephemeris_payloads(eph), want), name
    sym = 1.0 - 2.0 * np.concatenate([g.lnav_subframe(7 + i, i + 1, payload=want[i]) for i in range(3)]).astype(np.float64)
    back = g.lnav_ephemeris(g.decode_navigation_host(sym[None, :], "LNAV"), 0)
    assert back.valid == 1
    for other in g.Ephemeris.FIELDS:
        expect = value if other == name else (iode if other == "iode" else (1 if other == "valid" else 0))
        assert getattr(back, other) == expect, (name, other, getattr(back, other), expect)


def test_mismatched_iode_and_failed_parity(g):
    rng = np.random.default_rng(4)
    eph = eph_from_raw(g, raw_extreme("r", rng))
    bits = g.lnav_ephemeris_payloads(eph)
    wrong = bits.copy()
    wrong[2, 168 + 7] ^= 1  # subframe 3's own IODE, its last bit
    sym = 1.0 - 2.0 * np.concatenate([g.lnav_subframe(50 + i, i + 1, payload=wrong[i]) for i in range(3)]).astype(np.float64)
    nav = g.decode_navigation_host(sym[None, :], "LNAV")
    assert nav.ok[0, :3].all()
    bad = g.lnav_ephemeris(nav, 0)
    assert bad.valid == 0 and bad.reason == 2
    sym = symbols_of(g, eph)
    assert g.lnav_ephemeris(g.decode_navigation_host(sym[None, :], "LNAV"), 0).valid == 1
    sym[300 + 4 * 30 + 11] *= -1.0  # one bit of word 5 of subframe 2: its parity fails
    nav = g.decode_navigation_host(sym[None, :], "LNAV")
    assert nav.status[0, 1] == 0x7ff & ~(2 << 4)
    bad = g.lnav_ephemeris(nav, 0)
    assert bad.valid == 0 and bad.reason == 1
    # no frames at all
    none = g.lnav_ephemeris(g.decode_navigation_host(np.ones((1, 10)), "LNAV"), 0)
    assert none.valid == 0 and none.reason == 1


@pytest.fixture(scope="module")
def host_fixes(g):
    return {name: g.position_fix_host(*fc.case(name).args(), **CONVERGED) for name in fc.ALL}


@pytest.fixture(scope="module")
def ref_fixes():
    out = {}
    for name in fc.ALL:
        c = fc.case(name)
        out[name] = [ref.fix(c.ephs, c.tx_ms[e], c.tx_frac[e], c.rx_ms[e], c.rx_frac[e]) for e in range(c.E)]
    return out


@pytest.mark.parametrize("name", fc.ALL)
def test_satellite_states_against_the_restatement(g, host_fixes, ref_fixes, name):
    c, f = fc.case(name), host_fixes[name]
    tk = ref.wrap_week(c.tx_ms * 1e-3 - c.ephs["toe"][None, :])[c.tx_ms >= 0]
    if name == "mid":
        assert tk.min() < -3000 and tk.max() > 3000  # t_k of both signs
    else:  # the week's end lies between toe (and toc) and the transmissions
        late = c.tx_ms[1:][c.tx_ms[1:] >= 0]
        assert (np.abs(late * 1e-3 - c.ephs["toe"][0]) > 302400).all() and (np.abs(late * 1e-3 - c.ephs["toc"][0]) > 302400).all()
        assert np.abs(tk).max() < 3000
    if name == "week_start":
        assert (c.tx_ms[0][c.tx_ms[0] >= 0] > 604799000).all() and c.rx_ms[0] < 1000  # sent in the week before
    pos = np.stack([r["sat"] for r in ref_fixes[name]])
    dts = np.stack([r["dts"] for r in ref_fixes[name]])
    err_m, err_s = np.abs(f.sat[..., :3] - pos).max(), np.abs(f.sat[..., 3] - dts).max()
    print(f"{name}: satellite state max |error| {err_m:.3e} m, clock {err_s:.3e} s")
    assert (np.linalg.norm(f.sat[..., :3], axis=-1)[c.tx_ms >= 0] > 2.6e7).all() and not f.sat[c.tx_ms < 0].any()
    assert err_m <= 1e-6 and err_s <= 1e-12


@pytest.mark.parametrize("name", fc.ALL)
def test_fixes_against_the_restatement_and_the_truth(g, host_fixes, ref_fixes, name):
    c, f = fc.case(name), host_fixes[name]
    assert (f.status == 0).all() and (f.num_used == (c.tx_ms >= 0).sum(axis=1)).all() and (f.num_valid == f.num_used).all()
    xyz = np.stack([r["xyz"] for r in ref_fixes[name]])
    bias = np.array([r["clock_bias_s"] for r in ref_fixes[name]])
    err_m, err_s = np.abs(f.xyz - xyz).max(), np.abs(f.clock_bias_s - bias).max()
    truth_m = np.linalg.norm(f.xyz - c.truth_xyz, axis=1).max()
    print(f"{name}: fix max |error| {err_m:.3e} m, {err_s:.3e} s against the restatement; {truth_m:.3e} m against the truth")
    assert err_m <= 1e-5 and err_s <= 1e-13
    assert truth_m <= 1e-3 and np.abs(f.clock_bias_s - c.truth_bias_s).max() <= 1e-3 / ref.C_LIGHT
    # the other outputs: residuals, elevations, the used set, the dilution of precision
    assert np.abs(f.resid - np.stack([r["resid"] for r in ref_fixes[name]])).max() <= 1e-5
    assert np.abs(f.sin_el - np.stack([r["sin_el"] for r in ref_fixes[name]])).max() <= 1e-9
    assert np.array_equal(f.used.astype(bool), c.tx_ms >= 0)
    assert (f.rms_residual_m < 1e-6).all() and (f.last_step_m < 1e-6).all() and (f.iterations <= 8).all()
    for e in range(c.E):
        los = ref_fixes[name][e]["sat"]  # the unweighted dilution of precision from the restatement's geometry
        ok = c.tx_ms[e] >= 0
        _, u = ref.geometry(los[ok], xyz[e])
        q = np.linalg.inv(np.concatenate([-u, np.ones((ok.sum(), 1))], axis=1).T @ np.concatenate([-u, np.ones((ok.sum(), 1))], axis=1))
        assert abs(f.pdop[e] - np.sqrt(np.trace(q[:3, :3]))) < 1e-9 and abs(f.gdop[e] - np.sqrt(np.trace(q))) < 1e-9


def test_weights_and_mask_against_the_restatement(g):
    c = fc.case("mid")
    rng = np.random.default_rng(8)
    w = rng.uniform(0.2, 3.0, c.tx_ms.shape)
    w[1, np.flatnonzero(c.tx_ms[1] >= 0)[0]] = 0.0   # excluded by its weight
    w[2, np.flatnonzero(c.tx_ms[2] >= 0)[1]] = np.nan
    # the case's transmit times are consistent: perturb them (metres of noise) so that weights and the used set matter
    noisy = c.copy()
    noisy.tx_frac = np.where(c.tx_ms >= 0, np.clip(c.tx_frac + rng.normal(0.0, 3.0, c.tx_ms.shape) / ref.C_LIGHT, 0.0, 0.000999), 0.0)
    mask = float(np.sin(np.radians(15.0)))
    assert (((c.sin_el > 0) & (c.sin_el < mask - 0.01)).sum(axis=1) >= 1).all() and ((c.sin_el > mask + 0.01).sum(axis=1) >= 5).all()
    f = g.position_fix_host(*noisy.args(), weights=w, mask_sin=mask, **CONVERGED)
    lb = g.positioning
    assert (f.status == lb.MASKED).all()
    for e in range(c.E):
        r = ref.fix(noisy.ephs, noisy.tx_ms[e], noisy.tx_frac[e], noisy.rx_ms[e], noisy.rx_frac[e], weights=w[e], mask_sin=mask)
        assert np.array_equal(f.used[e].astype(bool), r["used"]) and f.num_used[e] == r["used"].sum() < f.num_valid[e], e
        assert np.abs(f.xyz[e] - r["xyz"]).max() <= 1e-5 and abs(f.clock_bias_s[e] - r["clock_bias_s"]) <= 1e-13, e
        assert np.abs(f.sin_el[e] - r["sin_el"]).max() <= 1e-9 and np.abs(f.resid[e] - r["resid"]).max() <= 1e-5
        assert 0.05 < f.rms_residual_m[e] < 30.0 and abs(f.rms_residual_m[e] - np.sqrt(np.mean(r["resid"][r["used"]] ** 2))) < 1e-5
    assert not f.used[1, np.flatnonzero(c.tx_ms[1] >= 0)[0]] and not f.used[2, np.flatnonzero(c.tx_ms[2] >= 0)[1]]
    # and without the mask the weights alone
    f = g.position_fix_host(*noisy.args(), weights=w, **CONVERGED)
    for e in range(c.E):
        r = ref.fix(noisy.ephs, noisy.tx_ms[e], noisy.tx_frac[e], noisy.rx_ms[e], noisy.rx_frac[e], weights=w[e])
        assert f.status[e] == 0 and np.abs(f.xyz[e] - r["xyz"]).max() <= 1e-5 and np.array_equal(f.used[e].astype(bool), r["used"])


SPECIALS = ("three", "weights_three", "nan", "nan_rx", "twins", "max_iter_1", "mask_starved")


@pytest.mark.parametrize("kind", SPECIALS)
def test_special_epoch_gets_its_status_and_its_neighbours_stay_exact(g, kind):
    lb = g.positioning
    e, config = 3, dict(CONVERGED)
    base = fc.case("week_start")
    if kind == "twins":
        base = fc.twinned(base, e)
    w0 = np.ones(base.tx_ms.shape)
    c, w = base.copy(), w0.copy()
    if kind == "max_iter_1":
        config["max_iter"], want = 1, lb.NOT_CONVERGED
    elif kind == "mask_starved":  # a mask so high that fewer than four stay above it in epoch e, and at least four elsewhere or none
        top = np.sort(base.sin_el[e][base.tx_ms[e] >= 0])[::-1]
        config["mask_sin"], want = float((top[2] + top[3]) / 2), lb.MASK_STARVED
    else:
        want = fc.special(c, e, kind, w)
    before = g.position_fix_host(*base.args(), weights=w0, **config)
    after = g.position_fix_host(*c.args(), weights=w, **config)
    f = after.fixes[e]
    print(kind, "status", f["status"], "valid", f["num_valid"], "used", f["num_used"], "iterations", f["iterations"])
    assert f["status"] & want, (kind, f["status"])
    if kind in ("max_iter_1", "mask_starved"):  # the outputs stand
        assert before.fixes.tobytes() == after.fixes.tobytes()
        if kind == "max_iter_1":
            assert (after.status == lb.NOT_CONVERGED).all() and (after.iterations == 1).all() and after.xyz.all()
        else:
            assert f["status"] == lb.MASK_STARVED and np.linalg.norm(after.xyz[e] - base.truth_xyz[e]) < 1e-3 and f["num_used"] == f["num_valid"]
            assert (after.status[np.arange(base.E) != e] & ~(lb.MASKED | lb.MASK_STARVED) == 0).all()
        return
    assert f["status"] == want
    for name in ("x", "y", "z", "clock_bias_s", "rms_residual_m", "last_step_m", "gdop", "pdop"):
        assert f[name] == 0.0, name
    assert not after.resid[e].any() and not after.sin_el[e].any() and not after.used[e].any()
    assert f["num_valid"] == {"three": 3, "nan": 0, "nan_rx": 0, "twins": 4}.get(kind, before.num_valid[e])
    assert f["num_used"] == {"three": 3, "weights_three": 3, "nan": 0, "nan_rx": 0, "twins": 4}[kind]
    if kind in ("three", "weights_three", "twins"):
        assert after.sat[e][c.tx_ms[e] >= 0].all()  # the satellites' states do not depend on the fix
    others = np.arange(base.E) != e
    assert before.fixes[others].tobytes() == after.fixes[others].tobytes()
    for name in ("sat", "resid", "sin_el", "used"):
        assert np.array_equal(getattr(before, name)[others], getattr(after, name)[others]), name
    assert (after.status[others] == 0).all()


def test_sums_that_are_not_finite_set_their_own_bit(g):
    """a start so far away that the squares of the range overflow: the sums are not finite, which is GAT_FIX_NONFINITE and not a
    singular system -- also where the geometry is singular besides; an epoch with too few satellites keeps its own bit"""
    lb = g.positioning
    c = fc.twinned(fc.case("week_start"), 3).copy()
    w = np.ones(c.tx_ms.shape)
    assert fc.special(c, 3, "twins", w) == lb.SINGULAR and fc.special(c, 5, "three", w) == lb.FEW_SATS
    near = g.position_fix_host(*c.args(), **CONVERGED)
    far = g.position_fix_host(*c.args(), init_xyz=(1e200, 0.0, 0.0), **CONVERGED)
    assert near.status.tolist() == [0, 0, 0, lb.SINGULAR, 0, lb.FEW_SATS, 0, 0]
    assert far.status.tolist() == [lb.NONFINITE] * 5 + [lb.FEW_SATS] + [lb.NONFINITE] * 2 and (far.iterations == 0).all()
    assert not far.xyz.any() and not far.resid.any() and not far.used.any() and np.array_equal(far.sat, near.sat)
    assert (far.num_valid == near.num_valid).all() and (far.num_used == near.num_used).all()


def test_unusable_ephemeris_is_not_an_error(g):
    c = fc.case("mid").copy()
    k = int(np.argmax(c.sin_el[0]))
    for field, value in (("valid", 0), ("e", 0.5), ("sqrt_a", 0.0)):
        ephs = c.ephs.copy()
        ephs[field][k] = value
        f = g.position_fix_host(ephs, c.tx_ms, c.tx_frac, c.rx_ms, c.rx_frac, **CONVERGED)
        seen = (c.tx_ms >= 0).sum(axis=1) - (c.tx_ms[:, k] >= 0)
        assert (f.status == 0).all() and (f.num_valid == seen).all() and not f.used[:, k].any() and not f.sat[:, k].any()
        assert np.linalg.norm(f.xyz - c.truth_xyz, axis=1).max() < 1e-3


def test_optional_outputs_and_default_config(g):
    c = fc.case("week_end")
    full = g.position_fix_host(*c.args())
    assert (full.status == 0).all() and np.linalg.norm(full.xyz - c.truth_xyz, axis=1).max() < 1e-3 and (full.last_step_m < 1e-4).all()
    for outs in ((), ("sat",), ("resid", "used"), ("sin_el",)):
        part = g.position_fix_host(*c.args(), outputs=outs)
        assert part.fixes.tobytes() == full.fixes.tobytes()
        for name in outs:
            assert np.array_equal(getattr(part, name), getattr(full, name))
        with pytest.raises(AttributeError):
            getattr(part, [n for n in ("sat", "resid", "sin_el", "used") if n not in outs][0])
    near = g.position_fix_host(*c.args(), init_xyz=tuple(c.truth_xyz[0] + 1000.0))
    assert near.iterations[0] < full.iterations[0] and np.linalg.norm(near.xyz - c.truth_xyz, axis=1).max() < 1e-3


def test_every_refusal_without_a_write(g):
    import ctypes as C

    from gpuacceleratedtracking_amd import _lib
    from gpuacceleratedtracking_amd.positioning import fix_config
    from gpuacceleratedtracking_amd.streams import addr

    lib = g.load_library()
    c = fc.case("mid")
    E, K = c.E, c.K
    ephs = np.ascontiguousarray(c.ephs)
    canary = 0xA5
    outs = {"fixes": np.full(E * 80, canary, np.uint8), "sat": np.full(E * K * 32, canary, np.uint8), "resid": np.full(E * K * 8, canary, np.uint8),
            "sin_el": np.full(E * K * 8, canary, np.uint8), "used": np.full(E * K, canary, np.uint8)}

    def run(cfg, E=E, K=K, **null):
        p = {"eph": addr(ephs), "tx_ms": addr(c.tx_ms), "tx_frac": addr(c.tx_frac), "rx_ms": addr(c.rx_ms), "rx_frac": addr(c.rx_frac),
             "fixes": addr(outs["fixes"])}
        p.update({k: None for k in null})
        rc = lib.gat_position_fix_host(p["eph"], p["tx_ms"], p["tx_frac"], p["rx_ms"], p["rx_frac"], None, E, K, None if cfg is None else C.byref(cfg),
                                       p["fixes"], addr(outs["sat"]), addr(outs["resid"]), addr(outs["sin_el"]), addr(outs["used"]))
        assert rc == 0 or all((a == canary).all() for a in outs.values()), "a refused call wrote"
        return rc

    ARG, RANGE = 1, 2
    for name in ("eph", "tx_ms", "tx_frac", "rx_ms", "rx_frac", "fixes"):
        assert run(fix_config(), **{name: True}) == ARG, name
    assert run(None) == ARG
    bad = fix_config()
    bad.struct_size = 52
    assert run(bad) == ARG
    assert run(fix_config(), E=0) == ARG and run(fix_config(), K=0) == ARG and run(fix_config(), E=-1) == ARG
    assert run(fix_config(max_iter=0)) == ARG and run(fix_config(tol_m=0.0)) == ARG and run(fix_config(tol_m=float("nan"))) == ARG
    assert run(fix_config(flags=1)) == ARG and run(fix_config(mask_sin=float("nan"))) == ARG
    assert run(fix_config(), K=65) == RANGE and run(fix_config(), E=(1 << 24) + 1) == RANGE
    assert run(fix_config()) == 0 and not (outs["fixes"] == canary).all()
    # the plan refuses what the call refuses (but for the pointers) and reports the work split
    with pytest.raises(_lib.GatError):
        g.position_plan(5, 65)
    with pytest.raises(_lib.GatError):
        g.position_plan(0, 5)
    with pytest.raises(_lib.GatError):
        g.position_plan(5, 5, max_iter=0)
    plan = g.position_plan(1 << 24, 64)
    assert plan["waves_per_workgroup"] * plan["workgroups"] == 1 << 24 and plan["threads"] == 64 * plan["waves_per_workgroup"]
    assert plan["scratch_bytes"] == 0 and g.position_plan(plan["waves_per_workgroup"] + 1, 4)["workgroups"] == 2
    # the ephemeris entry points
    rec = np.zeros((), dtype=_lib.EPHEMERIS_DTYPE)
    bits = np.zeros((3, 190), np.uint8)
    assert lib.gat_lnav_ephemeris_host(None, 3, addr(rec)) == ARG and lib.gat_lnav_ephemeris_host(None, 0, None) == ARG
    assert lib.gat_lnav_ephemeris_host(None, -1, addr(rec)) == ARG and lib.gat_lnav_ephemeris_host(None, 0, addr(rec)) == 0 and rec["reason"] == 1
    assert lib.gat_lnav_ephemeris_words_host(None, addr(bits)) == ARG and lib.gat_lnav_ephemeris_words_host(addr(rec), None) == ARG
