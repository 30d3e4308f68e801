"""An independent FP64 restatement of the position fix in numpy, in the textbook form of the GPS interface specification's user
algorithm: numpy's sin, cos and arctan2, the true anomaly as an angle, Kepler's equation iterated until it stands still, and the
least-squares step by ``np.linalg.lstsq``.  It shares no text with the library's rule; the tests compare the two within bounds
derived from the arithmetic, never bit for bit.  An ephemeris is anything indexable by field name (a record of the structured
array), a time of the week a pair (whole milliseconds, fraction in seconds).  The clock and the orbit compute in the type they are
given: float64, or numpy's long double through ``satellite_long``, for the tests whose bound is the rule's own rounding."""
import numpy as np

MU = 3.986005e14
OMEGA_E = 7.2921151467e-5
C_LIGHT = 299792458.0
F_REL = -4.442807633e-10
WEEK = 604800.0


def _real(x):
    """float64, or numpy's long double where the caller brought one: every function below computes in the type it is given"""
    x = np.asarray(x)
    return x if x.dtype == np.longdouble else x.astype(np.float64)


def wrap_week(dt):
    return (_real(dt) + WEEK / 2) % WEEK - WEEK / 2


def eccentric_anomaly(mean, ecc):
    big_e = np.array(_real(mean), copy=True)
    for _ in range(20):  # Newton; quadratic, at rest long before
        big_e = big_e - (big_e - ecc * np.sin(big_e) - mean) / (1.0 - ecc * np.cos(big_e))
    return big_e


def clock_correction(eph, t_sv):
    """Delta t_sv of the satellite's own time t_sv (seconds of week): the polynomial, the relativistic term and T_GD (L1)"""
    a = eph["sqrt_a"] ** 2
    tk = wrap_week(t_sv - eph["toe"])
    big_e = eccentric_anomaly(eph["m0"] + (np.sqrt(MU / a ** 3) + eph["delta_n"]) * tk, eph["e"])
    dt = wrap_week(t_sv - eph["toc"])
    return eph["af0"] + eph["af1"] * dt + eph["af2"] * dt ** 2 + F_REL * eph["e"] * eph["sqrt_a"] * np.sin(big_e) - eph["tgd"]


def orbit(eph, t):
    """ECEF position [.., 3] at GPS time t (seconds of week), in the frame of that instant"""
    a = eph["sqrt_a"] ** 2
    tk = wrap_week(t - eph["toe"])
    ecc = eph["e"]
    big_e = eccentric_anomaly(eph["m0"] + (np.sqrt(MU / a ** 3) + eph["delta_n"]) * tk, ecc)
    nu = np.arctan2(np.sqrt(1.0 - ecc ** 2) * np.sin(big_e), np.cos(big_e) - ecc)
    phi = nu + eph["omega"]
    u = phi + eph["cus"] * np.sin(2 * phi) + eph["cuc"] * np.cos(2 * phi)
    r = a * (1.0 - ecc * np.cos(big_e)) + eph["crs"] * np.sin(2 * phi) + eph["crc"] * np.cos(2 * phi)
    inc = eph["i0"] + eph["idot"] * tk + eph["cis"] * np.sin(2 * phi) + eph["cic"] * np.cos(2 * phi)
    lon = eph["omega0"] + (eph["omega_dot"] - OMEGA_E) * tk - OMEGA_E * eph["toe"]
    xp, yp = r * np.cos(u), r * np.sin(u)
    return np.stack([xp * np.cos(lon) - yp * np.cos(inc) * np.sin(lon), xp * np.sin(lon) + yp * np.cos(inc) * np.cos(lon), yp * np.sin(inc)],
                    axis=-1)


def satellite(eph, tx_ms, tx_frac):
    """(position [.., 3] at transmission, Delta t_sv) from the satellite's own time of transmission"""
    t_sv = np.asarray(tx_ms, dtype=np.float64) * 1e-3 + tx_frac
    dts = clock_correction(eph, t_sv)
    return orbit(eph, t_sv - dts), dts


def satellite_long(eph, tx_ms, tx_frac):
    """``satellite`` in numpy's long double (64 bits of mantissa on x86): every field and both parts of the time raised first, the
    milliseconds divided by 1000 there, so that no rounding of a double is left in it -- the yardstick where the bound is derived
    from the rule's own roundings (tests/test_position_domain_host.py).  eph: a record or records of the structured array."""
    if np.finfo(np.longdouble).eps > 1e-18:
        raise RuntimeError("numpy's long double is no wider than double here")
    wide = {name: np.asarray(eph[name]).astype(np.longdouble) for name in eph.dtype.names if eph.dtype[name].kind == "f"}
    t_sv = np.asarray(tx_ms).astype(np.longdouble) / np.longdouble(1000) + np.asarray(tx_frac).astype(np.longdouble)
    dts = clock_correction(wide, t_sv)
    return orbit(wide, t_sv - dts), dts


def pseudorange(rx_ms, rx_frac, tx_ms, tx_frac):
    dms = (np.asarray(rx_ms, dtype=np.int64) - np.asarray(tx_ms, dtype=np.int64) + 302400000) % 604800000 - 302400000
    return C_LIGHT * (dms * 1e-3 + (np.asarray(rx_frac) - np.asarray(tx_frac)))


def rotated(pos, tau):
    """the satellite in the frame of the reception, the Earth having turned for tau seconds"""
    th = OMEGA_E * np.asarray(tau)
    c, s = np.cos(th), np.sin(th)
    return np.stack([c * pos[..., 0] + s * pos[..., 1], -s * pos[..., 0] + c * pos[..., 1], pos[..., 2]], axis=-1)


def geometry(pos, xyz):
    """(range, unit vectors to the satellites) with the travel time iterated to rest"""
    tau = np.full(pos.shape[:-1], 0.075)
    for _ in range(6):
        d = rotated(pos, tau) - xyz
        rng = np.linalg.norm(d, axis=-1)
        tau = rng / C_LIGHT
    return rng, d / rng[..., None]


def solve(pos, dts, rho, weights=None, start=(0.0, 0.0, 0.0, 0.0), tol=1e-9, max_iter=30):
    """weighted least squares over the given satellites: (state [4] = x, y, z, c * clock error; residuals; unit vectors; iterations)"""
    st = np.array(start, dtype=np.float64)
    w = np.ones(len(rho)) if weights is None else np.asarray(weights, dtype=np.float64)
    for it in range(max_iter):
        rng, los = geometry(pos, st[:3])
        v = rho - (rng + st[3] - C_LIGHT * dts)
        a = np.concatenate([-los, np.ones((len(rho), 1))], axis=1)
        step = np.linalg.lstsq(a * np.sqrt(w)[:, None], v * np.sqrt(w), rcond=None)[0]
        st = st + step
        if np.linalg.norm(step[:3]) < tol:
            break
    rng, los = geometry(pos, st[:3])
    return st, rho - (rng + st[3] - C_LIGHT * dts), los, it + 1


def fix(ephs, tx_ms, tx_frac, rx_ms, rx_frac, weights=None, mask_sin=-1.0, start=(0.0, 0.0, 0.0)):
    """One epoch: ``ephs`` a structured array [K], times of the K channels and of the reception.  A channel counts with a
    non-negative ms, a finite fraction and a valid ephemeris; with ``mask_sin`` the satellites below it at the first solution leave
    and the rest is solved again.  Returns a dict: xyz, clock_bias_s, used [K], sin_el [K], resid [K], sat [K, 3], dts [K]."""
    tx_ms, tx_frac = np.asarray(tx_ms), np.asarray(tx_frac, dtype=np.float64)
    ok = (tx_ms >= 0) & np.isfinite(tx_frac) & (ephs["valid"] != 0)
    w = np.ones(len(tx_ms)) if weights is None else np.asarray(weights, dtype=np.float64)
    use = ok & np.isfinite(w) & (w > 0)
    pos, dts = satellite(ephs, np.where(ok, tx_ms, 0), np.where(ok, tx_frac, 0.0))
    rho = pseudorange(rx_ms, rx_frac, np.where(ok, tx_ms, 0), np.where(ok, tx_frac, 0.0))
    st, _, _, _ = solve(pos[use], dts[use], rho[use], w[use], start=tuple(start) + (0.0,))
    rng, los = geometry(pos, st[:3])
    sin_el = los @ (st[:3] / np.linalg.norm(st[:3]))
    if mask_sin > -1.0:
        keep = use & (sin_el >= mask_sin)
        if keep.sum() != use.sum() and keep.sum() >= 4:
            use = keep
            st, _, _, _ = solve(pos[use], dts[use], rho[use], w[use], start=st)
            rng, los = geometry(pos, st[:3])
            sin_el = los @ (st[:3] / np.linalg.norm(st[:3]))
    resid = rho - (rng + st[3] - C_LIGHT * dts)
    return {"xyz": st[:3], "clock_bias_s": st[3] / C_LIGHT, "used": use, "sin_el": np.where(ok, sin_el, 0.0), "resid": np.where(ok, resid, 0.0),
            "sat": np.where(ok[:, None], pos, 0.0), "dts": np.where(ok, dts, 0.0), "ok": ok}


def transmit_times(ephs, xyz, rx_ms, rx_frac, clock_bias_s):
    """What a receiver at ``xyz`` whose clock reads (rx_ms, rx_frac) and is ``clock_bias_s`` ahead of GPS time would measure of every
    satellite: (tx_ms [K], tx_frac [K], sin of the geometric elevation [K]).  The light-time equation is iterated in offsets from
    the reception so that no bit of the fractions is lost in seconds of the week."""
    k = len(ephs)
    t_rx = float(rx_ms) * 1e-3 + rx_frac - clock_bias_s  # GPS time of the reception
    tau = np.full(k, 0.075)
    for _ in range(8):
        pos = orbit(ephs, wrap_week(t_rx - tau) % WEEK)
        d = rotated(pos, tau) - np.asarray(xyz)
        tau = np.linalg.norm(d, axis=-1) / C_LIGHT
    sin_el = (d / np.linalg.norm(d, axis=-1)[:, None]) @ (np.asarray(xyz) / np.linalg.norm(xyz))
    dts = np.zeros(k)
    for _ in range(4):  # the satellite's own reading: t_sv = t_gps + Delta t_sv(t_sv)
        dts = clock_correction(ephs, (t_rx - tau + dts) % WEEK)
    off = rx_frac - clock_bias_s - tau + dts  # t_sv minus the whole milliseconds of the reception
    m = np.floor(off * 1e3)
    tx_frac = off - m * 1e-3
    m, tx_frac = np.where(tx_frac >= 1e-3, m + 1, m), np.where(tx_frac >= 1e-3, tx_frac - 1e-3, tx_frac)
    m, tx_frac = np.where(tx_frac < 0, m - 1, m), np.where(tx_frac < 0, tx_frac + 1e-3, tx_frac)
    tx_ms = (int(rx_ms) + m.astype(np.int64)) % 604800000
    return tx_ms.astype(np.int32), tx_frac, sin_el
