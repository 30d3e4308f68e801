"""An independent restatement of the velocity fix in numpy, in the textbook form of the GPS interface specification's user algorithm
(the satellite's velocity from the rates of the orbit's angles) on top of tests/fix_ref.py: numpy's sin, cos and arctan2, the true
anomaly as an angle, Kepler's equation and the travel time iterated until they stand still, the solve by ``np.linalg.lstsq``, the
geodetic coordinates by the closed form.  It shares no text with the library's rule; the tests compare the two within bounds
derived from the arithmetic, never bit for bit.  Like fix_ref the satellite's part computes in the type it is given (float64, or
numpy's long double through ``satellite_rates_long``).

``range_rate_truth`` is no model of the Doppler at all: it solves the light-time equation for a moving receiver in long double a
little before and a little after the reception and differences the two ranges."""
import numpy as np

from tests import fix_ref as ref

WGS84_A = 6378137.0
WGS84_E2 = 6.69437999014e-3
L1_HZ = 1575.42e6


# ---- the satellite ------------------------------------------------------------------------------------------------------------------
def _mean_motion(eph):
    return np.sqrt(ref.MU / (eph["sqrt_a"] ** 2) ** 3) + eph["delta_n"]


def clock_rate(eph, t_sv):
    """d(Delta t_sv) / d t_sv: the polynomial's derivative and the relativistic term's, F e sqrt_a cos E dE/dt"""
    ecc = eph["e"]
    n = _mean_motion(eph)
    big_e = ref.eccentric_anomaly(eph["m0"] + n * ref.wrap_week(t_sv - eph["toe"]), ecc)
    e_dot = n / (1.0 - ecc * np.cos(big_e))
    return eph["af1"] + 2.0 * eph["af2"] * ref.wrap_week(t_sv - eph["toc"]) + ref.F_REL * ecc * eph["sqrt_a"] * np.cos(big_e) * e_dot


def orbit_velocity(eph, t):
    """ECEF velocity [.., 3] at GPS time t, in the frame of that instant: the rates of the anomalies, of the argument of latitude,
    of the radius, the inclination and the node, through the orbital plane into the rotating frame"""
    a = eph["sqrt_a"] ** 2
    ecc = eph["e"]
    n = _mean_motion(eph)
    tk = ref.wrap_week(t - eph["toe"])
    big_e = ref.eccentric_anomaly(eph["m0"] + n * tk, ecc)
    nu = np.arctan2(np.sqrt(1.0 - ecc ** 2) * np.sin(big_e), np.cos(big_e) - ecc)
    phi = nu + eph["omega"]
    u = phi + eph["cus"] * np.sin(2 * phi) + eph["cuc"] * np.cos(2 * phi)
    r = a * (1.0 - ecc * np.cos(big_e)) + eph["crs"] * np.sin(2 * phi) + eph["crc"] * np.cos(2 * phi)
    inc = eph["i0"] + eph["idot"] * tk + eph["cis"] * np.sin(2 * phi) + eph["cic"] * np.cos(2 * phi)
    lon = eph["omega0"] + (eph["omega_dot"] - ref.OMEGA_E) * tk - ref.OMEGA_E * eph["toe"]
    e_dot = n / (1.0 - ecc * np.cos(big_e))
    nu_dot = e_dot * np.sqrt(1.0 - ecc ** 2) / (1.0 - ecc * np.cos(big_e))
    u_dot = nu_dot * (1.0 + 2.0 * (eph["cus"] * np.cos(2 * phi) - eph["cuc"] * np.sin(2 * phi)))
    r_dot = a * ecc * np.sin(big_e) * e_dot + 2.0 * nu_dot * (eph["crs"] * np.cos(2 * phi) - eph["crc"] * np.sin(2 * phi))
    inc_dot = eph["idot"] + 2.0 * nu_dot * (eph["cis"] * np.cos(2 * phi) - eph["cic"] * np.sin(2 * phi))
    lon_dot = eph["omega_dot"] - ref.OMEGA_E
    xp, yp = r * np.cos(u), r * np.sin(u)
    xp_dot, yp_dot = r_dot * np.cos(u) - yp * u_dot, r_dot * np.sin(u) + xp * u_dot
    x = xp * np.cos(lon) - yp * np.cos(inc) * np.sin(lon)
    y = xp * np.sin(lon) + yp * np.cos(inc) * np.cos(lon)
    vx = xp_dot * np.cos(lon) - yp_dot * np.cos(inc) * np.sin(lon) + yp * np.sin(inc) * np.sin(lon) * inc_dot - y * lon_dot
    vy = xp_dot * np.sin(lon) + yp_dot * np.cos(inc) * np.cos(lon) - yp * np.sin(inc) * np.cos(lon) * inc_dot + x * lon_dot
    vz = yp_dot * np.sin(inc) + yp * np.cos(inc) * inc_dot
    return np.stack([vx, vy, vz], axis=-1)


def satellite_rates(eph, tx_ms, tx_frac):
    """(velocity [.., 3] at transmission, clock rate) from the satellite's own time of transmission, as ``fix_ref.satellite``"""
    t_sv = np.asarray(tx_ms, dtype=np.float64) * 1e-3 + tx_frac
    return orbit_velocity(eph, t_sv - ref.clock_correction(eph, t_sv)), clock_rate(eph, t_sv)


def widened(eph):
    """every real field of a record or records of the structured array in numpy's long double"""
    if np.finfo(np.longdouble).eps > 1e-18:
        raise RuntimeError("numpy's long double is no wider than double here")
    return {name: np.asarray(eph[name]).astype(np.longdouble) for name in eph.dtype.names if eph.dtype[name].kind == "f"}


def satellite_rates_long(eph, tx_ms, tx_frac):
    """``satellite_rates`` in long double, as ``fix_ref.satellite_long``"""
    wide = widened(eph)
    t_sv = np.asarray(tx_ms).astype(np.longdouble) / np.longdouble(1000) + np.asarray(tx_frac).astype(np.longdouble)
    return orbit_velocity(wide, t_sv - ref.clock_correction(wide, t_sv)), clock_rate(wide, t_sv)


# ---- the Doppler's model and its solve ------------------------------------------------------------------------------------------------
def _rows(ephs, tx_ms, tx_frac, xyz):
    """of every channel at the receiver position: (k los [K, 3], k los . Vr [K], c ddts [K]) -- the travel time iterated to rest, the
    satellite and its velocity turned into the frame of the reception, k from the satellite's inertial velocity along the line of
    sight"""
    pos, _ = ref.satellite(ephs, tx_ms, tx_frac)
    vel, ddts = satellite_rates(ephs, tx_ms, tx_frac)
    tau = np.full(pos.shape[:-1], 0.075)
    for _ in range(8):
        d = ref.rotated(pos, tau) - xyz
        tau = np.linalg.norm(d, axis=-1) / ref.C_LIGHT
    los = d / np.linalg.norm(d, axis=-1)[..., None]
    pr, vr = ref.rotated(pos, tau), ref.rotated(vel, tau)
    inertial = vr + ref.OMEGA_E * np.stack([-pr[..., 1], pr[..., 0], np.zeros_like(tau)], axis=-1)
    k = 1.0 / (1.0 + (los * inertial).sum(axis=-1) / ref.C_LIGHT)
    return k[..., None] * los, k * (los * vr).sum(axis=-1), ref.C_LIGHT * ddts


def doppler(ephs, tx_ms, tx_frac, xyz, v_ecef, drift, carrier_hz=L1_HZ, range_rate=None):
    """the Doppler observable [K] of a receiver at ``xyz`` moving at ``v_ecef`` whose clock drifts by ``drift`` s/s: -lambda D = range
    rate + c drift - c ddts.  ``range_rate``: the channels' range rates from elsewhere (``range_rate_truth``) instead of the model's."""
    klos, klv, cddts = _rows(ephs, tx_ms, tx_frac, np.asarray(xyz, dtype=np.float64))
    if range_rate is None:
        range_rate = klv - klos @ np.asarray(v_ecef, dtype=np.float64)
    return -(np.asarray(range_rate, dtype=np.float64) + ref.C_LIGHT * drift - cddts) * (carrier_hz / ref.C_LIGHT)


def velocity(ephs, tx_ms, tx_frac, doppler_hz, xyz, use, weights=None, carrier_hz=L1_HZ):
    """One epoch: the weighted least-squares velocity and drift over the channels ``use`` [K] (bool) at the receiver position ``xyz``.
    Returns a dict: v_ecef [3], clock_drift, resid [K] (of every channel)."""
    klos, klv, cddts = _rows(ephs, tx_ms, tx_frac, np.asarray(xyz, dtype=np.float64))
    a = np.concatenate([-klos, np.ones((len(klv), 1))], axis=1)
    y = -(ref.C_LIGHT / carrier_hz) * np.asarray(doppler_hz, dtype=np.float64) - klv + cddts
    w = np.ones(len(klv)) if weights is None else np.asarray(weights, dtype=np.float64)
    s = np.linalg.lstsq(a[use] * np.sqrt(w[use])[:, None], y[use] * np.sqrt(w[use]), rcond=None)[0]
    return {"v_ecef": s[:3], "clock_drift": s[3] / ref.C_LIGHT, "resid": y - a @ s}


# ---- the model-free truth -------------------------------------------------------------------------------------------------------------
def _range_long(wide, xyz, t):
    """the range c tau [K] in long double: tau = |R3(OmegaE tau) r(t - tau) - xyz| / c iterated to rest; t the GPS time of reception"""
    c = np.longdouble(ref.C_LIGHT)
    tau = np.full(wide["e"].shape, np.longdouble(0.075))
    for _ in range(10):
        pos = ref.orbit(wide, (t - tau) % np.longdouble(ref.WEEK))
        th = np.longdouble(ref.OMEGA_E) * tau
        d = np.stack([np.cos(th) * pos[..., 0] + np.sin(th) * pos[..., 1], -np.sin(th) * pos[..., 0] + np.cos(th) * pos[..., 1], pos[..., 2]],
                     axis=-1) - xyz
        tau = np.sqrt((d * d).sum(axis=-1)) / c
    return c * tau


def range_rate_truth(ephs, xyz, v_ecef, t_rx, h=0.05):
    """d(range) / dt [K] at the GPS time ``t_rx`` (seconds of the week) of a receiver that is at ``xyz`` then and moves at ``v_ecef``:
    the central difference of two light-time solutions at t_rx -+ h, in long double.  Truncation h^2 / 6 times the range's third
    derivative (6.4e-5 m/s^3 for a GPS orbit seen from the ground: 2.7e-8 m/s at h = 0.05)."""
    wide = widened(ephs)
    xyz, v = np.asarray(xyz).astype(np.longdouble), np.asarray(v_ecef).astype(np.longdouble)
    t, h = np.longdouble(t_rx), np.longdouble(h)
    return ((_range_long(wide, xyz + h * v, t + h) - _range_long(wide, xyz - h * v, t - h)) / (2 * h)).astype(np.float64)


# ---- the local frame ------------------------------------------------------------------------------------------------------------------
def geodetic(xyz):
    """(latitude, longitude, height) of ECEF points [.., 3] on WGS-84 by the closed form (Heikkinen 1982, no iteration), in the type
    given.  Not for points within some 40 km of the Earth's centre."""
    xyz = np.asarray(xyz)
    x, y, z = xyz[..., 0], xyz[..., 1], xyz[..., 2]
    one = x.dtype.type(1)
    a, e2 = x.dtype.type(WGS84_A), x.dtype.type(WGS84_E2)
    b2 = a * a * (one - e2)
    b = np.sqrt(b2)
    ep2 = (a * a - b2) / b2
    p = np.sqrt(x * x + y * y)
    f = 54 * b2 * z * z
    g = p * p + (one - e2) * z * z - e2 * (a * a - b2)
    c = e2 * e2 * f * p * p / g ** 3
    s = np.cbrt(one + c + np.sqrt(c * c + 2 * c))
    k = s + one + one / s
    pp = f / (3 * k * k * g * g)
    q = np.sqrt(one + 2 * e2 * e2 * pp)
    # at the poles the radicand is zero but for its rounding
    r0 = -pp * e2 * p / (one + q) + np.sqrt(np.maximum(a * a / 2 * (one + one / q) - pp * (one - e2) * z * z / (q * (one + q)) - pp * p * p / 2, 0))
    uu = np.sqrt((p - e2 * r0) ** 2 + z * z)
    vv = np.sqrt((p - e2 * r0) ** 2 + (one - e2) * z * z)
    z0 = b2 * z / (a * vv)
    return np.arctan2(z + ep2 * z0, p), np.arctan2(y, x), uu * (one - b2 / (a * vv))


def enu_axes(lat, lon):
    """(east, north, up) unit vectors [.., 3] each"""
    sl, cl, so, co = np.sin(lat), np.cos(lat), np.sin(lon), np.cos(lon)
    return (np.stack([-so, co, np.zeros_like(so)], axis=-1), np.stack([-sl * co, -sl * so, cl], axis=-1), np.stack([cl * co, cl * so, sl], axis=-1))
