"""An independent FP64 restatement of the range corrections in numpy, from the text of the GPS interface specification's
single-frequency user algorithm (figure 20-4): the geodetic latitude iterated until it stands still, the elevation by ``np.arcsin``,
the azimuth and the longitude by ``np.arctan2``, numpy's cosine, and Chao's mapping with numpy's tangent.  The satellites and the
lines of sight are tests/fix_ref.py's.  It shares no text with the library's rule; the tests compare the two within bounds derived
from the arithmetic, never bit for bit."""
import numpy as np

from tests import fix_ref as ref

PI_GPS = 3.1415926535898
C_LIGHT = ref.C_LIGHT
L1 = 1575.42e6
WGS_A, WGS_E2 = 6378137.0, 6.69437999014e-3
DAY = 86400.0


def geodetic(xyz):
    """(latitude, longitude [rad], height [m]) on the WGS-84 ellipsoid"""
    x, y, z = (np.asarray(xyz, dtype=np.float64)[..., i] for i in range(3))
    p = np.hypot(x, y)
    lat = np.arctan2(z, p * (1.0 - WGS_E2))
    for _ in range(30):
        n = WGS_A / np.sqrt(1.0 - WGS_E2 * np.sin(lat) ** 2)
        lat = np.arctan2(z + WGS_E2 * n * np.sin(lat), p)
    n = WGS_A / np.sqrt(1.0 - WGS_E2 * np.sin(lat) ** 2)
    return lat, np.arctan2(y, x), p * np.cos(lat) + z * np.sin(lat) - n * (1.0 - WGS_E2 * np.sin(lat) ** 2)


def look(ephs, tx_ms, tx_frac, xyz):
    """(elevation [K], azimuth [K], latitude, longitude) of the satellites from the receiver at xyz, against the ellipsoid's normal"""
    pos, _ = ref.satellite(ephs, tx_ms, tx_frac)
    _, los = ref.geometry(pos, np.asarray(xyz, dtype=np.float64))
    lat, lon, _ = geodetic(xyz)
    east = np.array([-np.sin(lon), np.cos(lon), 0.0])
    north = np.array([-np.sin(lat) * np.cos(lon), -np.sin(lat) * np.sin(lon), np.cos(lat)])
    up = np.array([np.cos(lat) * np.cos(lon), np.cos(lat) * np.sin(lon), np.sin(lat)])
    return np.arcsin(np.clip(los @ up, -1.0, 1.0)), np.arctan2(los @ east, los @ north), float(lat), float(lon)


def klobuchar(alpha, beta, lat, lon, el, az, t_gps, carrier_hz=L1):
    """The ionospheric delay [m] and what it passed on the way: a dict with iono and xx, phi_i (before the clip), per and amp (before
    they are raised), t (before the wraps), F.  Angles in radians in, semicircles inside, as the specification has them."""
    big_e, phi_u, lam_u = el / PI_GPS, lat / PI_GPS, lon / PI_GPS
    psi = 0.0137 / (big_e + 0.11) - 0.022
    phi_raw = phi_u + psi * np.cos(az)
    phi_i = np.clip(phi_raw, -0.416, 0.416)
    lam_i = lam_u + psi * np.sin(az) / np.cos(PI_GPS * phi_i)
    phi_m = phi_i + 0.064 * np.cos(PI_GPS * (lam_i - 1.617))
    t_raw = 43200.0 * lam_i + t_gps
    t = np.where(t_raw >= DAY, t_raw - DAY, t_raw)
    t = np.where(t < 0.0, t + DAY, t)
    big_f = 1.0 + 16.0 * (0.53 - big_e) ** 3
    per_raw = beta[0] + beta[1] * phi_m + beta[2] * phi_m ** 2 + beta[3] * phi_m ** 3
    amp_raw = alpha[0] + alpha[1] * phi_m + alpha[2] * phi_m ** 2 + alpha[3] * phi_m ** 3
    per, amp = np.maximum(per_raw, 72000.0), np.maximum(amp_raw, 0.0)
    xx = 2.0 * PI_GPS * (t - 50400.0) / per
    day = big_f * (5e-9 + amp * (1.0 - xx ** 2 / 2.0 + xx ** 4 / 24.0))
    night = big_f * 5e-9
    seconds = np.where(np.abs(xx) < 1.57, day, night)
    return {"iono": C_LIGHT * seconds * (L1 / carrier_hz) ** 2, "xx": xx, "phi_i": phi_raw, "per": per_raw, "amp": amp_raw, "t": t_raw, "F": big_f,
            "night": C_LIGHT * night * (L1 / carrier_hz) ** 2}


def tropo(el, zd, zw):
    """Chao's mapping of the zenith delays [m] at the elevation el [rad]"""
    md = 1.0 / (np.sin(el) + 0.00143 / (np.tan(el) + 0.0445))
    mw = 1.0 / (np.sin(el) + 0.00035 / (np.tan(el) + 0.017))
    return zd * md + zw * mw


def tropo_zenith(height_m, sin_lat, humidity=0.5):
    """Saastamoinen's zenith delays (hydrostatic, wet) over the standard atmosphere"""
    pres = 1013.25 * (1.0 - 2.2557e-5 * height_m) ** 5.2568
    temp = 288.15 - 6.5e-3 * height_m
    e = 6.108 * humidity * np.exp((17.15 * temp - 4684.0) / (temp - 38.45))
    return 0.0022768 * pres / (1.0 - 0.00266 * (1.0 - 2.0 * sin_lat ** 2) - 2.8e-7 * height_m), 0.002277 * (1255.0 / temp + 0.05) * e


def corrections(ephs, tx_ms, tx_frac, rx_ms, rx_frac, xyz, clock_bias_s, alpha, beta, zd, zw, carrier_hz=L1):
    """One epoch at the state (xyz, clock_bias_s): a dict of [K] arrays -- iono, tropo [m], sin_el, cos_a, sin_a, and klobuchar's
    by-products -- for every channel, whether it is seen or not (the caller masks)"""
    el, az, lat, lon = look(ephs, tx_ms, tx_frac, xyz)
    t_gps = (int(rx_ms) % 86400000) * 1e-3 + rx_frac - clock_bias_s
    out = klobuchar(alpha, beta, lat, lon, el, az, t_gps, carrier_hz)
    out.update(tropo=tropo(el, zd, zw), sin_el=np.sin(el), cos_a=np.cos(az), sin_a=np.sin(az), el=el, az=az)
    return out


def margins_ok(r, floor_sin=0.0, alpha=None, rel=1e-6):
    """bool [K]: the restatement's own values stay farther than ``rel`` (relative) from every discontinuity of the model: |xx| = 1.57,
    |phi_i| = 0.416, PER = 72000, AMP = 0 (relative to the sum of |alpha|), the day's two wraps, and floor_sin (absolute: a sine)"""
    scale = float(np.sum(np.abs(alpha))) if alpha is not None else 1e-8
    return ((np.abs(np.abs(r["xx"]) - 1.57) > rel * 1.57) & (np.abs(np.abs(r["phi_i"]) - 0.416) > rel * 0.416) & (np.abs(r["per"] - 72000.0) > rel * 72000.0)
            & (np.abs(r["amp"]) > rel * scale) & (np.abs(r["t"] - DAY) > rel * DAY) & (np.abs(r["t"]) > rel * DAY) & (np.abs(r["sin_el"] - floor_sin) > rel))
