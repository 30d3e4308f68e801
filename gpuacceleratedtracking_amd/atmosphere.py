"""Atmosphere (include/gat.h, "atmosphere"): the ionospheric and tropospheric delay of every channel at a first fix, and transmit
times corrected by them that the fixes take as they are::

    nav = loop.navigation(mon)                                     # gat_nav_decode
    iono = lnav_page18(nav, channel).klobuchar                     # gat_lnav_page18_host: the eight broadcast coefficients
    fix, corr = position_fix_corrected(ephs, tx_ms, tx_frac, rx_ms, rx_frac, iono=iono, tropo="standard")
    corr.iono, corr.tropo, corr.elevation_deg, corr.azimuth_deg    # per epoch and channel
    vel = velocity_fix(ephs, tx_ms, corr.tx_frac_dev, doppler_hz, fix)

``position_fix_corrected`` is fix -> ``range_corrections`` -> fix (or RAIM), every step enqueued on the device and nothing read
back.  The work is libgat's HIP kernel (``range_corrections``) or its host twin with the same bits (``range_corrections_host``).  The
zenith delays of the troposphere are the caller's: ``tropo_zenith`` is Saastamoinen's model over a standard atmosphere, outside
the rule (1 m of height is 0.3 mm of delay)."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from .context import Context, get_context
from .navigation import NavResult
from .positioning import PositionFix, _device_args, _host_args, position_fix, position_fix_raim
from .results import PlannedResult, host_check, new_plan, plan_report, wanted
from .streams import addr, keep_alive, vp

IONO, TROPO = _lib.GAT_ATM_IONO, _lib.GAT_ATM_TROPO
NO_FIX, NO_GEODETIC = _lib.GAT_ATM_NO_FIX, _lib.GAT_ATM_NO_GEODETIC
CH_CORRECTED, CH_LOW, CH_NONFINITE = _lib.GAT_ATM_CH_CORRECTED, _lib.GAT_ATM_CH_LOW, _lib.GAT_ATM_CH_NONFINITE
OUTPUTS = ("delay", "geom", "channel_status", "epoch_status")
_SHAPES = {"delay": (2,), "geom": (3,), "channel_status": ()}
_DTYPES = {"delay": "float64", "geom": "float64", "channel_status": "uint8", "epoch_status": "int32"}
_FIX_KEYS = ("max_iter", "tol_m", "mask_sin", "init_xyz", "flags")


class Klobuchar:
    """The eight coefficients of the broadcast ionosphere model: ``alpha`` (s, s/sc, s/sc^2, s/sc^3) and ``beta`` (the same units)."""

    def __init__(self, alpha=(0.0, 0.0, 0.0, 0.0), beta=(0.0, 0.0, 0.0, 0.0)):
        self.alpha, self.beta = tuple(float(v) for v in alpha), tuple(float(v) for v in beta)
        if len(self.alpha) != 4 or len(self.beta) != 4:
            raise ValueError("alpha and beta have four coefficients each")

    def __eq__(self, other):
        return isinstance(other, Klobuchar) and (self.alpha, self.beta) == (other.alpha, other.beta)

    def __repr__(self):
        return f"Klobuchar(alpha={self.alpha!r}, beta={self.beta!r})"


class Page18:
    """``gat_lnav_page18``: ``record`` (structured scalar: valid, data_id, sv_id, wnt, dt_ls, wnlsf, dn, dt_lsf, alpha, beta, a0, a1,
    tot), every field as an attribute, and ``klobuchar``."""

    def __init__(self, record):
        self.record = np.array(record, dtype=_lib.PAGE18_DTYPE).reshape(())

    def __getattr__(self, name):
        if name in _lib.PAGE18_DTYPE.names:
            v = self.__dict__["record"][name]
            return v.item() if v.ndim == 0 else v.copy()
        raise AttributeError(name)

    klobuchar = property(lambda self: Klobuchar(self.record["alpha"], self.record["beta"]))


def lnav_page18(nav: NavResult, channel: int) -> Page18:
    """``gat_lnav_page18_host`` on one channel's frames: the newest good subframe 4 with SV ID 56.  ``valid`` is 0 where there is none."""
    frames = np.ascontiguousarray(nav.frames[int(channel)])
    rec = np.zeros((), dtype=_lib.PAGE18_DTYPE)
    rc = _lib.load().gat_lnav_page18_host(addr(frames), int(frames.shape[0]), addr(rec))
    host_check(rc, "gat_lnav_page18_host")
    return Page18(rec)


def lnav_page18_payload(iono=None, *, a0: float = 0.0, a1: float = 0.0, tot: float = 0.0, wnt: int = 0, dt_ls: int = 0, wnlsf: int = 0, dn: int = 0,
                        dt_lsf: int = 0, data_id: int = 1) -> np.ndarray:
    """``gat_lnav_page18_words_host``: uint8 ``[190]``, the quantised payload bits of subframe 4, page 18 -- what
    ``lnav_subframe(tow, 4, payload=)`` takes.  ``iono``: a ``Klobuchar``, a ``Page18`` (its record as it is) or None (zeros)."""
    if isinstance(iono, Page18):
        rec = iono.record.copy()
    else:
        rec = np.zeros((), dtype=_lib.PAGE18_DTYPE)
        k = Klobuchar() if iono is None else iono
        rec["alpha"], rec["beta"] = k.alpha, k.beta
        rec["data_id"], rec["sv_id"] = data_id, 56
        rec["a0"], rec["a1"], rec["tot"], rec["wnt"], rec["dt_ls"], rec["wnlsf"], rec["dn"], rec["dt_lsf"] = a0, a1, tot, wnt, dt_ls, wnlsf, dn, dt_lsf
    bits = np.zeros(190, dtype=np.uint8)
    rc = _lib.load().gat_lnav_page18_words_host(addr(rec), addr(bits))
    host_check(rc, "gat_lnav_page18_words_host")
    return bits


def atan2_host(y, x) -> np.ndarray:
    """``gat_atm_atan2_host``: the rule's arctangent of every pair, float64"""
    y, x = np.broadcast_arrays(np.asarray(y, dtype=np.float64), np.asarray(x, dtype=np.float64))
    y, x = np.ascontiguousarray(y), np.ascontiguousarray(x)
    out = np.zeros(y.shape, dtype=np.float64)
    host_check(_lib.load().gat_atm_atan2_host(addr(y), addr(x), int(y.size), addr(out)), "gat_atm_atan2_host")
    return out


def atm_config(iono=None, zenith=None, carrier_hz: float = 1575.42e6, floor_sin: float = 0.0, flags: int | None = None) -> _lib.AtmConfig:
    """``gat_atm_config`` from Python values.  ``iono``: a ``Klobuchar`` / ``Page18`` or None (no ionosphere); ``zenith``: None (no
    troposphere), a pair (hydrostatic, wet) for the config's scalars, or an array ``[E, 2]`` (passed to the call, not held here).
    ``flags``: None for what these two say.  Nothing else is checked: the library refuses."""
    cfg = _lib.AtmConfig()
    cfg.struct_size = C.sizeof(_lib.AtmConfig)
    if isinstance(iono, Page18):
        iono = iono.klobuchar
    if iono is not None:
        for i in range(4):
            cfg.alpha[i], cfg.beta[i] = iono.alpha[i], iono.beta[i]
    if isinstance(zenith, (tuple, list)):
        cfg.zenith_dry_m, cfg.zenith_wet_m = float(zenith[0]), float(zenith[1])
    cfg.flags = ((IONO if iono is not None else 0) | (TROPO if zenith is not None else 0)) if flags is None else int(flags)
    cfg.carrier_hz, cfg.floor_sin = float(carrier_hz), float(floor_sin)
    return cfg


class RangeCorrections(PlannedResult):
    """The outputs of one call.  Raw: ``tx_frac_out`` float64 ``[E, K]`` and, where asked for, ``delay`` ``[E, K, 2]`` (iono, tropo,
    m), ``geom`` ``[E, K, 3]`` (sin el, cos A, sin A), ``channel_status`` uint8 ``[E, K]``, ``epoch_status`` int32 ``[E]``; ``zenith``
    ``[E, 2]`` where the call was given one.  ``tx_frac_dev`` is ``tx_frac_out`` as the call left it (a device tensor of the device
    call), to pass on without a look.  Derived: ``tx_frac``, ``iono``, ``tropo``, ``sin_el``, ``elevation_deg``, ``azimuth_deg``,
    ``corrected`` (bool ``[E, K]``)."""

    def __getattr__(self, name):
        if name in OUTPUTS or name == "zenith":
            if name not in self._raw:
                raise AttributeError(f"{name} was not asked for (outputs=)" if name in OUTPUTS else "the call was given no zenith array")
            return self._h()[name]
        raise AttributeError(name)

    tx_frac_dev = property(lambda self: self._raw["tx_frac_out"])
    tx_frac_out = property(lambda self: self._h()["tx_frac_out"])
    tx_frac = tx_frac_out
    iono = property(lambda self: self.delay[..., 0], doc="float64 [E, K]: m")
    tropo = property(lambda self: self.delay[..., 1], doc="float64 [E, K]: m")
    sin_el = property(lambda self: self.geom[..., 0])
    elevation_deg = property(lambda self: np.degrees(np.arcsin(self.geom[..., 0])))
    azimuth_deg = property(lambda self: np.degrees(np.arctan2(self.geom[..., 2], self.geom[..., 1])) % 360.0)
    corrected = property(lambda self: (self.channel_status & CH_CORRECTED) != 0)


def _fix_records(fix, host: bool):
    """the gat_fix records of a call: a ``PositionFix`` gives its own (as the call left them, or read back for the host twin)"""
    if isinstance(fix, PositionFix):
        return (fix._h() if host else fix._raw)["fixes"]
    return fix


def range_corrections(ephs, tx_ms, tx_frac, rx_ms, rx_frac, fix, *, iono=None, zenith=None, carrier_hz: float = 1575.42e6, floor_sin: float = 0.0,
                      outputs=None, ctx: Context | None = None, flags: int | None = None) -> RangeCorrections:
    """``gat_range_corrections`` on the device.  ``ephs``, the four times: as ``position_fix`` takes them.  ``fix``: the ``PositionFix``
    of ``position_fix`` / ``position_fix_raim`` or a uint8 device tensor of ``E`` ``gat_fix`` records.  ``iono``: a ``Klobuchar`` (or the
    ``Page18`` that holds one), None: no ionosphere.  ``zenith``: a float64 device tensor ``[E, 2]`` (hydrostatic, wet; m), a pair of
    floats for every epoch, None: no troposphere.  ``outputs``: which of "delay", "geom", "channel_status", "epoch_status" to write
    (None: all).  Enqueues on the context's stream and returns at once."""
    want = wanted(outputs, OUTPUTS, OUTPUTS)
    E, K, dev, eph_dev = _device_args(ephs, tx_ms, tx_frac, rx_ms, rx_frac, None)
    records = _fix_records(fix, host=False)
    if not isinstance(records, torch.Tensor) or records.dtype != torch.uint8 or not records.is_contiguous() or records.device != dev \
            or records.numel() != E * _lib.FIX_DTYPE.itemsize:
        raise ValueError(f"fix must hold {E} gat_fix records as a contiguous uint8 tensor on the device of tx_ms")
    zen = zenith if isinstance(zenith, torch.Tensor) else None
    if zen is not None and (zen.dtype != torch.float64 or not zen.is_contiguous() or zen.device != dev or zen.shape != (E, 2)):
        raise ValueError("zenith must be a contiguous float64 [E, 2] tensor on the device of tx_ms, or a pair of floats")
    if ctx is None:
        ctx = get_context(dev)
    cfg = atm_config(iono, zenith, carrier_hz, floor_sin, flags)
    raw = {"tx_frac_out": torch.empty((E, K), dtype=torch.float64, device=dev)}
    for name in want:
        raw[name] = torch.empty((E,) if name == "epoch_status" else (E, K) + _SHAPES[name], dtype=getattr(torch, _DTYPES[name]), device=dev)
    ctx.check(ctx.lib.gat_range_corrections(ctx._h, vp(eph_dev), vp(tx_ms), vp(tx_frac), vp(rx_ms), vp(rx_frac), vp(records), vp(zen), E, K,
                                            C.byref(cfg), vp(raw["tx_frac_out"]), *[vp(raw.get(n)) for n in OUTPUTS]), "gat_range_corrections")
    if zen is not None:
        raw["zenith"] = zen
    return keep_alive(RangeCorrections(raw, ctx), eph_dev, tx_ms, tx_frac, rx_ms, rx_frac, records, zen)


def range_corrections_host(ephs, tx_ms, tx_frac, rx_ms, rx_frac, fix, *, iono=None, zenith=None, carrier_hz: float = 1575.42e6,
                           floor_sin: float = 0.0, outputs=None, flags: int | None = None) -> RangeCorrections:
    """``gat_range_corrections_host``: the same rule and the same bits over numpy arrays; needs no device.  ``fix``: a ``PositionFix``
    (of either call: it is read back) or a structured ``gat_fix`` array ``[E]``; ``zenith``: an array ``[E, 2]``, a pair or None."""
    want = wanted(outputs, OUTPUTS, OUTPUTS)
    recs, tx_ms, tx_frac, rx_ms, rx_frac, _, E, K = _host_args(ephs, tx_ms, tx_frac, rx_ms, rx_frac, None)
    records = np.ascontiguousarray(_fix_records(fix, host=True))
    if records.dtype != _lib.FIX_DTYPE or records.shape != (E,):
        raise ValueError("fix must be gat_fix records [E]")
    zen = None
    if zenith is not None and not isinstance(zenith, (tuple, list)):
        zen = np.ascontiguousarray(zenith, dtype=np.float64)
        if zen.shape != (E, 2):
            raise ValueError("zenith must be [E, 2] or a pair of floats")
    cfg = atm_config(iono, zenith, carrier_hz, floor_sin, flags)
    raw = {"tx_frac_out": np.zeros((E, K), dtype=np.float64)}
    for name in want:
        raw[name] = np.zeros((E,) if name == "epoch_status" else (E, K) + _SHAPES[name], dtype=_DTYPES[name])
    rc = _lib.load().gat_range_corrections_host(addr(recs), addr(tx_ms), addr(tx_frac), addr(rx_ms), addr(rx_frac), addr(records), addr(zen), E, K,
                                                C.byref(cfg), addr(raw["tx_frac_out"]), *[addr(raw.get(n)) for n in OUTPUTS])
    host_check(rc, "gat_range_corrections_host")
    if zen is not None:
        raw["zenith"] = zen
    return RangeCorrections(raw)


def atmosphere_plan(num_epochs: int, num_channels: int, *, carrier_hz: float = 1575.42e6, floor_sin: float = 0.0, flags: int = IONO | TROPO) -> dict:
    """``gat_range_corrections_plan``: the workgroups, their waves and threads, and the LDS and scratch bytes (both 0) of such a call."""
    cfg = atm_config(None, None, carrier_hz, floor_sin, flags)
    plan = new_plan(_lib.FixPlan)
    rc = _lib.load().gat_range_corrections_plan(int(num_epochs), int(num_channels), C.byref(cfg), C.byref(plan))
    host_check(rc, "gat_range_corrections_plan")
    return plan_report(plan)


# ---- the zenith delays: Saastamoinen over a standard atmosphere, outside the rule ------------------------------------------------------
def tropo_zenith(height_m, sin_lat, pressure_hpa=None, temperature_k=None, humidity=0.5):
    """The zenith delays ``[..., 2]`` (hydrostatic, wet; m) at ``height_m`` above the ellipsoid and the latitude of sine ``sin_lat``,
    numpy arrays or torch tensors alike: P = 1013.25 (1 - 2.2557e-5 h)^5.2568 hPa and T = 288.15 - 6.5e-3 h K where not given, e =
    6.108 RH exp((17.15 T - 4684) / (T - 38.45)) hPa, z_d = 0.0022768 P / (1 - 0.00266 (1 - 2 sin^2 phi) - 2.8e-7 h), z_w = 0.002277
    (1255 / T + 0.05) e."""
    xp = torch if isinstance(height_m, torch.Tensor) else np
    if xp is np:
        height_m, sin_lat = np.asarray(height_m, dtype=np.float64), np.asarray(sin_lat, dtype=np.float64)
    P = 1013.25 * (1.0 - 2.2557e-5 * height_m) ** 5.2568 if pressure_hpa is None else pressure_hpa
    T = 288.15 - 6.5e-3 * height_m if temperature_k is None else temperature_k
    e = 6.108 * humidity * xp.exp((17.15 * T - 4684.0) / (T - 38.45))
    zd = 0.0022768 * P / (1.0 - 0.00266 * (1.0 - 2.0 * sin_lat * sin_lat) - 2.8e-7 * height_m)
    zw = 0.002277 * (1255.0 / T + 0.05) * e + 0.0 * zd  # zd's shape where a given temperature is a scalar
    return xp.stack([zd, zw], **({"dim": -1} if xp is torch else {"axis": -1}))


def tropo_zenith_from_fix(fix_records):
    """``tropo_zenith`` of the standard atmosphere at every fix: ``fix_records`` is a ``PositionFix`` of a device call or a uint8 device
    tensor of ``E`` ``gat_fix`` records; the height and the latitude come from x, y, z by torch operations on the device (eight
    fixed-point steps on the WGS-84 ellipsoid), nothing is read back.  Float64 ``[E, 2]``; zeros for a record without a position."""
    rec = _fix_records(fix_records, host=False)
    v = rec.reshape(-1, _lib.FIX_DTYPE.itemsize).view(torch.float64)
    first = _lib.FIX_DTYPE.fields["x"][1] // 8
    x, y, z = v[:, first], v[:, first + 1], v[:, first + 2]
    a, e2 = 6378137.0, 6.69437999014e-3
    p = torch.sqrt(x * x + y * y)
    r = torch.sqrt(p * p + z * z)
    s = z / r
    for _ in range(8):
        n = a / torch.sqrt(1.0 - e2 * s * s)
        zp = z + e2 * n * s
        q = torch.sqrt(zp * zp + p * p)
        s, c = zp / q, p / q
    h = p * c + z * s - a * torch.sqrt(1.0 - e2 * s * s)
    good = (r >= 1.0e6) & torch.isfinite(r)
    zen = tropo_zenith(torch.where(good, h, torch.zeros_like(h)), torch.where(good, s, torch.zeros_like(s)))
    return torch.where(good[:, None], zen, torch.zeros_like(zen)).contiguous()


def position_fix_corrected(ephs, tx_ms, tx_frac, rx_ms, rx_frac, weights=None, *, iono=None, tropo="standard", raim: bool = False,
                           carrier_hz: float = 1575.42e6, floor_sin: float = 0.0, outputs=None, ctx: Context | None = None, **config):
    """fix -> corrections -> fix on the device, nothing read back: ``position_fix`` on the times as they are, ``range_corrections`` at
    that fix, then ``position_fix`` (``raim``: ``position_fix_raim``) on the corrected transmit times.  ``iono``: a ``Klobuchar`` or
    None; ``tropo``: "standard" (``tropo_zenith_from_fix`` of the first fix), a zenith array ``[E, 2]`` or pair, None.  ``config``: the
    fix's (``max_iter``, ``tol_m``, ``mask_sin``, ``init_xyz``) for both fixes and, with ``raim``, ``position_fix_raim``'s own for the
    second; ``outputs``: the second fix's.  Returns (the second fix, the ``RangeCorrections``)."""
    fix_cfg = {k: v for k, v in config.items() if k in _FIX_KEYS}
    if not raim and len(fix_cfg) != len(config):
        raise TypeError(f"unknown arguments {sorted(set(config) - set(_FIX_KEYS))}")
    first = position_fix(ephs, tx_ms, tx_frac, rx_ms, rx_frac, weights, outputs=(), ctx=ctx, **fix_cfg)
    zenith = tropo_zenith_from_fix(first) if isinstance(tropo, str) and tropo == "standard" else tropo
    if isinstance(zenith, str):
        raise ValueError('tropo must be "standard", a zenith array [E, 2], a pair or None')
    corr = range_corrections(ephs, tx_ms, tx_frac, rx_ms, rx_frac, first, iono=iono, zenith=zenith, carrier_hz=carrier_hz, floor_sin=floor_sin, ctx=ctx)
    second = position_fix_raim if raim else position_fix
    return second(ephs, tx_ms, corr.tx_frac_dev, rx_ms, rx_frac, weights, outputs=outputs, ctx=ctx, **config), corr
