"""Navigation data (include/gat.h, "navigation data"): frames out of the monitor's data symbols::

    mon = loop.monitor(acc_re, acc_im)                           # gat_track_monitor: symbols up to the Costas loop's sign
    nav = loop.navigation(mon)                                   # gat_nav_decode: enqueued, not synchronised
    nav.synced, nav.frame_offset, nav.inverted                   # where a subframe begins, and the sign the loop locked to
    nav.ok, nav.tow, nav.subframe_id                             # per channel and frame: every check passed, the TOW count, the ID
    nav.words                                                    # uint32 [K, max_frames, 10]: the checked words, for an ephemeris decoder

``GPSL1`` carries the legacy message (LNAV: hard bits, ten words of (32,26) parity to a 300-bit subframe), ``GPSL5`` carries CNAV
(rate-1/2 K = 7 convolutional symbols, decoded by a Viterbi decoder on the device, 300-bit messages with CRC-24Q).  The work is
libgat's HIP kernels (``decode_navigation``) or its host twin with the same bits (``decode_navigation_host``).  A ``NavResult`` of
the device call keeps device tensors and reads them back (after ``ctx.sync()``) at the first look at a value.

The encoders a simulation needs are here too: ``lnav_subframe``, ``cnav_message``, ``cnav_fec_encode``."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from .context import Context, get_context
from .monitor import TrackMonitor
from .results import PlannedResult, host_check, new_plan, plan_report
from .streams import addr, keep_alive, vp

LNAV, CNAV = _lib.GAT_NAV_LNAV, _lib.GAT_NAV_CNAV
FRAME_BITS = _lib.GAT_NAV_FRAME_BITS
PREAMBLE = (1, 0, 0, 0, 1, 0, 1, 1)
_PARITY_MASKS = (0xBB1F3480, 0x5D8F9A40, 0xAEC7CD00, 0x5763E680, 0x6BB1F340, 0x8B7A89C0)
_CRC24Q = 0x1864CFB


def nav_format_for(system) -> int:
    """``GAT_NAV_LNAV`` for ``GPSL1``, ``GAT_NAV_CNAV`` for ``GPSL5``.  ``system``: a ``GNSSSystem`` or its name."""
    name = system if isinstance(system, str) else system.name
    if name == "GPSL1":
        return LNAV
    if name == "GPSL5":
        return CNAV
    raise ValueError(f"no navigation message known for {name!r}")


def _format(fmt) -> int:
    if isinstance(fmt, (int, np.integer)):
        return int(fmt)
    if isinstance(fmt, str) and fmt.upper() in ("LNAV", "CNAV"):
        return LNAV if fmt.upper() == "LNAV" else CNAV
    return nav_format_for(fmt)


def nav_config(fmt, symbol_capacity: int, max_frames: int | None, min_frames: int) -> _lib.NavConfig:
    """``gat_nav_config`` from Python values (``max_frames=None``: every whole frame the capacity holds, at least 1).  Nothing is
    checked: the library refuses."""
    cfg = _lib.NavConfig()
    cfg.struct_size = C.sizeof(_lib.NavConfig)
    cfg.format, cfg.symbol_capacity = _format(fmt), int(symbol_capacity)
    bits = int(symbol_capacity) // (2 if cfg.format == CNAV else 1)
    cfg.max_frames = max(1, bits // FRAME_BITS) if max_frames is None else int(max_frames)
    cfg.min_frames = int(min_frames)
    return cfg


class NavResult(PlannedResult):
    """The decoder's outputs of one call.  Raw: ``channels`` (structured ``[K]``: frame_offset, symbol_phase, inverted, score,
    second_score, num_frames, num_bits, tow_steps), ``frames`` (structured ``[K, max_frames]``: status, tow, id, prn, words),
    ``decoded`` uint8 ``[K, P, bit_capacity]`` (every phase, before the polarity), ``path_metric`` int32 ``[K, P]``.  Derived:
    ``frame_offset``, ``inverted``, ``symbol_phase``, ``score``, ``second_score``, ``num_frames``, ``tow_steps`` ``[K]``; ``synced``;
    ``words``, ``tow``, ``subframe_id`` / ``message_type``, ``prn``, ``status``, ``ok`` ``[K, max_frames]``; ``bits``: a list of the
    channels' bits of the chosen phase with the polarity undone."""

    _VIEWS = {"channels": (_lib.NAV_CHANNEL_DTYPE, False), "frames": (_lib.NAV_FRAME_DTYPE, True)}

    def __init__(self, raw: dict, fmt: int, ctx: Context | None = None):
        super().__init__(raw, ctx)
        self.format = int(fmt)

    channels = property(lambda self: self._h()["channels"])
    frames = property(lambda self: self._h()["frames"])
    decoded = property(lambda self: self._h()["decoded"])
    path_metric = property(lambda self: self._h()["path_metric"])
    frame_offset = property(lambda self: self.channels["frame_offset"].copy())
    inverted = property(lambda self: self.channels["inverted"].copy())
    symbol_phase = property(lambda self: self.channels["symbol_phase"].copy())
    score = property(lambda self: self.channels["score"].copy())
    second_score = property(lambda self: self.channels["second_score"].copy())
    num_frames = property(lambda self: self.channels["num_frames"].copy())
    tow_steps = property(lambda self: self.channels["tow_steps"].copy())
    synced = property(lambda self: self.channels["frame_offset"] >= 0)
    words = property(lambda self: self.frames["words"].copy())
    tow = property(lambda self: self.frames["tow"].copy())
    status = property(lambda self: self.frames["status"].copy())
    prn = property(lambda self: self.frames["prn"].copy())
    subframe_id = property(lambda self: self.frames["id"].copy())
    message_type = subframe_id

    @property
    def ok(self) -> np.ndarray:
        """every check of the frame passed (the preamble and all ten parities, or the preamble and the CRC)"""
        return self.frames["status"] == (0x3 if self.format == CNAV else 0x7ff)

    @property
    def bits(self) -> list:
        ch, dec = self.channels, self.decoded
        return [dec[k, ch["symbol_phase"][k], :ch["num_bits"][k]] ^ np.uint8(ch["inverted"][k]) for k in range(dec.shape[0])]


def _resolve(mon_or_sym_re, fmt, channels):
    """(sym_re, monitor records or None, format) of the first arguments of both calls"""
    if isinstance(mon_or_sym_re, TrackMonitor):
        mon = mon_or_sym_re
        if fmt is None:
            if mon.symbol_blocks not in (20, 10):
                raise ValueError("format cannot be told from the monitor's symbol length: pass format")
            fmt = LNAV if mon.symbol_blocks == 20 else CNAV
        return mon._raw["sym_re"], (mon._raw["channels"] if channels is None else channels), _format(fmt)
    if fmt is None:
        raise ValueError("format must be given with bare symbols")
    return mon_or_sym_re, channels, _format(fmt)


def decode_navigation(mon_or_sym_re, format=None, *, channels=None, max_frames: int | None = None, min_frames: int = 1,
                      ctx: Context | None = None) -> NavResult:
    """``gat_nav_decode`` on the device.  ``mon_or_sym_re``: a ``TrackMonitor`` of the device call -- its ``sym_re`` and channel
    records are passed as they are, nothing is copied and nothing read back -- or a float64 device tensor ``[K, capacity]`` with
    ``channels`` None (every row is full) or the monitor's records.  ``format``: ``GAT_NAV_LNAV`` / ``GAT_NAV_CNAV``, "LNAV" /
    "CNAV", a ``GNSSSystem``, or None with a monitor of 20 (LNAV) or 10 (CNAV) blocks a symbol.  Enqueues on the context's
    stream and returns at once."""
    sym, recs, fmt = _resolve(mon_or_sym_re, format, channels)
    if not isinstance(sym, torch.Tensor) or sym.dtype != torch.float64 or sym.dim() != 2 or not sym.is_contiguous():
        raise ValueError("the symbols must be a contiguous float64 device tensor [K, capacity]")
    K, cap = (int(v) for v in sym.shape)
    if recs is not None and (not isinstance(recs, torch.Tensor) or not recs.is_contiguous() or recs.numel() * recs.element_size() != K * 32):
        raise ValueError("channels must be the monitor's K records on the device")
    if ctx is None:
        ctx = mon_or_sym_re._ctx if isinstance(mon_or_sym_re, TrackMonitor) and mon_or_sym_re._ctx is not None else get_context(sym.device)
    cfg = nav_config(fmt, cap, max_frames, min_frames)
    P, dev = (2 if fmt == CNAV else 1), sym.device
    raw = {"channels": torch.empty((K, 8), dtype=torch.int32, device=dev),
           "frames": torch.empty((K, max(int(cfg.max_frames), 0) * 14), dtype=torch.int32, device=dev),
           "decoded": torch.empty((K, P, cap // P), dtype=torch.uint8, device=dev),
           "path_metric": torch.empty((K, P), dtype=torch.int32, device=dev)}
    rc = ctx.lib.gat_nav_decode(ctx._h, vp(sym), vp(recs), K, C.byref(cfg), vp(raw["channels"]), vp(raw["frames"]), vp(raw["decoded"]),
                                vp(raw["path_metric"]))
    ctx.check(rc, "gat_nav_decode")
    return keep_alive(NavResult(raw, fmt, ctx), sym, recs)


def decode_navigation_host(mon_or_sym_re, format=None, *, channels=None, max_frames: int | None = None, min_frames: int = 1) -> NavResult:
    """``gat_nav_decode_host``: the same rule and the same bits over a float64 numpy array ``[K, capacity]`` (or a ``TrackMonitor``
    of either call, read back); needs no device."""
    if isinstance(mon_or_sym_re, TrackMonitor):
        mon = mon_or_sym_re
        _, _, fmt = _resolve(mon, format, channels)
        sym, recs = mon._h()["sym_re"], (mon.channels if channels is None else channels)
    else:
        sym, recs, fmt = _resolve(mon_or_sym_re, format, channels)
    sym = np.ascontiguousarray(sym, dtype=np.float64)
    if sym.ndim != 2:
        raise ValueError("the symbols must be [K, capacity]")
    K, cap = sym.shape
    if recs is not None:
        recs = np.ascontiguousarray(recs)
        if recs.nbytes != K * 32:
            raise ValueError("channels must be the monitor's K records")
    cfg = nav_config(fmt, cap, max_frames, min_frames)
    P = 2 if fmt == CNAV else 1
    raw = {"channels": np.zeros(K, dtype=_lib.NAV_CHANNEL_DTYPE), "frames": np.zeros((K, max(int(cfg.max_frames), 0)), dtype=_lib.NAV_FRAME_DTYPE),
           "decoded": np.zeros((K, P, cap // P), dtype=np.uint8), "path_metric": np.zeros((K, P), dtype=np.int32)}
    rc = _lib.load().gat_nav_decode_host(addr(sym), addr(recs), K, C.byref(cfg), addr(raw["channels"]), addr(raw["frames"]),
                                         addr(raw["decoded"]), addr(raw["path_metric"]))
    host_check(rc, "gat_nav_decode_host")
    return NavResult(raw, fmt)


def nav_plan(num_channels: int, symbol_capacity: int, format, max_frames: int | None = None, min_frames: int = 1) -> dict:
    """``gat_nav_decode_plan``: the counts, the scratch bytes and the workgroups of each kernel of such a call."""
    cfg = nav_config(format, symbol_capacity, max_frames, min_frames)
    plan = new_plan(_lib.NavPlan)
    rc = _lib.load().gat_nav_decode_plan(int(num_channels), C.byref(cfg), C.byref(plan))
    host_check(rc, "gat_nav_decode_plan")
    return plan_report(plan)


# ---- encoders: what a simulation sends ---------------------------------------------------------------------------------------------
def _bits_of(value: int, count: int) -> list:
    return [(int(value) >> (count - 1 - i)) & 1 for i in range(count)]


def _payload(payload, count: int) -> list:
    p = [] if payload is None else [int(v) & 1 for v in np.asarray(payload).reshape(-1)]
    if len(p) > count:
        raise ValueError(f"the payload holds more than {count} bits")
    return p + [0] * (count - len(p))


def _lnav_word(d: int, d29: int, d30: int, solve: bool = False) -> int:
    """The thirty sent bits of the source bits d (24 bits, d1 the MSB) after a word that ended in D29* = d29, D30* = d30;
    ``solve``: d23 and d24 are chosen so that the word ends in D29 = D30 = 0."""
    for t in range(4) if solve else (None,):
        src = d if t is None else (d & ~3) | t
        x = (d29 << 31) | (d30 << 30) | (src << 6)
        par = 0
        for m in _PARITY_MASKS:
            par = (par << 1) | (bin(x & m).count("1") & 1)
        if t is None or (par & 3) == 0:
            return ((src ^ (0xFFFFFF if d30 else 0)) << 6) | par
    raise AssertionError("no solution")  # the two equations are independent in d23 and d24


def lnav_subframe(tow: int, subframe_id: int, payload=None, *, tlm: int = 0, flags: int = 0) -> np.ndarray:
    """One LNAV subframe as 300 bits (uint8): the TLM word (preamble, ``tlm``: its 16 further bits), the HOW (``tow``: the 17-bit
    count, ``flags``: alert and anti-spoof, ``subframe_id``) and words 3 .. 10 from ``payload`` (up to 190 bits, zero-filled), with
    the parity of every word and the solved bits of the HOW and of word 10, after a word that ended in D29 = D30 = 0."""
    p = _payload(payload, 190)
    src = [(0x8B << 16) | (int(tlm) & 0xFFFF), ((int(tow) & 0x1FFFF) << 7) | ((int(flags) & 3) << 5) | ((int(subframe_id) & 7) << 2)]
    for w in range(7):
        src.append(int("".join(str(b) for b in p[24 * w:24 * w + 24]), 2))
    src.append(int("".join(str(b) for b in p[168:190]), 2) << 2)
    out, d29, d30 = [], 0, 0
    for w, d in enumerate(src):
        sent = _lnav_word(d, d29, d30, solve=w in (1, 9))
        out += _bits_of(sent, 30)
        d29, d30 = (sent >> 1) & 1, sent & 1
    return np.array(out, dtype=np.uint8)


def crc24q(bits) -> int:
    """CRC-24Q of a bit sequence: polynomial 0x1864CFB, initial value 0, MSB first, not reflected."""
    crc = 0
    for b in np.asarray(bits).reshape(-1):
        crc ^= (int(b) & 1) << 23
        crc <<= 1
        if crc & 0x1000000:
            crc ^= _CRC24Q
    return crc


def cnav_message(prn: int, msg_type: int, tow: int, payload=None) -> np.ndarray:
    """One CNAV message as 300 bits (uint8): preamble, ``prn`` (6 bits), ``msg_type`` (6), ``tow`` (17), ``payload`` (up to 239 bits
    from the alert flag on, zero-filled) and the CRC-24Q of those 276 bits."""
    body = list(PREAMBLE) + _bits_of(prn, 6) + _bits_of(msg_type, 6) + _bits_of(tow, 17) + _payload(payload, 239)
    return np.array(body + _bits_of(crc24q(body), 24), dtype=np.uint8)


def cnav_fec_encode(bits) -> np.ndarray:
    """The rate-1/2 K = 7 code of CNAV from a zero register: two symbols (uint8) a bit, G1 = 171 first, then G2 = 133 (octal)."""
    out, s = [], 0
    for u in (int(v) & 1 for v in np.asarray(bits).reshape(-1)):
        out.append((u ^ (s >> 5) ^ (s >> 4) ^ (s >> 3) ^ s) & 1)
        out.append((u ^ (s >> 4) ^ (s >> 3) ^ (s >> 1) ^ s) & 1)
        s = (u << 5) | (s >> 1)
    return np.array(out, dtype=np.uint8)
