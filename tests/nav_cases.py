"""Known-answer streams and the call harness of the navigation data tests: a stream is a junk prefix, frames and a junk suffix, as
bits (LNAV) or as the symbols of the convolutional code (CNAV); a call writes its outputs into one canary-filled byte buffer with
guard bands between them, the same layout on the host and on the device, so that two calls compare as whole buffers."""
import ctypes as C

import numpy as np

from tests import nav_ref as ref

CANARY = 0xA5
GUARD = 64
OUTPUTS = ("channels", "frames", "decoded", "path_metric")
CHANNEL_DTYPE = np.dtype([(n, "<i4") for n in ("frame_offset", "symbol_phase", "inverted", "score", "second_score", "num_frames", "num_bits",
                                                "tow_steps")])
FRAME_DTYPE = np.dtype([("status", "<i4"), ("tow", "<i4"), ("id", "<i4"), ("prn", "<i4"), ("words", "<u4", (10,))])
MON_DTYPE = np.dtype([("symbol_offset", "<i4"), ("start", "<i4"), ("num_symbols", "<i4"), ("reserved", "<i4"), ("e_max", "<f8"), ("e_second", "<f8")])


def junk(rng, n):
    """random bits without three equal ones in a row: the preamble 10001011 holds 000 and its inverse 111, so junk holds neither"""
    b = rng.integers(0, 2, n).astype(np.uint8)
    for i in range(2, n):
        if b[i - 1] == b[i - 2]:
            b[i] = b[i - 1] ^ 1
    return b


def junk_runs(rng, n):
    """junk by its runs, for many rows at once: runs of one or two equal bits"""
    return np.repeat(np.arange(n, dtype=np.uint8) & 1, rng.integers(1, 3, n))[:n]


def lnav_frames(rng, F, tow0=1000, break_frame=None):
    out = []
    for f in range(F):
        sf = ref.lnav_subframe((tow0 + f) % ref.TOW_MOD, f % 5 + 1, list(rng.integers(0, 2, 190)), tlm=int(rng.integers(0, 1 << 14)) << 2)
        if f == break_frame:
            sf = sf.copy()
            sf[30 + 10] ^= 1  # one bit of word 2: its parity fails and the frame no longer hits
        out.append(sf)
    return np.concatenate(out) if out else np.zeros(0, np.uint8)


def cnav_frames(rng, F, tow0=2000, prn=7, break_frame=None):
    out = []
    for f in range(F):
        m = ref.cnav_message(prn, 10 + f % 4, (tow0 + f) % ref.TOW_MOD, list(rng.integers(0, 2, 239)))
        if f == break_frame:
            m = m.copy()
            m[150] ^= 1  # the CRC fails: no hit
        out.append(m)
    return np.concatenate(out) if out else np.zeros(0, np.uint8)


def stream_bits(rng, fmt, prefix, F, suffix, **kw):
    body = (cnav_frames if fmt == ref.CNAV else lnav_frames)(rng, F, **kw)
    return np.concatenate([junk(rng, prefix), body, junk(rng, suffix)])


def to_symbols(fmt, bits, inverted=False, phase=0, amplitude=1.0):
    """+-amplitude symbols of a bit stream (a 0 bit is positive): the bits themselves, or their convolutional code after `phase`
    leading symbols that belong to no pair"""
    s = bits if fmt == ref.LNAV else np.concatenate([np.zeros(phase, np.uint8), ref.fec_encode(bits)])
    x = amplitude * (1.0 - 2.0 * s.astype(np.float64))
    return -x if inverted else x


def rows(streams, cap=None, fill=np.nan):
    """[K, cap] symbols (filled beyond each stream) and the monitor records that carry the counts"""
    cap = max(len(s) for s in streams) if cap is None else cap
    sym = np.full((len(streams), cap), fill)
    mon = np.zeros(len(streams), MON_DTYPE)
    for k, s in enumerate(streams):
        sym[k, :len(s)] = s
        mon[k] = (0, 0, len(s), 0, 1.0, 0.5)
    return sym, mon


# ---- the call harness ------------------------------------------------------------------------------------------------------------------
def config(lib_mod, fmt, cap, max_frames, min_frames=1):
    cfg = lib_mod.NavConfig()
    cfg.struct_size = C.sizeof(lib_mod.NavConfig)
    cfg.format, cfg.symbol_capacity, cfg.max_frames, cfg.min_frames = fmt, cap, max_frames, min_frames
    return cfg


def layout(K, fmt, cap, max_frames):
    P = 2 if fmt == ref.CNAV else 1
    sizes = {"channels": K * 32, "frames": K * max(max_frames, 0) * 56, "decoded": K * P * (max(cap, 0) // P), "path_metric": K * P * 4}
    at, off = {}, GUARD
    for name in OUTPUTS:
        at[name] = (off, sizes[name])
        off = (off + sizes[name] + GUARD + 63) // 64 * 64
    return at, off + GUARD


def canaries_intact(buf, at, want=OUTPUTS):
    mask = np.ones(buf.size, bool)
    for name in want:
        o, n = at[name]
        mask[o:o + n] = False
    return bool(np.all(buf[mask] == CANARY))


def take(buf, at, name, K, fmt):
    o, n = at[name]
    raw = buf[o:o + n]
    if name == "channels":
        return raw.view(CHANNEL_DTYPE)
    if name == "frames":
        return raw.view(FRAME_DTYPE).reshape(K, -1)
    if name == "decoded":
        return raw.reshape(K, 2 if fmt == ref.CNAV else 1, -1)
    return raw.view(np.int32).reshape(K, -1)


def host_call(g, sym, mon, cfg, want=OUTPUTS, K=None):
    """(status, buffer, layout) of gat_nav_decode_host over numpy inputs (None: a null pointer)"""
    K = sym.shape[0] if K is None else K
    at, total = layout(max(K, 1), cfg.format if cfg.format in (0, 1) else 0, cfg.symbol_capacity, cfg.max_frames)
    buf = np.full(total, CANARY, np.uint8)
    ptr = {n: (buf.ctypes.data + at[n][0] if n in want else None) for n in OUTPUTS}
    rc = g.load_library().gat_nav_decode_host(None if sym is None else sym.ctypes.data, None if mon is None else mon.ctypes.data, K,
                                              None if cfg is None else C.byref(cfg), ptr["channels"], ptr["frames"], ptr["decoded"], ptr["path_metric"])
    return rc, buf, at


def device_enqueue(g, ctx, sym_t, mon_t, cfg, want=OUTPUTS):
    """the same call on the device, enqueued and not synchronised: (status, device buffer, layout); sym_t float64 [K, cap] and mon_t
    (uint8 view of the records, or None) are device tensors"""
    import torch

    K = sym_t.shape[0]
    at, total = layout(K, cfg.format, cfg.symbol_capacity, cfg.max_frames)
    buf = torch.full((total,), CANARY, dtype=torch.uint8, device=sym_t.device)
    ptr = {n: (C.c_void_p(buf.data_ptr() + at[n][0]) if n in want else None) for n in OUTPUTS}
    rc = ctx.lib.gat_nav_decode(ctx._h, C.c_void_p(sym_t.data_ptr()), None if mon_t is None else C.c_void_p(mon_t.data_ptr()), K, C.byref(cfg),
                                ptr["channels"], ptr["frames"], ptr["decoded"], ptr["path_metric"])
    return rc, buf, at


def device_call(g, ctx, sym_t, mon_t, cfg, want=OUTPUTS):
    """device_enqueue, synchronised and read back: (status, buffer, layout)"""
    rc, buf, at = device_enqueue(g, ctx, sym_t, mon_t, cfg, want)
    ctx.sync()
    return rc, buf.cpu().numpy(), at


def check_against_ref(buf, at, fmt, sym, counts, max_frames, min_frames, what="", decoded=None):
    """every output of a call, as integers, against the restatement; returns the restatement's records.  decoded: what
    ref.decode_bits gave for these symbols and counts in an earlier check, so that one stream is decoded once"""
    K = sym.shape[0]
    dec, pm = ref.decode_bits(fmt, sym, counts) if decoded is None else decoded
    assert np.array_equal(take(buf, at, "decoded", K, fmt), dec), (what, "decoded")
    assert np.array_equal(take(buf, at, "path_metric", K, fmt), pm), (what, "path_metric")
    chans, frames = take(buf, at, "channels", K, fmt), take(buf, at, "frames", K, fmt)
    recs = []
    for k in range(K):
        rec, fr = ref.search(fmt, dec[k], int(counts[k]), max_frames, min_frames)
        assert {n: int(chans[k][n]) for n in CHANNEL_DTYPE.names} == rec, (what, k, chans[k], rec)
        for f in range(max_frames):
            want = fr[f] if f < len(fr) else (0, 0, 0, 0, [0] * 10)
            got = frames[k, f]
            assert (int(got["status"]), int(got["tow"]), int(got["id"]), int(got["prn"]), [int(w) for w in got["words"]]) == tuple(want), (what, k, f)
        recs.append(rec)
    return recs


def check_certificate(buf, at, sym, counts, sent_phase=None, rows=None):
    """CNAV: the path metric of every (channel, phase) is the metric of the decoded bits (ref.path_certificate); sent_phase[k]:
    the phase at which row k is a code word, where that metric is then no smaller than the sent symbols' own; rows: all, or these"""
    K = sym.shape[0]
    dec, pm = take(buf, at, "decoded", K, ref.CNAV), take(buf, at, "path_metric", K, ref.CNAV)
    for k in range(K) if rows is None else rows:
        n = int(counts[k])
        q = ref.quantise(sym[k], n).astype(np.int64)
        for ph in (0, 1):
            T = max(n - ph, 0) // 2
            window = q[ph:ph + 2 * T]
            assert ref.path_certificate(window, dec[k, ph, :T]) == pm[k, ph], (k, ph, "the metric is not the returned path's")
            if sent_phase is not None and sent_phase[k] == ph:
                assert pm[k, ph] >= int((window * np.sign(sym[k, ph:ph + 2 * T])).sum()), (k, ph, "the sent path scores higher")
