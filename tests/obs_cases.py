"""Consistent parameter histories for the observables' tests.  A history is what a loop would have left that tracked a signal whose
time of transmission is known at some anchor blocks: between two anchors the code advances by the same amount every block (so
the code rate of the span is read off the anchors), outside them at a given rate; every record's code phase is the fraction of
the running transmit time, every wrap is whole (0, 1 or 2 periods a block, more with a long block), and the carrier runs at any
frequency of either sign.  With it come the monitor's and the decoder's records for a frame that begins at a chosen transmit
millisecond -- or the accumulators whose bit edges sit at the history's code-period boundaries, for the real monitor and decoder."""
import numpy as np

import gpuacceleratedtracking_amd._lib as _lib

WEEK_MS = 604800000
LC, FC = 1023, 1.023e6
FS, N = 2.046e6, 2046


def base_config(**kw) -> dict:
    """GPS L1 C/A at 2.046 MHz, 1 ms blocks, LNAV"""
    cfg = dict(format=0, code_length=LC, code_freq_nominal_hz=FC, block_seconds=N / FS, block_samples=N, sampling_freq_hz=FS, symbol_blocks=20,
               if_hz=0.0)
    cfg.update(kw)
    return cfg


class History:
    """records: structured [B + 1, K]; ms: int64 [B + 1, K], the whole milliseconds of the transmit time at every block start (of the
    week), so that the truth of block b is (ms[b], tau[b] / fc)"""

    def __init__(self, records, ms):
        self.records, self.ms = records, ms
        self.B, self.K = records.shape[0] - 1, records.shape[1]

    @property
    def tx_frac(self):
        return self.records["code_phase_chips"] / FC


def _walk(tau, step, forward: bool, Lc: float):
    """one block on: (tau', whole periods passed)"""
    x = tau + step if forward else tau - step
    w = np.floor(x / Lc)
    t = x - w * Lc
    over = t >= Lc  # rounding at the upper edge
    t, w = np.where(over, t - Lc, t), np.where(over, w + 1, w)
    under = t < 0.0
    t, w = np.where(under, t + Lc, t), np.where(under, w - 1, w)
    return t, w.astype(np.int64)


def history(B: int, anchors, anchor_ms, anchor_tau, *, rate_before=None, rate_after=None, carrier_hz=0.0, carrier_phase0=0.0,
            block_seconds=N / FS, code_length=LC, prn=None) -> History:
    """anchors: ascending block indices [A]; anchor_ms int [A, K] and anchor_tau float [A, K]: the transmit time there.  rate_before /
    rate_after [K]: the code rate in chips/s before the first and after the last anchor (default nominal).  carrier_hz: [K] or
    [B + 1, K]; the carrier phase is kept in [0, 1)."""
    anchors = [int(a) for a in anchors]
    anchor_ms, anchor_tau = np.atleast_2d(np.asarray(anchor_ms, np.int64)), np.atleast_2d(np.asarray(anchor_tau, np.float64))
    K, Lc, T = anchor_ms.shape[1], float(code_length), float(block_seconds)
    nominal = Lc * 1000.0
    tau, ms, rate = np.zeros((B + 1, K)), np.zeros((B + 1, K), np.int64), np.zeros((B + 1, K))
    rb = np.broadcast_to(np.asarray(nominal if rate_before is None else rate_before, np.float64), (K,))
    ra = np.broadcast_to(np.asarray(nominal if rate_after is None else rate_after, np.float64), (K,))
    for j, a in enumerate(anchors):
        tau[a], ms[a] = anchor_tau[j], anchor_ms[j]
    for b in range(anchors[0] - 1, -1, -1):  # backwards from the first anchor
        rate[b] = rb
        tau[b], w = _walk(tau[b + 1], rb * T, False, Lc)
        ms[b] = ms[b + 1] + w
    for j in range(len(anchors) - 1):  # between anchors: equal steps
        a0, a1 = anchors[j], anchors[j + 1]
        dms = (anchor_ms[j + 1] - anchor_ms[j] + WEEK_MS // 2) % WEEK_MS - WEEK_MS // 2
        step = (dms * Lc + (anchor_tau[j + 1] - anchor_tau[j])) / (a1 - a0)
        for b in range(a0, a1):
            rate[b] = step / T
            t, w = _walk(tau[b], step, True, Lc)
            if b + 1 < a1:
                tau[b + 1], ms[b + 1] = t, ms[b] + w
        assert np.abs(((tau[a1 - 1] + step) - tau[a1]) / Lc - np.rint(((tau[a1 - 1] + step) - tau[a1]) / Lc)).max() < 1e-7
    for b in range(anchors[-1], B):  # onwards from the last
        rate[b] = ra
        tau[b + 1], w = _walk(tau[b], ra * T, True, Lc)
        ms[b + 1] = ms[b] + w
    rate[B] = ra
    ms %= WEEK_MS
    rec = np.zeros((B + 1, K), dtype=_lib.PARAMS_DTYPE)
    rec["prn"] = np.arange(K) if prn is None else prn
    rec["code_freq_hz"], rec["code_phase_chips"] = rate, tau
    fcarr = np.broadcast_to(np.asarray(carrier_hz, np.float64), (B + 1, K))
    phi = np.zeros((B + 1, K))
    phi[0] = carrier_phase0
    for b in range(B):
        x = phi[b] + fcarr[b] * T
        phi[b + 1] = x - np.floor(x)
    rec["carrier_freq_hz"], rec["carrier_phase_cycles"] = fcarr, phi
    return History(rec, ms)


def from_truth(B: int, tx_ms0, tx_frac0, doppler_hz, *, carrier_center_hz=1575.42e6, if_hz=0.0, **kw) -> History:
    """a history from the transmit time at block 0 and a constant Doppler a channel: the code runs at fc (1 + doppler / carrier)"""
    dop = np.asarray(doppler_hz, np.float64)
    rate = FC * (1.0 + dop / carrier_center_hz)
    return history(B, [0], [tx_ms0], [np.asarray(tx_frac0, np.float64) * FC], rate_after=rate, carrier_hz=if_hz + dop, **kw)


def period_index(h: History):
    """int64 [B + 1, K]: the transmit millisecond (not wrapped into the week from block 0 on) in which the middle of block b lies,
    up to the block's own stretch -- the period whose bit dominates the block's prompt"""
    first = h.ms[0]
    rel = (h.ms - first + WEEK_MS // 2) % WEEK_MS - WEEK_MS // 2  # the history is far shorter than half a week
    return first + rel + np.floor(h.records["code_phase_chips"] / LC + 0.5).astype(np.int64)


def sync_records(h: History, frame_ms, *, tow=None, num_frames=3, max_frames=4, tow_steps=None, P=1, Pd=20, full=0x7FF):
    """The monitor's and the decoder's records, written by hand, of a frame 0 that begins at transmit millisecond frame_ms [K] (a
    multiple of 6000 unless tow is given): g is the block whose start is nearest that instant.  Returns (mon [K], nav [K], frames
    [K, max_frames], g [K])."""
    K = h.K
    frame_ms = np.broadcast_to(np.asarray(frame_ms, np.int64), (K,))
    mon, nav = np.zeros(K, _lib.MONITOR_CHANNEL_DTYPE), np.zeros(K, _lib.NAV_CHANNEL_DTYPE)
    frames = np.zeros((K, max_frames), _lib.NAV_FRAME_DTYPE)
    pidx = period_index(h)
    g = np.zeros(K, np.int64)
    for k in range(K):
        target = pidx[0, k] + ((frame_ms[k] - pidx[0, k] % WEEK_MS + WEEK_MS // 2) % WEEK_MS - WEEK_MS // 2)
        at = np.flatnonzero(pidx[:, k] >= target)
        assert at.size and pidx[at[0], k] == target, "the frame's first millisecond is not inside the history"
        g[k] = at[0]
        mon["start"][k] = mon["symbol_offset"][k] = g[k] % Pd
        mon["num_symbols"][k] = (h.B - mon["start"][k]) // Pd
        symbols = g[k] // Pd  # whole symbols before the frame: with two a bit, an odd count is symbol phase 1
        nav["symbol_phase"][k] = symbols % P
        nav["frame_offset"][k] = symbols // P
        nav["num_frames"][k], nav["score"][k] = num_frames, num_frames
        nav["tow_steps"][k] = num_frames - 1 if tow_steps is None else tow_steps
        t0 = (frame_ms[k] // 6000 + 1) % 100800 if tow is None else np.broadcast_to(np.asarray(tow), (K,))[k]
        for f in range(min(num_frames, max_frames)):
            frames["status"][k, f], frames["tow"][k, f], frames["id"][k, f] = full, (t0 + f) % 100800, f % 5 + 1
    return mon, nav, frames, g


def standard(B=700, K=4, *, seed=3, frame_lead=120, week_ms0=244800000 - 150, tau_g_fraction=None, sync=None, spread=3, **kw):
    """A ready case: K channels with transmit times a few tens of ms apart, Dopplers of both signs (large enough for wraps of 0 and 2
    periods within the history), the frame beginning about frame_lead blocks in, at the next multiple of 6000 ms.  The fraction of
    a period at the frame block is kept outside [0.35, 0.65] (tau_g_fraction [K] forces it).  Returns (History, mon, nav, frames, g)."""
    rng = np.random.default_rng(seed)
    dop = rng.uniform(2000.0, 5000.0, K) * np.where(np.arange(K) % 2 == 0, 1.0, -1.0)
    code_dop = np.where(np.arange(K) % 2 == 0, 40.0, -40.0)  # chips/s: far beyond a satellite's, legal for the rule
    frac = rng.uniform(0.0, 1.0, K)
    frac = np.where((frac > 0.3) & (frac < 0.7), frac * 0.3, frac)
    frac[:2] = [0.996, 0.004][:K]  # close under a boundary and rising, close over one and falling: a wrap of 2 and a wrap of 0
    if tau_g_fraction is not None:
        frac = np.broadcast_to(np.asarray(tau_g_fraction, np.float64), (K,)).copy()
    frame_ms = (week_ms0 // 6000 + 1) * 6000 % WEEK_MS
    # every channel is anchored at block frame_lead, spread (k mod 8) ms and the fraction before its frame: its frame block comes that
    # many blocks later, and the nearest boundary there is the frame's first millisecond
    g0 = frame_lead + (np.arange(K) % 8) * spread
    ms_a = (frame_ms - (g0 - frame_lead) - np.where(frac >= 0.5, 1, 0)) % WEEK_MS
    rate = FC + code_dop
    h = history(B, [frame_lead], [ms_a], [frac * LC], rate_before=rate, rate_after=rate, carrier_hz=kw.get("if_hz", 0.0) + dop,
                carrier_phase0=rng.uniform(0.0, 1.0, K), block_seconds=kw.get("block_seconds", N / FS))
    mon, nav, frames, g = sync_records(h, frame_ms, **(sync or {}))
    assert (g == g0).all(), (g, g0)
    return h, mon, nav, frames, g


def prompt_signs(h: History, frame_ms, frame_bits, rng):
    """float64 [B, K]: +1 / -1, the sign of the data bit that dominates each block -- the bits of frame_bits[k] (one bit per 20 ms
    from transmit millisecond frame_ms[k] on), random bits before and after"""
    pidx = period_index(h)[:-1]
    out = np.zeros(pidx.shape)
    for k in range(h.K):
        rel = pidx[:, k] - (pidx[0, k] + ((frame_ms[k] - pidx[0, k] % WEEK_MS + WEEK_MS // 2) % WEEK_MS - WEEK_MS // 2))
        bit = np.floor_divide(rel, 20)
        bits = np.asarray(frame_bits[k], np.int64)
        lo, hi = int(bit.min()), int(bit.max())
        table = rng.integers(0, 2, hi - lo + 1)
        inside = np.arange(lo, hi + 1)
        sel = (inside >= 0) & (inside < len(bits))
        table[sel] = bits[inside[sel]]
        out[:, k] = 1.0 - 2.0 * table[bit - lo]
    return out
