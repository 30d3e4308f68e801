"""A textbook restatement of the observables' rule (include/gat.h, "observables") in numpy: ``np.cumsum`` of the rounded differences
of neighbouring records, Python integers for the arithmetic of the week.  Written from the header's text, not from csrc/gat_obs.h;
the only floating-point results are the single quotients of the rule, so the host twin must agree bit for bit."""
import numpy as np

WEEK_MS = 604800000
BAD_RECORD, NO_BIT_SYNC, NO_FRAME_SYNC, FRAME_OUTSIDE, NO_TOW, EDGE_AMBIGUOUS = 1, 2, 4, 8, 16, 32
BELOW_MS = float(np.nextafter(1e-3, 0.0))


def wrap_half_week(d: int) -> int:
    d %= WEEK_MS
    return d - WEEK_MS if d >= WEEK_MS // 2 else d


def reference(hist, mon, nav, frames, *, format, code_length, code_freq_nominal_hz, block_seconds, block_samples, sampling_freq_hz,
              symbol_blocks, max_frames, if_hz=0.0, min_tow_steps=0, epoch_first=0, epoch_stride=1, num_epochs=None, rx="from_tx",
              travel_ms=68, edge_margin=0.1):
    """hist: structured [B + 1, K] (gat_channel_params); mon, nav: structured [K]; frames: structured [K, >= max_frames].  Returns a
    dict of the nine outputs (channels as a list of dicts)."""
    B, K = hist.shape[0] - 1, hist.shape[1]
    E = (B - epoch_first) // epoch_stride + 1 if num_epochs is None else num_epochs
    Lc, fc, T = float(code_length), float(code_freq_nominal_hz), float(block_seconds)
    P = 2 if format == 1 else 1
    full = 0x3 if format == 1 else 0x7FF
    tau, phi = hist["code_phase_chips"], hist["carrier_phase_cycles"]
    fcode, fcarr = hist["code_freq_hz"], hist["carrier_freq_hz"]
    with np.errstate(all="ignore"):
        q = ((tau[:-1] + fcode[:-1] * T) - tau[1:]) / Lc
        d = (phi[:-1] + fcarr[:-1] * T) - phi[1:]
        w, c = np.rint(q), np.rint(d)
        bad_q = ~(np.abs(q - w) <= 1e-6) | ~(np.abs(q) < 2.0 ** 31)
        bad_d = ~(np.abs(d - c) <= 1e-6) | ~(np.abs(d) < 2.0 ** 31)
    finite = np.isfinite(tau) & np.isfinite(phi) & np.isfinite(fcode) & np.isfinite(fcarr)
    bad = (~finite).any(axis=0) | bad_q.any(axis=0) | bad_d.any(axis=0)
    w = np.where(bad_q, 0.0, w).astype(np.int64)
    c = np.where(bad_d, 0.0, c).astype(np.int64)
    n = np.concatenate([np.zeros((1, K), np.int64), np.cumsum(w, axis=0)])
    W = np.concatenate([np.zeros((1, K), np.int64), np.cumsum(c, axis=0)])
    b_e = epoch_first + epoch_stride * np.arange(E)
    bad |= ~((tau[b_e] >= 0.0) & (tau[b_e] < Lc)).all(axis=0)

    out = {"tx_ms": np.full((E, K), -1, np.int32), "tx_frac": np.zeros((E, K)), "rx_ms": np.full(E, -1, np.int32), "rx_frac": np.zeros(E),
           "carrier_cycles": np.zeros((E, K), np.int64), "carrier_frac": np.zeros((E, K)), "doppler_hz": np.zeros((E, K)),
           "code_rate_hz": np.zeros((E, K)), "channels": []}
    for k in range(K):
        status, g, synced = 0, -1, False
        if mon["start"][k] < 0:
            status |= NO_BIT_SYNC
        if nav["frame_offset"][k] < 0:
            status |= NO_FRAME_SYNC
        if status == 0:
            synced = True
            g = int(mon["start"][k]) + (int(nav["symbol_phase"][k]) + P * int(nav["frame_offset"][k])) * symbol_blocks
            if g > B or g < 0:
                status |= FRAME_OUTSIDE
        fstar = next((f for f in range(min(int(nav["num_frames"][k]), max_frames)) if frames["status"][k, f] == full), None)
        frame0_ms = 0
        if fstar is None or nav["tow_steps"][k] < min_tow_steps:
            status |= NO_TOW
        else:
            frame0_ms = 6000 * ((int(frames["tow"][k, fstar]) - 1 - fstar) % 100800)
        inside = synced and not status & FRAME_OUTSIDE
        is_bad = bool(bad[k]) or (inside and not 0.0 <= tau[g, k] < Lc)
        if is_bad:
            status |= BAD_RECORD
        rec = dict(status=status, frame_block=g if synced else 0, tow_frame=0 if status & NO_TOW else fstar, frame0_ms=frame0_ms,
                   edge_period=0, edge_fraction=0.0)
        pstar = 0
        if inside and not is_bad:
            x = tau[g, k] / Lc
            pstar = int(n[g, k]) + int(np.rint(x))
            rec["edge_period"], rec["edge_fraction"] = pstar, float(x)
            if abs(x - 0.5) < edge_margin:
                rec["status"] |= EDGE_AMBIGUOUS
        out["channels"].append(rec)
        measured = (rec["status"] & ~EDGE_AMBIGUOUS) == 0
        if not is_bad:
            out["carrier_cycles"][:, k] = W[b_e, k]
            out["carrier_frac"][:, k] = phi[b_e, k]
            out["doppler_hz"][:, k] = fcarr[b_e, k] - if_hz
            out["code_rate_hz"][:, k] = fcode[b_e, k]
        if measured:
            for e, b in enumerate(b_e):
                out["tx_ms"][e, k] = (frame0_ms + (int(n[b, k]) - pstar)) % WEEK_MS
                f = tau[b, k] / fc
                out["tx_frac"][e, k] = BELOW_MS if f >= 1e-3 else f

    # reception
    if isinstance(rx, str):
        a = epoch_first
        seen = [k for k in range(K) if out["tx_ms"][0, k] >= 0]
        anchor = None
        if seen:
            ref = int(out["tx_ms"][0, seen[0]])
            best = max(seen, key=lambda k: (wrap_half_week(int(out["tx_ms"][0, k]) - ref), out["tx_frac"][0, k], -k))
            anchor = ((int(out["tx_ms"][0, best]) + travel_ms) % WEEK_MS, float(out["tx_frac"][0, best]))
    else:
        a, anchor = 0, (int(rx[0]), float(rx[1]))
    if anchor is not None:
        Fs = int(sampling_freq_hz)
        for e, b in enumerate(b_e):
            num = (int(b) - a) * int(block_samples) * 1000
            ms_add, rem = divmod(num, Fs)
            frac = anchor[1] + float(rem) / (float(sampling_freq_hz) * 1000.0)
            if frac >= 1e-3:
                frac, ms_add = frac - 1e-3, ms_add + 1
            out["rx_ms"][e], out["rx_frac"][e] = (anchor[0] + ms_add) % WEEK_MS, frac
    return out
