"""An independent restatement of the carrier smoothing's rule (include/gat.h, "carrier smoothing") for the tests: plain Python
loops, exact Python integers for q, C, SS and S (no modular arithmetic: the library's sums modulo 2^64 must give the same S),
Python floats (IEEE doubles) for every expression as the header writes it."""
from __future__ import annotations

import math

import numpy as np

U = 2.0 ** -48
WEEK, HALF = 604800000, 302400000
MEASURED, GAP, CMC, RATE = 1, 2, 4, 8
CHANNEL_DTYPE = np.dtype([(n, "<i4") for n in ("measured", "arcs", "cmc_resets", "rate_resets")])


def _wrap_once(d: int) -> int:
    if d >= HALF:
        return d - WEEK
    if d < -HALF:
        return d + WEEK
    return d


def _int64(d: int) -> int:
    return (d + 2 ** 63) % 2 ** 64 - 2 ** 63


def smooth_ref(tx_ms, tx_frac, rx_ms, rx_frac, cycles, cfrac, doppler=None, valid=None, *, window, carrier_hz, if_hz, epoch_seconds,
               cmc_gate_s, rate_gate_cycles=None) -> dict:
    """every output of the call as a dict of numpy arrays; ``rate_gate_cycles`` None: no rate test"""
    E, K = np.shape(tx_ms)
    rate = rate_gate_cycles is not None
    out = {"tx_frac_out": np.array(tx_frac, dtype=np.float64), "count": np.zeros((E, K), np.int32), "cmc_s": np.zeros((E, K), np.float64),
           "status": np.zeros((E, K), np.uint8), "channels": np.zeros(K, CHANNEL_DTYPE)}
    W, fL, Te, g = int(window), float(carrier_hz), float(epoch_seconds), float(cmc_gate_s)
    if_cycles = float(if_hz) * Te
    rxm, rxf = [int(v) for v in rx_ms], [float(v) for v in rx_frac]
    for k in range(K):
        txm, txf = [int(v) for v in tx_ms[:, k]], [float(v) for v in tx_frac[:, k]]
        cyc, cf = [int(v) for v in cycles[:, k]], [float(v) for v in cfrac[:, k]]
        dop = [float(v) for v in doppler[:, k]] if rate else None
        ok = [txm[e] >= 0 and rxm[e] >= 0 and math.isfinite(txf[e]) and math.isfinite(rxf[e]) and math.isfinite(cf[e])
              and (not rate or math.isfinite(dop[e])) and (valid is None or valid[e, k] != 0) for e in range(E)]
        C, SS, arc = [0] * E, [0] * E, [-1] * E
        c = ss = 0
        a = -1
        counts = [0, 0, 0, 0]
        for e in range(E):
            st, q = 0, 0
            if ok[e]:
                st = MEASURED
                if e == 0 or not ok[e - 1]:
                    st |= GAP
                else:
                    dms = _wrap_once(rxm[e] - rxm[e - 1]) - _wrap_once(txm[e] - txm[e - 1])
                    dphi = float(_int64(cyc[e] - cyc[e - 1])) + (cf[e] - cf[e - 1])
                    dphin = dphi - if_cycles
                    delta = float(dms) * 1e-3 + ((rxf[e] - rxf[e - 1]) - (txf[e] - txf[e - 1])) + dphin / fL
                    if abs(dms) > 1000 or not (abs(delta) <= g):
                        st |= CMC
                    if rate and not (abs(dphin - 0.5 * (dop[e] + dop[e - 1]) * Te) <= float(rate_gate_cycles)):
                        st |= RATE
                    if st == MEASURED:
                        q = int(np.rint(delta / U))
                counts[0] += 1
                counts[1] += 1 if st & (GAP | CMC | RATE) else 0
                counts[2] += 1 if st & CMC else 0
                counts[3] += 1 if st & RATE else 0
                if st & (GAP | CMC | RATE):
                    a = e
            c += q
            ss += c
            C[e], SS[e], arc[e] = c, ss, a if ok[e] else -1
            out["status"][e, k] = st
        out["channels"][k] = tuple(counts)
        for e in range(E):
            if arc[e] < 0:
                continue
            n = min(e - arc[e] + 1, W)
            S = SS[e] - (SS[e - n] if e - n >= 0 else 0) - n * C[e]
            m = (float(S) * U) / float(n)
            out["tx_frac_out"][e, k] = txf[e] - m
            out["count"][e, k] = n
            out["cmc_s"][e, k] = float(C[e] - C[arc[e]]) * U
    return out
