"""An independent FP64 restatement of the tracking monitor's rule (include/gat.h, "tracking monitor"): plain Python loops over
numpy float64 scalars in the stated order, no call into the library.  Slow on purpose; the tests keep its inputs small and share
its results."""
from __future__ import annotations

import math

import numpy as np

NH10 = np.array([1 - 2 * int(c) for c in "0000110101"], dtype=np.int8)
NH20 = np.array([1 - 2 * int(c) for c in "00000100110101001110"], dtype=np.int8)


def prompts(acc_re, acc_im, prompt_index, weights=None):
    """P[k][b] complex128 from float32 [B, K, L, M]: the plain sum over m, or sum_m conj(w[k][m]) acc in m order."""
    B, K, _, M = acc_re.shape
    pr, pi = np.zeros((K, B)), np.zeros((K, B))
    for b in range(B):
        for k in range(K):
            re = im = np.float64(0.0)
            for m in range(M):
                ar, ai = np.float64(acc_re[b, k, prompt_index, m]), np.float64(acc_im[b, k, prompt_index, m])
                if weights is None:
                    re, im = re + ar, im + ai
                else:
                    wr, wi = np.float64(weights[k, m].real), np.float64(weights[k, m].imag)
                    re = re + (wr * ar + wi * ai)
                    im = im + (wr * ai - wi * ar)
            pr[k, b], pi[k, b] = re, im
    return pr, pi


def windows(pr, pi, W):
    """[K][NW] dicts of the window sums, blocks in order; the last window takes what is left."""
    K, B = pr.shape
    out = []
    for k in range(K):
        row = []
        for b0 in range(0, B, W):
            s = dict(sum_p2=np.float64(0), sum_p4=np.float64(0), sum_d=np.float64(0), sum_i=np.float64(0), sum_q=np.float64(0), blocks=0)
            for b in range(b0, min(b0 + W, B)):
                I, Q = pr[k, b], pi[k, b]
                p = I * I + Q * Q
                s["sum_p2"] += p
                s["sum_p4"] += p * p
                s["sum_d"] += I * I - Q * Q
                s["sum_i"] += I
                s["sum_q"] += Q
                s["blocks"] += 1
            row.append(s)
        out.append(row)
    return out


def symbol(pr, pi, k, b0, overlay):
    sr = si = wbp = np.float64(0.0)
    for i, o in enumerate(overlay):
        I, Q = pr[k, b0 + i], pi[k, b0 + i]
        sr = sr + np.float64(o) * I
        si = si + np.float64(o) * Q
        wbp = wbp + (I * I + Q * Q)
    return sr, si, wbp


def energies(pr, pi, overlay):
    """E[k][c] and J."""
    K, B = pr.shape
    Pd = len(overlay)
    J = max(0, (B - Pd + 1) // Pd) if B - Pd + 1 > 0 else 0
    E = np.zeros((K, Pd))
    for k in range(K):
        for c in range(Pd):
            e = np.float64(0.0)
            for j in range(J):
                sr, si, _ = symbol(pr, pi, k, c + j * Pd, overlay)
                e = e + (sr * sr + si * si)
            E[k, c] = e
    return E, J


def channel(E_k, J, B, Pd, first_block, forced=None):
    """(stream offset, c*, J_k, e_max, e_second) of one channel."""
    if forced is not None and forced >= 0:
        c = (forced - first_block) % Pd
    elif J > 0:
        c = 0
        for i in range(1, Pd):
            if E_k[i] > E_k[c]:
                c = i
    else:
        return -1, -1, 0, 0.0, 0.0
    others = [E_k[i] for i in range(Pd) if i != c]
    e_max, e_second = (E_k[c], max(others) if others else 0.0) if J > 0 else (0.0, 0.0)
    return (first_block + c) % Pd, c, max(0, (B - c) // Pd), float(e_max), float(e_second)


def symbols(pr, pi, k, c, Jk, overlay, cap):
    sr, si, wbp = np.zeros(cap), np.zeros(cap), np.zeros(cap)
    for j in range(Jk):
        sr[j], si[j], wbp[j] = symbol(pr, pi, k, c + j * len(overlay), overlay)
    return sr, si, wbp


def monitor(acc_re, acc_im, prompt_index, W, overlay, first_block=0, forced=None, weights=None, series=None):
    """The whole call as a dict; ``series``: (pr, pi) computed before (shared between calls on the same accumulators)."""
    pr, pi = series if series is not None else prompts(acc_re, acc_im, prompt_index, weights)
    K, B = pr.shape
    Pd = len(overlay)
    E, J = energies(pr, pi, overlay)
    cap = B // Pd
    out = dict(pr=pr, pi=pi, windows=windows(pr, pi, W), energy=E, J=J, channels=[], sym_re=np.zeros((K, cap)), sym_im=np.zeros((K, cap)),
               sym_wbp=np.zeros((K, cap)))
    for k in range(K):
        ch = channel(E[k], J, B, Pd, first_block, forced)
        out["channels"].append(ch)
        if ch[1] >= 0:
            out["sym_re"][k], out["sym_im"][k], out["sym_wbp"][k] = symbols(pr, pi, k, ch[1], ch[2], overlay, cap)
    return out


# ---- what the caller makes of the sums ------------------------------------------------------------------------------------------
def phase_lock(w):
    return w["sum_d"] / w["sum_p2"]


def cn0_m2m4(w, T):
    m2, m4 = w["sum_p2"] / w["blocks"], w["sum_p4"] / w["blocks"]
    rad = 2.0 * m2 * m2 - m4
    if not rad > 0.0:
        return math.nan
    pd = math.sqrt(rad)
    ratio = pd / ((m2 - pd) * T)
    return 10.0 * math.log10(ratio) if ratio > 0.0 else math.nan


def cn0_nwpr(sr, si, wbp, n, Pd, T):
    if Pd == 1 or n < 1:
        return math.nan
    mu = sum((sr[j] * sr[j] + si[j] * si[j]) / wbp[j] for j in range(n)) / n
    if not 1.0 < mu < Pd:
        return math.nan
    return 10.0 * math.log10((mu - 1.0) / ((Pd - mu) * T))


def prompts_as_acc(p):
    """complex [K, B] prompts as float32 accumulators [B, K, 1, 1] (one tap, one antenna): the values are rounded to float32."""
    re = np.ascontiguousarray(p.real.T[:, :, None, None].astype(np.float32))
    im = np.ascontiguousarray(p.imag.T[:, :, None, None].astype(np.float32))
    return re, im
