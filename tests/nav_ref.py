"""Independent numpy restatement of the navigation data layer (include/gat.h, "navigation data"), written from the equations of
the signal specifications and not from the package's code or its parity masks: the LNAV parity by the six equations of IS-GPS-200
over the source bits, CRC-24Q by long division, the convolutional code by its delays, the quantiser, a Viterbi decoder batched
over rows of one length, the frame search, the choice and the frame records.  Everything is compared as integers.  Beside the
Viterbi decoder stand two oracles that hold no trellis: every path of a short stream by the code's definition (exhaustive_ml),
and the metric of a returned path at any length (path_certificate)."""
import numpy as np

LNAV, CNAV = 0, 1
FRAME, TAIL = 300, 32
PREAMBLE = np.array([1, 0, 0, 0, 1, 0, 1, 1], np.uint8)
TOW_MOD = 100800

# D25 .. D30: (which starred bit, the source bits d_i of the sum), IS-GPS-200 table 20-XIV
PARITY_EQ = [(29, (1, 2, 3, 5, 6, 10, 11, 12, 13, 14, 17, 18, 20, 23)),
             (30, (2, 3, 4, 6, 7, 11, 12, 13, 14, 15, 18, 19, 21, 24)),
             (29, (1, 3, 4, 5, 7, 8, 12, 13, 14, 15, 16, 19, 20, 22)),
             (30, (2, 4, 5, 6, 8, 9, 13, 14, 15, 16, 17, 20, 21, 23)),
             (30, (1, 3, 5, 6, 7, 9, 10, 14, 15, 16, 17, 18, 21, 22, 24)),
             (29, (3, 5, 6, 8, 9, 10, 11, 13, 15, 19, 22, 23, 24))]
G = np.array([int(c) for c in bin(0x1864CFB)[2:]], np.uint8)  # 25 coefficients, x^24 first


# ---- LNAV ------------------------------------------------------------------------------------------------------------------------
def lnav_parity(d, d29s, d30s):
    """D25 .. D30 of the SOURCE bits d[0 .. 24) after a word that ended in D29* and D30*"""
    return [((d29s if star == 29 else d30s) + sum(int(d[i - 1]) for i in idx)) & 1 for star, idx in PARITY_EQ]


def lnav_check(rx, d29s, d30s):
    """(parity good, source bits) of thirty received bits"""
    d = [int(b) ^ d30s for b in rx[:24]]
    return lnav_parity(d, d29s, d30s) == [int(b) for b in rx[24:30]], d


def lnav_encode_word(d, d29s, d30s, solve=False):
    d = [int(v) for v in d]
    if solve:  # d24 from D29 = 0, then d23 from D30 = 0
        d[23] = 0
        d[23] = lnav_parity(d, d29s, d30s)[4]
        d[22] = 0
        d[22] = lnav_parity(d, d29s, d30s)[5]
    return [b ^ d30s for b in d] + lnav_parity(d, d29s, d30s)


def bits_of(v, n):
    return [(int(v) >> (n - 1 - i)) & 1 for i in range(n)]


def value(bits):
    v = 0
    for b in bits:
        v = (v << 1) | int(b)
    return v


def lnav_subframe(tow, sid, payload, tlm=0, flags=0):
    p = list(payload) + [0] * (190 - len(payload))
    words = [list(PREAMBLE) + bits_of(tlm, 16), bits_of(tow, 17) + bits_of(flags, 2) + bits_of(sid, 3) + [0, 0]]
    words += [p[24 * w:24 * w + 24] for w in range(7)] + [p[168:190] + [0, 0]]
    out, a, b = [], 0, 0
    for w, d in enumerate(words):
        sent = lnav_encode_word(d, a, b, solve=w in (1, 9))
        out += sent
        a, b = sent[28], sent[29]
    return np.array(out, np.uint8)


def lnav_frame(b):
    """status, tow, id, prn, words of 300 polarity-corrected bits"""
    status = int(np.array_equal(b[:8], PREAMBLE))
    words, a, c = [], 0, 0
    for w in range(10):
        rx = b[30 * w:30 * w + 30]
        ok, d = lnav_check(rx, a, c)
        status |= int(ok) << (w + 1)
        words.append((value(d) << 6) | value(rx[24:30]))
        a, c = int(rx[28]), int(rx[29])
    d2 = bits_of(words[1] >> 6, 24)
    return status, value(d2[:17]), value(d2[19:22]), 0, words


def lnav_hit(b):
    if not np.array_equal(b[:8], PREAMBLE):
        return False
    ok1, _ = lnav_check(b[0:30], 0, 0)
    ok2, d2 = lnav_check(b[30:60], int(b[28]), int(b[29]))
    return ok1 and ok2 and int(b[58]) == 0 and int(b[59]) == 0 and 1 <= value(d2[19:22]) <= 5


# ---- CNAV ------------------------------------------------------------------------------------------------------------------------
def poly_mod(bits):
    """the remainder of the bit polynomial (first bit the highest power) by the CRC-24Q generator, 24 bits"""
    r = np.array(bits, np.uint8).copy()
    for i in range(len(r) - 24):
        if r[i]:
            r[i:i + 25] ^= G
    return r[-24:] if len(r) >= 24 else np.concatenate([np.zeros(24 - len(r), np.uint8), r])


def crc24q(bits):
    return value(poly_mod(list(bits) + [0] * 24))


def cnav_message(prn, mtype, tow, payload):
    body = list(PREAMBLE) + bits_of(prn, 6) + bits_of(mtype, 6) + bits_of(tow, 17) + list(payload) + [0] * (239 - len(payload))
    return np.array(body + bits_of(crc24q(body), 24), np.uint8)


def cnav_hit(b):
    return np.array_equal(b[:8], PREAMBLE) and not poly_mod(b[:FRAME]).any()


def cnav_frame(b):
    status = int(np.array_equal(b[:8], PREAMBLE)) | (int(not poly_mod(b[:FRAME]).any()) << 1)
    return status, value(b[20:37]), value(b[14:20]), value(b[8:14]), [value(b[30 * w:30 * w + 30]) for w in range(10)]


def fec_encode(bits, state=0):
    """the code of bits [..., T] (two symbols a bit, G1's first) from a register that holds `state` (an int, or ints that
    broadcast over the leading axes): the six inputs before the first bit, the newest in bit 5; 0: a transmitter that starts"""
    bits = np.asarray(bits, np.uint8)
    before = ((np.asarray(state)[..., None] >> np.arange(6)) & 1).astype(np.uint8)
    lead = np.broadcast_shapes(before.shape[:-1], bits.shape[:-1])
    u = np.concatenate([np.broadcast_to(before, lead + (6,)), np.broadcast_to(bits, lead + bits.shape[-1:])], axis=-1)
    t = np.arange(6, u.shape[-1])
    c1 = u[..., t] ^ u[..., t - 1] ^ u[..., t - 2] ^ u[..., t - 3] ^ u[..., t - 6]
    c2 = u[..., t] ^ u[..., t - 2] ^ u[..., t - 3] ^ u[..., t - 5] ^ u[..., t - 6]
    return np.stack([c1, c2], axis=-1).reshape(lead + (-1,))


def correlate(q, bits, state=0):
    """the metric of a path: the code of bits [..., T] from `state` as +-1 symbols (a 0 is positive) against q[0 .. 2 T)"""
    q = np.asarray(q, np.int64)
    return ((1 - 2 * fec_encode(bits, state).astype(np.int64)) * q[:2 * np.shape(bits)[-1]]).sum(axis=-1)


# Two oracles of the Viterbi decoder that share nothing with a trellis: no add-compare-select, no survivors, no traceback.
def exhaustive_ml(q):
    """Every path of T <= 10 steps by the code's definition: the metric of each of the 2^T input sequences from its best initial
    state, int64 [2^T], indexed by the sequence read as a number, its first bit the highest."""
    T = len(q) // 2
    assert T <= 10
    seqs = ((np.arange(1 << T)[:, None] >> np.arange(T - 1, -1, -1)) & 1).astype(np.uint8)
    return correlate(q, seqs, np.arange(64)[:, None]).max(axis=0)


def check_exhaustive_ml(q, bits, metric):
    """path_metric is the largest metric of any path, and the returned bits are one of the paths that attain it.  Returns how
    many input sequences do."""
    per_seq = exhaustive_ml(q)
    assert int(metric) == int(per_seq.max()), (metric, per_seq.max())
    assert per_seq[value(bits)] == per_seq.max(), ("the returned bits are not a best path", list(bits), metric)
    return int((per_seq == per_seq.max()).sum())


def path_certificate(q, bits):
    """The metric of the returned path at any length: the bits encoded again from each of the 64 initial states -- only the first
    six steps depend on the state -- against q, the largest of them.  Equal to path_metric when the traceback returned the path
    whose metric the forward pass reported.  It proves that metric and path belong together, not that the path is the best."""
    bits = np.asarray(bits, np.uint8)
    head = bits[:6]
    tail = int(correlate(q, bits)) - int(correlate(q, head))  # from step 6 on the register holds the path's own bits
    return tail + int(correlate(q, head, np.arange(64)).max())


def quantise(x, n):
    """q[0 .. n) of one row's first n symbols"""
    x = np.asarray(x[:n], np.float64)
    x = np.where(np.isfinite(x), x, 0.0)
    rows = -(-n // 64)
    a = np.zeros(rows * 64)
    a[:n] = np.abs(x)
    part = np.zeros(64)
    with np.errstate(all="ignore"):  # a sum may overflow to +inf, a scale may be subnormal: both are inputs of the rule
        for r in a.reshape(rows, 64):
            part = part + r
        S = 0.0
        for v in part:
            S = S + v
        unit = np.float64(S) / np.float64(n)
        if not np.isfinite(unit) or not unit > 0.0:
            return np.zeros(n, np.int8)
        v = (x * 16.0) / unit
        return np.where(v >= 127.0, 127, np.where(v <= -127.0, -127, np.rint(v))).astype(np.int8)


def _trellis_tables():
    s = np.arange(64)
    u = s >> 5
    tab = []
    for b in (0, 1):
        prev = ((s & 31) << 1) | b
        d = [(prev >> (6 - i)) & 1 for i in range(1, 7)]  # d[i-1]: the input i steps ago
        c1 = u ^ d[0] ^ d[1] ^ d[2] ^ d[5]
        c2 = u ^ d[1] ^ d[2] ^ d[4] ^ d[5]
        tab.append((prev, 1 - 2 * c1, 1 - 2 * c2))
    return tab


def viterbi(q):
    """q: int [R, 2 T], rows decoded side by side.  Returns (bits uint8 [R, T], largest final metric int32 [R])."""
    q = np.asarray(q, np.int32)
    R, T = q.shape[0], q.shape[1] // 2
    (p0, a0, b0), (p1, a1, b1) = _trellis_tables()
    m = np.zeros((R, 64), np.int32)
    surv = np.zeros((T, R, 64), bool)
    for t in range(T):
        x, y = q[:, 2 * t, None], q[:, 2 * t + 1, None]
        m0, m1 = m[:, p0] + a0 * x + b0 * y, m[:, p1] + a1 * x + b1 * y
        surv[t] = m1 > m0
        m = np.where(surv[t], m1, m0).astype(np.int32)
    state = np.argmax(m, axis=1)  # the first of the largest
    metric = m[np.arange(R), state]
    bits = np.zeros((R, T), np.uint8)
    rows = np.arange(R)
    for t in range(T - 1, -1, -1):
        bits[:, t] = state >> 5
        state = ((state & 31) << 1) | surv[t, rows, state]
    return bits, metric.astype(np.int32)


# ---- the whole call -----------------------------------------------------------------------------------------------------------------
def decode_bits(fmt, sym, counts):
    """decoded uint8 [K, P, bit_cap] and path_metric int32 [K, P] of symbols [K, cap] with counts n_k"""
    K, cap = sym.shape
    P = 2 if fmt == CNAV else 1
    dec, pm = np.zeros((K, P, cap // P), np.uint8), np.zeros((K, P), np.int32)
    if fmt == LNAV:
        for k in range(K):
            x = sym[k, :counts[k]]
            dec[k, 0, :counts[k]] = np.where(np.isfinite(x), x, 0.0) < 0
        return dec, pm
    groups = {}
    for k in range(K):
        qk = quantise(sym[k], counts[k])
        for ph in (0, 1):
            T = max(counts[k] - ph, 0) // 2
            groups.setdefault(T, []).append((k, ph, qk[ph:ph + 2 * T]))
    for T, members in groups.items():
        bits, metric = viterbi(np.stack([m[2] for m in members]).reshape(len(members), 2 * T))
        for (k, ph, _), b, mt in zip(members, bits, metric):
            dec[k, ph, :T], pm[k, ph] = b, mt
    return dec, pm


def search(fmt, dec_k, counts_k, max_frames, min_frames):
    """(channel record as a dict, frames as a list of (status, tow, id, prn, words)) of one channel's decoded bits [P, bit_cap]"""
    P = dec_k.shape[0]
    hit_fn, frame_fn = (cnav_hit, cnav_frame) if fmt == CNAV else (lnav_hit, lnav_frame)
    scores = np.zeros((P, FRAME, 2), np.int64)
    nbits, nsearch = [], []
    for ph in range(P):
        nb = max(counts_k - ph, 0) // 2 if fmt == CNAV else counts_k
        ns = max(nb - TAIL, 0) if fmt == CNAV else nb
        nbits.append(nb), nsearch.append(ns)
        for p in (0, 1):
            b = dec_k[ph, :ns] ^ p
            if ns < FRAME:
                continue
            win = np.lib.stride_tricks.sliding_window_view(b, 8)[:ns - FRAME + 1]
            for pos in np.nonzero((win == PREAMBLE).all(axis=1))[0]:
                if hit_fn(b[pos:pos + FRAME]):
                    # a hit at pos counts for the candidate o = pos mod 300 (frames start at o + 300 f and lie wholly inside)
                    scores[ph, pos % FRAME, p] += 1
    flat = scores.reshape(-1)
    c = int(np.argmax(flat))  # the first of the largest: lowest phase, then offset, then polarity
    best, second = int(flat[c]), int(np.delete(flat, c).max())
    ph, o, p = c // (2 * FRAME), c // 2 % FRAME, c % 2
    sync = best >= min_frames
    if not sync:
        ph, p = 0, 0
    F = min((nsearch[ph] - o) // FRAME if sync and nsearch[ph] - o >= FRAME else 0, max_frames)
    b = dec_k[ph] ^ p
    frames = [frame_fn(b[o + FRAME * f:o + FRAME * (f + 1)]) for f in range(F)]
    good = 0x3 if fmt == CNAV else 0x7ff
    steps = sum(1 for x, y in zip(frames, frames[1:]) if x[0] == good and y[0] == good and y[1] == (x[1] + 1) % TOW_MOD)
    rec = dict(frame_offset=o if sync else -1, symbol_phase=ph, inverted=p, score=best, second_score=second, num_frames=F, num_bits=nbits[ph],
               tow_steps=steps)
    return rec, frames
