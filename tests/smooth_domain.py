"""The carrier smoothing's whole domain (include/gat.h, "carrier smoothing"), for the tests of the host twin and of the device: pure
numpy on top of tests/smooth_cases.py, every condition asserted here, on the CPU, against the restatement (tests/smooth_ref.py) alone.

``lanes_case(K)``   K in LANES_K: every split of a chunk's workgroup into rows x lanes (lanes 2 .. 64, a K one past a power of two
                    among them), E = two chunks and three epochs, arc starts on the first and the last epoch of every chunk and of
                    three rows' runs, on channel 0 (slips) and on channel K - 1 (gaps and slips).
``deep_case(n)``    n in DEEP_CHUNKS chunks of K = 5, the last chunk of one epoch: a lane of the channel kernel holds 1, 2 and 3
                    chunks, lanes past the last chunk idle; a channel measured throughout (a look-back over every chunk), one
                    measured in one middle chunk alone, one in the last epoch alone, one dead, one with slips and gaps at 1 %.
``hostile_tiles()`` K = 8, E = two chunks and three: every hostile entry on a channel of its own (HOSTILE_CHANNELS) at epochs 255,
                    256 and 299 (a pair of values: also 300) among clean channels, labelled with the status bits the rule gives
                    the epochs it names; an entry of rx_ms or rx_frac is the whole epoch's and has a tile of its own.
``gate_case()``     dyadic values as smooth_cases.wrap_case: a delta exactly on cmc_gate_s is accepted, the next double above it
                    begins an arc; the same pair on the rate gate.
"""
import functools

import numpy as np

from tests import smooth_cases as sc
from tests import smooth_ref

CHUNK = 256
E_EDGES = 2 * CHUNK + 3
LANES_K = (2, 3, 4, 8, 9, 16, 17, 32, 33, 63)
DEEP_CHUNKS = (64, 66, 129)
DEEP_WINDOWS = (7, 257, 65536)
M, GAP, CMC, RATE = smooth_ref.MEASURED, smooth_ref.GAP, smooth_ref.CMC, smooth_ref.RATE
INT32_MIN, INT32_MAX = -(2 ** 31), 2 ** 31 - 1
INT64_MIN, INT64_MAX = -(2 ** 63), 2 ** 63 - 1
MAX_DOUBLE = float(np.finfo(np.float64).max)
HALF_WEEK_MS = 302400000


_REFS = {}  # (id of the case, configuration): (the case, kept alive; its outputs)


def reference(case: sc.Case, **over) -> dict:
    """the restatement's outputs of a case, computed once per (case, configuration) and never changed"""
    key = (id(case),) + tuple(sorted(over.items()))
    if key not in _REFS:
        cfg = case.config(**over)
        _REFS[key] = (case, smooth_ref.smooth_ref(case.tx_ms, case.tx_frac, case.rx_ms, case.rx_frac, case.carrier_cycles, case.carrier_frac,
                                                  case.doppler_hz if cfg["rate_gate_cycles"] is not None else None, case.valid, **cfg))
    return _REFS[key][1]


def lanes_of(K: int) -> int:
    """gat.h (gat_smooth_plan): lanes is the power of two that holds K; rows x lanes = 256 threads, a row walks lanes epochs"""
    lanes = 1
    while lanes < K:
        lanes *= 2
    return lanes


def expected_plan(E: int, K: int) -> dict:
    lanes = lanes_of(K)
    return {"lanes": lanes, "rows": CHUNK // lanes, "run_epochs": lanes, "num_chunks": -(-E // CHUNK), "chunk_epochs": CHUNK}


# ---- every lanes split --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lanes_case(K: int, window: int = 7) -> sc.Case:
    E, run = E_EDGES, lanes_of(K)
    rows = CHUNK // run
    chunk_edges = [255, 256, 511, 512]
    run_edges = sorted({c * CHUNK + r * run + i for c in (0, 1) for r in {1, rows // 2, rows - 1} for i in (0, run - 1)} - set(chunk_edges))
    last_edges = [e for e in run_edges if e not in (255, 510)]  # channel K - 1 is not measured at 255 and 510: its gaps
    slips = [(e, 0, 400) for e in chunk_edges + run_edges] + [(e, K - 1, -300) for e in last_edges + [512]]
    case = sc.synthetic(7000 + K, E, K, window=window, slips=slips, mask_p=0.01, week_wrap=True, rate_gate_cycles=0.5,
                        dead_channel=3 if K >= 5 else None)
    if K >= 5:
        gaps = np.random.default_rng(E + K).random((E, K)) < 0.01
        gaps[:, [0, 2, K - 1]] = False
        case.tx_ms[gaps] = -1
        case.valid[:, 2] = 1  # measured throughout: its look-back is the window's
    # the arc starts stand on measured epochs behind measured ones; channel K - 1: a gap before 256 and before 511
    for k in (0, K - 1):
        for e in chunk_edges + run_edges:
            case.valid[e - 1:e + 1, k] = 1
    case.valid[[255, 510], K - 1] = 0
    case.valid[[256, 511, 512], K - 1] = 1
    st = reference(case)["status"]
    assert all(st[e, 0] & CMC for e in chunk_edges + run_edges), "channel 0's slips"
    assert (st[256, K - 1] & GAP) and (st[511, K - 1] & GAP) and (st[512, K - 1] & CMC) and all(st[e, K - 1] & CMC for e in last_edges)
    case.run_edges, case.chunk_edges = run_edges, chunk_edges
    return case


# ---- several chunks a lane of the channel kernel ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def deep_case(chunks: int) -> sc.Case:
    E, K = CHUNK * chunks - (CHUNK - 1), 5
    rng = np.random.default_rng(chunks)
    # channel 4: a slip and a gap in every chunk, and as many again scattered: about 1.4 % of its epochs begin an arc
    full = np.arange(chunks - 1) * CHUNK
    scattered = np.union1d(np.flatnonzero(rng.random(E) < 0.003), full + 100)
    scattered = scattered[scattered > 0]
    case = sc.synthetic(9000 + chunks, E, K, window=DEEP_WINDOWS[0], slips=[(int(e), 4, 400) for e in scattered], rate_gate_cycles=0.5)
    middle = chunks // 2
    case.tx_ms[:middle * CHUNK, 1] = -1
    case.tx_ms[(middle + 1) * CHUNK:, 1] = -1
    case.tx_ms[:E - 1, 2] = -1
    case.tx_ms[:, 3] = -1
    gaps = rng.random(E) < 0.003
    for keep in (99, 100, 199, 201):  # the chunk's own slip and gap stand between measured epochs
        gaps[full + keep] = False
    gaps[full + 200] = True
    case.tx_ms[gaps, 4] = -1
    per = -(-chunks // 64)
    ref = reference(case, window=65536)
    st, ch = ref["status"], ref["channels"]
    assert (st[0, 0] & GAP) and (st[1:, 0] == M).all() and ref["count"][:, 0].max() == min(E, 65536) and ref["count"][E - 1, 0] == min(E, 65536)
    assert tuple(ch[1]) == (CHUNK, 1, 0, 0) and tuple(ch[2]) == (1, 1, 0, 0) and tuple(ch[3]) == (0, 0, 0, 0) and st[E - 1, 2] == M | GAP
    # every full chunk, so every lane's group of chunks, holds resets of both kinds and every count of channel 4
    for c in range(chunks - 1):
        s = slice(c * CHUNK, (c + 1) * CHUNK)
        assert (st[s, 4] & GAP).any() and (st[s, 4] & CMC).any() and (st[s, 4] & RATE).any() and (st[s, 4] == M).any()
    assert ch[4]["cmc_resets"] > chunks // 2 and ch[4]["arcs"] > ch[4]["cmc_resets"]
    case.per, case.chunks = per, chunks
    return case


# ---- hostile entries ------------------------------------------------------------------------------------------------------------------
HOSTILE_K = 8
HOSTILE_CHANNELS = (1, 3, 5, 6)
CLEAN_CHANNELS = (0, 2, 4, 7)
AT = (255, 256, 299)  # the last epoch of a chunk, the first of the next, the fourth of a row's run of eight
X = M | CMC | RATE


class Entry:
    """label; apply(case, k): puts the entry on channel k (k = None: on the epochs, for every channel); want: {epoch: the status
    the label names}, for channel k or for every channel"""

    def __init__(self, label, apply, want, epoch_wide=False):
        self.label, self.apply, self.want, self.epoch_wide = label, apply, want, epoch_wide


def _pair(field, a, b):
    """a at 255 and 299, b at 256 and 300"""
    def apply(c, k):
        arr = getattr(c, field)
        for e, v in ((255, a), (256, b), (299, a), (300, b)):
            if arr.ndim == 2:
                arr[e, k] = v
            else:
                arr[e] = v
    return apply


def _single(field, v):
    def apply(c, k):
        arr = getattr(c, field)
        for e in AT:
            if arr.ndim == 2:
                arr[e, k] = v
            else:
                arr[e] = v
    return apply


def _dms(target):
    """the whole milliseconds of the transmit time step so that dms is exactly `target` at each epoch of AT, the fraction taking the
    step back: the growth of the pseudorange is the clean channel's"""
    def apply(c, k):
        for e in AT:
            cur = smooth_ref._wrap_once(int(c.rx_ms[e]) - int(c.rx_ms[e - 1])) - smooth_ref._wrap_once(int(c.tx_ms[e, k]) - int(c.tx_ms[e - 1, k]))
            shift = target - cur
            c.tx_ms[e:, k] = c.tx_ms[e:, k] - shift
            c.tx_frac[e:, k] = c.tx_frac[e:, k] + shift * 1e-3
            assert (c.tx_ms[:, k] >= 0).all()
    return apply


def _difference(d):
    """tx_ms[e] - tx_ms[e - 1] = d: at 255, 256 and 299 one after another where the times stay within int32 and not negative, else at
    255 and 299 (256 then sees the way back)"""
    def apply(c, k):
        for e in AT if d > 0 else (255, 299):
            c.tx_ms[e, k] = int(c.tx_ms[e - 1, k]) + d
        assert (c.tx_ms[:, k] >= 0).all()
    return apply


def _all(status, also=()):
    return {e: status for e in AT + tuple(also)}


def entries():
    out = []
    # the int64 extremes of the cycle count: the difference is taken modulo 2^64 (-1 and +1 between the two: not named, a small step)
    out.append(Entry("cycles=INT64_MIN,INT64_MAX", _pair("carrier_cycles", INT64_MIN, INT64_MAX), {255: X, 257: X, 299: X, 301: X}))
    out.append(Entry("cycles=INT64_MAX,INT64_MIN", _pair("carrier_cycles", INT64_MAX, INT64_MIN), {255: X, 257: X, 299: X, 301: X}))
    for v, name in ((1e300, "1e300"), (MAX_DOUBLE, "max")):
        # finite, so measured; the difference of the pair at max is not: !(fabs(delta) <= g) and the rate test catch it
        out.append(Entry(f"carrier_frac=+-{name}", _pair("carrier_frac", v, -v), _all(X, (257, 300, 301))))
        out.append(Entry(f"tx_frac=+-{name}", _pair("tx_frac", v, -v), _all(M | CMC, (257, 300, 301))))  # the rate test reads no time
        out.append(Entry(f"rx_frac=+-{name}", _pair("rx_frac", v, -v), _all(M | CMC, (257, 300, 301)), epoch_wide=True))
    for v, name in ((np.nan, "nan"), (np.inf, "+inf"), (-np.inf, "-inf")):
        gone = {255: 0, 256: 0, 257: M | GAP, 299: 0, 300: M | GAP}
        out.append(Entry(f"carrier_frac={name}", _single("carrier_frac", v), gone))
        out.append(Entry(f"tx_frac={name}", _single("tx_frac", v), gone))
        out.append(Entry(f"rx_frac={name}", _single("rx_frac", v), gone, epoch_wide=True))
    # each finite, the sum of the two is not: 0.5 * (inf) * Te
    out.append(Entry("doppler_hz=1e308,1e308", _pair("doppler_hz", 1e308, 1e308), _all(M | RATE, (257, 300, 301))))
    for v in (0, 604799999, INT32_MAX):
        out.append(Entry(f"tx_ms={v}", _single("tx_ms", v), _all(M | CMC, (257, 300))))  # 256 after 255: dms = 20 and a delta of 0.02 s
    out.append(Entry("tx_ms=INT32_MIN", _single("tx_ms", INT32_MIN), {255: 0, 256: 0, 257: M | GAP, 299: 0, 300: M | GAP}))
    out.append(Entry("rx_ms=-1", _single("rx_ms", -1), {255: 0, 256: 0, 257: M | GAP, 299: 0, 300: M | GAP}, epoch_wide=True))
    for target in (1000, -1000):
        out.append(Entry(f"dms={target}", _dms(target), _all(M, (257, 300))))  # |dms| > 1000 is false and the fraction takes the second back
    for target in (1001, -1001):
        out.append(Entry(f"dms={target}", _dms(target), {**_all(M | CMC), 257: M, 300: M}))
    for s in (1, -1):
        for d in (-1, 0, 1):
            diff = s * (HALF_WEEK_MS + d)
            out.append(Entry(f"tx_ms step {diff}", _difference(diff), {255: M | CMC, 256: M | CMC, 299: M | CMC, 300: M | CMC}))
    for b in (1, 2, 128, 255):
        out.append(Entry(f"valid={b}", _single("valid", b), _all(M, (257, 300))))
    return out


@functools.lru_cache(maxsize=None)
def hostile_base() -> sc.Case:
    """clean channels: no gap, a mask of ones, slips at the chunk's edge on channel 0; the times moved by 1e5 s so that a step of half
    a week down stays a time"""
    c = sc.synthetic(4242, E_EDGES, HOSTILE_K, window=100, slips=[(255, 0, 400), (256, 0, 400)], rate_gate_cycles=0.5)
    c.tx_ms, c.rx_ms = c.tx_ms + 100000000, c.rx_ms + 100000000
    c.valid = np.ones((c.E, c.K), np.uint8)
    assert c.tx_ms.min() > HALF_WEEK_MS + 1 and int(c.tx_ms.max()) + 2 * (HALF_WEEK_MS + 1) <= INT32_MAX
    st = reference(c)["status"]
    assert (st[1:, 1:] == M).all() and (st[0] == M | GAP).all()  # the calm tile: one arc a channel
    return c


class HostileTile:
    """case; entries: (Entry, channel or None); clean: the channels that must keep the calm tile's bytes (none where the entry is the
    whole epoch's)"""

    def __init__(self, case, placed, clean):
        self.case, self.entries, self.clean = case, placed, clean


@functools.lru_cache(maxsize=None)
def hostile_tiles():
    base = hostile_base()
    ens = entries()
    per_channel = [en for en in ens if not en.epoch_wide]
    tiles = []
    for first in range(0, len(per_channel), len(HOSTILE_CHANNELS)):
        c = base.copy()
        placed = list(zip(per_channel[first:first + len(HOSTILE_CHANNELS)], HOSTILE_CHANNELS))
        for en, k in placed:
            en.apply(c, k)
        tiles.append(HostileTile(c, placed, CLEAN_CHANNELS))
    for en in ens:
        if en.epoch_wide:
            c = base.copy()
            en.apply(c, None)
            tiles.append(HostileTile(c, [(en, None)], ()))
    # the condition: the restatement alone gives every entry the bits its label names, and leaves the clean channels alone
    calm = reference(base)
    for t in tiles:
        ref = reference(t.case)
        for en, k in t.entries:
            for e, want in en.want.items():
                got = ref["status"][e, 1:] if k is None else ref["status"][e, k:k + 1]  # channel 0 has its slips at 255 and 256
                assert (got == want).all(), (en.label, e, k, got, want)
        for k in t.clean:
            for name in ("tx_frac_out", "count", "cmc_s", "status"):
                assert ref[name][:, k].tobytes() == calm[name][:, k].tobytes(), (name, k)
    assert len({en.label for t in tiles for en, _ in t.entries}) == len(ens) == 37
    return tuple(tiles)


# ---- the gates, exactly ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def gate_case() -> sc.Case:
    """K = 2, every value dyadic.  Channel 0: tx_frac 0, g, 0, g+ (the next double above g), 0 from epoch 253 on: delta = -g, +g
    (accepted: q = -+2^30), -g+, +g+ (each begins an arc).  Channel 1: carrier_frac 0, 0.5, 0, 0.5+, 0 with no Doppler and a rate gate
    of 0.5 cycles: accepted twice, then GAT_SMOOTH_RATE twice; half a cycle over the carrier frequency is far inside g."""
    E, g, r = CHUNK + 4, 2.0 ** -18, 0.5
    z = np.zeros((E, 2))
    tx_frac, cfrac = z.copy(), z.copy()
    tx_frac[253:258, 0] = (0.0, g, 0.0, float(np.nextafter(g, 1.0)), 0.0)
    cfrac[253:258, 1] = (0.0, r, 0.0, float(np.nextafter(r, 1.0)), 0.0)
    case = sc.Case(tx_ms=np.zeros((E, 2), np.int32), tx_frac=tx_frac, rx_ms=np.zeros(E, np.int32), rx_frac=np.zeros(E),
                   carrier_cycles=np.zeros((E, 2), np.int64), carrier_frac=cfrac, doppler_hz=z.copy(), valid=None, window=100, if_hz=0.0,
                   epoch_seconds=1.0, cmc_gate_s=g, rate_gate_cycles=r)
    assert g * sc.C_LIGHT / sc.C_LIGHT == g  # the Python layer's gate in metres gives the gate back
    ref = reference(case)
    assert ref["status"][252:259, 0].tolist() == [M, M, M, M, M | CMC, M | CMC, M] and ref["status"][252:259, 1].tolist() == [M, M, M, M, M | RATE, M | RATE, M]
    assert ref["cmc_s"][254, 0] == -g and ref["cmc_s"][255, 0] == 0.0 and ref["count"][255, 0] == 100 and ref["count"][256, 0] == 1
    assert ref["count"][255, 1] == 100 and ref["count"][256, 1] == 1 and ref["count"][257, 1] == 1
    return case
