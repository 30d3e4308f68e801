"""The navigation data layer on the device (gat_nav_decode): every case runs the kernels and the host twin on the same inputs into
canary-filled buffers of one layout and compares the two as whole byte buffers -- integers throughout, canaries included --, then
the outputs with the numpy restatement (tests/nav_ref.py), and then with what was sent.  Trellis and quantiser: every length at
which the survivor chunks of 64 steps change (one and two chunks, +-1, both parities), one, three and seventy channels, a capacity
above the count with NaN beyond it, different counts per channel through monitor records; clean, noisy, all-zero, non-finite,
huge, tiny and saturating symbols.  Frame synchronisation, both formats: the offsets, both polarities, both CNAV phases, bit
counts on each side of one and two whole frames, a broken middle frame, junk, a tie, max_frames and min_frames."""
import numpy as np
import pytest

from tests import nav_cases as nc
from tests import nav_ref as ref

pytestmark = pytest.mark.gpu

LENGTHS = [0, 1, 2, 3, 13, 14, 126, 127, 128, 129, 130, 131, 255, 256, 257, 258, 2106, 6553]
SIGMA_2DB = float(np.sqrt(1.0 / (2.0 * 10.0 ** 0.2)))  # Es/N0 = 2 dB on unit symbols


@pytest.fixture(scope="module")
def env():
    import torch

    import gpuacceleratedtracking_amd as g
    from gpuacceleratedtracking_amd import _lib
    g.load_library()
    return g, _lib, g.get_context(torch.device("cuda")), torch


def both(env, fmt, sym, mon, max_frames, min_frames=1, want=nc.OUTPUTS, what=""):
    """the device call and the twin on one input: equal buffers; returns (buffer, layout)"""
    g, _lib, ctx, torch = env
    cfg = nc.config(_lib, fmt, sym.shape[1], max_frames, min_frames)
    rc_h, buf_h, at = nc.host_call(g, sym, mon, cfg, want)
    # a capacity of 0: the row pointer must still be an address
    sym_t = torch.from_numpy(sym).cuda() if sym.size else torch.zeros((sym.shape[0], 1), dtype=torch.float64).cuda()
    mon_t = None if mon is None else torch.from_numpy(mon.view(np.uint8).copy()).cuda()
    rc_d, buf_d, at_d = nc.device_call(g, ctx, sym_t, mon_t, cfg, want)
    assert rc_h == 0 and rc_d == 0 and at == at_d, (what, rc_h, rc_d)
    assert nc.canaries_intact(buf_h, at, want) and nc.canaries_intact(buf_d, at, want), what
    diff = np.nonzero(buf_h != buf_d)[0]
    assert diff.size == 0, (what, "device and twin differ first at byte", int(diff[0]), at)
    return buf_d, at


def coded(rng, n, sigma=0.25):
    """n symbols of a random message's code, lightly noisy"""
    bits = rng.integers(0, 2, n // 2 + 1).astype(np.uint8)
    return (1.0 - 2.0 * ref.fec_encode(bits)[:n]) + sigma * rng.standard_normal(n)


@pytest.mark.parametrize("K", [1, 3, 70])
def test_trellis_lengths(env, K):
    rng = np.random.default_rng(100 + K)
    groups = [LENGTHS[i:i + K] for i in range(0, len(LENGTHS), K)] if K < 70 else [[LENGTHS[(7 * k) % len(LENGTHS)] for k in range(K)]]
    for lens in groups:
        lens = lens + [lens[-1]] * (K - len(lens))
        sym, mon = nc.rows([coded(rng, n) for n in lens], cap=max(lens) + 5)  # NaN beyond each count, inside the capacity
        buf, at = both(env, ref.CNAV, sym, mon, 3, what=lens)
        nc.check_against_ref(buf, at, ref.CNAV, sym, lens, 3, 1, what=lens)
    # the whole row without records: the capacity is the count
    sym = np.stack([coded(rng, 257) for _ in range(K)])
    buf, at = both(env, ref.CNAV, sym, None, 1)
    nc.check_against_ref(buf, at, ref.CNAV, sym, [257] * K, 1, 1)


def test_noisy_symbols_decode_as_sent(env):
    """Es/N0 = 2 dB, seeds 0 .. 19, 1053 bits each: about 80 of the 2106 hard symbols are wrong, the decoder returns the sent bits
    outside the last 40 (checked with this rule on the host)"""
    sent, streams = [], []
    for seed in range(20):
        rng = np.random.default_rng(seed)
        bits = rng.integers(0, 2, 1053).astype(np.uint8)
        sent.append(bits)
        streams.append(1.0 - 2.0 * ref.fec_encode(bits) + SIGMA_2DB * rng.standard_normal(2106))
    sym, mon = nc.rows(streams)
    buf, at = both(env, ref.CNAV, sym, mon, 3)
    dec = nc.take(buf, at, "decoded", 20, ref.CNAV)
    for seed in range(20):
        raw = int(((streams[seed] < 0) != (ref.fec_encode(sent[seed]) == 1)).sum())
        wrong = int((dec[seed, 0, :1013] != sent[seed][:1013]).sum())
        print(seed, "raw symbol errors", raw, "decoded bit errors", wrong)
        assert raw > 50 and wrong == 0, seed
    nc.check_against_ref(buf, at, ref.CNAV, sym, [2106] * 20, 3, 1)


def test_degenerate_symbols(env):
    rng = np.random.default_rng(5)
    n = 700
    clean = coded(rng, n, 0.0)
    holes = coded(rng, n)
    holes[rng.integers(0, n, 40)] = np.nan
    holes[rng.integers(0, n, 20)] = np.inf
    holes[rng.integers(0, n, 20)] = -np.inf
    outliers = coded(rng, n)
    outliers[rng.integers(0, n, 30)] *= 1e6  # the scale follows them: the rest quantises to 0, these saturate
    streams = [clean, np.zeros(n), holes, coded(rng, n) * 1e30, coded(rng, n) * 1e-30, outliers, np.full(n, np.nan), np.full(n, -np.inf),
               coded(rng, n) * 1e300, -np.zeros(n)]
    sym, mon = nc.rows(streams, cap=n + 3)
    for fmt in (ref.CNAV, ref.LNAV):
        buf, at = both(env, fmt, sym, mon, 2, what=fmt)
        nc.check_against_ref(buf, at, fmt, sym, [n] * len(streams), 2, 1, what=fmt)
    dec = nc.take(buf, at, "decoded", len(streams), ref.LNAV)
    assert not dec[1].any() and not dec[6].any() and not dec[7].any()  # zeros and non-finite symbols are 0 bits


def sync_streams(fmt, rng):
    """(symbols, expected (offset, phase, inverted, score)) of the grid: offsets x bit counts on each side of one and two frames"""
    tail = ref.TAIL if fmt == ref.CNAV else 0
    streams, expect = [], []
    i = 0
    for o in (0, 1, 137, 299):
        for extra in (299, 300, 301, 599, 600, 601):
            inv, phase = bool(i & 1), (i >> 1) & 1 if fmt == ref.CNAV else 0
            i += 1
            bits = nc.stream_bits(rng, fmt, o, 2, 1 + tail)[:o + extra + tail]
            x = nc.to_symbols(fmt, bits, inverted=inv, phase=phase)
            streams.append(x)
            F = extra // ref.FRAME
            expect.append((o if F else -1, phase if F else 0, int(inv) if F else 0, F))
    return streams, expect


@pytest.mark.parametrize("fmt", [ref.LNAV, ref.CNAV])
def test_frame_sync_grid(env, fmt):
    rng = np.random.default_rng(40 + fmt)
    streams, expect = sync_streams(fmt, rng)
    sym, mon = nc.rows(streams)
    counts = [len(s) for s in streams]
    buf, at = both(env, fmt, sym, mon, 3)
    recs = nc.check_against_ref(buf, at, fmt, sym, counts, 3, 1)
    frames = nc.take(buf, at, "frames", len(streams), fmt)
    for k, (rec, (o, ph, inv, F)) in enumerate(zip(recs, expect)):
        assert (rec["frame_offset"], rec["symbol_phase"], rec["inverted"], rec["score"], rec["num_frames"]) == (o, ph, inv, F, F), (k, rec)
        assert rec["tow_steps"] == max(F - 1, 0)
        good = 0x3 if fmt == ref.CNAV else 0x7ff
        assert all(frames[k, f]["status"] == good for f in range(F)) and not frames[k, F:]["status"].any()
        if F:
            assert frames[k, 0]["tow"] == (2000 if fmt == ref.CNAV else 1000)


@pytest.mark.parametrize("fmt", [ref.LNAV, ref.CNAV])
def test_frame_sync_cases(env, fmt):
    rng = np.random.default_rng(60 + fmt)
    tail = ref.TAIL if fmt == ref.CNAV else 0
    prefix = 83 if fmt == ref.CNAV else 137
    scene = nc.to_symbols(fmt, nc.stream_bits(rng, fmt, prefix, 3, 55 + tail), inverted=True)          # the CPU-checked scene
    broken = nc.to_symbols(fmt, nc.stream_bits(rng, fmt, prefix, 3, 55 + tail, break_frame=1))         # a bad middle frame
    junk = nc.to_symbols(fmt, nc.junk(rng, 1000))
    one = nc.cnav_frames if fmt == ref.CNAV else nc.lnav_frames
    tie_bits = np.concatenate([nc.junk(rng, 10), one(rng, 1), nc.junk(rng, 37), one(rng, 1, tow0=5), nc.junk(rng, 20 + tail)])
    tie = nc.to_symbols(fmt, tie_bits)                                                              # offsets 10 and 47, one hit each
    sym, mon = nc.rows([scene, broken, junk, tie, np.zeros(0)], fill=0.0)
    counts = [len(scene), len(broken), len(junk), len(tie), 0]
    good = 0x3 if fmt == ref.CNAV else 0x7ff
    for max_frames, min_frames in ((4, 1), (2, 1), (4, 3), (1, 4)):
        buf, at = both(env, fmt, sym, mon, max_frames, min_frames, what=(max_frames, min_frames))
        recs = nc.check_against_ref(buf, at, fmt, sym, counts, max_frames, min_frames, what=(max_frames, min_frames))
        frames = nc.take(buf, at, "frames", 5, fmt)
        r = recs[0]
        synced = 3 >= min_frames
        assert (r["frame_offset"], r["symbol_phase"], r["inverted"], r["score"], r["second_score"]) == (prefix if synced else -1, 0, int(synced), 3, 0)
        assert r["num_frames"] == (min(3, max_frames) if synced else 0) and r["tow_steps"] == max(r["num_frames"] - 1, 0)
        r = recs[1]
        assert r["score"] == 2 and r["frame_offset"] == (prefix if 2 >= min_frames else -1) and r["tow_steps"] == 0
        if r["num_frames"] >= 2:  # the broken frame is written, and its status says what failed
            assert frames[1, 0]["status"] == good and frames[1, 1]["status"] == (good & ~(2 if fmt == ref.CNAV else 4))
        assert recs[2]["frame_offset"] == -1 and recs[2]["score"] == 0 and recs[2]["num_frames"] == 0 and not frames[2]["status"].any()
        r = recs[3]
        assert (r["score"], r["second_score"], r["frame_offset"]) == (1, 1, 10 if min_frames <= 1 else -1)
        assert {n: recs[4][n] for n in recs[4]} == dict(frame_offset=-1, symbol_phase=0, inverted=0, score=0, second_score=0, num_frames=0,
                                                        num_bits=0, tow_steps=0)


def test_output_subsets_and_empty_capacity(env):
    """every output alone, and a capacity of 0: nothing but the asked outputs is written"""
    rng = np.random.default_rng(9)
    for fmt in (ref.LNAV, ref.CNAV):
        tail = ref.TAIL if fmt == ref.CNAV else 0
        sym, mon = nc.rows([nc.to_symbols(fmt, nc.stream_bits(rng, fmt, 5, 1, 9 + tail)), coded(rng, 100)], fill=0.0)
        full, at = both(env, fmt, sym, mon, 2)
        for want in (("channels",), ("frames",), ("decoded",), ("path_metric",), ("frames", "path_metric")):
            buf, at2 = both(env, fmt, sym, mon, 2, want=want, what=want)
            for name in want:
                o, n = at[name]
                assert np.array_equal(buf[o:o + n], full[o:o + n]), (fmt, want, name)
        buf, at = both(env, fmt, np.zeros((3, 0)), None, 2)
        assert nc.take(buf, at, "channels", 3, fmt)["frame_offset"].tolist() == [-1, -1, -1] and not nc.take(buf, at, "frames", 3, fmt)["status"].any()
