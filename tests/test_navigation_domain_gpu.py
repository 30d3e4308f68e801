"""The navigation decoder (gat_nav_decode) over its whole domain and work split: the device code the first grid
(tests/test_navigation_gpu.py) never runs, or runs on one side of a branch.  Every case goes through one `both`: the device call
and the host twin into canary-filled buffers of one layout, compared as whole byte buffers; then the numpy restatement
(nc.check_against_ref) where it is affordable; then what was sent, or the two oracles of tests/nav_ref.py that hold no trellis
(every path of a short stream; the metric of a returned path).  tests/test_navigation_domain_host.py runs the same case functions
with the twin alone, so every input and every expected value is proven on the CPU first.

Each gap and the shape that reaches it:
  the second trip of nav_pick_kernel's TOW loop (f = lane, lane + 64, ..; f + 1 < num_frames): 70 frames > 65, with a TOW
      count that starts at 100800 - 30 and so steps 100799 -> 0 after frame 29; max_frames = 66 clamps inside the second trip
      (65 pairs: lane 0 takes f = 0 and f = 64); a repeated TOW count and a TOW field of 131071 lose their steps     (case A)
  more than one workgroup of nav_frame_kernel: 5 x 70 = 350 units > 256, every frame real; 3 x 1000 = 3000 units in 12
      workgroups, all but three records zero                                                                           (case B)
  K = 4096: 8192 trellis workgroups, 1024 choice workgroups of four waves, the last one full                         (case C)
  symbol_capacity = 2^20: 2^19 steps, 8192 survivor chunks a (channel, phase), the largest row offsets               (case C)
  counts outside the row, read on the device: -1, -2^31, 306 and 2^31 - 1 beside 305 and 0, capacity 305             (case D)
  the quantiser on its edges: 16 x / unit exactly on a half, on 126, 126.5, 127 and 127.5 with unit == 1.0; a subnormal
      unit; a sum of |x| that is +inf, from one term and from finite terms                                           (case E)
  nav_best_merge inside a lane and across lanes: offsets 10 and 42 are candidates 20 and 84 = 20 + 64, 106 is 212 = 20 + 192;
      (47, 10): the lower candidate comes later; a winner of score 2 at offset 200 (candidate 400, lane 16) with the runner-up
      at offset 232 (464, lane 16), 8 (16, lane 16 too: a lower candidate of the same lane) and 9 (18, lane 18)       (case F)
  the decoder against an oracle that shares no recursion: 40 streams of at most 10 steps, every path enumerated      (case G)
  the device entry point's refusals, three differently shaped calls in flight on one scratch, decode_navigation's
      argument errors                                                                                                (case H)

Measured on the device: see DESIGN.md, section 4.14."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import nav_cases as nc
from tests import nav_ref as ref
from tests.test_navigation_gpu import both, coded, env  # noqa: F401  (env: the fixture; both: replaced by the host file)

pytestmark = pytest.mark.gpu

FORMATS = [ref.LNAV, ref.CNAV]
TOW0 = ref.TOW_MOD - 30  # frame 29 carries 100799, frame 30 carries 0
ARG, RANGE = 1, 2


def tail_of(fmt):
    return ref.TAIL if fmt == ref.CNAV else 0


def good_of(fmt):
    return 0x3 if fmt == ref.CNAV else 0x7ff


def frames_of(fmt):
    return nc.cnav_frames if fmt == ref.CNAV else nc.lnav_frames


def around(rng, fmt, prefix, body, suffix):
    """junk, the frames, junk (and the bits the CNAV search leaves out)"""
    return np.concatenate([nc.junk(rng, prefix), body, nc.junk(rng, suffix + tail_of(fmt))])


@functools.lru_cache(maxsize=None)
def body70(fmt):
    """70 frames whose TOW count crosses the end of the week; built once, never changed"""
    body = frames_of(fmt)(np.random.default_rng(700 + fmt), 70, tow0=TOW0)
    body.setflags(write=False)
    return body


# ---- A: many frames and the rollover ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def long_rows(fmt):
    """(symbols, records, counts, the restatement's decoded bits and metrics) of case A: the 70 frames at offset 17, inverted (CNAV
    at symbol phase 1); their first half; frame 40 repeating frame 39's TOW count; CNAV: a TOW field that steps 131071 -> 0"""
    rng = np.random.default_rng(710 + fmt)
    phase, make = (1 if fmt == ref.CNAV else 0), frames_of(fmt)
    full = nc.to_symbols(fmt, around(rng, fmt, 17, body70(fmt), 5), inverted=True, phase=phase)
    assert len(full) == (42109 if fmt == ref.CNAV else 21022)
    repeat = np.concatenate([make(rng, 40, tow0=TOW0), make(rng, 1, tow0=TOW0 + 39), make(rng, 29, tow0=TOW0 + 41)])
    streams = [full, full[:len(full) // 2], nc.to_symbols(fmt, around(rng, fmt, 17, repeat, 5), inverted=True, phase=phase)]
    if fmt == ref.CNAV:
        field = np.concatenate([ref.cnav_message(7, 10, tow, list(rng.integers(0, 2, 239))) for tow in (131070, 131071, 0, 1, 2)])
        streams.append(nc.to_symbols(fmt, around(rng, fmt, 17, field, 5), inverted=True, phase=phase))
    sym, mon = nc.rows(streams)
    counts = [len(s) for s in streams]
    return sym, mon, counts, ref.decode_bits(fmt, sym, counts)


@pytest.mark.parametrize("fmt", FORMATS)
def test_many_frames_and_the_rollover(env, fmt):
    sym, mon, counts, decoded = long_rows(fmt)
    phase = 1 if fmt == ref.CNAV else 0
    for max_frames in (100, 66):
        buf, at = both(env, fmt, sym, mon, max_frames, what=max_frames)
        recs = nc.check_against_ref(buf, at, fmt, sym, counts, max_frames, 1, what=max_frames, decoded=decoded)
        frames = nc.take(buf, at, "frames", len(counts), fmt)
        # the full row, its half, the repeated count: frames and steps between neighbours, of the written frames only
        for k, (F, lost) in enumerate(((70, 0), (34, 0), (70, 2))):  # the repeated count loses 39 -> 40 and 40 -> 41
            r, n = recs[k], min(F, max_frames)
            assert (r["frame_offset"], r["symbol_phase"], r["inverted"], r["score"], r["second_score"]) == (17, phase, 1, F, 0), (k, r)
            assert (r["num_frames"], r["tow_steps"]) == (n, n - 1 - lost), (k, r)
            assert np.all(frames[k, :n]["status"] == good_of(fmt)) and not frames[k, n:]["status"].any()
        assert frames[0, :min(70, max_frames)]["tow"].tolist() == [(TOW0 + f) % ref.TOW_MOD for f in range(min(70, max_frames))]
        assert frames[0, 29]["tow"] == 100799 and frames[0, 30]["tow"] == 0  # the step across the rollover is one of the 69
        assert recs[2]["tow_steps"] == (67 if max_frames == 100 else 63)
        if fmt == ref.CNAV:
            # 131070 -> 131071 -> 0 -> 1 -> 2: a field above the week is no count, (tow + 1) % 100800 follows neither of its steps
            assert frames[3, :5]["tow"].tolist() == [131070, 131071, 0, 1, 2] and (recs[3]["num_frames"], recs[3]["tow_steps"]) == (5, 2)
            nc.check_certificate(buf, at, sym, counts, sent_phase=[1, 1, 1, 1])


# ---- B: the frames kernel beyond a workgroup --------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
def test_frames_beyond_one_workgroup(env, fmt):
    g = env[0]
    rng = np.random.default_rng(720 + fmt)
    offsets = (0, 1, 137, 299, 17)
    streams = [nc.to_symbols(fmt, around(rng, fmt, o, body70(fmt), 305 - o), inverted=bool(k & 1)) for k, o in enumerate(offsets)]
    sym, mon = nc.rows(streams)
    assert g.nav_plan(5, sym.shape[1], fmt, max_frames=70)["frame_workgroups"] == 2  # 350 units
    buf, at = both(env, fmt, sym, mon, 70)
    recs = nc.check_against_ref(buf, at, fmt, sym, [len(s) for s in streams], 70, 1)
    frames = nc.take(buf, at, "frames", 5, fmt)
    for k, o in enumerate(offsets):
        r = recs[k]
        assert (r["frame_offset"], r["inverted"], r["score"], r["second_score"], r["num_frames"], r["tow_steps"]) == (o, k & 1, 70, 0, 70, 69), (k, r)
        assert np.all(frames[k]["status"] == good_of(fmt)) and frames[k]["tow"].tolist() == [(TOW0 + f) % ref.TOW_MOD for f in range(70)]
    # one frame a row and room for a thousand: zero records around three real ones
    offsets = (0, 7, 299)
    streams = [nc.to_symbols(fmt, around(rng, fmt, o, frames_of(fmt)(rng, 1, tow0=50 + k), 3)) for k, o in enumerate(offsets)]
    sym, mon = nc.rows(streams)
    assert g.nav_plan(3, sym.shape[1], fmt, max_frames=1000)["frame_workgroups"] == 12  # 3000 units
    buf, at = both(env, fmt, sym, mon, 1000)
    recs = nc.check_against_ref(buf, at, fmt, sym, [len(s) for s in streams], 1000, 1)
    frames = nc.take(buf, at, "frames", 3, fmt)
    for k, o in enumerate(offsets):
        assert (recs[k]["frame_offset"], recs[k]["score"], recs[k]["num_frames"], recs[k]["tow_steps"]) == (o, 1, 1, 0), (k, recs[k])
        assert frames[k, 0]["status"] == good_of(fmt) and frames[k, 0]["tow"] == 50 + k
        assert not frames[k, 1:].view(np.uint8).any()


# ---- C: the bounds ----------------------------------------------------------------------------------------------------------------
def test_4096_channels_cnav(env):
    g = env[0]
    K, cap = 4096, 140
    rng = np.random.default_rng(730)
    cycle = (0, 1, 2, 3, 127, 128, 129, 130, 139, 140)
    counts = [cycle[k % len(cycle)] for k in range(K)]
    sym, mon = nc.rows([coded(rng, n) for n in counts], cap=cap)
    plan = g.nav_plan(K, cap, ref.CNAV, max_frames=1)
    assert plan["trellis_workgroups"] == 8192 and plan["pick_workgroups"] == 1024
    buf, at = both(env, ref.CNAV, sym, mon, 1)
    nc.check_against_ref(buf, at, ref.CNAV, sym, counts, 1, 1)
    nc.check_certificate(buf, at, sym, counts, rows=range(0, K, 7))  # every count of the cycle of ten, 586 rows


def test_4096_channels_lnav(env):
    g = env[0]
    K, cap = 4096, 330
    rng = np.random.default_rng(731)
    streams, where = [], {}
    for k in range(K):
        if k % 4 == 1:  # a frame that ends with the row's symbols
            o = (0, 1, 29, 30)[(k // 4) % 4]
            where[k] = o
            streams.append(nc.to_symbols(ref.LNAV, np.concatenate([nc.junk_runs(rng, o), nc.lnav_frames(rng, 1, tow0=k)]), inverted=bool(k & 8)))
        else:
            streams.append(nc.to_symbols(ref.LNAV, nc.junk_runs(rng, cap)))
    sym, mon = nc.rows(streams, cap=cap)
    assert g.nav_plan(K, cap, ref.LNAV, max_frames=2)["pick_workgroups"] == 1024
    buf, at = both(env, ref.LNAV, sym, mon, 2)
    recs = nc.check_against_ref(buf, at, ref.LNAV, sym, [len(s) for s in streams], 2, 1)
    frames = nc.take(buf, at, "frames", K, ref.LNAV)
    for k in range(K):
        r = recs[k]
        want = (where[k], (k >> 3) & 1, 1, 1) if k in where else (-1, 0, 0, 0)
        assert (r["frame_offset"], r["inverted"], r["score"], r["num_frames"]) == want, (k, r)
        if k in where:
            assert frames[k, 0]["status"] == 0x7ff and frames[k, 0]["tow"] == k


@pytest.mark.parametrize("fmt", FORMATS)
def test_capacity_two_to_the_twenty(env, fmt):
    """The restatement's per-step loop is not run here (1.2 s for 40 000 symbols): device == twin, then the path certificate for
    both phases.  The metrics cannot overflow: |branch metric| <= 254 a step and 2^19 steps give at most 1.33e8 < 2^31.
    The device call takes 81.5 ms for CNAV and 1.9 ms for LNAV on an MI355X; the test 0.23 s and 0.02 s."""
    cap = 1 << 20
    sym = np.random.default_rng(740 + fmt).standard_normal((1, cap))
    buf, at = both(env, fmt, sym, None, 2)
    dec = nc.take(buf, at, "decoded", 1, fmt)
    if fmt == ref.CNAV:
        nc.check_certificate(buf, at, sym, [cap])
        pm = nc.take(buf, at, "path_metric", 1, fmt)
        assert 0 < pm.min() and pm.max() <= 254 * (cap // 2)
    else:
        assert np.array_equal(dec[0, 0], (sym[0] < 0).astype(np.uint8))
    assert nc.take(buf, at, "channels", 1, fmt)["num_bits"][0] == cap // (2 if fmt == ref.CNAV else 1)


# ---- D: the monitor's counts -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
def test_counts_outside_the_row(env, fmt):
    """a finite, non-zero fill beyond the 300 coded symbols: reading past a count, or not up to a clamped one, changes the answer"""
    rng = np.random.default_rng(750 + fmt)
    K, cap = 6, 305
    sym = np.full((K, cap), 0.25)
    for k in range(K):
        sym[k, :300] = coded(rng, 300) if fmt == ref.CNAV else nc.to_symbols(fmt, nc.lnav_frames(rng, 1, tow0=9 + k))
    mon = np.zeros(K, nc.MON_DTYPE)
    mon["num_symbols"] = [-1, -2 ** 31, 306, 2 ** 31 - 1, 305, 0]
    counts = [0, 0, 305, 305, 305, 0]
    buf, at = both(env, fmt, sym, mon, 2)
    recs = nc.check_against_ref(buf, at, fmt, sym, counts, 2, 1)
    dec, pm = nc.take(buf, at, "decoded", K, fmt), nc.take(buf, at, "path_metric", K, fmt)
    for k in range(K):
        if counts[k] == 0:
            assert recs[k]["num_bits"] == 0 and recs[k]["frame_offset"] == -1 and not dec[k].any() and not pm[k].any(), k
        elif fmt == ref.LNAV:
            assert (recs[k]["num_bits"], recs[k]["frame_offset"], recs[k]["score"]) == (305, 0, 1) and not dec[k, 0, 300:].any(), k
        else:
            assert recs[k]["num_bits"] == 152 and pm[k].min() > 0, k
    if fmt == ref.CNAV:
        nc.check_certificate(buf, at, sym, counts)


# ---- E: the quantiser's edges ------------------------------------------------------------------------------------------------------
def tie_symbols(rng):
    """256 symbols whose magnitudes are multiples of 1/32 with the sum 256: every partial sum is exact, unit == 1.0, and
    16 x / unit is x * 16 itself -- on a half for every odd multiple, and on 126, 126.5, 127 and 127.5"""
    j = np.arange(16)
    mags = np.concatenate([(j + 0.5) / 16, 2 - (j + 0.5) / 16, np.repeat(np.array([126, 126.5, 127, 127.5]) / 16, 2)])
    n = 256 - len(mags)
    units = round((256 - mags.sum()) * 32)  # what the filler has to add, in 1/32
    filler = np.full(n, units // n)
    filler[:units % n] += 1
    d = rng.integers(0, 16, n // 2)  # moved from one of a pair to the other: the sum stays
    filler[0:2 * len(d):2] += d
    filler[1:2 * len(d):2] -= d
    x = np.concatenate([mags, filler / 32.0])
    x *= rng.choice([-1.0, 1.0], len(x))
    return rng.permutation(x)


def test_quantiser_exact_ties(env):
    rng = np.random.default_rng(760)
    sym = np.stack([tie_symbols(rng) for _ in range(3)])
    n = sym.shape[1]
    for x in sym:
        assert n == 256 and np.abs(x).sum() / n == 1.0
        assert int(((np.abs(x) * 16) % 1 == 0.5).sum()) >= 32
        q = ref.quantise(x, n)
        assert {126, 127} <= set(np.abs(q).tolist()) and (np.abs(x) == 126.5 / 16).sum() == 2
        assert np.all(np.abs(q[np.abs(x) == 126.5 / 16]) == 126) and np.all(np.abs(q[np.abs(x) == 127.5 / 16]) == 127)  # ties to even; saturation
        assert np.all(np.abs(q[np.abs(x) == 0.5 / 16]) == 0) and np.all(np.abs(q[np.abs(x) == 1.5 / 16]) == 2)
    buf, at = both(env, ref.CNAV, sym, None, 1)
    nc.check_against_ref(buf, at, ref.CNAV, sym, [n] * len(sym), 1, 1)
    nc.check_certificate(buf, at, sym, [n] * len(sym))


def test_quantiser_scales(env):
    rng = np.random.default_rng(761)
    n = 700
    bits = rng.integers(0, 2, n // 2).astype(np.uint8)
    clean = 1.0 - 2.0 * ref.fec_encode(bits)
    with np.errstate(over="ignore"):
        streams = [(clean + 0.25 * rng.standard_normal(n)) * s for s in (1e-310, 5e-324, 1.7e308, 1e306)]
        assert np.isfinite(streams[3]).all() and not np.isfinite(np.abs(streams[3]).sum())  # every term finite, the sum is not
    sym, mon = nc.rows(streams, cap=n + 3)
    buf, at = both(env, ref.CNAV, sym, mon, 1)
    nc.check_against_ref(buf, at, ref.CNAV, sym, [n] * 4, 1, 1)
    dec, pm = nc.take(buf, at, "decoded", 4, ref.CNAV), nc.take(buf, at, "path_metric", 4, ref.CNAV)
    for k in (0, 1):  # a subnormal unit still decodes: 16 a symbol when all agree
        assert pm[k, 0] > 10000 and np.array_equal(dec[k, 0, :n // 2 - 40], bits[:n // 2 - 40]), (k, pm[k])
    assert not pm[2:].any() and not dec[2:].any()  # the unit is +inf: q is 0, every path ties, the bits are 0
    nc.check_certificate(buf, at, sym, [n] * 4)


# ---- F: ties and seconds of the choice ----------------------------------------------------------------------------------------------
def hits_at(rng, fmt, spec):
    """symbols of a stream with `count` frames in a row from each position of spec = ((position, count), ..), junk elsewhere; a
    frame at position p counts for the candidate offset p mod 300"""
    parts, pos = [], 0
    for i, (p, count) in enumerate(spec):
        parts += [nc.junk(rng, p - pos), frames_of(fmt)(rng, count, tow0=5 + 10 * i)]
        pos = p + ref.FRAME * count
    return nc.to_symbols(fmt, np.concatenate(parts + [nc.junk(rng, 20 + tail_of(fmt))]))


@pytest.mark.parametrize("fmt", FORMATS)
def test_ties_and_seconds_of_the_choice(env, fmt):
    rng = np.random.default_rng(770 + fmt)
    specs = [((10, 1), (342, 1)),              # offsets 10 and 42: candidates 20 and 84, one lane
             ((10, 1), (342, 1), (706, 1)),    # and 106: candidate 212, the same lane, three ways
             ((47, 1), (610, 1)),              # offsets 47, then 10: the lower candidate comes later
             ((200, 2), (908, 1)),             # the winner at 200 (candidate 400, lane 16); one hit at 8 (16: its lane, and lower)
             ((200, 2), (832, 1)),             # one hit at 232 (464: its lane, and higher)
             ((200, 2), (909, 1))]             # one hit at 9 (18: another lane, and lower)
    assert 20 % 64 == 84 % 64 == 212 % 64 and 400 % 64 == 464 % 64 == 16 % 64 != 18 % 64  # candidate (0 * 300 + o) * 2 + 0, lane c % 64
    streams = [hits_at(rng, fmt, s) for s in specs]
    sym, mon = nc.rows(streams, fill=0.0)
    counts = [len(s) for s in streams]
    buf, at = both(env, fmt, sym, mon, 4)
    recs = nc.check_against_ref(buf, at, fmt, sym, counts, 4, 1)
    for k, r in enumerate(recs):
        want = (10, 1, 1) if k < 3 else (200, 2, 1)
        assert (r["frame_offset"], r["score"], r["second_score"], r["symbol_phase"], r["inverted"]) == want + (0, 0), (k, r)
    buf, at = both(env, fmt, sym, mon, 4, 2)  # min_frames = 2: the ties no longer synchronise, the scores stay
    recs = nc.check_against_ref(buf, at, fmt, sym, counts, 4, 2)
    assert [(r["frame_offset"], r["score"], r["second_score"]) for r in recs] == [(-1, 1, 1)] * 3 + [(200, 2, 1)] * 3


# ---- G: the decoder against every path ---------------------------------------------------------------------------------------------
def ml_streams():
    """40 streams of T = 1 .. 10 steps (2 T symbols, or one more): 20 of integers -3 .. 3, where equal metrics are common, 20 Gaussian"""
    rng = np.random.default_rng(780)
    out = []
    for i in range(40):
        n = 2 * (1 + i % 10) + (i // 10) % 2
        out.append(rng.integers(-3, 4, n).astype(np.float64) if i < 20 else rng.standard_normal(n))
    return out


def every_path_of_short_streams(env):
    """path_metric is the largest metric of all 64 x 2^T paths and the returned bits attain it, for both phases of 40 rows of one
    call.  Returns how many (row, phase) pairs have several best input sequences, and how many of those have seven steps or more:
    below that, inputs that differ trade against the unknown register and give the same symbols; from there on, equal metrics
    are equal sums of different symbols, and the tie rules of the step and of the final state are on trial."""
    streams = ml_streams()
    sym, mon = nc.rows(streams, cap=24)
    counts = [len(s) for s in streams]
    buf, at = both(env, ref.CNAV, sym, mon, 1)
    nc.check_against_ref(buf, at, ref.CNAV, sym, counts, 1, 1)
    dec, pm = nc.take(buf, at, "decoded", 40, ref.CNAV), nc.take(buf, at, "path_metric", 40, ref.CNAV)
    several, long_ones = 0, 0
    for k, n in enumerate(counts):
        q = ref.quantise(sym[k], n)
        for ph in (0, 1):
            T = (n - ph) // 2
            best = ref.check_exhaustive_ml(q[ph:ph + 2 * T], dec[k, ph, :T], pm[k, ph])
            several, long_ones = several + (best > 1), long_ones + (best > 1 and T >= 7)
            assert not dec[k, ph, T:].any()
    return several, long_ones


def test_every_path_of_short_streams(env):
    several, long_ones = every_path_of_short_streams(env)
    assert several >= 10 and long_ones >= 10


# ---- H: the entry point and the surface (the device alone) -------------------------------------------------------------------------
def test_device_refusals_write_nothing(env):
    g, _lib, ctx, torch = env
    K, cap = 3, 700
    sym_t = torch.from_numpy(np.random.default_rng(790).standard_normal((K, cap))).cuda()
    at, total = nc.layout(K, 0, cap, 2)  # room for the valid call's outputs: a refused call writes none of them
    pending = []

    def call(code, what, fmt=0, K=K, null_sym=False, cfg_null=False, want=nc.OUTPUTS, **fields):
        cfg = nc.config(_lib, fmt, cap, 2, 1)
        for name, v in fields.items():
            setattr(cfg, name, v)
        buf = torch.full((total,), nc.CANARY, dtype=torch.uint8, device=sym_t.device)
        rc = ctx.lib.gat_nav_decode(ctx._h, None if null_sym else C.c_void_p(sym_t.data_ptr()), None, K, None if cfg_null else C.byref(cfg),
                                    *[C.c_void_p(buf.data_ptr() + at[n][0]) if n in want else None for n in nc.OUTPUTS])
        assert rc == code, (what, rc)
        assert ctx.lib.gat_last_error(ctx._h), what
        pending.append((what, buf))

    call(ARG, "null sym_re", null_sym=True)
    call(ARG, "null config", cfg_null=True)
    call(ARG, "struct_size", struct_size=C.sizeof(_lib.NavConfig) - 4)
    call(ARG, "struct_size 0", struct_size=0)
    call(ARG, "K = 0", K=0)
    call(ARG, "K < 0", K=-1)
    call(ARG, "capacity < 0", symbol_capacity=-1)
    call(ARG, "max_frames = 0", max_frames=0)
    call(ARG, "min_frames = 0", min_frames=0)
    call(ARG, "format 2", format=2)
    call(ARG, "format -1", format=-1)
    call(ARG, "every output null", want=())
    # these would need large buffers if they ran: they are refused before anything is touched
    call(RANGE, "K = 4097", K=4097)
    call(RANGE, "capacity above 2^20", symbol_capacity=(1 << 20) + 1)
    call(RANGE, "scratch above 1 GiB", fmt=1, K=4096, symbol_capacity=1 << 20)
    call(RANGE, "frame workgroups", K=4096, max_frames=(1 << 31) - 1)
    ctx.sync()
    for what, buf in pending:
        assert bool((buf == nc.CANARY).all()), what
    # and the same call, accepted: every output is written
    rc, buf, at = nc.device_call(g, ctx, sym_t, None, nc.config(_lib, 0, cap, 2, 1))
    assert rc == 0 and nc.canaries_intact(buf, at) and all(not np.all(buf[o:o + n] == nc.CANARY) for o, n in at.values())


def in_flight_calls():
    """(format, symbols, max_frames, outputs) of three calls that differ in shape and in what they keep in scratch"""
    rng = np.random.default_rng(791)
    big = np.stack([nc.to_symbols(ref.CNAV, around(rng, ref.CNAV, k, nc.cnav_frames(rng, 3, tow0=100 * k), 200), inverted=bool(k & 2),
                                  phase=k & 1)[:2111] for k in range(70)])
    small = np.stack([nc.to_symbols(ref.LNAV, around(rng, ref.LNAV, 40 * k, nc.lnav_frames(rng, 1), 100))[:400] for k in range(2)])
    assert big.shape == (70, 2111) and small.shape == (2, 400)
    return [(ref.CNAV, big, 3, nc.OUTPUTS), (ref.LNAV, small, 1, nc.OUTPUTS), (ref.CNAV, big, 3, ("frames",))]


def in_flight_twin(g, _lib, calls):
    """the twin's buffers of those calls; the last one holds three good frames for each of its 70 channels"""
    out = []
    for fmt, sym, max_frames, want in calls:
        rc, buf, at = nc.host_call(g, sym, None, nc.config(_lib, fmt, sym.shape[1], max_frames), want)
        assert rc == 0 and nc.canaries_intact(buf, at, want)
        out.append((buf, at))
    frames = nc.take(out[2][0], out[2][1], "frames", 70, ref.CNAV)
    assert np.all(frames["status"] == 0x3) and frames[:, 0]["tow"].tolist() == [100 * k for k in range(70)]
    return out


def test_calls_in_flight_share_the_scratch(env):
    """three calls, no synchronisation between them: q, the survivors, the scores -- and for the third the decoded bits and the
    records too -- lie in the context's one scratch buffer, which the stream's order protects"""
    g, _lib, ctx, torch = env
    calls = in_flight_calls()
    tensors = {id(sym): torch.from_numpy(sym).cuda() for _, sym, _, _ in calls}
    pending = []
    for i, (fmt, sym, max_frames, want) in enumerate(calls):
        rc, buf, at = nc.device_enqueue(g, ctx, tensors[id(sym)], None, nc.config(_lib, fmt, sym.shape[1], max_frames), want)
        assert rc == 0, i
        if i == 0:
            info = ctx.last_launch_info()
            assert info["workgroups"] == 140 and info["threads"] == 64
        pending.append((buf, at))
    ctx.sync()
    for i, ((buf, at), (buf_h, at_h)) in enumerate(zip(pending, in_flight_twin(g, _lib, calls))):
        assert at == at_h and np.array_equal(buf.cpu().numpy(), buf_h), i


def test_decode_navigation_argument_errors(env):
    g, _lib, ctx, torch = env
    from gpuacceleratedtracking_amd.monitor import TrackMonitor
    sym = torch.from_numpy(np.random.default_rng(792).standard_normal((2, 400))).cuda()
    nav = g.decode_navigation(sym, "LNAV", ctx=ctx)
    assert nav.frame_offset.shape == (2,)
    before = ctx.last_launch_info()
    seven = TrackMonitor({"sym_re": sym, "channels": torch.zeros(64, dtype=torch.uint8).cuda()}, 1e-3, 7, 2.0, ctx)
    for what, args, kw in (("float32", (sym.float(), "LNAV"), {}),
                           ("1-D", (sym[0], "LNAV"), {}),
                           ("not contiguous", (sym.t(), "LNAV"), {}),
                           ("channels of 31 bytes a record", (sym, "LNAV"), dict(channels=torch.zeros(62, dtype=torch.uint8).cuda())),
                           ("no format", (sym,), {}),
                           ("7 blocks a symbol", (seven,), {})):
        with pytest.raises(ValueError):
            g.decode_navigation(*args, ctx=ctx, **kw)
            pytest.fail(what)
    with pytest.raises(_lib.GatError):
        g.decode_navigation(sym, "LNAV", max_frames=0, ctx=ctx)
    assert ctx.last_launch_info() == before  # nothing was enqueued
    assert g.decode_navigation(seven, "LNAV", channels=None, ctx=ctx).num_frames.shape == (2,)  # with a format the monitor goes through
