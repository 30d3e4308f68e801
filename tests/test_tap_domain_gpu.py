"""Every kernel across the whole domain of the tap list (include/gat.h: 1 .. GAT_MAX_TAPS shifts in any order, duplicates
allowed, num_samples + max|shift| < 2^30) and at its bounds.

The kernels switch on the tap list more than on anything else: the planner sorts it stably and cuts it into launches of at
most kMaxTapsPerLaunch = 8 taps within kMaxLaunchSpan = 2048 samples, each mapping its outputs back through tap_index; the
vector kernel's LDS replica is sized for kMaxReplicaSpan = 512 unless a launch's span is wider (span_sz), and taps at an odd
distance from a launch's first tap read a second copy (tap_off = rep_copy_stride + d - 1); the matrix-core kernels take
L <= 16 within a span of 768 (the f32 kernel's replica row 256 + span, the split-bf16 kernel's flat column packing and its
chip-sign ring of two or four row tiles); the resident correlator serves lists of one launch only.  Here every path of the
correlator runs a table of tap lists that straddles each of those switches:

A. integer samples at zero carrier: every output is an integer sum below 2^24, exact in f32 and in the bf16 splits,
   compared with == against an int64 reference built on oracle.gen_code_replica; outputs no launch writes keep a sentinel;
B. float signals with an IF against the FP64 oracle at 1e-5, host and device records, with and without GAT_FLAG_ATOMIC;
C. a shuffled list of distinct shifts gives the permuted outputs of the sorted list, bit for bit (the same launches);
D. GAT_FLAG_GRAPH keys on the shifts: list, reversed list, list again each replay their own outputs;
E. the resident correlator at its limits (8 taps, span 2048, a duplicate, far negative shifts) and one step past them;
F. the tracking loop on a shuffled list follows the sorted list's trajectory bit for bit;
G. the refusals at the tap bounds (L = 0, L = 33, N + max|shift| = 2^30) leave the outputs untouched, and the replica
   generators at first_shift = +-(2^30 - count - 1) match the oracle bit for bit.

Run with -m gpu."""
import functools

import numpy as np
import pytest

import oracle
from tests.helpers import (PATHS, RTOL, check_close, code_table, configure, correlate, geometry, reset,
                           standard_codes_after)  # noqa: F401  (standard_codes_after: a fixture)

pytestmark = pytest.mark.gpu

FS = 16777216.0  # 2^24 Hz: code rate / fs is exactly the ratio asked for
SPAN_LIMIT = 1 << 30
SENTINEL_A = 0.5  # no integer sum: an output that no launch wrote is caught by ==
MC_KIND = {"mc-f32": 1, "mc-bf16-f32": 2, "mc-bf16-i16": 2, "mc-bf16-i8": 2}


@pytest.fixture(scope="module")
def g():
    import gpuacceleratedtracking_amd as g
    g.load_library()
    return g


@pytest.fixture()
def ctx(g, standard_codes_after):
    """The default context, its kernel selection, tiling and options restored after the test."""
    c = g.get_context()
    yield c
    reset(g, c)


# ---- the tap lists ------------------------------------------------------------------------------------------------------------
def _span_list(s, odd, rng):
    """Taps within a span of exactly s, one of them at 0.  odd = False: every distance from the first tap even but the span
    itself (odd for odd s); odd = True: distances 1 and 3 as well -- the launch reads the shifted replica copy."""
    b = -((s // 2) & ~1)
    d = {0, 2, -b, (s - 2) & ~1, s} if not odd else {0, 1, 3, -b, s - 1, s}
    return rng.permutation(b + np.array(sorted(d)))


def _mc_list(L, s, rng):
    """L taps spread over a span of exactly s (duplicates where s < L - 1), one of them at 0, shuffled."""
    d = np.round(np.linspace(0, s, L)).astype(np.int64)
    return rng.permutation(d - d[L // 2])


@functools.lru_cache(maxsize=None)
def tap_lists(N):
    """name -> int32 shift list for a block of N samples.  Each entry names the switch it exercises."""
    rng = np.random.default_rng(1234)
    far = SPAN_LIMIT - 1 - N  # N + max|shift| = 2^30 - 1: the largest reach the ABI accepts
    T = {
        # one tap: a launch of span 0; the whole window in front of the block; the whole window behind it
        "one-0": [0],
        "one-before": [-N - 5],
        "one-after": [3 * N],
        # order and duplicates: a descending list; 32 distinct shifts shuffled within a span of 200 (four launches by
        # count, every tap_index of every launch a different caller position); 32 equal shifts (span 0 in every launch);
        # 16 pairs of equal shifts, the partners 16 places apart in the caller's list (different launches)
        "order-3": [1, 0, -1],
        "shuffled-32": rng.permutation(np.concatenate([[0], rng.choice(np.r_[-100:0, 1:101], 31, replace=False)])),
        "equal-32": [7] * 32,
        "dup-pairs-32": (lambda v: np.concatenate([v, rng.permutation(v)]))(
            np.concatenate([[0], rng.choice(np.r_[-60:0, 1:61], 15, replace=False)])),
        # count boundary: one launch of 8; 9 = two launches of 8 + 1; 17 = three launches, and past the matrix kernels' 16
        "count-8": np.arange(-4, 4) * 3,
        "count-9": rng.permutation(np.arange(-4, 5) * 3),
        "count-17": rng.permutation(np.arange(-8, 9)),
        # split by span and count: 9 taps within 88 samples (a launch of 8, and the 9th joins ...) plus one at +5000
        "split-9+far": rng.permutation(np.concatenate([np.arange(-4, 5) * 11, [5000]])),
        # the matrix kernels' limit by span: 769 (and any span in 769 .. 2048 is one vector launch)
        "mc-8-769": _mc_list(8, 769, rng),
        # far shifts: N + max|shift| = 2^30 - 1 on either side, and both in one list (a launch each)
        "far-pos": rng.permutation([far, far - 1, far - 2, far - 7]),
        "far-neg": rng.permutation([-far, -far + 3, -far + 1]),
        "far-both": [-far, 0, far],
    }
    # vector span boundaries: the default replica sizing (512) and the launch span (2048), one below, at and one above
    for s in (511, 512, 513, 2047, 2048, 2049):
        T[f"span-{s}-even"] = _span_list(s, False, rng)
        T[f"span-{s}-odd"] = _span_list(s, True, rng)
    # the matrix kernels: 6 .. 16 taps (one channel per 32-column tile from 9 on, straddling two tiles for most L) at
    # spans 0 (all equal), 1, and the 768 bound
    for L in (6, 7, 8, 11, 16):
        for s in (0, 1, 767, 768):
            T[f"mc-{L}-{s}"] = _mc_list(L, s, rng)
    return {k: np.ascontiguousarray(v, dtype=np.int32) for k, v in T.items()}


def span_of(sh):
    return int(sh.max()) - int(sh.min())


def launch_groups(sh):
    """Tap counts of the vector kernel's launches: the sorted taps cut greedily into groups of <= 8 within 2048 samples of
    the group's first tap (gat_planner.cpp)."""
    s = np.sort(np.asarray(sh, dtype=np.int64))
    out, t0 = [], 0
    while t0 < s.size:
        t1 = t0 + 1
        while t1 < s.size and t1 - t0 < 8 and s[t1] - s[t0] <= 2048:
            t1 += 1
        out.append(t1 - t0)
        t0 = t1
    return out


def in_mc_limits(sh):
    return len(sh) <= 16 and span_of(sh) <= 768


# ---- the channels ---------------------------------------------------------------------------------------------------------------
# six channels: the code rates fs / 4 (the far lists' rate, at which 2^30 binds on the ICD tables) and a few others below one
# chip per sample; code phases of both signs.  K = 6 keeps >= 12 (channel, tap) columns for a single tap on the matrix kernels.
RATIOS = [0.25, 1.023e6 / FS, 0.6, 0.37, 0.9, 0.25]
TAUS = [3.25, 0.7, -12.3, 517.9, -2.5e3 - 0.4, 50.1]
TABLES = ["GPSL1", "GPSL5", "caller-101"]


@functools.lru_cache(maxsize=None)
def table(name):
    if name == "caller-101":
        return code_table(101, 4, 101, "pm1")
    return oracle.codes(name, 32)


def channels(codes):
    P, lc = codes.shape
    return [((3 * k + 1) % P, r, float(np.fmod(t, lc)) if abs(t) > lc else t) for k, (r, t) in enumerate(zip(RATIOS, TAUS))]


def span_ok(ratio, tau, reach, lc):
    """The code-span bound of include/gat.h (far from its edge for every channel here)."""
    return abs(tau) + ratio * reach + 1.0 < min(float(SPAN_LIMIT), 2097152.0 * lc)


def records(g, chans, fs=FS):
    return g.make_params(np.array([c[0] for c in chans]), np.array([c[1] for c in chans]) * fs, 0.0,
                         np.array([c[2] for c in chans]), 0.0)[None, :]


@functools.lru_cache(maxsize=None)
def int_signal(M, S, seed=17):
    """Independent integer samples in -128 .. 127 per antenna, re and im, over the whole stride (what lies behind the
    block must not be read)."""
    rng = np.random.default_rng(seed + 1000 * M + S)
    return (rng.integers(-128, 128, (M, S)).astype(np.float32), rng.integers(-128, 128, (M, S)).astype(np.float32))


_REF = {}


def int_reference(tab, name, sh, N, M, S):
    """Exact outputs [1, K, L, M] of the integer case: per tap the int64 dot product of the samples with
    oracle.gen_code_replica; the channels outside the code-span bound are marked in `valid`."""
    key = (tab, name, N, M, S)
    if key not in _REF:
        codes = table(tab)
        lc = codes.shape[1]
        re, im = int_signal(M, S)
        xr, xi = re[:, :N].astype(np.int64), im[:, :N].astype(np.int64)
        reach = N + int(np.abs(sh.astype(np.int64)).max())
        chans = channels(codes)
        ref = np.zeros((1, len(chans), len(sh), M), dtype=np.complex128)
        valid = np.array([span_ok(r, t, reach, lc) for _, r, t in chans])
        for k, (p, r, t) in enumerate(chans):
            if not valid[k]:
                continue
            for l, s in enumerate(sh):
                rep = oracle.gen_code_replica(codes, p, r * FS, FS, t, int(s), N).astype(np.int64)
                ref[0, k, l] = (xr @ rep).astype(np.float64) + 1j * (xi @ rep).astype(np.float64)
        assert np.abs(ref).max() < 2 ** 24
        _REF[key] = (ref, valid)
    return _REF[key]


def expect_kind(path, sh):
    """The matrix-core kernel the path must run for this list (0: the vector kernel)."""
    return MC_KIND[path] if path in MC_KIND and in_mc_limits(sh) else 0


def want_ok(path, info, sh):
    """The path's launch info.  The channel-looping tilings keep 2 MT L KT <= 96 accumulator registers: four antennas loop
    over four channels up to three taps per launch, over two up to six, else one channel per workgroup."""
    if path in ("tiling-4-2-4", "tiling-4-4-16"):
        taps = max(launch_groups(sh))
        kt = {"tiling-4-2-4": 2, "tiling-4-4-16": 4}[path]
        while kt > 1 and 4 * taps * kt > 48:
            kt //= 2
        return info["channels_per_wg"] == kt
    return "want" not in PATHS[path] or PATHS[path]["want"](info)


def check_exact(got, ref, valid, what):
    bad = []
    for k in range(ref.shape[1]):
        if valid[k]:
            if not np.array_equal(got[0, k], ref[0, k]):
                diff = np.argwhere(got[0, k] != ref[0, k])
                bad.append((k, "taps", sorted({int(d[0]) for d in diff})[:8], got[0, k][tuple(diff[0])], ref[0, k][tuple(diff[0])]))
        elif not (np.isnan(got[0, k].real).all() and np.isnan(got[0, k].imag).all()):
            bad.append((k, "not NaN past the code-span bound"))
    assert not bad, f"{what}: {bad[:6]}"


def run_int_case(g, ctx, path, tab, name, sh, M=None, N0=4096):
    N, M_, _ = geometry(path, N0, 4, 1)
    M = M or M_
    S = (N + 7) // 8 * 8
    codes = table(tab)
    ref, valid = int_reference(tab, name, sh, N, M, S)
    re, im = int_signal(M, S)
    got, info = correlate(g, ctx, path, re, im, records(g, channels(codes)), N, FS, sh, sentinel=SENTINEL_A,
                          check_want=False)
    what = f"{path} {tab} {name} M={M} {info}"
    kind = expect_kind(path, sh)
    if path in MC_KIND:
        assert info["matrix_core"] == kind, what
    if kind or path not in MC_KIND:
        if not (tab == "GPSL5" and path == "one-wave"):  # (one-wave workgroups read int8 rows of <= 2048 bytes)
            assert want_ok(path, info, sh), what
    check_exact(got, ref, valid, what)


# ---- A. exact integer sums on every path --------------------------------------------------------------------------------------
@pytest.mark.parametrize("tab", TABLES)
@pytest.mark.parametrize("path", list(PATHS))
def test_tap_lists_exact(g, ctx, path, tab):
    ctx.set_codes(table(tab))
    configure(g, ctx, path)
    N, _, _ = geometry(path, 4096, 4, 1)
    for name, sh in tap_lists(N).items():
        run_int_case(g, ctx, path, tab, name, sh)


@pytest.mark.parametrize("M", [16, 32, 64])
@pytest.mark.parametrize("path", ["mc-bf16-f32", "mc-bf16-i16", "mc-bf16-i8", "mc-f32"])
def test_matrix_lists_exact_by_row_tiles(g, ctx, path, M):
    """The matrix-core lists on one, two and four 16-antenna row tiles (the split-bf16 kernel's chip-sign ring exists from
    two row tiles on), both tables on which the matrix kernels run."""
    for tab in ("GPSL1", "caller-101"):
        ctx.set_codes(table(tab))
        configure(g, ctx, path)
        for name, sh in tap_lists(4096).items():
            if in_mc_limits(sh) or name in ("mc-8-769", "count-17"):
                run_int_case(g, ctx, path, tab, name, sh, M=M)


# ---- B. float signals against the FP64 oracle ---------------------------------------------------------------------------------
B_LISTS = ["order-3", "shuffled-32", "dup-pairs-32", "count-9", "split-9+far", "span-2049-odd", "span-513-even", "mc-11-767",
           "mc-16-1"]
IF_HZ = 2.5e5


@functools.lru_cache(maxsize=None)
def float_case(N, M, layout):
    """Four channels summed into a float signal with an IF (quantised for the integer layouts), and its records."""
    from tests.helpers import make_case
    c = make_case(31 + layout, "GPSL1", N=N, M=M, K=4, fs=N / 1e-3, if_hz=IF_HZ, noise=0.3)
    S = (N + 7) // 8 * 8  # (block stride: aligned rows for the vector loads)
    c["re"], c["im"] = (np.pad(x, ((0, 0), (0, S - N))) for x in (c["re"], c["im"]))
    if layout in (2, 3):
        q = 3000.0 if layout == 2 else 100.0
        s = q / max(np.abs(c["re"]).max(), np.abs(c["im"]).max())
        c["re"], c["im"] = np.rint(c["re"] * s).astype(np.float32), np.rint(c["im"] * s).astype(np.float32)
    return c


_OREF = {}


def float_reference(c, layout, name, sh):
    key = (c["N"], c["M"], layout, name)
    if key not in _OREF:
        _OREF[key] = oracle.correlate_f64(c["re"], c["im"], c["codes"], c["prm"], c["fs"], sh, N=c["N"])
    return _OREF[key]


@pytest.mark.parametrize("path", list(PATHS))
def test_tap_lists_against_oracle(g, ctx, path):
    configure(g, ctx, path)
    ctx.set_codes(oracle.codes("GPSL1", 32))
    N, M, _ = geometry(path, 4096, 4, 1)
    layout = PATHS[path].get("layout", 0)
    c = float_case(N, M, layout)
    lists = tap_lists(N)
    for name in B_LISTS:
        sh = lists[name]
        ref = float_reference(c, layout, name, sh)
        got, info = correlate(g, ctx, path, c["re"], c["im"], c["prm"], N, c["fs"], sh, check_want=False)
        kind = expect_kind(path, sh)
        if path in MC_KIND:
            assert info["matrix_core"] == kind, (path, name, info)
        check_close(got, ref, rtol=RTOL, what=f"{path} {name} device records {info}")
        got_h, info_h = correlate(g, ctx, path, c["re"], c["im"], c["prm"], N, c["fs"], sh, host=True, check_want=False)
        check_close(got_h, ref, rtol=RTOL, what=f"{path} {name} host records {info_h}")
        got_a, info_a = correlate(g, ctx, path, c["re"], c["im"], c["prm"], N, c["fs"], sh, check_want=False,
                                  flags=g.GAT_FLAG_ATOMIC)
        assert info_a["matrix_core"] == info["matrix_core"], (path, name, info_a)
        check_close(got_a, ref, rtol=RTOL, what=f"{path} {name} atomic {info_a}")


# ---- C. permutation invariance, bit for bit -----------------------------------------------------------------------------------
C_LISTS = ["shuffled-32", "count-9", "count-17", "split-9+far", "span-2049-odd", "span-512-odd", "mc-11-767", "mc-8-769",
           "far-both"]


@pytest.mark.parametrize("path", list(PATHS))
def test_shuffled_list_gives_permuted_outputs(g, ctx, path):
    """The planner sorts the taps stably: a shuffled list of distinct shifts runs the sorted list's launches with another
    tap_index, so its outputs are the sorted list's, permuted, bit for bit."""
    configure(g, ctx, path)
    ctx.set_codes(oracle.codes("GPSL1", 32))
    N, M, _ = geometry(path, 4096, 4, 1)
    c = float_case(N, M, PATHS[path].get("layout", 0))
    lists = tap_lists(N)
    for name in C_LISTS:
        sh = lists[name]
        assert np.unique(sh).size == sh.size, name
        srt = np.sort(sh)
        base, info0 = correlate(g, ctx, path, c["re"], c["im"], c["prm"], N, c["fs"], srt, check_want=False)
        for perm in (sh, srt[::-1].copy(), np.random.default_rng(5).permutation(srt)):
            perm = np.ascontiguousarray(perm, dtype=np.int32)
            got, info = correlate(g, ctx, path, c["re"], c["im"], c["prm"], N, c["fs"], perm, check_want=False)
            rank = np.searchsorted(srt, perm)
            assert info["matrix_core"] == info0["matrix_core"] == expect_kind(path, sh), (path, name, info)
            # (bits: a channel past the code-span bound -- a code rate above one chip per sample on the far lists -- is NaN)
            assert np.array_equal(got.view(np.int64), base[:, :, rank].view(np.int64)), (path, name, list(perm)[:8], info)


# ---- D. the graph cache keys on the shifts ------------------------------------------------------------------------------------
@pytest.mark.parametrize("mc", [0, 3])
def test_graph_replay_follows_the_list(g, mc):
    """GAT_FLAG_GRAPH on the same buffers: list A, reversed A, A, reversed A -- the first two record, the last two replay;
    each call gives the eager outputs of its own list."""
    import torch
    c = g.get_context(own_stream=True)
    c.set_codes(g.GPSL1().codes)
    reset(g, c)
    c.set_matrix_core(mc)
    try:
        N, M = 4096, 16
        fc = float_case(N, M, 0)
        re, im = torch.from_numpy(fc["re"]).to(c.device), torch.from_numpy(fc["im"]).to(c.device)
        prm = c.params_to_device(fc["prm"])
        K = fc["prm"].shape[1]
        o_re = torch.zeros((1, K, 11, M), device=c.device)
        o_im = torch.zeros_like(o_re)
        torch.cuda.synchronize()
        desc = g._lib.SignalDesc(re.data_ptr(), im.data_ptr(), g.GAT_LAYOUT_PLANAR, M, N, N, N, 0)
        a = tap_lists(N)["mc-11-767"]
        lists = [a, a[::-1].copy(), a, a[::-1].copy()]
        eager = []
        for sh in lists[:2]:
            c.downconvert_and_correlate(desc, prm, 1, K, sh, fc["fs"], o_re, o_im)
            c.sync()
            eager.append(torch.complex(o_re, o_im).cpu().numpy())
        assert c.last_launch_info()["matrix_core"] == (2 if mc == 3 else 0)
        for i, sh in enumerate(lists):
            o_re.fill_(SENTINEL_A)
            o_im.fill_(SENTINEL_A)
            c.sync()
            c.downconvert_and_correlate(desc, prm, 1, K, sh, fc["fs"], o_re, o_im, g.GAT_FLAG_GRAPH)
            c.sync()
            got = torch.complex(o_re, o_im).cpu().numpy()
            assert np.array_equal(got.view(np.float32), eager[i % 2].view(np.float32)), (mc, i)
        assert not np.array_equal(eager[0], eager[1])
    finally:
        reset(g, c)


# ---- E. the resident correlator at its tap limits -----------------------------------------------------------------------------
def test_resident_at_its_tap_limits(g, ctx):
    """8 shuffled taps with a duplicate within a span of exactly 2048, half a billion samples before the block: exact
    against the integer reference and equal to the ordinary call.  9 taps, or a span of 2049: GAT_ERR_UNSUPPORTED."""
    import torch
    tab = "GPSL1"
    codes = table(tab)
    ctx.set_codes(codes)
    N, M = 4096, 4
    base = -(1 << 29)
    sh = np.ascontiguousarray(np.random.default_rng(3).permutation(base + np.array([0, 5, 5, 2, 700, 1031, 1999, 2048])),
                              dtype=np.int32)
    ref, valid = int_reference(tab, "resident", sh, N, M, N)
    assert valid.all()
    re, im = int_signal(M, N)
    prm = records(g, channels(codes))
    got, _ = correlate(g, ctx, "default-planar", re, im, prm, N, FS, sh, sentinel=SENTINEL_A)
    check_exact(got, ref, valid, "ordinary call")
    d_re, d_im = torch.from_numpy(re).to(ctx.device), torch.from_numpy(im).to(ctx.device)
    torch.cuda.synchronize()
    desc = g._lib.SignalDesc(d_re.data_ptr(), d_im.data_ptr(), g.GAT_LAYOUT_PLANAR, M, N, N, N, 0)
    K = prm.shape[1]
    with ctx.open_resident(desc, K, sh, FS) as res:
        o_re, o_im = res.correlate(np.ascontiguousarray(prm[0]))
        out = (o_re.astype(np.float64) + 1j * o_im.astype(np.float64))[None]
    check_exact(out, ref, valid, "resident")
    assert np.array_equal(out, got)
    for bad in (np.append(sh, base + 1000), np.where(sh == sh.max(), sh.max() + 1, sh)):
        with pytest.raises(g._lib.GatError) as e:
            ctx.open_resident(desc, K, np.ascontiguousarray(bad, dtype=np.int32), FS)
        assert e.value.status == 4, (len(bad), span_of(bad), e.value)


# ---- F. the tracking loop on a shuffled list ----------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", [False, True])
def test_tracking_loop_on_a_shuffled_list(g, graph):
    """TrackingLoop takes early / prompt / late from the list's order: a shuffled five-tap list follows the sorted list's
    parameter and state trajectory bit for bit, its accumulators the sorted list's permuted."""
    import torch
    system = g.GPSL1()
    N, M, fs, nblk = 4000, 2, 4e6, 8
    prns = np.array([4, 19])
    dop = np.array([-700.0, 1300.0])
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        prm_sig = g.make_params(prns - 1, 1.023e6, dop, [[120.0, 515.5]], 0.0, shape=(2 * nblk, 2))
        re, im = g.gen_signal_stream(system, prm_sig, fs, N, M)
        srt = np.array([-2, -1, 0, 1, 2], dtype=np.int32)
        shf = np.array([1, -2, 0, 2, -1], dtype=np.int32)
        rank = np.searchsorted(srt, shf)

        def make(sh):
            return g.TrackingLoop(system, prns, N, M, fs, sh, init_carrier_doppler=dop + 4.0,
                                  init_code_phase=np.array([120.2, 515.3]), dll_bandwidth_hz=4.0)
        a, b = make(srt), make(shf)
        for rep in range(2):  # (with graph: the first call records, the second replays)
            ra, ia = a.run(re, im, nblk, start=rep * nblk * N, graph=graph)
            rb, ib = b.run(re, im, nblk, start=rep * nblk * N, graph=graph)
            side.synchronize()
            assert torch.equal(ra[:, :, rank], rb) and torch.equal(ia[:, :, rank], ib), (graph, rep)
            assert a.params().tobytes() == b.params().tobytes(), (graph, rep)
            assert a.state().tobytes() == b.state().tobytes(), (graph, rep)


# ---- G. bounds and refusals ---------------------------------------------------------------------------------------------------
def _refused(g, ctx, call, status):
    with pytest.raises(g._lib.GatError) as e:
        call()
    assert e.value.status == status, e.value


def test_tap_bounds_refused_with_outputs_untouched(g, ctx):
    """N + max|shift| = 2^30, L = 0 and L = 33: GAT_ERR_RANGE from both entry points (GAT_ERR_ARG for a bad L from the graph
    entry), the outputs keep their sentinel.  One sample inside the bound the call runs."""
    import torch
    codes = table("GPSL1")
    ctx.set_codes(codes)
    N, M = 4096, 4
    re, im = int_signal(M, N)
    d_re, d_im = torch.from_numpy(re).to(ctx.device), torch.from_numpy(im).to(ctx.device)
    desc = g._lib.SignalDesc(d_re.data_ptr(), d_im.data_ptr(), g.GAT_LAYOUT_PLANAR, M, N, N, N, 0)
    prm = records(g, channels(codes))
    K = prm.shape[1]
    prm_d = ctx.params_to_device(prm)
    o_re = torch.full((1, K, 40, M), SENTINEL_A, device=ctx.device)
    o_im = torch.full_like(o_re, SENTINEL_A)
    torch.cuda.synchronize()
    over = SPAN_LIMIT - N
    cases = [("2^30 +", np.array([0, over], np.int32), 2, 2), ("2^30 -", np.array([-over, 3], np.int32), 2, 2),
             ("L = 0", np.zeros(0, np.int32), 2, 1), ("L = 33", np.arange(33, dtype=np.int32), 2, 1)]
    for what, sh, status, graph_status in cases:
        for params, flags, st in ((prm, 0, status), (prm_d, 0, status), (prm_d, g.GAT_FLAG_GRAPH, graph_status)):
            _refused(g, ctx, lambda: ctx.downconvert_and_correlate(desc, params, 1, K, sh, FS, o_re, o_im, flags), st)
            ctx.sync()
            assert (o_re == SENTINEL_A).all() and (o_im == SENTINEL_A).all(), (what, flags)
    # one inside: accepted and exact
    for sgn in (1, -1):
        sh = np.array([0, sgn * (over - 1)], np.int32)
        ref, valid = int_reference("GPSL1", f"bound {sgn}", sh, N, M, N)
        got, _ = correlate(g, ctx, "default-planar", re, im, prm, N, FS, sh, sentinel=SENTINEL_A)
        check_exact(got, ref, valid, f"bound {sgn}")


def test_span_bound_channel_near_the_tap_bound(g, ctx):
    """At N + max|shift| = 2^30 - 1, a channel whose code rate breaks the code-span bound next to good ones: device records
    give NaN for exactly that channel (every path's planner default), host records are refused with the outputs untouched;
    on the 101-chip table 2^21 * Lc binds first for the fs / 4 channel."""
    import torch
    for tab in ("GPSL1", "caller-101"):
        codes = table(tab)
        ctx.set_codes(codes)
        P, lc = codes.shape
        N, M = 4096, 4
        far = SPAN_LIMIT - 1 - N
        sh = np.array([far, -3, far - 9], np.int32)
        chans = channels(codes) + [(1, 1.0, 0.5)]  # 1 chip per sample over a reach of 2^30 - 1: past the bound
        reach = N + far
        valid = np.array([span_ok(r, t, reach, lc) for _, r, t in chans])
        assert not valid[-1] and valid[1] and valid[0] == (tab == "GPSL1")
        re, im = int_signal(M, N)
        prm = records(g, chans)
        got, _ = correlate(g, ctx, "default-planar", re, im, prm, N, FS, sh, sentinel=SENTINEL_A)
        ref, _ = int_reference(tab, "far-bound", sh, N, M, N)
        check_exact(got[:, :-1], ref, valid[:-1], f"{tab} device records")
        assert np.isnan(got[0, -1]).all()
        d_re, d_im = torch.from_numpy(re).to(ctx.device), torch.from_numpy(im).to(ctx.device)
        desc = g._lib.SignalDesc(d_re.data_ptr(), d_im.data_ptr(), g.GAT_LAYOUT_PLANAR, M, N, N, N, 0)
        o_re = torch.full((1, len(chans), 3, M), SENTINEL_A, device=ctx.device)
        o_im = torch.full_like(o_re, SENTINEL_A)
        torch.cuda.synchronize()
        _refused(g, ctx, lambda: ctx.downconvert_and_correlate(desc, prm, 1, len(chans), sh, FS, o_re, o_im), 2)
        ctx.sync()
        assert (o_re == SENTINEL_A).all() and (o_im == SENTINEL_A).all(), tab


def test_replica_generators_at_the_shift_bound(g, ctx):
    """gat_gen_code_replica and gat_gen_code_replica_multi at first_shift = +-(2^30 - count - 1) bit for bit against
    oracle.gen_code_replica; one sample further both are refused and write nothing."""
    import torch
    codes = table("GPSL1")
    ctx.set_codes(codes)
    count = 4099
    chans = [(p, r, t) for p, r, t in channels(codes)]
    prm = records(g, chans)
    prm_d = ctx.params_to_device(prm[0])
    for sgn in (1, -1):
        first = sgn * (SPAN_LIMIT - count - 1)
        want = np.stack([oracle.gen_code_replica(codes, p, r * FS, FS, t, first, count) for p, r, t in chans])
        rep = torch.full((len(chans), count + 8), SENTINEL_A, device=ctx.device)
        ctx.gen_code_replica_multi(rep, count, prm_d, len(chans), FS, first)
        got = rep.cpu().numpy()
        assert np.array_equal(got[:, :count], want) and (got[:, count:] == SENTINEL_A).all(), sgn
        one = torch.full((count + 8,), SENTINEL_A, device=ctx.device)
        for k, (p, r, t) in enumerate(chans):
            ctx.gen_code_replica(one, count, p, r * FS, FS, t, first)
            assert np.array_equal(one.cpu().numpy()[:count], want[k]), (sgn, k)
        over = first + sgn
        rep.fill_(SENTINEL_A)
        one.fill_(SENTINEL_A)
        _refused(g, ctx, lambda: ctx.gen_code_replica_multi(rep, count, prm_d, len(chans), FS, over), 2)
        _refused(g, ctx, lambda: ctx.gen_code_replica(one, count, chans[0][0], chans[0][1] * FS, FS, chans[0][2], over), 2)
        ctx.sync()
        assert (rep == SENTINEL_A).all() and (one == SENTINEL_A).all(), sgn
