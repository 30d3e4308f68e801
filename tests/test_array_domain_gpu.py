"""GPU tests of the antenna-array path over its whole domain and work split (csrc/gat_array.hip, csrc/gat_array_plan.h):
every antenna count, every regime of the covariance's work split, the edges of the value domain, the device weights and
weighted loop update against their host twins and the FP64 numpy reference (tests/array_ref.py), and the beamformer under
cancellation.

The covariance metric is array_ref.covariance_error: every element against sqrt(R_ii R_jj).  Its bound per case is
max(helpers.RTOL, 3 x f32ref), where f32ref is the same metric of numpy's complex64 product of the same samples
(array_ref.covariance_f32) against the FP64 reference -- the float32 reference's own error, printed by every check --, and
the factor 3 is room for another summation order.  Integer layouts whose sums stay below 2^24 are compared exactly.

The work split is the covariance's pure plan: cov_plan (csrc/gat_array_plan.h) states the call's rule, and the walk over
its launches is csrc/gat_est_plan.h.  A launch wants W = 8 CUs workgroups for the streaming kernel (M <= 8, aligned) and
W = 4 CUs for the tiled one, per_est = max(1, W / E) of them for each of its E estimates.  With blocks = min(bpe, B) <
per_est a block is cut into splits = min(ceil(per_est / blocks), max(1, N / min_seg)) segments, of a length rounded up to
`round_to` (splits is then ceil(N / seg_len)); min_seg = 4 round_to with round_to = 256 loads of 16 bytes (1024 / 512 /
1024 / 2048 samples by layout) for the streaming kernel, min_seg = 8 round_to with round_to = the tile geometry's chunk for
the tiled one.  G = min(blocks x splits, per_est) workgroups share an estimate's blocks x splits units.  An entry call
takes at most e_max = min(2^20, 256 MB / (8 M^2 bytes)) estimates per launch.  The regime tests below state their
arithmetic for any CU count from 64 to 512, that is W in 256 .. 2048 (tiled) and 512 .. 4096 (streaming); the plan's own
host test (tests/estplan) pins the same numbers for each of those device sizes."""
import ctypes as C

import numpy as np
import pytest

from tests import array_ref
from tests.helpers import RTOL
from tests.test_array_gpu import LAYOUTS, VEC, make_samples, run_covariance

pytestmark = pytest.mark.gpu

ARG, RANGE = 1, 2  # GAT_ERR_ARG, GAT_ERR_RANGE


@pytest.fixture(scope="module")
def g():
    import gpuacceleratedtracking_amd as g
    g.load_library()
    return g


def vp(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


# ---- samples and the check ----------------------------------------------------------------------------------------------------
def spread_samples(rng, M, ld, layout):
    """make_samples; on the float layouts every antenna besides gets its own gain, the gains spread evenly (in dB) over
    60 dB in a random order, and a DC offset of half its own rms: an antenna 60 dB below its neighbour, all-positive
    cross terms.  Returned as stored (float32 values in complex128)."""
    x = make_samples(rng, M, ld, layout)
    if layout in (2, 3):
        return x
    gain = 10.0 ** (-rng.permutation(np.linspace(0.0, 60.0, M)) / 20.0)
    x = gain[:, None] * (x + (0.6 + 0.4j))
    return x.real.astype(np.float32).astype(np.float64) + 1j * x.imag.astype(np.float32).astype(np.float64)


def check(got, x, N, B, bpe, S, what):
    """the module docstring's bound; prints the kernel's error and the float32 reference's"""
    ref = array_ref.covariance(x, N, B, bpe, S)
    f32ref = array_ref.covariance_error(array_ref.covariance_f32(x, N, B, bpe, S), ref).max()
    err = array_ref.covariance_error(got, ref)
    bound = max(RTOL, 3.0 * f32ref)
    print(f"{what}: error {np.nanmax(err):.3e} (estimate {int(np.nanargmax(err))}), float32 reference {f32ref:.3e}, bound {bound:.3e}")
    assert got.shape == ref.shape and (err <= bound).all(), (what, float(np.nanmax(err)), bound, int(np.sum(~(err <= bound))))
    return ref


def aligned_stride(N):
    return -(-N // 8) * 8  # whole 16-byte loads on every layout


# ---- antenna counts -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("M", range(1, 65))
def test_every_antenna_count(g, M, layout):
    """M = 1 .. 64 on every layout, aligned (M <= 8: every instance of the streaming kernel; above: every tile count and
    remainder of the tiled one): 5 blocks of 1237 samples (no multiple of any vector width) in estimates of 2, the last
    estimate one block"""
    rng = np.random.default_rng(5000 + 4 * M + layout)
    N, B, bpe = 1237, 5, 2
    S = aligned_stride(N)
    x = spread_samples(rng, M, B * S, layout)
    check(run_covariance(g, x, layout, N, B, bpe, S), x, N, B, bpe, S, f"M {M} layout {layout}")


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("M", range(1, 9))
def test_small_antenna_counts_through_the_tiled_kernel(g, M, layout):
    """M = 1 .. 8 where the streaming kernel does not apply: the base one sample off a 16-byte boundary, and an aligned base
    with an odd block stride (M = 1, one tile: 512 phases)"""
    rng = np.random.default_rng(6000 + 4 * M + layout)
    N, B, bpe, S = 1237, 5, 2, 1241
    x = spread_samples(rng, M, B * S, layout)
    check(run_covariance(g, x, layout, N, B, bpe, S, offset=1), x, N, B, bpe, S, f"base off by one, M {M} layout {layout}")
    check(run_covariance(g, x, layout, N, B, bpe, S, offset=0, ant_pad=3), x, N, B, bpe, S, f"odd block stride, M {M} layout {layout}")


# ---- the work split -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("M,N", ((9, 9000), (33, 3000), (64, 1000)))
def test_tiled_split_blocks_with_a_ragged_last_segment(g, M, N, layout):
    """splits > 1 on the tiled kernel, several blocks per estimate.  B = 5, bpe = 3: E = 2, estimates of 3 and 2 blocks,
    per_est = W / 2 = 128 .. 1024 > blocks = 3, so splits = min(ceil(per_est / 3) >= 43, N / min_seg).  The geometry
    (cov_tile_geom) gives chunk 255 / 88 / 24 at M = 9 / 33 / 64, min_seg = 8 chunk = 2040 / 704 / 192, and N / min_seg =
    4 / 4 / 5 binds for every CU count: seg_len = 2295 / 792 / 216 (N / splits rounded up to a chunk), splits = 4 / 4 / 5,
    the last segment 2115 / 624 / 136 samples: no whole number of chunks.  G = min(3 splits, per_est) = 12 / 12 / 15."""
    rng = np.random.default_rng(7000 + M + layout)
    B, bpe = 5, 3
    S = aligned_stride(N)
    x = spread_samples(rng, M, B * S, layout)
    check(run_covariance(g, x, layout, N, B, bpe, S), x, N, B, bpe, S, f"tiled split, M {M} layout {layout}")


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("M", (1, 5, 8))
def test_streaming_split_blocks_with_a_ragged_last_segment(g, M, layout):
    """splits > 1 on the streaming kernel, several blocks per estimate.  With v = the layout's samples per 16-byte load,
    round_to = 256 v and min_seg = 1024 v.  N = 3072 v + 777, B = 5, bpe = 3: E = 2, per_est = W / 2 = 256 .. 2048 >
    blocks = 3, splits = min(ceil(per_est / 3) >= 86, N / min_seg = 3) = 3 for every CU count; seg_len = ceil(N / 3) =
    1024 v + 259 rounded up to 1280 v, splits = ceil(N / 1280 v) = 3, the last segment 512 v + 777 samples: it ends in
    777 mod v = 1 samples that no 16-byte load covers.  G = min(9, per_est) = 9."""
    rng = np.random.default_rng(7100 + M + layout)
    N, B, bpe = 3072 * VEC[layout] + 777, 5, 3
    S = aligned_stride(N)
    x = spread_samples(rng, M, B * S, layout)
    check(run_covariance(g, x, layout, N, B, bpe, S), x, N, B, bpe, S, f"streaming split, M {M} layout {layout}")


@pytest.mark.parametrize("M,layout,offset", ((4, 0, 0), (8, 3, 0), (2, 2, 0), (3, 1, 0), (4, 0, 1), (16, 1, 0), (33, 2, 0), (64, 3, 0)))
def test_more_units_than_workgroups(g, M, layout, offset):
    """5000 blocks of 37 samples in ONE estimate: per_est = W <= 4096 < blocks = 5000, so splits = 1 and G = per_est: 5000
    units on at most 4096 workgroups (on 256 CUs 2048 streaming / 1024 tiled), every workgroup takes units g, g + G, ...
    and some one more than others"""
    rng = np.random.default_rng(7200 + M + layout + offset)
    N, B, S = 37, 5000, 40
    x = spread_samples(rng, M, B * S, layout)
    check(run_covariance(g, x, layout, N, B, B, S, offset=offset), x, N, B, B, S, f"units > workgroups, M {M} layout {layout} offset {offset}")


@pytest.mark.parametrize("M,layout,offset,bpe", ((4, 0, 0, 1), (8, 2, 0, 1), (3, 3, 0, 3), (2, 1, 1, 1), (16, 0, 0, 1), (20, 3, 0, 3)))
def test_more_estimates_than_workgroups(g, M, layout, offset, bpe):
    """E > W: bpe = 1 with B = 5003 blocks (E = 5003), and bpe = 3 with B = 15001 (E = 5001: bpe does not divide B, the
    last estimate has one block); N = 12.  per_est = max(1, W / E) = 1 since W <= 4096 < E, so splits = 1, G = 1: one
    workgroup per estimate (which takes all 3 units of it at bpe = 3), and the finishing kernel adds ONE slice.  Every
    estimate is checked."""
    rng = np.random.default_rng(7300 + M + layout + offset)
    N, S = 12, 16
    B = 5003 if bpe == 1 else 15001
    x = spread_samples(rng, M, B * S, layout)
    got = run_covariance(g, x, layout, N, B, bpe, S, offset=offset)
    assert got.shape[0] == (5003 if bpe == 1 else 5001)
    check(got, x, N, B, bpe, S, f"estimates > workgroups, M {M} layout {layout} offset {offset} bpe {bpe}")


def test_estimate_batches_at_64_antennas(g):
    """The entry point's batch loop, M = 64: a slice is 8 M^2 = 32 KB, e_max = 256 MB / 32 KB = 8192, and E = 8192 + 5
    estimates of one block of N = 3 go in two launches (8192 and 5), the second with the sample pointer and the outputs
    offset by 8192 blocks / estimates.  per_est = 1 (W <= 2048 < 8192): 256 MB of scratch; the two output planes are
    8197 x 64 x 64 floats = 134 MB each (the test holds two calls' worth on the host, and the FP64 reference: about
    1.6 GB of host memory); the samples are 4 MB.  Every estimate is checked."""
    rng = np.random.default_rng(7400)
    M, N, S, B = 64, 3, 4, 8192 + 5
    x = spread_samples(rng, M, B * S, 1)
    got = run_covariance(g, x, 1, N, B, 1, S)
    check(got, x, N, B, 1, S, "batches, M 64")


def test_estimate_batches_at_one_antenna(g):
    """The batch loop at its other bound, M = 1: e_max = min(2^20, 256 MB / 8) = 2^20, and E = 2^20 + 3 estimates of one
    aligned planar block of N = 4 go in two launches (2^20 and 3).  per_est = 1: 8 MB of scratch, 4 MB per output plane,
    2 x 16 MB of samples.  Every estimate is checked."""
    rng = np.random.default_rng(7401)
    M, N, S, B = 1, 4, 4, 2 ** 20 + 3
    x = spread_samples(rng, M, B * S, 0)
    got = run_covariance(g, x, 0, N, B, 1, S)
    check(got, x, N, B, 1, S, "batches, M 1")


# ---- values -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,offset", ((4, 0), (8, 0), (4, 1), (16, 0), (33, 0)))
def test_int16_full_scale(g, M, offset):
    """-32768 and 32767 in the first and the last 16-byte load of a block and in its ragged tail (both parts of a pair, both
    signs: the unpack is a shift pair), on samples that use the whole int16 range; sums far above 2^24, so the bound is the
    metric's"""
    rng = np.random.default_rng(7500 + M + offset)
    N, B, bpe, S = 1027, 3, 2, 1032
    x = make_samples(rng, M, B * S, 2) * 8.0
    x = np.clip(x.real, -32768, 32767) + 1j * np.clip(x.imag, -32768, 32767)
    for b in range(B):
        for m in range(M):
            lo, hi = (-32768, 32767) if (m + b) % 2 == 0 else (32767, -32768)
            for n, v in ((0, lo + 1j * hi), (1, hi + 1j * lo), (3, lo + 1j * lo), (1020, hi + 1j * hi), (1023, lo + 1j * hi), (1024, hi + 1j * lo),
                         (1026, lo + 1j * lo)):
                x[m, b * S + n] = v
    check(run_covariance(g, x, 2, N, B, bpe, S, offset=offset), x, N, B, bpe, S, f"int16 full scale, M {M} offset {offset}")


@pytest.mark.parametrize("M", (1, 2, 5, 8, 16, 33))
@pytest.mark.parametrize("N,amp", ((256, 127), (100, 127), (1, 2047), (2, 2047)))
def test_covariance_is_exact_on_int16(g, M, N, amp):
    """|R_ij| <= 2 amp^2 N: 2 x 127^2 x 256 = 8 258 048 and 2 x 2047^2 x 2 = 16 760 836 are below 2^24 = 16 777 216, every
    partial sum is an integer float32 holds: exact, through the streaming kernel (offset 0, M <= 8) and the tiled one"""
    rng = np.random.default_rng(7600 + N + M)
    B, S = 3, 256
    x = rng.integers(-amp, amp + 1, (M, B * S)).astype(np.float64) + 1j * rng.integers(-amp, amp + 1, (M, B * S)).astype(np.float64)
    x[:, 0] = -amp - 1j * amp
    x[0, N - 1] = amp + 1j * amp
    for offset in (0, 1):
        got = run_covariance(g, x, 2, N, B, 1, S, offset=offset)
        ref = array_ref.covariance(x, N, B, 1, S)
        assert np.array_equal(got, ref), (M, N, offset, np.abs(got - ref).max())


@pytest.mark.parametrize("M,logN,layout,offset", ((4, 21, 0, 0), (8, 21, 1, 0), (4, 21, 0, 1), (16, 19, 0, 0), (64, 17, 1, 0)))
def test_float_gains_over_60_db_with_a_dc_offset(g, M, logN, layout, offset):
    """one long block, antenna gains spread over 60 dB, a DC offset on each (all diagonal terms and the offsets' cross terms
    positive: the sums a single running float32 sum drifts on); the float32 reference's own error here is about 3e-6 at
    N = 2^21 and 1e-6 at 2^17 .. 2^19, so the bound is RTOL to about 1e-5"""
    rng = np.random.default_rng(7700 + M + logN + offset)
    N = 2 ** logN
    x = spread_samples(rng, M, N, layout)
    check(run_covariance(g, x, layout, N, 1, 1, N, offset=offset), x, N, 1, 1, N, f"60 dB, M {M} N 2^{logN} layout {layout} offset {offset}")


@pytest.mark.parametrize("M,layout,offset", ((4, 0, 0), (8, 2, 0), (4, 1, 1), (16, 0, 0), (33, 3, 0)))
def test_an_antenna_of_zeros(g, M, layout, offset):
    """one antenna all zero: its row and column are exactly zero (covariance_error asserts it), the rest meets the bound;
    MVDR on that covariance gives NaN weights without loading (not positive definite) and finite ones with loading"""
    import torch
    rng = np.random.default_rng(7800 + M + layout)
    N, B, bpe, S = 1237, 4, 4, 1240
    x = spread_samples(rng, M, B * S, layout)
    dead = M // 2
    x[dead] = 0.0
    got = run_covariance(g, x, layout, N, B, bpe, S, offset=offset)
    assert (got[0, dead] == 0).all() and (got[0, :, dead] == 0).all()
    check(got, x, N, B, bpe, S, f"zero antenna, M {M} layout {layout}")
    dev = g.get_context().device
    cov = torch.from_numpy(got[0].astype(np.complex64)).to(dev)
    a = torch.from_numpy(np.exp(2j * np.pi * rng.uniform(0, 1, (2, M)))).to(dev)
    assert np.isnan(g.beamformer_weights(cov, a, mode="mvdr").cpu().numpy()).all()
    assert np.isfinite(g.beamformer_weights(cov, a, mode="mvdr", loading=1e-3).cpu().numpy()).all()


@pytest.mark.parametrize("M,layout,offset,where", ((4, 0, 0, 5), (8, 1, 0, 1236), (3, 0, 1, 700), (16, 0, 0, 0), (33, 1, 0, 1236)))
def test_one_nan_sample_stays_in_its_row_and_column(g, M, layout, offset, where):
    """a NaN in one sample of one antenna (ordinary data with a defined answer): that antenna's row and column of its
    estimate are NaN, every other element still meets the bound, and the other estimates are untouched"""
    rng = np.random.default_rng(7900 + M + layout)
    N, B, bpe, S = 1237, 4, 2, 1240
    x = spread_samples(rng, M, B * S, layout)
    bad = M - 1
    x[bad, 2 * S + where] = np.nan + 0j  # block 2: estimate 1
    got = run_covariance(g, x, layout, N, B, bpe, S, offset=offset, nan_ok=True)
    assert np.isnan(got[1, bad, :].real).all() and np.isnan(got[1, :, bad].real).all()
    keep = np.arange(M) != bad
    assert np.isfinite(got[0]).all() and np.isfinite(got[1][np.ix_(keep, keep)]).all()
    if M > 1:
        check(got[:, keep][:, :, keep], x[keep], N, B, bpe, S, f"NaN sample, M {M} layout {layout}: the other antennas")


# ---- the device weighted update -----------------------------------------------------------------------------------------------
def _to_dev(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)


def _from_dev(t, dtype):
    return t.cpu().numpy().view(dtype)


@pytest.mark.parametrize("L,taps", ((3, (0, 1, 2)), (5, (4, 1, 0))))
@pytest.mark.parametrize("M", (1, 3, 16, 64))
@pytest.mark.parametrize("K", (1, 64, 65, 200))
def test_device_weighted_update_matches_reference_and_host_twin(g, K, M, L, taps):
    """gat_tracking_update_weighted on hand-filled accumulators, five consecutive updates (the filter integrators carry
    state): against array_ref.tracking_update_weighted and against gat_tracking_update_host_weighted at the tolerances of
    test_update_matches_oracle_restatement (rtol 1e-12 / atol 1e-9 on the parameters, 1e-10 / 1e-9 on the state); K = 65
    and 200 need more than one workgroup; L = 5 with late < prompt < early"""
    import torch
    import oracle
    from tests.test_array_host import _loop_case, _vp
    ctx = g.get_context()
    dev, lib = ctx.device, ctx.lib
    _, _, _, rng, cfg, cur, st = _loop_case(g, seed=8000 + K + M + L, K=K, M=M, L=L, taps=taps)
    cfgd = {n: getattr(cfg, n) for n, _ in cfg._fields_}
    w = (rng.standard_normal((K, M)) + 1j * rng.standard_normal((K, M))) / M
    w_re, w_im = np.ascontiguousarray(w.real), np.ascontiguousarray(w.imag)
    d_wre, d_wim = torch.from_numpy(w_re).to(dev), torch.from_numpy(w_im).to(dev)
    d_st, d_cur, d_nxt = _to_dev(st, dev), _to_dev(cur, dev), _to_dev(cur, dev)
    h_st, h_cur, h_nxt = st.copy(), cur.copy(), cur.copy()
    ostate = {n: st[n].copy() for n in st.dtype.names}
    ocur = oracle.make_params(cur["prn"], cur["code_freq_hz"], cur["carrier_freq_hz"], cur["code_phase_chips"], cur["carrier_phase_cycles"])
    params = ("code_freq_hz", "carrier_freq_hz", "code_phase_chips", "carrier_phase_cycles")
    for it in range(5):
        acc = (rng.standard_normal((K, L, M)) + 1j * rng.standard_normal((K, L, M))).astype(np.complex64) * 1000
        re, im = np.ascontiguousarray(acc.real), np.ascontiguousarray(acc.imag)
        d_re, d_im = torch.from_numpy(re).to(dev), torch.from_numpy(im).to(dev)
        rc = lib.gat_tracking_update_weighted(ctx._h, vp(d_re), vp(d_im), K, M, C.byref(cfg), vp(d_st), vp(d_cur), vp(d_nxt), vp(d_wre), vp(d_wim))
        assert rc == 0, rc
        ctx.sync()
        d_cur, d_nxt = d_nxt, d_cur
        assert lib.gat_tracking_update_host_weighted(_vp(re), _vp(im), K, M, C.byref(cfg), _vp(h_st), _vp(h_cur), _vp(h_nxt), _vp(w_re), _vp(w_im)) == 0
        h_cur, h_nxt = h_nxt, h_cur
        ocur, ostate = array_ref.tracking_update_weighted(acc, w, cfgd, ostate, ocur)
        got, gst = _from_dev(d_cur, cur.dtype), _from_dev(d_st, st.dtype)
        assert (got["prn"] == cur["prn"]).all()
        for f in params:
            assert np.allclose(got[f], ocur[f], rtol=1e-12, atol=1e-9), (it, f, "reference")
            assert np.allclose(got[f], h_cur[f], rtol=1e-12, atol=1e-9), (it, f, "host twin")
        for name in ostate:
            assert np.allclose(gst[name], ostate[name], rtol=1e-10, atol=1e-9), (it, name, "reference")
            assert np.allclose(gst[name], h_st[name], rtol=1e-10, atol=1e-9), (it, name, "host twin")


@pytest.mark.parametrize("K,M,L,taps", ((65, 3, 3, (0, 1, 2)), (5, 16, 5, (4, 1, 0))))
def test_device_weighted_update_without_weights_and_refusals(g, K, M, L, taps):
    """both weight pointers null: the bits of gat_tracking_update over three updates.  Refusals: exactly one null weight
    pointer GAT_ERR_ARG, a tap index outside the list GAT_ERR_RANGE, K = 0 GAT_ERR_ARG -- and nothing written."""
    import torch
    from tests.test_array_host import _loop_case
    ctx = g.get_context()
    dev, lib = ctx.device, ctx.lib
    _, _, _, rng, cfg, cur, st = _loop_case(g, seed=8100 + K, K=K, M=M, L=L, taps=taps)
    a = [_to_dev(st, dev), _to_dev(cur, dev), _to_dev(cur, dev)]
    b = [_to_dev(st, dev), _to_dev(cur, dev), _to_dev(cur, dev)]
    for it in range(3):
        acc = (rng.standard_normal((K, L, M)) + 1j * rng.standard_normal((K, L, M))).astype(np.complex64) * 1000
        d_re, d_im = torch.from_numpy(np.ascontiguousarray(acc.real)).to(dev), torch.from_numpy(np.ascontiguousarray(acc.imag)).to(dev)
        assert lib.gat_tracking_update_weighted(ctx._h, vp(d_re), vp(d_im), K, M, C.byref(cfg), vp(a[0]), vp(a[1]), vp(a[2]), None, None) == 0
        assert lib.gat_tracking_update(ctx._h, vp(d_re), vp(d_im), K, M, C.byref(cfg), vp(b[0]), vp(b[1]), vp(b[2])) == 0
        ctx.sync()
        a[1], a[2] = a[2], a[1]
        b[1], b[2] = b[2], b[1]
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), it
    assert not torch.equal(a[1], a[2])  # (the update did move the parameters)
    w = torch.zeros((K, M), dtype=torch.float64, device=dev)
    before = [t.clone() for t in a]
    call = lambda k, c, wr, wi: lib.gat_tracking_update_weighted(ctx._h, vp(d_re), vp(d_im), k, M, C.byref(c), vp(a[0]), vp(a[1]), vp(a[2]), wr, wi)  # noqa: E731
    assert call(K, cfg, vp(w), None) == ARG and call(K, cfg, None, vp(w)) == ARG
    assert call(0, cfg, vp(w), vp(w)) == ARG
    for field in ("early_index", "prompt_index", "late_index"):
        for v in (L, -1):
            bad = type(cfg).from_buffer_copy(cfg)
            setattr(bad, field, v)
            assert call(K, bad, vp(w), vp(w)) == RANGE, (field, v)
    ctx.sync()
    assert all(torch.equal(x, y) for x, y in zip(a, before))


# ---- weights ------------------------------------------------------------------------------------------------------------------
def _device_weights(g, R, a, mode, loading, K=None):
    """gat_array_weights on a covariance rounded to float32 planes; returns (status, w complex128 [K, M])"""
    import torch
    ctx = g.get_context()
    dev = ctx.device
    M = R.shape[0] if R is not None else a.shape[1] if a is not None else 4
    K = (a.shape[0] if a is not None else 1) if K is None else K
    t = lambda v, dt: torch.from_numpy(np.ascontiguousarray(v, dtype=dt)).to(dev)  # noqa: E731
    c_re, c_im = (t(R.real, np.float32), t(R.imag, np.float32)) if R is not None else (None, None)
    a_re, a_im = (t(a.real, np.float64), t(a.imag, np.float64)) if a is not None else (None, None)
    w_re = torch.full((max(K, 1), M), 7.0, dtype=torch.float64, device=dev)
    w_im = torch.full((max(K, 1), M), 7.0, dtype=torch.float64, device=dev)
    rc = ctx.lib.gat_array_weights(ctx._h, vp(c_re), vp(c_im), M, vp(a_re), vp(a_im), K, mode, loading, vp(w_re), vp(w_im))
    ctx.sync()
    return rc, w_re.cpu().numpy() + 1j * w_im.cpu().numpy()


@pytest.mark.parametrize("K", (1, 64, 65, 1000, 65535))
@pytest.mark.parametrize("M", (1, 2, 3, 5, 8, 9, 33, 63, 64))
def test_device_weights_equal_host_twin_bit_for_bit(g, M, K):
    """every mode, loading 0 and 1e-3, jammers 0 and 50 dB over the noise: the device weights have the host twin's BITS (both
    run gat_array.h's one sequence of FP64 operations per element, compiled without contraction), and match
    numpy.linalg.solve to test_array_host.py's 1e-8 in the relative 2-norm at cond <= 1e7 (asserted)"""
    from tests.test_array_host import f32_cov, host_weights
    rng = np.random.default_rng(8200 + 70 * M + K % 997)
    a = np.exp(2j * np.pi * rng.uniform(0, 1, (K, M)))
    for jnr in (0.0, 50.0):
        R = f32_cov(array_ref.jammer_covariance(M, jnr, rng)[0])
        cond = np.linalg.cond(R)
        assert cond <= 1e7, cond
        for mode in (g.GAT_BF_MVDR, g.GAT_BF_POWER_INVERSION, g.GAT_BF_CONVENTIONAL):
            for loading in (0.0, 1e-3):
                rc, w = _device_weights(g, R, a, mode, loading)
                rh, wh = host_weights(g, R, a, mode, loading)
                assert rc == 0 and rh == 0, (rc, rh)
                same = np.array_equal(w.view(np.uint64), wh.view(np.uint64))
                diff = np.abs(w - wh).max()
                if not same:
                    print(f"M {M} K {K} jammer {jnr} dB mode {mode} loading {loading}: device and host differ by {diff:.3e}")
                assert same, (mode, loading, jnr, diff)
                ref = array_ref.weights(R, a, mode, loading)
                err = np.linalg.norm(w - ref, axis=1) / np.linalg.norm(ref, axis=1)
                assert err.max() <= 1e-8, (mode, loading, jnr, err.max())


def test_device_weights_zero_steering_and_refusals(g):
    """a steering vector of zeros in conventional mode: NaN weights for that channel alone (the host answers GAT_ERR_RANGE);
    the entry point's refusals, as test_weights_error_codes has them for the host twin"""
    from tests.test_array_host import f32_cov, host_weights
    rng = np.random.default_rng(8300)
    M = 4
    R = f32_cov(array_ref.jammer_covariance(M, 20.0, rng)[0])
    a = np.exp(2j * np.pi * rng.uniform(0, 1, (3, M)))
    a[1] = 0.0
    rc, w = _device_weights(g, None, a, g.GAT_BF_CONVENTIONAL, 0.0)
    assert rc == 0 and np.isnan(w[1]).all() and np.allclose(w[[0, 2]], a[[0, 2]] / 4.0, rtol=1e-14, atol=0)
    assert host_weights(g, None, a, g.GAT_BF_CONVENTIONAL)[0] == RANGE
    a = a[:1]
    assert _device_weights(g, R, a, g.GAT_BF_MVDR, 0.0, K=65535 + 1)[0] == RANGE
    big = np.eye(65, dtype=np.complex128)
    assert _device_weights(g, big, np.ones((1, 65), dtype=np.complex128), g.GAT_BF_MVDR, 0.0)[0] == RANGE  # more than 64 antennas
    assert _device_weights(g, R, a, 3, 0.0)[0] == ARG and _device_weights(g, R, a, -1, 0.0)[0] == ARG  # mode
    assert _device_weights(g, R, None, g.GAT_BF_MVDR, 0.0)[0] == ARG  # MVDR without steering
    assert _device_weights(g, None, a, g.GAT_BF_MVDR, 0.0)[0] == ARG  # MVDR without a covariance
    assert _device_weights(g, None, None, g.GAT_BF_POWER_INVERSION, 0.0, K=1)[0] == ARG  # power inversion without a covariance
    assert _device_weights(g, R, a, g.GAT_BF_MVDR, -1e-3)[0] == ARG
    assert _device_weights(g, R, a, g.GAT_BF_MVDR, float("nan"))[0] == ARG
    assert _device_weights(g, R, a, g.GAT_BF_MVDR, float("inf"))[0] == ARG
    assert _device_weights(g, R, a, g.GAT_BF_MVDR, 0.0, K=0)[0] == ARG
    import torch
    ctx = g.get_context()
    t = lambda v, dt: torch.from_numpy(np.ascontiguousarray(v, dtype=dt)).to(ctx.device)  # noqa: E731
    c_re, c_im, a_re, a_im = t(R.real, np.float32), t(R.imag, np.float32), t(a.real, np.float64), t(a.imag, np.float64)
    out = torch.zeros((1, M), dtype=torch.float64, device=ctx.device)
    assert ctx.lib.gat_array_weights(ctx._h, vp(c_re), vp(c_im), M, vp(a_re), vp(a_im), 1, 1, 0.0, None, vp(out)) == ARG  # null output
    assert ctx.lib.gat_array_weights(ctx._h, vp(c_re), vp(c_im), M, vp(a_re), vp(a_im), 1, 1, 0.0, vp(out), None) == ARG
    ctx.sync()


# ---- beamform under cancellation ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,K,L,M", ((1, 5, 51, 16), (1, 257, 1, 16), (3, 5, 17, 64), (2, 7, 37, 33), (1, 3, 85, 2), (2, 4, 32, 1)))
def test_beamform_keeps_a_null(g, B, K, L, M):
    """The FP64 antenna sum is why this kernel exists: a null subtracts nearly equal terms.  acc = s[b, k, l] v[k, m] rounded
    to float32 with |s| about 1e6 and |v| = 1; w is built in FP64 orthogonal to the float32-rounded v (projected out,
    renormalised) plus a component along v sized so that the true output is about 1e-6 of sum_m |w_m| |acc_m|.  Per
    element |got - ref| <= 2^-23 |ref| + 64 x 2^-52 x sum_m |w_m| |acc_m|: the float32 rounding of the output (real and
    imaginary part each, so twice 2^-24 on the modulus) and an M-term FP64 sum, M <= 64.  A float32 antenna sum errs by about
    2^-24 of sum |w| |acc|, that is 6e-2 of the output.  The reference sums in extended precision (numpy longdouble).
    B K L = 255 and 257 sit either side of one workgroup's 256 rows; M = 1 has nothing to cancel (w is then just small)."""
    import torch
    ctx = g.get_context()
    rng = np.random.default_rng(8400 + B + K + L + M)
    v = np.exp(2j * np.pi * rng.uniform(0, 1, (K, M))).astype(np.complex64).astype(np.complex128)
    s = 1e6 * np.exp(2j * np.pi * rng.uniform(0, 1, (B, K, L))) * rng.uniform(0.5, 2.0, (B, K, L))
    acc = (s[..., None] * v[None, :, None, :]).astype(np.complex64)
    w = rng.standard_normal((K, M)) + 1j * rng.standard_normal((K, M))
    vn = np.sum(np.abs(v) ** 2, axis=1, keepdims=True)
    if M > 1:
        w -= v * np.sum(np.conj(v) * w, axis=1, keepdims=True) / vn  # now v^H w = 0
        w /= np.linalg.norm(w, axis=1, keepdims=True)
        w += 1e-6 * np.sum(np.abs(w), axis=1, keepdims=True) * v / vn  # y = conj(c) s v^H v with c = 1e-6 sum|w| / M
    else:
        w *= 1e-6
    a_re = torch.from_numpy(np.ascontiguousarray(acc.real)).to(ctx.device)
    a_im = torch.from_numpy(np.ascontiguousarray(acc.imag)).to(ctx.device)
    y_re, y_im = g.beamform(a_re, a_im, torch.from_numpy(w).to(ctx.device))
    got = y_re.cpu().numpy().astype(np.float64) + 1j * y_im.cpu().numpy().astype(np.float64)
    assert got.shape == (B, K, L)
    ld = np.longdouble
    assert np.finfo(ld).eps <= 2.0 ** -60, "the reference needs an extended-precision longdouble"
    wr, wi = w.real.astype(ld)[None, :, None, :], w.imag.astype(ld)[None, :, None, :]
    ar, ai = acc.real.astype(ld), acc.imag.astype(ld)
    ref = (np.sum(wr * ar + wi * ai, axis=-1).astype(np.float64) + 1j * np.sum(wr * ai - wi * ar, axis=-1).astype(np.float64))
    mag = np.sum(np.abs(w)[None, :, None, :] * np.abs(acc.astype(np.complex128)), axis=-1)
    bound = 2.0 ** -23 * np.abs(ref) + 64 * 2.0 ** -52 * mag
    err = np.abs(got - ref)
    print(f"beamform B {B} K {K} L {L} M {M}: |ref| / sum|w||acc| {np.median(np.abs(ref) / mag):.2e}, worst error / bound {np.max(err / bound):.3f}")
    if M > 1:
        assert np.median(np.abs(ref) / mag) < 1e-5  # the case does cancel
    assert (err <= bound).all(), (np.max(err / bound), int(np.sum(err > bound)))


# ---- the Python surface -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", (1, 2, 3))
@pytest.mark.parametrize("start", (0, 1, 5))
def test_python_covariance_on_interleaved_tensors(g, layout, start):
    """array.spatial_covariance on float32 / int16 / int8 [M, Ntot, 2] tensors, start 0 / 1 / 5 samples in (1 and 5: no
    16-byte boundary, the tiled kernel), block strides N, N + 3 and -- one block -- 0; blocks_per_estimate beyond
    num_blocks is one estimate"""
    import torch
    ctx = g.get_context()
    rng = np.random.default_rng(8500 + layout + start)
    M, N, B = 4, 1000, 3
    ntot = 5 + (B - 1) * (N + 3) + N
    x = make_samples(rng, M, ntot, layout)
    dt = {1: torch.float32, 2: torch.int16, 3: torch.int8}[layout]
    sig = torch.from_numpy(np.stack([x.real, x.imag], axis=-1)).to(dt).to(ctx.device)
    for stride in (N, N + 3):
        R = g.spatial_covariance(sig, N, B, blocks_per_estimate=2, start=start, block_stride=stride).cpu().numpy()
        assert R.shape == (2, M, M) and R.dtype == np.complex64
        check(R.astype(np.complex128), x[:, start:], N, B, 2, stride, f"python layout {layout} start {start} stride {stride}")
    R = g.spatial_covariance(sig, N, 1, start=start, block_stride=0).cpu().numpy()
    check(R.astype(np.complex128), x[:, start:], N, 1, 1, N, f"python layout {layout} start {start}, one block, stride 0")
    R = g.spatial_covariance(sig, N, B, blocks_per_estimate=B + 4, start=start).cpu().numpy()
    assert R.shape == (1, M, M)
    check(R.astype(np.complex128), x[:, start:], N, B, B, N, f"python layout {layout} start {start}, bpe > B")
    with pytest.raises(g.GatError):  # stride 0 with several blocks: the C entry refuses it
        g.spatial_covariance(sig, N, B, start=start, block_stride=0)
    with pytest.raises(ValueError):  # too short a signal
        g.spatial_covariance(sig, N, B, start=start + 6, block_stride=N + 3)
    with pytest.raises(ValueError):
        g.spatial_covariance(sig, ntot + 1, 1)
    with pytest.raises(ValueError):
        g.spatial_covariance(sig, N, B, blocks_per_estimate=0)
