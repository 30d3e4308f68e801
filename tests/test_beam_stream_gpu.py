"""GPU tests of the sample beamformer (include/gat.h gat_beamform_samples, csrc/gat_beam.hip): y[n, j, b] = sum_m conj(w[j][m])
x[n, m, b] against the FP64 restatement tests/beam_ref.py, and what it is for: the acquisition search under a jammer.

The bound is derived, not measured: a complex dot product of length M is two real FMA chains of length 2 M on weights rounded
once, |y - y64| <= (4 M + 4) 2^-24 sum_m |w_m| |x_m| per sample (twice the first-order bound).  No relative test on y: in a
null |y| << sum |w| |x|.  Every parity run also asserts identical bits on a second call, that a sentinel in every element of the
output allocation the call must not write (before the base, between blocks and beams, after the end) is untouched, and that
there is no NaN."""
import ctypes as C

import numpy as np
import pytest

from tests import beam_ref
from tests.helpers import check_close
from tests.test_array_gpu import LAYOUTS, SCENE, VEC, make_samples, scene_directions, scene_interference

pytestmark = pytest.mark.gpu

OUT_LAYOUTS = (0, 1)  # GAT_LAYOUT_PLANAR, GAT_LAYOUT_INTERLEAVED
SENTINEL = 7.0
OK, ERR_ARG, ERR_RANGE, ERR_UNSUPPORTED = 0, 1, 2, 4


@pytest.fixture(scope="module")
def g():
    import gpuacceleratedtracking_amd as g
    g.load_library()
    return g


def random_weights(rng, J, M):
    """random complex weights with |w| spread over 40 dB"""
    return 10.0 ** rng.uniform(-2.0, 0.0, (J, M)) * np.exp(2j * np.pi * rng.uniform(0, 1, (J, M)))


def put_signal(g, x, layout, offset=0, ant_pad=0):
    """x complex128 [M, ld] into a device buffer whose antenna rows are ld + ant_pad samples apart and which starts `offset`
    samples into its allocation (run_covariance's arrangement).  Returns (tensors to keep, re pointer, im pointer, ant_stride)."""
    import torch
    dev = g.get_context().device
    M, ld = x.shape
    row = ld + ant_pad
    total = offset + M * row + 16
    if layout == 0:
        bufs = [torch.zeros(total, dtype=torch.float32, device=dev) for _ in range(2)]
        for buf, plane in zip(bufs, (x.real, x.imag)):
            buf[offset:offset + M * row].view(M, row)[:, :ld] = torch.from_numpy(plane.astype(np.float32)).to(dev)
        return bufs, bufs[0].data_ptr() + 4 * offset, bufs[1].data_ptr() + 4 * offset, row
    dt = {1: torch.float32, 2: torch.int16, 3: torch.int8}[layout]
    buf = torch.zeros((total, 2), dtype=dt, device=dev)
    buf[offset:offset + M * row].view(M, row, 2)[:, :ld] = torch.from_numpy(np.stack([x.real, x.imag], axis=-1)).to(dt).to(dev)
    return [buf], buf.data_ptr() + g.SAMPLE_BYTES[layout] * offset, None, row


def run_beams(g, x, w, layout, out_layout, N, B, block_stride, out_block_stride=None, offset=0, ant_pad=0, out_offset=4, beam_pad=4,
              nan_ok=False, want_vec=None):
    """The call on x (complex128 [M, ld], B blocks block_stride apart) and w (complex128 [J, M]).  The output allocation starts
    out_offset elements before the descriptor's base, puts beams B * out_block_stride + beam_pad elements apart and ends 16
    elements after the last beam; it is filled with the sentinel.  Two calls on fresh allocations: identical bits, the sentinel
    untouched wherever the call must not write, no NaN (unless nan_ok).  Returns complex128 [B, J, N]."""
    import torch
    ctx = g.get_context()
    dev = ctx.device
    M, J = x.shape[0], w.shape[0]
    keep, p_re, p_im, row = put_signal(g, x, layout, offset, ant_pad)
    desc = g._lib.SignalDesc(p_re, p_im, layout, M, N, row, block_stride, 0)
    obs = N if out_block_stride is None else out_block_stride
    orow = B * obs + beam_pad
    total = out_offset + J * orow + 16
    w_re = torch.from_numpy(np.ascontiguousarray(w.real, dtype=np.float64)).to(dev)
    w_im = torch.from_numpy(np.ascontiguousarray(w.imag, dtype=np.float64)).to(dev)
    written = np.zeros(total, dtype=bool)
    idx = out_offset + (np.arange(J)[:, None, None] * orow + np.arange(B)[None, :, None] * obs + np.arange(N)[None, None, :])  # [J, B, N]
    written[idx.reshape(-1)] = True
    outs = []
    for _ in range(2):
        if out_layout == 0:
            o = [torch.full((total,), SENTINEL, dtype=torch.float32, device=dev) for _ in range(2)]
            odesc = g._lib.SignalDesc(o[0].data_ptr() + 4 * out_offset, o[1].data_ptr() + 4 * out_offset, 0, J, N, orow, obs, 0)
        else:
            o = [torch.full((total, 2), SENTINEL, dtype=torch.float32, device=dev)]
            odesc = g._lib.SignalDesc(o[0].data_ptr() + 8 * out_offset, None, 1, J, N, orow, obs, 0)
        ctx.check(ctx.lib.gat_beamform_samples(ctx._h, C.byref(desc), B, C.c_void_p(w_re.data_ptr()), C.c_void_p(w_im.data_ptr()), J,
                                               C.byref(odesc)), "gat_beamform_samples")
        ctx.sync()
        if want_vec is not None:
            assert ctx.last_launch_info()["vec"] == want_vec, (ctx.last_launch_info(), M, J, layout, out_layout)
        h = [t.cpu().numpy() for t in o]
        planes = h if out_layout == 0 else [h[0][:, 0], h[0][:, 1]]
        outs.append(planes)
    for p0, p1 in zip(*outs):
        assert p0.tobytes() == p1.tobytes(), "a repeat call gave other bits"
        assert (p0[~written] == SENTINEL).all(), "the call wrote outside its elements"
    y = (outs[0][0][idx].astype(np.float64) + 1j * outs[0][1][idx].astype(np.float64)).transpose(1, 0, 2)  # [B, J, N]
    if not nan_ok:
        assert not np.isnan(y).any()
    return y


def check_bound(y, x, w, N, B, S, what, factor=1.0):
    ref, bd = beam_ref.beams(x, w, N, B, S), beam_ref.bound(x, w, N, B, S)
    err = np.abs(y - ref)
    worst = float((err / np.maximum(bd, 1e-300)).max())
    assert (err <= factor * bd).all(), f"{what}: |y - y64| reaches {worst:.3f} of the bound"
    return worst


def pad(n, to):
    return -(-n // to) * to


# ---- 1: every antenna and beam count -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_layout", OUT_LAYOUTS)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("M", (1, 2, 3, 4, 5, 6, 7, 8, 9, 16, 33, 63, 64))
def test_every_antenna_and_beam_count(g, M, layout, out_layout):
    """aligned blocks (M <= 8: the streaming kernel, else the general one; gat_last_launch_info says which ran), 3 blocks of
    1000 samples, 1 to 64 beams: one beam, a partial and a full tile of 4 and of 8, one over, the most"""
    N, B = 1000, 3
    S = pad(N, 8)
    rng = np.random.default_rng(1000 * M + 10 * layout + out_layout)
    x = make_samples(rng, M, B * S, layout)
    worst = 0.0
    for J in (1, 2, 4, 5, 8, 9, 64):
        w = random_weights(rng, J, M)
        y = run_beams(g, x, w, layout, out_layout, N, B, S, out_block_stride=S, want_vec=4 if M <= 8 else 1)
        worst = max(worst, check_bound(y, x, w, N, B, S, f"M {M} J {J} layout {layout} out {out_layout}"))
    print(f"M {M} layout {layout} out {out_layout}: worst error {worst:.3f} of the bound")


# ---- 2: block lengths and tails ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_layout", OUT_LAYOUTS)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("N", (1, 2, 3, 7, 8, 9, 255, 256, 257, 4097))
def test_block_lengths_and_tails(g, N, layout, out_layout):
    """block lengths around the load group and the workgroup's stride; block_stride rounded up to the load group on the input
    and to 4 on the output, so every block is aligned and only its tail is ragged"""
    B = 3
    S, OS = pad(N, max(VEC[layout], 4)), pad(N, 4)
    for M in (1, 4, 8):
        rng = np.random.default_rng(7 * N + layout + 100 * M + out_layout)
        x = make_samples(rng, M, B * S, layout)
        for J in (1, 3, 5):
            w = random_weights(rng, J, M)
            y = run_beams(g, x, w, layout, out_layout, N, B, S, out_block_stride=OS, want_vec=4)
            check_bound(y, x, w, N, B, S, f"N {N} M {M} J {J} layout {layout} out {out_layout}")


# ---- 3: misalignment -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_layout", OUT_LAYOUTS)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("M", (2, 4, 16))
def test_misaligned_bases_and_odd_strides(g, M, layout, out_layout):
    """input base 1 and 5 samples off, odd antenna and block strides, ant_pad 3; the same with the output 1 float off: the
    general kernel, no refusal, and the results of the aligned run to within twice the bound"""
    N, B, S = 1001, 3, 1003
    rng = np.random.default_rng(31 * M + layout + 7 * out_layout)
    x = make_samples(rng, M, B * S, layout)
    for J in (1, 5):
        w = random_weights(rng, J, M)
        bd = beam_ref.bound(x, w, N, B, S)
        # aligned: the same blocks 1008 samples apart, 1004 on the output
        xal = np.zeros((M, B * 1008), dtype=np.complex128)
        for b in range(B):
            xal[:, b * 1008:b * 1008 + N] = x[:, b * S:b * S + N]
        y_al = run_beams(g, xal, w, layout, out_layout, N, B, 1008, out_block_stride=1004, want_vec=4 if M <= 8 else 1)
        check_bound(y_al, x, w, N, B, S, f"aligned M {M} J {J}")
        odd_pad = (B * S + 1) % 2  # makes the antenna stride odd
        for offset, ant_pad, out_offset, obs in ((1, odd_pad, 4, 1004), (5, odd_pad, 4, 1004), (0, 3, 4, 1004), (0, 0, 5, 1003), (1, odd_pad, 5, 1003),
                                                 (0, 0, 4, 1003)):
            y = run_beams(g, x, w, layout, out_layout, N, B, S, out_block_stride=obs, offset=offset, ant_pad=ant_pad, out_offset=out_offset,
                          beam_pad=5, want_vec=1)
            check_bound(y, x, w, N, B, S, f"misaligned M {M} J {J} offset {offset} pad {ant_pad} out {out_offset}/{obs}")
            assert (np.abs(y - y_al) <= 2 * bd).all()


# ---- 4: more units than one grid pass ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,B,layout", ((4, 20000, 64, 0), (4, 20000, 64, 3), (1, 2 ** 21, 1, 0), (1, 2 ** 21, 1, 3), (2, 24, 4500, 0), (2, 24, 4500, 3)))
def test_many_work_units(g, M, N, B, layout):
    """blocks split into chunks, one long block over the whole grid, and more blocks than the grid has workgroups (every
    workgroup strides to a second unit): every sample checked"""
    rng = np.random.default_rng(N + B + layout)
    x = make_samples(rng, M, B * N, layout)
    for J, out_layout in ((1, 0), (4, 1)) if N < 2 ** 21 else ((2, 0),):
        w = random_weights(rng, J, M)
        y = run_beams(g, x, w, layout, out_layout, N, B, N, want_vec=4)
        check_bound(y, x, w, N, B, N, f"M {M} N {N} B {B} layout {layout} J {J}")


# ---- 5: integers at full scale -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout,full", ((2, 32767), (3, 127)))
@pytest.mark.parametrize("M", (4, 16))
def test_integers_at_full_scale(g, M, layout, full):
    """every sample +-full scale (and the most negative value once), unit-modulus weights: the bound holds"""
    N, B = 1000, 2
    S = pad(N, 8)
    rng = np.random.default_rng(M + layout)
    x = full * (rng.choice((-1.0, 1.0), (M, B * S)) + 1j * rng.choice((-1.0, 1.0), (M, B * S)))
    x[0, 0] = (-full - 1) * (1 + 1j)
    w = np.exp(2j * np.pi * rng.uniform(0, 1, (3, M)))
    for out_layout in OUT_LAYOUTS:
        y = run_beams(g, x, w, layout, out_layout, N, B, S, out_block_stride=S)
        check_bound(y, x, w, N, B, S, f"full scale M {M} layout {layout}")


# ---- 6: NaN in, NaN out, nowhere else ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,offset", ((4, 0), (4, 1), (16, 0)))
def test_one_nan_sample_and_one_nan_weight_row(g, M, offset):
    N, B, J = 1000, 3, 5
    S = pad(N, 8)
    rng = np.random.default_rng(60 + M + offset)
    x = make_samples(rng, M, B * S, 0)
    w = random_weights(rng, J, M)
    xn = x.copy()
    m, b, n = M - 1, 1, 613
    xn[m, b * S + n] = np.nan
    y = run_beams(g, xn, w, 0, 0, N, B, S, out_block_stride=S, offset=offset, nan_ok=True)
    want = np.zeros((B, J, N), dtype=bool)
    want[b, :, n] = True
    assert np.array_equal(np.isnan(y.real) | np.isnan(y.imag), want)
    ok = ~want
    ref, bd = beam_ref.beams(x, w, N, B, S), beam_ref.bound(x, w, N, B, S)
    assert (np.abs(y - ref)[ok] <= bd[ok]).all()
    wn = w.copy()
    wn[2, :] = np.nan  # what the device solver writes for a covariance that is not positive definite
    y = run_beams(g, x, wn, 0, 1, N, B, S, out_block_stride=S, offset=offset, nan_ok=True)
    want = np.zeros((B, J, N), dtype=bool)
    want[:, 2, :] = True
    assert np.array_equal(np.isnan(y.real) | np.isnan(y.imag), want)
    assert (np.abs(y - ref)[~want] <= bd[~want]).all()


# ---- the scene of tests/test_array_gpu.py with the satellite at an amplitude of its own -----------------------------------------
def scene(g, nblk, amp):
    """planar device tensors (re, im) [M, nblk * N]: the scene's satellite at amplitude `amp` (noise = 1 per antenna) plus its
    interference; the interference alone (CPU complex64); the satellite's steering vector"""
    system = g.GPSL1()
    N, M, fs, fc = SCENE["N"], SCENE["M"], SCENE["fs"], SCENE["fc"]
    dop, tau0, phi0 = SCENE["dop"], SCENE["tau0"], SCENE["phi0"]
    fcode = fc * (1 + dop / 1575.42e6)
    b = np.arange(nblk, dtype=np.float64)[:, None]
    tau = np.mod(tau0 + fcode * (N / fs) * b, 1023.0)
    phi = np.mod(phi0 + dop * (N / fs) * b, 1.0)
    prm = g.make_params(SCENE["prn"] - 1, fcode, dop, tau, 2 * np.pi * phi, shape=(nblk, 1))
    ss, _ = scene_directions(SCENE["seed"])
    re, im = g.gen_signal_stream(system, prm, fs, N, M, amplitude=amp, steering_cycles=ss)
    x_in = scene_interference(SCENE["seed"], nblk)
    re = (re + x_in.real.to(re.device)).contiguous()
    im = (im + x_in.imag.to(im.device)).contiguous()
    return re, im, x_in, np.exp(2j * np.pi * ss.astype(np.float32).astype(np.float64))


# ---- 7: linearity against the path that exists ---------------------------------------------------------------------------------
def test_correlating_the_beams_equals_beamforming_the_accumulators(g):
    """K = 3 channels with MVDR weights of their own: the beam stream correlated as one signal per channel (num_ants = 1,
    chan_stride = the beams' stride) against gat_beamform of the per-antenna accumulators of the same blocks.  The early and
    late taps get the prompt tap's scale as their absolute floor."""
    import torch
    ctx = g.get_context()
    system = g.GPSL1()
    ctx.set_codes(system.codes)
    K, M, N, B, fs = 3, 4, 4000, 2, 4e6
    prns = np.array([3, 11, 26])
    dop = np.array([850.0, -1400.0, 40.0])
    tau = np.array([[10.0, 400.5, 900.25]])
    prm = g.make_params(prns - 1, 1.023e6, dop, tau, 0.0, shape=(B, K))
    rng = np.random.default_rng(12)
    re, im = g.gen_signal_stream(system, prm, fs, N, M, steering_cycles=rng.uniform(0, 1, M), noise_sigma=0.5, seed=3)
    shifts = g.get_correlator_sample_shifts(system, g.EarlyPromptLateCorrelator(M, 3), fs, 0.5)
    L = len(shifts)
    R = g.spatial_covariance((re, im), N, B)
    steer = torch.from_numpy(np.exp(2j * np.pi * rng.uniform(0, 1, (K, M)))).to(re.device)
    w = g.beamformer_weights(R[0], steer, mode="mvdr")
    # the path that exists: per-antenna accumulators, then the weights
    desc = g._lib.SignalDesc(re.data_ptr(), im.data_ptr(), 0, M, N, re.stride(0), N, 0)
    acc_re = torch.empty((B, K, L, M), dtype=torch.float32, device=re.device)
    acc_im = torch.empty_like(acc_re)
    ctx.downconvert_and_correlate(desc, prm, B, K, shifts, fs, acc_re, acc_im)
    y_re, y_im = g.beamform(acc_re, acc_im, w)
    ref = y_re.cpu().numpy().astype(np.float64) + 1j * y_im.cpu().numpy().astype(np.float64)  # [B, K, L]
    # the new path: one beam per channel, each channel correlated on its own stream
    b_re, b_im = g.beamform_samples((re, im), w, N, B)
    bdesc = g._lib.SignalDesc(b_re.data_ptr(), b_im.data_ptr(), 0, 1, N, b_re.stride(0), N, b_re.stride(0))
    o_re = torch.empty((B, K, L, 1), dtype=torch.float32, device=re.device)
    o_im = torch.empty_like(o_re)
    ctx.downconvert_and_correlate(bdesc, prm, B, K, shifts, fs, o_re, o_im)
    ctx.sync()
    got = (o_re.cpu().numpy().astype(np.float64) + 1j * o_im.cpu().numpy().astype(np.float64))[..., 0]
    prompt = L // 2
    check_close(got[:, :, prompt, None, None], ref[:, :, prompt, None, None], what="prompt tap")
    for b in range(B):
        for k in range(K):
            floor = abs(ref[b, k, prompt])
            for tap in range(L):
                assert abs(got[b, k, tap] - ref[b, k, tap]) <= 1e-5 * max(floor, abs(ref[b, k, tap])), (b, k, tap)


# ---- 8: the null survives the stream -------------------------------------------------------------------------------------------
def test_the_null_survives_the_stream(g):
    """the scene's interference alone, 8 blocks, MVDR weights from its covariance: the GPU beam's mean power is within 0.05 dB
    of the FP64 w64^H x (the derived bound is 5e-4 of the output amplitude, 0.004 dB: 10x margin) and at least 25 dB below the
    conventional beam's (the guard of test_mvdr_nulls_the_jammer_end_to_end against a conjugate slip)"""
    import torch
    nblk, N = 8, SCENE["N"]
    ctx = g.get_context()
    x_in = scene_interference(SCENE["seed"], nblk)
    re = x_in.real.contiguous().to(ctx.device)
    im = x_in.imag.contiguous().to(ctx.device)
    ss, _ = scene_directions(SCENE["seed"])
    a = torch.from_numpy(np.exp(2j * np.pi * ss.astype(np.float32).astype(np.float64))).to(ctx.device)
    R = g.spatial_covariance((re, im), N, nblk)
    w = g.beamformer_weights(R[0], a, mode="mvdr")
    w_conv = g.beamformer_weights(None, a, mode="conventional")
    y_re, y_im = g.beamform_samples((re, im), torch.cat([w, w_conv]), N, nblk)
    y = y_re.cpu().numpy().astype(np.float64) + 1j * y_im.cpu().numpy().astype(np.float64)  # [2, nblk * N]
    x = x_in.numpy().astype(np.complex128)
    y64 = w.cpu().numpy().conj() @ x
    p = lambda v: float(np.mean(np.abs(v) ** 2))  # noqa: E731
    d_ref = 10 * np.log10(p(y[0]) / p(y64[0]))
    d_conv = 10 * np.log10(p(y[1]) / p(y[0]))
    print(f"beam power: GPU vs FP64 {d_ref:+.5f} dB; conventional over MVDR {d_conv:.1f} dB")
    assert not np.isnan(y).any()
    assert abs(d_ref) <= 0.05
    assert d_conv >= 25.0


# ---- 9: cold start under the jammer --------------------------------------------------------------------------------------------
def test_cold_start_under_the_jammer(g):
    """The scene with the satellite at amplitude 0.25 (54 dB-Hz; below the noise, as real ones are), 8 blocks, power-inversion
    weights from spatial_covariance of those blocks, acquire over PRNs 7, 3 and 20 (columns 6, 2, 19), 1 block, the default grid
    (29 Doppler bins of 500 Hz x 2000 code bins, s = 2).  On the raw 4-antenna signal nothing is detected: the search adds the
    antennas as |R|^2 and takes the jammer (40 dB over the noise) at full strength.  With weights= PRN 7 is detected within one
    Doppler bin of -2210 Hz and half a chip of 511.9, the other two are not.  Forecast on the CPU beforehand (scripts/beam_cold_start_forecast.py
    prints it), on the library's own conventions (the satellite from the FP64 oracle's generator with the scene's steering vector, the same interference,
    FP64 power-inversion weights, helpers.acq_power_oracle over the whole 29 x 2000 grid, gat_acq_stats_host on it): peak /
    second 1.006, 1.072, 1.113 on the antennas (nothing detected; PRN 7's peak in a wrong bin); in the beam PRN 7 3.288 at
    -2300.1 Hz and 511.950 chips (C/N0 of the beam's output 45.4 dB-Hz), the absent PRNs 1.126 and 1.032.  The threshold is 2.0
    and the ratio is above 2.5, so the amplitude stays at 0.25."""
    import torch
    nblk, N, fs = 8, SCENE["N"], SCENE["fs"]
    system = g.GPSL1()
    re, im, _, _ = scene(g, nblk, 0.25)
    cols = [SCENE["prn"] - 1, 2, 19]
    raw = g.acquire(system, (re, im), fs, cols, num_samples=N, num_blocks=1)
    print("raw:", [(r.prn, r.detected, round(r.peak_to_second, 3), r.carrier_doppler, r.code_phase) for r in raw])
    assert [r.detected for r in raw] == [0, 0, 0]
    R = g.spatial_covariance((re, im), N, nblk)
    w = g.beamformer_weights(R[0], None, mode="power_inversion")
    res = g.acquire(system, (re, im), fs, cols, num_samples=N, num_blocks=1, weights=w)
    print("beam:", [(r.prn, r.detected, round(r.peak_to_second, 3), r.carrier_doppler, r.code_phase, round(r.CN0, 1)) for r in res])
    assert [r.prn for r in res] == cols
    assert res[0].detected == 1
    assert abs(res[0].carrier_doppler - SCENE["dop"]) <= 500.0
    assert abs(((res[0].code_phase - SCENE["tau0"] + 511.5) % 1023.0) - 511.5) <= 0.5
    assert res[1].detected == 0 and res[2].detected == 0
    assert isinstance(w, torch.Tensor) and w.shape == (1, SCENE["M"])


# ---- 10: refusals and the Python surface ---------------------------------------------------------------------------------------
def test_refusals_leave_the_output_alone(g):
    import torch
    ctx = g.get_context()
    dev = ctx.device
    M, J, N, B = 4, 2, 256, 2
    sig = [torch.zeros(M * B * N + 64, dtype=torch.float32, device=dev) for _ in range(2)]
    out = [torch.full((J * B * N + 64,), SENTINEL, dtype=torch.float32, device=dev) for _ in range(2)]
    w_re = torch.ones((J, M), dtype=torch.float64, device=dev)
    w_im = torch.zeros_like(w_re)
    vp = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    SD = g._lib.SignalDesc

    def good_in(**kw):
        d = dict(re=sig[0].data_ptr(), im=sig[1].data_ptr(), layout=0, num_ants=M, num_samples=N, ant_stride=B * N, block_stride=N, chan_stride=0)
        d.update(kw)
        return SD(d["re"], d["im"], d["layout"], d["num_ants"], d["num_samples"], d["ant_stride"], d["block_stride"], d["chan_stride"])

    def good_out(**kw):
        d = dict(re=out[0].data_ptr(), im=out[1].data_ptr(), layout=0, num_ants=J, num_samples=N, ant_stride=B * N, block_stride=N, chan_stride=0)
        d.update(kw)
        return SD(d["re"], d["im"], d["layout"], d["num_ants"], d["num_samples"], d["ant_stride"], d["block_stride"], d["chan_stride"])

    def call(i=None, o=None, b=B, j=J, wr=w_re, wi=w_im, null_in=False, null_out=False):
        i = good_in() if i is None else i
        o = good_out() if o is None else o
        return ctx.lib.gat_beamform_samples(ctx._h, None if null_in else C.byref(i), b, vp(wr), vp(wi), j, None if null_out else C.byref(o))

    cases = [
        (call(null_in=True), ERR_ARG), (call(null_out=True), ERR_ARG), (call(wr=None), ERR_ARG), (call(wi=None), ERR_ARG),
        (call(i=good_in(re=None)), ERR_ARG), (call(o=good_out(re=None)), ERR_ARG),
        (call(b=0), ERR_ARG), (call(j=0, o=good_out(num_ants=0)), ERR_ARG),
        (call(i=good_in(ant_stride=-1)), ERR_ARG), (call(i=good_in(block_stride=-1)), ERR_ARG),
        (call(o=good_out(ant_stride=-1)), ERR_ARG), (call(o=good_out(block_stride=-1)), ERR_ARG),
        (call(i=good_in(num_ants=65)), ERR_RANGE), (call(j=65, o=good_out(num_ants=65)), ERR_RANGE),
        (call(o=good_out(num_ants=J + 1)), ERR_ARG), (call(o=good_out(num_samples=N - 1)), ERR_ARG),
        (call(o=good_out(layout=2, im=None)), ERR_UNSUPPORTED), (call(o=good_out(layout=3, im=None)), ERR_UNSUPPORTED),
        (call(i=good_in(chan_stride=8)), ERR_UNSUPPORTED), (call(o=good_out(chan_stride=8)), ERR_UNSUPPORTED),
        (call(o=good_out(im=None)), ERR_ARG), (call(o=good_out(layout=1)), ERR_ARG),
        # overlap: the output's real plane inside the input's, its imaginary plane inside the input's, touching from below by one element
        (call(o=good_out(re=sig[0].data_ptr() + 4 * N)), ERR_ARG), (call(o=good_out(im=sig[1].data_ptr())), ERR_ARG),
        (call(i=good_in(re=out[0].data_ptr() + 4 * (J * B * N - 1))), ERR_ARG),
        (call(i=good_in(im=out[1].data_ptr() + 4 * (J * B * N - 1))), ERR_ARG),
    ]
    for n, (rc, want) in enumerate(cases):
        assert rc == want, (n, rc, want)
    ctx.sync()
    for o in out:
        assert (o == SENTINEL).all()
    # the input ending exactly where the output begins is no overlap
    edge = torch.full((M * B * N + J * B * N,), SENTINEL, dtype=torch.float32, device=dev)
    rc = call(i=good_in(re=edge.data_ptr()), o=good_out(re=edge.data_ptr() + 4 * M * B * N))
    assert rc == OK
    # an interleaved output of the same geometry is accepted
    il = torch.full((J * B * N, 2), SENTINEL, dtype=torch.float32, device=dev)
    assert call(o=good_out(re=il.data_ptr(), im=None, layout=1)) == OK
    ctx.sync()


def test_python_surface(g):
    """beamform_samples on an interleaved int16 tensor with start = 5, a 1-D weight vector, interleaved=True, a padded output
    stride; acquire(weights=None) is the call without the argument"""
    import torch
    ctx = g.get_context()
    rng = np.random.default_rng(99)
    M, N, B, start = 4, 1000, 3, 5
    x = make_samples(rng, M, start + B * N, 2)
    sig = torch.from_numpy(np.stack([x.real, x.imag], axis=-1)).to(torch.int16).to(ctx.device)
    w = random_weights(rng, 1, M)[0]
    xs = x[:, start:]
    ref, bd = beam_ref.beams(xs, w[None], N, B), beam_ref.bound(xs, w[None], N, B)
    y_re, y_im = g.beamform_samples(sig, torch.from_numpy(w.astype(np.complex64)), N, B, start=start)
    assert y_re.shape == (1, B * N) and y_re.dtype == torch.float32
    w32 = w.astype(np.complex64).astype(np.complex128)
    ref32, bd32 = beam_ref.beams(xs, w32[None], N, B), beam_ref.bound(xs, w32[None], N, B)
    y = (y_re.cpu().numpy().astype(np.float64) + 1j * y_im.cpu().numpy()).reshape(1, B, N).transpose(1, 0, 2)
    assert (np.abs(y - ref32) <= bd32).all()
    il = g.beamform_samples(sig, torch.from_numpy(w), N, B, start=start, out_block_stride=N + 8, interleaved=True)
    assert il.shape == (1, B * (N + 8), 2)
    h = il.cpu().numpy().astype(np.float64).reshape(1, B, N + 8, 2)
    y = (h[..., :N, 0] + 1j * h[..., :N, 1]).transpose(1, 0, 2)
    assert (np.abs(y - ref) <= bd).all()
    assert (h[..., N:, :] == 0).all()  # the allocation's zeros between the blocks
    with pytest.raises(ValueError):
        g.beamform_samples(sig, torch.from_numpy(w[:-1]), N, B)
    with pytest.raises(ValueError):
        g.beamform_samples(sig, torch.from_numpy(w), N, B + 1, start=start)
    # acquire without weights is the existing call
    system = g.GPSL1()
    re, im, _, _ = scene(g, 1, 4.0)
    a = g.acquire(system, (re, im), SCENE["fs"], [6, 2], num_samples=SCENE["N"], keep_power=True)
    b = g.acquire(system, (re, im), SCENE["fs"], [6, 2], num_samples=SCENE["N"], keep_power=True, weights=None)
    import dataclasses
    for ra, rb in zip(a, b):
        for f in dataclasses.fields(ra):
            va, vb = getattr(ra, f.name), getattr(rb, f.name)
            if isinstance(va, torch.Tensor):
                assert torch.equal(va, vb), f.name
            elif isinstance(va, np.ndarray):
                assert np.array_equal(va, vb), f.name
            else:
                assert va == vb or (va != va and vb != vb), f.name
