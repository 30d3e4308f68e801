"""GPU tests of the antenna-array path (include/gat.h, "antenna-array processing"): the spatial covariance kernels against the
FP64 numpy reference (tests/array_ref.py), the device weights against their host twin, beamformed accumulators, a jammer nulled
end to end, and the beamformed tracking loop.

Where the nulling bounds come from: a numpy run of the scene below (4 antennas, N = 4000, a broadband jammer 30 to 50 dB over
the noise) showed covariances summed in float32 at two levels giving MVDR residuals within 0.01 dB of the FP64 ones (the 0.5 dB
asked for here is margin for summation order), and MVDR 38 dB below the conventional beamformer (the 25 dB asked for only
guards against a sign or conjugate slip)."""
import ctypes as C

import numpy as np
import pytest

import oracle
from tests import array_ref
from tests.helpers import check_close

pytestmark = pytest.mark.gpu

LAYOUTS = (0, 1, 2, 3)  # GAT_LAYOUT_PLANAR, _INTERLEAVED, _INTERLEAVED_I16, _INTERLEAVED_I8
VEC = {0: 4, 1: 2, 2: 4, 3: 8}  # samples one 16-byte load holds


@pytest.fixture(scope="module")
def g():
    import gpuacceleratedtracking_amd as g
    g.load_library()
    return g


# ---- spatial covariance -------------------------------------------------------------------------------------------------------
def make_samples(rng, M, ld, layout):
    """Correlated antennas (a common component under per-antenna noise, so that the off-diagonal elements carry signal), in
    the layout's number format.  Returns the values as complex128 [M, ld] exactly as stored."""
    common = rng.standard_normal(ld) + 1j * rng.standard_normal(ld)
    steer = np.exp(2j * np.pi * rng.uniform(0, 1, M))
    x = steer[:, None] * common[None, :] + 0.7 * (rng.standard_normal((M, ld)) + 1j * rng.standard_normal((M, ld)))
    if layout in (0, 1):
        return x.real.astype(np.float32).astype(np.float64) + 1j * x.imag.astype(np.float32).astype(np.float64)
    scale, lo, hi = (2000.0, -32768, 32767) if layout == 2 else (40.0, -128, 127)
    q = lambda v: np.clip(np.rint(v * scale), lo, hi)  # noqa: E731
    return q(x.real) + 1j * q(x.imag)


def run_covariance(g, x, layout, N, B, bpe, block_stride, offset=0, ant_pad=0, nan_ok=False):
    """x complex128 [M, ld] holding B blocks block_stride samples apart.  The device buffer puts antenna rows ld + ant_pad
    samples apart and starts `offset` samples into its allocation.  Two calls: returns the first result (complex128 [E, M, M])
    after asserting that the second one has the same bits and that the matrix is exactly Hermitian.  nan_ok: the samples
    hold a NaN on purpose, and NaN elements count as equal to their NaN mirror."""
    import torch
    ctx = g.get_context()
    dev = ctx.device
    M, ld = x.shape
    row = ld + ant_pad
    total = offset + M * row + 16
    if layout == 0:
        bufs = [torch.zeros(total, dtype=torch.float32, device=dev) for _ in range(2)]
        for buf, plane in zip(bufs, (x.real, x.imag)):
            buf[offset:offset + M * row].view(M, row)[:, :ld] = torch.from_numpy(plane.astype(np.float32)).to(dev)
        ptrs = (bufs[0].data_ptr() + 4 * offset, bufs[1].data_ptr() + 4 * offset)
    else:
        dt = {1: torch.float32, 2: torch.int16, 3: torch.int8}[layout]
        buf = torch.zeros((total, 2), dtype=dt, device=dev)
        pairs = torch.from_numpy(np.stack([x.real, x.imag], axis=-1)).to(dt).to(dev)
        buf[offset:offset + M * row].view(M, row, 2)[:, :ld] = pairs
        bufs = [buf]
        ptrs = (buf.data_ptr() + g.SAMPLE_BYTES[layout] * offset, None)
    desc = g._lib.SignalDesc(ptrs[0], ptrs[1], layout, M, N, row, block_stride, 0)
    E = -(-B // bpe)
    outs = []
    for _ in range(2):
        c_re = torch.full((E, M, M), 7.0, dtype=torch.float32, device=dev)
        c_im = torch.full((E, M, M), 7.0, dtype=torch.float32, device=dev)
        ctx.check(ctx.lib.gat_spatial_covariance(ctx._h, C.byref(desc), B, bpe, C.c_void_p(c_re.data_ptr()), C.c_void_p(c_im.data_ptr())),
                  "gat_spatial_covariance")
        ctx.sync()
        outs.append((c_re.cpu().numpy(), c_im.cpu().numpy()))
    (re0, im0), (re1, im1) = outs
    assert re0.tobytes() == re1.tobytes() and im0.tobytes() == im1.tobytes(), "a repeat call gave other bits"
    assert np.array_equal(re0, re0.transpose(0, 2, 1), equal_nan=nan_ok) and np.array_equal(im0, -im0.transpose(0, 2, 1), equal_nan=nan_ok), \
        "not exactly Hermitian"
    diag = im0[:, np.arange(M), np.arange(M)]
    assert (diag == 0).all() and not np.signbit(diag).any(), "the diagonal's imaginary part is not +0"
    return re0.astype(np.float64) + 1j * im0.astype(np.float64)


def check_covariance(got, ref, what):
    """element-wise by the project's metric (tests/helpers.py check_close: 1e-5 norm-wise per matrix and element-wise on the
    elements within a factor 10 of the largest)"""
    check_close(got[:, None], ref[:, None], what=what)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("M", (1, 2, 3, 4, 8, 16, 33, 64))
def test_covariance_matches_fp64_reference(g, M, layout):
    """every antenna count on every layout, aligned (M <= 8: the streaming kernel; else the LDS-tiled one): 5 blocks of
    2500 samples in estimates of 2 (the last estimate has one block), block stride padded to a whole 16-byte load"""
    rng = np.random.default_rng(100 * M + layout)
    N, B, bpe, S = 2500, 5, 2, 2504
    x = make_samples(rng, M, B * S, layout)
    got = run_covariance(g, x, layout, N, B, bpe, S)
    check_covariance(got, array_ref.covariance(x, N, B, bpe, S), f"M {M} layout {layout}")


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("N", (1, 2, 7, 255, 256, 4097, 20000))
def test_covariance_block_lengths(g, N, layout):
    """block lengths around the vector width and the workgroup's stride, 3 and 4 antennas, aligned block starts"""
    for M in (3, 4):
        rng = np.random.default_rng(7 * N + layout + M)
        B, bpe = 3, 3
        S = -(-N // 8) * 8
        x = make_samples(rng, M, B * S, layout)
        got = run_covariance(g, x, layout, N, B, bpe, S)
        check_covariance(got, array_ref.covariance(x, N, B, bpe, S), f"N {N} M {M} layout {layout}")


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("M", (2, 4, 16))
def test_covariance_misaligned_bases_and_odd_strides(g, M, layout):
    """the base one sample off a 16-byte boundary, odd antenna and block strides: the scalar-load path, no refusal"""
    rng = np.random.default_rng(31 * M + layout)
    N, B, bpe, S = 1001, 7, 3, 1003
    x = make_samples(rng, M, B * S, layout)
    got = run_covariance(g, x, layout, N, B, bpe, S, offset=1, ant_pad=(B * S + 1) % 2)
    check_covariance(got, array_ref.covariance(x, N, B, bpe, S), f"misaligned M {M} layout {layout}")
    # aligned base, odd block stride alone
    got = run_covariance(g, x, layout, N, B, bpe, S, offset=0, ant_pad=3)
    check_covariance(got, array_ref.covariance(x, N, B, bpe, S), f"odd strides M {M} layout {layout}")


@pytest.mark.parametrize("M,layout,offset", ((1, 0, 0), (4, 0, 0), (4, 1, 0), (2, 3, 0), (4, 2, 0), (4, 0, 1), (16, 0, 0)))
def test_covariance_of_one_long_block(g, M, layout, offset):
    """N = 2^21 in ONE block: the sums that a single running float32 sum misses 1e-5 on (streaming, scalar-load and tiled)"""
    rng = np.random.default_rng(2 ** 21 + M + layout)
    N = 2 ** 21
    x = make_samples(rng, M, N, layout)
    got = run_covariance(g, x, layout, N, 1, 1, N, offset=offset)
    check_covariance(got, array_ref.covariance(x, N, 1, 1), f"N 2^21 M {M} layout {layout} offset {offset}")


@pytest.mark.parametrize("M", (2, 4, 8, 16, 33))
@pytest.mark.parametrize("N", (1, 100, 256))
def test_covariance_is_exact_on_int8(g, M, N):
    """int8 pairs up to N = 256: |R_ij| <= 2 * 128^2 * 256 < 2^24, every sum is an integer float32 holds: exact, -128 included"""
    rng = np.random.default_rng(N + M)
    B, S = 3, 256
    x = rng.integers(-128, 128, (M, B * S)).astype(np.float64) + 1j * rng.integers(-128, 128, (M, B * S)).astype(np.float64)
    x[:, :2] = -128 - 128j
    x[0, 2] = 127 + 127j
    for offset in (0, 1):
        got = run_covariance(g, x, 3, N, B, 1, S, offset=offset)
        ref = array_ref.covariance(x, N, B, 1, S)
        assert np.array_equal(got, ref), (M, N, offset, np.abs(got - ref).max())


def test_covariance_python_surface_and_errors(g):
    """array.spatial_covariance on planar and interleaved tensors; the entry point's refusals"""
    import torch
    ctx = g.get_context()
    rng = np.random.default_rng(77)
    M, N, B = 4, 2000, 6
    x = make_samples(rng, M, B * N, 0)
    re = torch.from_numpy(x.real.astype(np.float32)).to(ctx.device)
    im = torch.from_numpy(x.imag.astype(np.float32)).to(ctx.device)
    R = g.spatial_covariance((re, im), N, B).cpu().numpy()
    assert R.shape == (1, M, M) and R.dtype == np.complex64
    check_covariance(R, array_ref.covariance(x, N, B, B), "python planar")
    il = torch.stack([re, im], dim=-1).contiguous()
    R4 = g.spatial_covariance(il, N, B, blocks_per_estimate=4).cpu().numpy()
    assert R4.shape == (2, M, M)
    check_covariance(R4, array_ref.covariance(x, N, B, 4), "python interleaved")
    desc = g._lib.SignalDesc(re.data_ptr(), im.data_ptr(), 0, M, N, B * N, N, 0)
    out = torch.empty((1, M, M), dtype=torch.float32, device=ctx.device)
    vp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    call = lambda d, b=B, e=B, o=out: ctx.lib.gat_spatial_covariance(ctx._h, C.byref(d), b, e, vp(o) if o is not None else None, vp(out))  # noqa: E731
    assert call(desc) == 0
    bad = g._lib.SignalDesc(re.data_ptr(), im.data_ptr(), 0, M, N, B * N, N, 8)
    assert call(bad) == 4  # chan_stride != 0: GAT_ERR_UNSUPPORTED
    bad = g._lib.SignalDesc(re.data_ptr(), im.data_ptr(), 0, 65, N, B * N, N, 0)
    assert call(bad) == 2  # more than 64 antennas
    bad = g._lib.SignalDesc(re.data_ptr(), None, 0, M, N, B * N, N, 0)
    assert call(bad) == 1  # planar without an imaginary plane
    assert call(desc, b=0) == 1 and call(desc, e=0) == 1 and call(desc, o=None) == 1
    ctx.sync()


# ---- weights and beamforming ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", (2, 4, 16, 64))
def test_device_weights_match_host_twin(g, M):
    import torch
    from tests.test_array_host import f32_cov, host_weights
    ctx = g.get_context()
    rng = np.random.default_rng(300 + M)
    K = 3
    a = np.exp(2j * np.pi * rng.uniform(0, 1, (K, M)))
    for jnr, sample in ((0.0, False), (50.0, False), (40.0, True)):
        R = f32_cov(array_ref.jammer_covariance(M, jnr, rng, snapshots=4000 if sample else None)[0])
        cov = torch.from_numpy(R.astype(np.complex64)).to(ctx.device)
        for mode, name in ((g.GAT_BF_MVDR, "mvdr"), (g.GAT_BF_POWER_INVERSION, "power_inversion"), (g.GAT_BF_CONVENTIONAL, "conventional")):
            for loading in (0.0, 1e-3):
                w = g.beamformer_weights(cov, torch.from_numpy(a).to(ctx.device), mode=name, loading=loading).cpu().numpy()
                rc, ref = host_weights(g, R, a, mode, loading)
                assert rc == 0 and w.shape == ref.shape and w.dtype == np.complex128
                err = np.linalg.norm(w - ref, axis=1) / np.linalg.norm(ref, axis=1)
                print(f"M {M} jammer {jnr} dB mode {name} loading {loading}: device vs host {err.max():.3e}")
                assert err.max() <= 1e-12, (name, loading, err)
    # not positive definite: NaN weights (the host twin answers GAT_ERR_RANGE)
    bad = R.copy()
    bad[M - 1, M - 1] = -1.0
    w = g.beamformer_weights(torch.from_numpy(bad.astype(np.complex64)).to(ctx.device), torch.from_numpy(a).to(ctx.device)).cpu().numpy()
    assert np.isnan(w).all()
    assert host_weights(g, bad, a, g.GAT_BF_MVDR)[0] == 2
    with pytest.raises(g.GatError):
        g.beamformer_weights(cov, torch.from_numpy(a).to(ctx.device), loading=-1.0)


@pytest.mark.parametrize("B,K,L,M", ((1, 1, 3, 4), (5, 3, 7, 16), (64, 12, 3, 64), (3, 2, 32, 33)))
def test_beamform_matches_numpy(g, B, K, L, M):
    import torch
    ctx = g.get_context()
    rng = np.random.default_rng(B + K + L + M)
    acc = ((rng.standard_normal((B, K, L, M)) + 1j * rng.standard_normal((B, K, L, M))) * 1000).astype(np.complex64)
    w = (rng.standard_normal((K, M)) + 1j * rng.standard_normal((K, M))) / M
    a_re = torch.from_numpy(np.ascontiguousarray(acc.real)).to(ctx.device)
    a_im = torch.from_numpy(np.ascontiguousarray(acc.imag)).to(ctx.device)
    y_re, y_im = g.beamform(a_re, a_im, torch.from_numpy(w).to(ctx.device))
    got = y_re.cpu().numpy().astype(np.float64) + 1j * y_im.cpu().numpy()
    assert got.shape == (B, K, L)
    check_close(got[..., None], array_ref.beamform(acc, w)[..., None], what="beamform")
    with pytest.raises(ValueError):
        g.beamform(a_re, a_im, torch.from_numpy(w[:, :-1]).to(ctx.device))


# ---- the scene: one satellite, unit noise, a broadband jammer 40 dB over it ---------------------------------------------------
SCENE = dict(N=4000, M=4, fs=4e6, fc=1.023e6, prn=7, dop=-2210.0, tau0=511.9, phi0=0.6, amp=4.0, jnr_db=40.0, seed=20240)


def scene_directions(seed):
    """steering phases (cycles) of the satellite and of the jammer"""
    rng = np.random.default_rng(seed)
    return rng.uniform(0, 1, SCENE["M"]), rng.uniform(0, 1, SCENE["M"])


def scene_interference(seed, nblk):
    """unit-power complex noise per antenna plus the jammer, from torch's CPU generator (the same numbers on every machine):
    complex64 [M, nblk * N] on the CPU"""
    import torch
    N, M = SCENE["N"], SCENE["M"]
    gen = torch.Generator().manual_seed(seed)
    noise = torch.randn((M, nblk * N, 2), generator=gen, dtype=torch.float32) * (0.5 ** 0.5)
    jam = torch.randn((nblk * N, 2), generator=gen, dtype=torch.float32) * (0.5 * 10.0 ** (SCENE["jnr_db"] / 10.0)) ** 0.5
    _, sj = scene_directions(seed)
    v = torch.from_numpy(np.exp(2j * np.pi * sj).astype(np.complex64))
    return torch.view_as_complex(noise) + v[:, None] * torch.view_as_complex(jam)[None, :]


def scene_signal(g, nblk):
    """the satellite from the library's generator (amplitude 4: 12 dB over the noise per antenna, its own steering vector) plus
    the interference.  Returns planar device tensors (re, im) [M, nblk * N], the interference alone (CPU complex64) and the
    satellite's steering vector."""
    import torch
    system = g.GPSL1()
    N, M, fs, fc = SCENE["N"], SCENE["M"], SCENE["fs"], SCENE["fc"]
    dop, tau0, phi0 = SCENE["dop"], SCENE["tau0"], SCENE["phi0"]
    fcode = fc * (1 + dop / 1575.42e6)
    b = np.arange(nblk, dtype=np.float64)[:, None]
    tau = np.mod(tau0 + fcode * (N / fs) * b, 1023.0)
    phi = np.mod(phi0 + dop * (N / fs) * b, 1.0)
    prm = g.make_params(SCENE["prn"] - 1, fcode, dop, tau, 2 * np.pi * phi, shape=(nblk, 1))
    ss, _ = scene_directions(SCENE["seed"])
    re, im = g.gen_signal_stream(system, prm, fs, N, M, amplitude=SCENE["amp"], steering_cycles=ss)
    x_in = scene_interference(SCENE["seed"], nblk)
    re = (re + x_in.real.to(re.device)).contiguous()
    im = (im + x_in.imag.to(im.device)).contiguous()
    return re, im, x_in, np.exp(2j * np.pi * ss.astype(np.float32).astype(np.float64))


def test_mvdr_nulls_the_jammer_end_to_end(g):
    """spatial_covariance -> beamformer_weights on the scene's first 8 blocks: the residual interference-plus-noise power
    w^H R_in w of the GPU weights is within 0.5 dB of the FP64 numpy MVDR's on the same samples, and at least 25 dB below the
    conventional beamformer's."""
    import torch
    nblk, N = 8, SCENE["N"]
    re, im, x_in, a = scene_signal(g, nblk)
    R = g.spatial_covariance((re, im), N, nblk)
    a_dev = torch.from_numpy(a).to(re.device)
    w = g.beamformer_weights(R[0], a_dev, mode="mvdr").cpu().numpy()[0]
    w_conv = g.beamformer_weights(None, a_dev, mode="conventional").cpu().numpy()[0]
    x = re.cpu().numpy().astype(np.float64) + 1j * im.cpu().numpy().astype(np.float64)
    R64 = array_ref.covariance(x, N, nblk, nblk)[0]
    check_covariance(R.cpu().numpy(), R64[None], "scene covariance")
    w64 = array_ref.weights(R64, a, 1)[0]
    xi = x_in.numpy().astype(np.complex128)
    R_in = xi @ xi.conj().T / xi.shape[1]
    resid = lambda v: float(np.real(np.conj(v) @ R_in @ v))  # noqa: E731
    d_ref = 10 * np.log10(resid(w) / resid(w64))
    d_conv = 10 * np.log10(resid(w_conv) / resid(w))
    print(f"residual: GPU MVDR vs FP64 MVDR {d_ref:+.4f} dB; conventional over MVDR {d_conv:.1f} dB")
    assert abs(np.conj(w) @ a - 1.0) <= 1e-12
    assert abs(d_ref) <= 0.5
    assert d_conv >= 25.0


def _lock(st, p, nblk):
    """the lock measures of test_closed_loop_single_satellite_converges: Doppler error (Hz), code-phase error (chips), the last
    PLL (cycles) and DLL (chips) discriminator outputs"""
    N, fs, fc = SCENE["N"], SCENE["fs"], SCENE["fc"]
    fcode = fc * (1 + SCENE["dop"] / 1575.42e6)
    tau_end = np.mod(SCENE["tau0"] + fcode * (N / fs) * nblk, 1023.0)
    dtau = abs(((p["code_phase_chips"][0] - tau_end + 511.5) % 1023.0) - 511.5)
    return (abs(st["carrier_doppler_hz"][0] - SCENE["dop"]), dtau, abs(st["last_pll_error_cycles"][0]), abs(st["last_dll_error_chips"][0]))


LOCK = (0.2, 0.02, 5e-3, 0.02)  # that test's thresholds on the four


def test_beamformed_loop_locks_where_the_plain_sum_does_not(g):
    """The scene over the 1500 blocks test_closed_loop_single_satellite_converges uses, the loop started 12 Hz and 0.12 chip
    off as there.  TrackingLoop(weights = MVDR from the first 8 blocks) meets that test's lock thresholds on Doppler, code
    phase and both discriminators; the unweighted loop on the same samples does not (the jammer is 28 dB over the
    satellite on every antenna, and the plain sum has no null).  Checked on the CPU beforehand with the FP64 restatement
    (oracle.np_correlate + array_ref.tracking_update_weighted on the same seed's samples): weighted
    7.8e-4 Hz, 5.9e-5 chip, 3.9e-4 cycle, 3.6e-4 chip -- locked; unweighted 26.8 Hz, 0.017 chip, 0.088 cycle, 0.30 chip -- not."""
    import torch
    nblk, N, M, fs = 1500, SCENE["N"], SCENE["M"], SCENE["fs"]
    system = g.GPSL1()
    re, im, _, a = scene_signal(g, nblk)
    R = g.spatial_covariance((re, im), N, 8)
    w = g.beamformer_weights(R[0], torch.from_numpy(a).to(re.device), mode="mvdr")
    shifts = g.get_correlator_sample_shifts(system, g.EarlyPromptLateCorrelator(M, 3), fs, 0.5)

    def run(weights):
        loop = g.TrackingLoop(system, np.array([SCENE["prn"]]), N, M, fs, shifts, init_carrier_doppler=np.array([SCENE["dop"] + 12.0]),
                              init_code_phase=np.array([SCENE["tau0"] + 0.12]), init_carrier_phase=0.0, dll_bandwidth_hz=4.0,
                              weights=weights)
        loop.run(re, im, nblk, keep=False)
        return _lock(loop.state(), loop.params().reshape(-1), nblk)

    weighted, plain = run(w), run(None)
    print("weighted loop:", weighted, "unweighted loop:", plain)
    assert all(v < t for v, t in zip(weighted, LOCK)), weighted
    assert not all(v < t for v, t in zip(plain, LOCK)), plain


def _small_scene(g, nblk):
    import torch
    system = g.GPSL1()
    N, M, fs = 4000, 4, 4e6
    prns = np.array([3, 11, 26])
    dop = np.array([850.0, -1400.0, 40.0])
    prm_sig = g.make_params(prns - 1, 1.023e6, dop, [[10.0, 400.5, 900.25]], 0.0, shape=(nblk, 3))
    rng = np.random.default_rng(12)
    re, im = g.gen_signal_stream(system, prm_sig, fs, N, M, steering_cycles=rng.uniform(0, 1, M), noise_sigma=0.5, seed=3)
    shifts = g.get_correlator_sample_shifts(system, g.EarlyPromptLateCorrelator(M, 3), fs, 0.5)
    w = torch.from_numpy((rng.standard_normal((3, M)) + 1j * rng.standard_normal((3, M))) / M)

    def make(weights=w):
        return g.TrackingLoop(system, prns, N, M, fs, shifts, init_carrier_doppler=dop + 5.0, init_code_phase=np.array([10.1, 400.4, 900.3]),
                              dll_bandwidth_hz=4.0, weights=weights)
    return re, im, make, N, M


def test_weighted_native_run_equals_stepwise_loop(g):
    """gat_tracking_run_weighted enqueues exactly the launches of step() x blocks: parameters, loop state and every block's
    accumulators are bit-identical; set_weights(None) is the unweighted loop, bit for bit."""
    nblk = 48
    re, im, make, N, M = _small_scene(g, nblk)
    a, b = make(), make()
    hist = []
    for i in range(nblk):
        a.step(re, im, start=i * N)
        hist.append(a.accumulators())
    acc_re, acc_im = b.run(re, im, nblk)
    got = (acc_re.cpu().numpy() + 1j * acc_im.cpu().numpy()).astype(np.complex64)
    assert np.array_equal(np.stack(hist).view(np.float32), got.view(np.float32))
    assert a.params().tobytes() == b.params().tobytes() and a.state().tobytes() == b.state().tobytes()
    plain = make(None)
    plain.run(re, im, nblk)
    assert plain.params().tobytes() != a.params().tobytes()  # the weights are used
    c = make()
    c.set_weights(None)
    c.run(re, im, nblk)
    assert c.params().tobytes() == plain.params().tobytes() and c.state().tobytes() == plain.state().tobytes()
    d = make(None)  # weights handed in later
    d.set_weights(a._w_re + 1j * a._w_im)
    for i in range(nblk):
        d.step(re, im, start=i * N)
    assert d.params().tobytes() == a.params().tobytes() and d.state().tobytes() == a.state().tobytes()


def test_weighted_graph_replay_equals_eager(g):
    """GAT_FLAG_GRAPH on the weighted run: replays equal the eager run bit for bit, and a weighted and an unweighted run over
    the same buffers do not share a recorded graph (the weight pointers are part of the key)."""
    import torch
    nblk = 32  # even: the ping-pong returns to buffer A after every call
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        re, im, make, N, M = _small_scene(g, nblk)
        eager, graph = make(), make()
        assert graph.ctx.stream.cuda_stream != 0
        out = (torch.empty((nblk, 3, 3, M), device=graph.ctx.device), torch.empty((nblk, 3, 3, M), device=graph.ctx.device))
        for rep in range(3):  # call 1 records, calls 2 and 3 replay
            e_re, e_im = eager.run(re, im, nblk)
            graph.run(re, im, nblk, graph=True, out=out)
            graph.ctx.sync()
            assert torch.equal(e_re, out[0]) and torch.equal(e_im, out[1]), rep
            assert eager.params().tobytes() == graph.params().tobytes() and eager.state().tobytes() == graph.state().tobytes()
        # the same loop object and buffers without weights: its own graph, the unweighted results
        eager.set_weights(None)
        graph.set_weights(None)
        for rep in range(2):
            e_re, e_im = eager.run(re, im, nblk)
            graph.run(re, im, nblk, graph=True, out=out)
            graph.ctx.sync()
            assert torch.equal(e_re, out[0]) and torch.equal(e_im, out[1]), rep
            assert eager.params().tobytes() == graph.params().tobytes() and eager.state().tobytes() == graph.state().tobytes()
