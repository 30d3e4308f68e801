"""The sample spectrum's host twin (gat_sample_spectrum_host) and the tone detector of gpuacceleratedtracking_amd/spectrum.py,
without a device: the twin against the FP64 restatement (tests/spec_ref.py) within the derived bound, the exact known answers,
the invariance of the bits under the partition of a block into one-segment blocks, every refusal with the output untouched, NaN
samples, and find_tones on host-twin spectra of tones in noise."""

import numpy as np
import pytest

from tests import spec_ref as ref
from tests.spec_ref import CF32, I8, I16, LAYOUTS, PLANAR, same_bits

ARG, RANGE, UNSUPPORTED = 1, 2, 4


@pytest.fixture(scope="module")
def sp():
    import gpuacceleratedtracking_amd as g
    g.load_library()
    return g.spectrum


HOPS = {"F": lambda F: F, "F/2": lambda F: F // 2, "F/4+4": lambda F: F // 4 + 4, "7": lambda F: 7, "1": lambda F: 1}


@pytest.mark.parametrize("hop", list(HOPS))
@pytest.mark.parametrize("F", [64, 128, 1024, 4096])
def test_host_twin_within_the_bound_of_the_fp64_restatement(sp, F, hop):
    """|power - power64| <= sum_s [(2 A + E) E + 2u(1 + u)(A + E)^2] + (S - 1)u / (1 - (S - 1)u) sum_s (A + E)^2 (1 + 2u(1 + u)) per bin, E =
    (11 log2 F + 1) u A, A = sum_n |w[n]| (|x_re| + |x_im|) of a segment: all four layouts -- random data at
    float (sigma 40), int16 and int8 full scale --, one and three antennas, two blocks on strides of their own, one sample off
    the buffers' start.  The bound is a worst case over the phases of F terms; random data adds like sqrt(F) of them, and the
    measured fractions printed here are 1e-3 and below (test_a_tone_on_a_bin_centre... has the case the bound is made for)."""
    H = HOPS[hop](F)
    N = F + 5 if hop == "1" else 2 * H + F + min(3, H - 1)
    rng = np.random.default_rng(F + H)
    for k, layout in enumerate(LAYOUTS):
        M = (1, 3)[(k + F // 64 + H) % 2]
        xr, xi = ref.random_samples(rng, layout, (2, M, N), special=False)
        w = ref.window(("hann", "blackman", "hamming", "rect")[k], F)
        got = ref.host_spectrum(sp, layout, xr, xi, w, F, H, block_stride=N + 3, ant_stride=2 * (N + 3) + 1, offset=1)
        want, _, A = ref.spectrum(xr, xi, w, F, H)
        lim = ref.bound_power(F, A)[..., None]
        worst = float((np.abs(got - want) / lim).max())
        print(f"F {F} H {H} layout {layout} M {M} S {A.shape[-1]}: worst error over its bound {worst:.2e}, relative to the largest bin {np.abs(got - want).max() / want.max():.2e}")
        assert worst <= 1.0
        assert np.abs(got - want).max() <= 1e-5 * want.max()  # and the north star's relative error next to the largest bin


@pytest.mark.parametrize("F", [64, 1024, 4096])
def test_a_tone_on_a_bin_centre_fills_the_bound_it_is_made_for(sp, F):
    """a unit-modulus tone on bin 5 under the rectangular window: |X[5]| = F is the A / sqrt(2) .. A the bound is stated in, so here
    the bound is 1e-5 of the answer and the check is a sharp one"""
    n = np.arange(2 * F, dtype=np.float64)
    x = 1000.0 * np.exp(2j * np.pi * (5.0 / F * n + 0.1))
    xr, xi = x.real.astype(np.float32)[None, None], x.imag.astype(np.float32)[None, None]
    w = ref.window("rect", F)
    got = ref.host_spectrum(sp, PLANAR, xr, xi, w, F, F // 2)
    want, _, A = ref.spectrum(xr, xi, w, F, F // 2)
    lim = ref.bound_power(F, A)[..., None]
    worst = float((np.abs(got - want) / lim).max())
    print(f"F {F}: worst error over its bound {worst:.3f}; the bound is {float(lim.max() / want.max()):.2e} of the largest bin")
    assert worst <= 1.0 and want.max() > 1e4 * lim.max()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("F,H,S", [(64, 64, 1), (256, 100, 7), (4096, 4096, 2)])
def test_the_constant_one_under_the_rectangular_window_is_exact(sp, layout, F, H, S):
    """power[0] = S F^2 and every other bin exactly 0: the twiddle at i = 0 is exactly (1, -0), every butterfly adds equal values or
    subtracts them to 0, and every other twiddle multiplies a zero"""
    N = (S - 1) * H + F + 2
    x = np.ones((1, 2, N), ref.DTYPE[layout])
    got = ref.host_spectrum(sp, layout, x, np.zeros_like(x), ref.window("rect", F), F, H)
    assert (got[..., 0] == np.float32(S * F * F)).all() and (got[..., 1:] == 0).all()


@pytest.mark.parametrize("F", [64, 512, 4096])
def test_a_unit_impulse_gives_a_flat_spectrum(sp, F):
    """x = 1 at n = 0 of every segment (H = F): every bin holds w[0]^2 S, up to the bound (the values are small integers times
    w[0]^2 through every stage, so in fact exactly)"""
    S = 3
    xr = np.zeros((1, 1, S * F), np.float32)
    xr[0, 0, ::F] = 1.0
    w = np.full(F, 0.75, np.float32)
    got = ref.host_spectrum(sp, PLANAR, xr, np.zeros_like(xr), w, F, F)
    _, _, A = ref.spectrum(xr, np.zeros_like(xr), w, F, F)
    assert (np.abs(got - 0.75 ** 2 * S) <= ref.bound_power(F, A)[..., None]).all()
    assert (got == np.float32(0.75 ** 2 * S)).all()


@pytest.mark.parametrize("layout,F,H,S", [(PLANAR, 64, 7, 9), (I8, 1024, 512, 5), (I16, 256, 256, 4), (CF32, 4096, 1032, 3)])
def test_a_block_is_the_float32_sum_in_order_of_its_one_segment_blocks(sp, layout, F, H, S):
    """partition invariance: S one-segment blocks described over the same memory (block_stride = H, N = F: a spectrogram), added
    in float32 in segment order from +0, are the block of S segments bit for bit"""
    from gpuacceleratedtracking_amd.frontend import host_desc
    rng = np.random.default_rng(S)
    N, M = (S - 1) * H + F + min(2, H - 1), 2
    xr, xi = ref.random_samples(rng, layout, (1, M, N), special=False)
    buf = ref.make_buffers(layout, 1, M, N, N + 1, 0)
    ref.put(buf, layout, ref.index(1, M, N, N + 1, 0), xr, xi)
    im = buf[1] if layout == PLANAR else None
    w = ref.window("hann", F)
    whole, parts = np.zeros((1, M, F), np.float32), np.zeros((S, M, F), np.float32)
    assert sp.sample_spectrum_host(host_desc(buf[0], im, layout, M, N, N + 1, 0), 1, w, F, H, whole) == 0
    assert sp.sample_spectrum_host(host_desc(buf[0], im, layout, M, F, N + 1, H), S, w, F, H, parts) == 0
    acc = np.zeros((M, F), np.float32)
    for s in range(S):
        acc = acc + parts[s]
    assert acc.dtype == np.float32 and same_bits(acc, whole[0])


def test_every_refusal_leaves_the_output_untouched(sp):
    from gpuacceleratedtracking_amd import _lib
    from gpuacceleratedtracking_amd.frontend import host_desc
    F, H, M, B = 64, 16, 2, 2
    N = F + 3 * H
    x = np.zeros((M * B * N + 8, 2), np.float32)
    planes = (np.zeros(M * B * N, np.float32), np.zeros(M * B * N, np.float32))
    out = np.full((B, M, F), -3.25, np.float32)
    w = np.ones(F, np.float32)

    def desc(**kw):
        d = host_desc(x, None, CF32, M, N, B * N, N)
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    def cfg(F=F, H=H, flags=0, size=None):
        c = sp._config(F, H, flags)
        if size is not None:
            c.struct_size = size
        return c

    def call(d="default", nb=B, window=w, c=None, o=out):
        return sp.sample_spectrum_host(desc() if isinstance(d, str) else d, nb, window, F, H, o, config=cfg() if c is None else c)

    S_MAX = _lib.GAT_MAX_SPECTRUM_SEGMENTS
    inside = np.frombuffer(x.data, np.float32, B * M * F, 64)  # an output inside the input's bytes
    cases = [
        (ARG, dict(d=None)), (ARG, dict(window=None)), (ARG, dict(o=None)), (ARG, dict(c=cfg(size=12))), (ARG, dict(c=cfg(size=24))),
        (ARG, dict(nb=0)), (ARG, dict(nb=-1)), (ARG, dict(c=cfg(flags=1))), (ARG, dict(c=cfg(flags=1 << 31))),
        (ARG, dict(d=desc(num_samples=0))), (ARG, dict(d=desc(num_ants=0))), (ARG, dict(d=desc(ant_stride=-1))), (ARG, dict(d=desc(block_stride=-1))),
        (ARG, dict(d=desc(ant_stride=0))), (ARG, dict(d=desc(block_stride=0))), (ARG, dict(d=desc(layout=4))), (ARG, dict(d=desc(layout=-1))),
        (ARG, dict(d=desc(im=planes[1].ctypes.data))), (ARG, dict(d=host_desc(planes[0], None, PLANAR, M, N, B * N, N))),
        (ARG, dict(d=desc(num_samples=F - 1))), (ARG, dict(o=inside)),
        (RANGE, dict(c=cfg(F=32))), (RANGE, dict(c=cfg(F=96))), (RANGE, dict(c=cfg(F=8192))), (RANGE, dict(c=cfg(F=0))), (RANGE, dict(c=cfg(F=-64))),
        (RANGE, dict(c=cfg(H=0))), (RANGE, dict(c=cfg(H=F + 1))), (RANGE, dict(c=cfg(H=-1))),
        (RANGE, dict(d=desc(num_samples=F + S_MAX, block_stride=1, ant_stride=1), c=cfg(H=1))),  # S = 4097 (refused before anything is read)
        (RANGE, dict(d=desc(num_ants=65, ant_stride=1))),
        (UNSUPPORTED, dict(d=desc(chan_stride=8))),
    ]
    for code, kw in cases:
        assert call(**kw) == code, kw
        assert (out == -3.25).all(), kw
    # the limits themselves pass: S = 4096 of hop 1, and an output that ends where the input begins
    big = np.zeros((F + S_MAX - 1, 2), np.float32)
    o1 = np.full((1, 1, F), -3.25, np.float32)
    assert sp.sample_spectrum_host(host_desc(big, None, CF32, 1, F + S_MAX - 1, 0, 0), 1, w, F, 1, o1) == 0 and (o1 == 0).all()
    assert call() == 0 and (out == 0).all()


def test_a_nan_sample_poisons_exactly_the_segments_that_hold_it(sp):
    """a spectrogram (one-segment blocks every H samples) of a stream with one NaN: the blocks whose F samples hold it are NaN
    in every bin -- under the Hann window too, whose w[0] = 0 meets it in one of them: 0 * NaN is NaN --, every other block has
    the clean stream's bits; an inf sample does the same except under a zero window value, where it is NaN just the same"""
    from gpuacceleratedtracking_amd.frontend import host_desc
    rng = np.random.default_rng(2)
    F, H, S = 128, 32, 12
    N = (S - 1) * H + F
    xr, xi = ref.random_samples(rng, PLANAR, (1, 1, N), special=False)
    w = ref.window("hann", F)
    clean = np.zeros((S, 1, F), np.float32)
    assert sp.sample_spectrum_host(host_desc(xr.reshape(-1), xi.reshape(-1), PLANAR, 1, F, N, H), S, w, F, H, clean) == 0
    assert np.isfinite(clean).all()
    for pos, bad in ((5 * H, np.nan), (5 * H, np.inf), (7 * H + 3, -np.inf), (N - 1, np.nan)):
        dr = xr.copy()
        dr[0, 0, pos] = bad
        got = np.zeros((S, 1, F), np.float32)
        assert sp.sample_spectrum_host(host_desc(dr.reshape(-1), xi.reshape(-1), PLANAR, 1, F, N, H), S, w, F, H, got) == 0
        holds = np.array([s * H <= pos < s * H + F for s in range(S)])
        assert holds.any() and not holds.all()
        assert not np.isfinite(got[holds]).any() and (np.isnan(got[holds]).all() or not np.isnan(bad))
        assert same_bits(got[~holds], clean[~holds])
        whole = np.zeros((1, 1, F), np.float32)  # and the block of all segments, which sums them
        assert sp.sample_spectrum_host(host_desc(dr.reshape(-1), xi.reshape(-1), PLANAR, 1, N, N, 0), 1, w, F, H, whole) == 0
        assert not np.isfinite(whole).any()


def test_named_windows_are_the_periodic_forms_narrowed_once(sp):
    for name in sp.WINDOWS:
        for F in (64, 1024):
            w = sp.window_values(name, F)
            assert w.dtype == np.float32 and same_bits(w, ref.window(name, F))
            if name != "rect":
                assert same_bits(w[1:], w[1:][::-1].copy()) and w[F // 2] == w.max()  # periodic: w[n] = w[F - n]
    assert sp.window_values(np.arange(64.0), 64).dtype == np.float32
    with pytest.raises(ValueError):
        sp.window_values("kaiser", 64)
    with pytest.raises(ValueError):
        sp.window_values(np.ones(63), 64)


def test_stream_partition_covers_every_segment_once(sp):
    for total, F, H, M, want in [(40000, 1024, 512, 2, 2048), (40000, 1024, 512, 2, 8), (1 << 24, 64, 1, 1, 1), (1024, 1024, 512, 64, 2048), (5000, 64, 7, 3, 40)]:
        S_total, S_block, B, S_rest = sp.stream_partition(total, F, H, M, want)
        assert S_total == (total - F) // H + 1 and B >= 1 and 1 <= S_block <= 4096 and 0 <= S_rest < S_block
        assert B * S_block + S_rest == S_total
        assert B * S_block * H + ((S_rest - 1) * H + F if S_rest else F - H) <= total  # the last segment ends inside the stream


# ---- find_tones on host-twin spectra ----------------------------------------------------------------------------------------------
def mean_spectrum(sp, xr, xi, s=ref.TONE_SCENE):
    """float64 [M, F]: the twin's sums over the scene as one block, divided by the segment count"""
    F, H = s["F"], s["H"]
    out = ref.host_spectrum(sp, PLANAR, xr, xi, ref.window("hann", F), F, H)
    return out[0].astype(np.float64) / ref.num_segments(s["N"], F, H)


def wrapped(d):
    return (d + 0.5) % 1.0 - 0.5


@pytest.mark.parametrize("amp", ref.TONE_AMPS)
@pytest.mark.parametrize("nu", ref.TONE_NUS)
def test_find_tones_places_a_tone_within_a_twentieth_of_a_bin(sp, nu, amp):
    """Two antennas x 40000 samples of noise, sigma = 14.13, and one tone; F = 1024, H = 512, Hann: 77 segments.  The tone is 40,
    17 or 7 dB over the noise power in the band (amplitude 1997.6, 141.3, 44.7), on a bin centre's neighbourhood, between two
    bins (nu F = 159.03, 0.50002), at a negative frequency (-0.31207) and at the band's edge (0.4999).  A numpy FP64 forecast
    of exactly this gave errors <= 0.0003 bin and peaks 34 - 68 dB over the median; the twin on this file's noise (seed 11) gives
    0.00001 - 0.0015 bin and 33.9 - 68.4 dB: the limit of 0.05 bin leaves more than an order."""
    F = ref.TONE_SCENE["F"]
    xr, xi = ref.tone_scene([(nu, amp, 0.3)])
    tones = sp.find_tones(mean_spectrum(sp, xr, xi))
    print(f"nu {nu} amplitude {amp}: {tones}")
    assert len(tones) == 1
    err_bins = abs(wrapped(tones[0][0] - nu)) * F
    print(f"   error {err_bins:.5f} bin, {tones[0][1]:.1f} dB over the median")
    assert err_bins <= 0.05 and -0.5 <= tones[0][0] < 0.5 and tones[0][1] > 30.0


def test_find_tones_finds_nothing_in_noise(sp):
    """the scene without a tone, three noise seeds: nothing at the default 10 dB.  The forecast's largest bin (mean of 77 segments
    x 2 antennas summed, 1024 bins) lay 1.2 dB over the median (these seeds: 1.08 - 1.15 dB); the threshold leaves 8 dB"""
    for seed in (11, 12, 13):
        xr, xi = ref.tone_scene([], seed=seed)
        psd = mean_spectrum(sp, xr, xi)
        p = psd.sum(axis=0)
        print(f"seed {seed}: largest bin {10 * np.log10(p.max() / np.median(p)):.2f} dB over the median")
        assert sp.find_tones(psd) == []
        assert 10 * np.log10(p.max() / np.median(p)) < 3.0


def test_find_tones_finds_two_tones_strongest_first(sp):
    F = ref.TONE_SCENE["F"]
    xr, xi = ref.tone_scene([(0.155, 141.3, 0.3), (-0.31207, 1997.6, 0.7)])
    tones = sp.find_tones(mean_spectrum(sp, xr, xi))
    print(tones)
    assert len(tones) == 2 and tones[0][1] > tones[1][1]
    assert abs(wrapped(tones[0][0] + 0.31207)) * F <= 0.05 and abs(wrapped(tones[1][0] - 0.155)) * F <= 0.05
    # one tone allowed: the stronger; a window that is not Hann: the bin centre
    assert len(sp.find_tones(mean_spectrum(sp, xr, xi), max_tones=1)) == 1
    centre = sp.find_tones(mean_spectrum(sp, xr, xi), window="rect")
    assert [round(t[0] * F) for t in centre] == [round(-0.31207 * F), round(0.155 * F)] and all(float(t[0] * F).is_integer() for t in centre)
