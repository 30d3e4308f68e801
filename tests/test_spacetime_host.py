"""Space-time adaptive processing without a device: the package's surface, the filter's host twin (gat_spacetime_filter_host)
against the FP64 restatement (tests/st_ref.py) within the documented bound over every layout pair, exact answers, the invariance of
the bits under the partition of a stream into overlap-save blocks, every refusal with the output untouched, NaN propagation, one
tap against the beamformer's restatement, and the jammed scene in FP64 and with the twin."""
import numpy as np
import pytest

from tests import beam_ref
from tests import fir_ref as lay
from tests import st_ref as ref
from tests.fir_ref import CF32, I8, I16, LAYOUTS, OUT_LAYOUTS, PLANAR

ARG, RANGE, UNSUPPORTED = 1, 2, 4
MT = [(1, 1), (1, 16), (2, 5), (3, 3), (4, 7), (4, 16), (7, 9), (13, 4), (64, 1)]


@pytest.fixture(scope="module")
def g():
    import gpuacceleratedtracking_amd as g
    g.load_library()
    return g


def host_case(g, rng, li, lo, B, M, N, T, J, pad_in=0, pad_out=0, off_in=0, off_out=0, in_stride=None, small=False):
    """random samples in layout li -- B blocks of N every in_stride samples: overlapping where in_stride < N, and then block b
    continues block b - 1 --, an output of layout lo for J beams full of sentinels, and the two descriptors; x: the stream as
    complex128 [M, span]"""
    No = N - T + 1
    ibs = N + pad_in if in_stride is None else in_stride
    span = (B - 1) * ibs + N
    ias, obs = span + pad_in, No + pad_out
    oas = B * obs + pad_out
    if small:
        sr, si = (rng.integers(-9, 10, (M, span)).astype(lay.DTYPE[li]) for _ in range(2))
    else:
        sr, si = lay.random_samples(rng, li, (M, span), special=False)
    ibuf = lay.make_buffers(li, 1, M, span, ias, 0, off_in)
    lay.put(ibuf, li, lay.index(1, M, span, ias, 0, off_in), sr[None], si[None])
    obuf = lay.make_buffers(lo, B, J, No, oas, obs, off_out, fill=-3.25)
    oidx = lay.index(B, J, No, oas, obs, off_out)
    idesc = g.spacetime.host_desc(ibuf[0], ibuf[1] if li == PLANAR else None, li, M, N, ias, ibs, off_in)
    odesc = g.spacetime.host_desc(obuf[0], obuf[1] if lo == PLANAR else None, lo, J, No, oas, obs, off_out)
    x = sr.astype(np.float64) + 1j * si.astype(np.float64)
    return dict(x=x, ibuf=ibuf, obuf=obuf, oidx=oidx, idesc=idesc, odesc=odesc, No=No, ibs=ibs, B=B, lo=lo, N=N, T=T)


def host_output(c):
    yr, yi = lay.get(c["obuf"], c["lo"], c["oidx"])
    return yr.astype(np.float64) + 1j * yi.astype(np.float64)


def random_weights(rng, J, Q):
    return (rng.standard_normal((J, Q)) + 1j * rng.standard_normal((J, Q))) / np.sqrt(Q)


def test_the_surface():
    """the entry points are declared, bound and exported (on the parent commit none of them exists)"""
    import gpuacceleratedtracking_amd as g
    from gpuacceleratedtracking_amd import _lib
    lib = g.load_library()
    for name in ("gat_spacetime_covariance", "gat_spacetime_filter", "gat_spacetime_filter_host"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    for name in ("spacetime_covariance", "spacetime_steering", "spacetime_weights", "spacetime_filter", "spacetime_filter_host",
                 "spacetime_stream", "spacetime_delay"):
        assert callable(getattr(g, name))
    assert _lib.GAT_MAX_ST_TAPS == 16
    assert g.spacetime_delay(5, 2) == 2 and g.spacetime_delay(1, 0) == 0
    with pytest.raises(ValueError):
        g.spacetime_delay(5, 5)
    a = g.spacetime_steering(np.array([1.0, 2j]), 3, 1)
    assert a.shape == (1, 6) and np.array_equal(a.numpy()[0], np.array([0, 0, 1.0, 2j, 0, 0]))
    assert g.spacetime.stream_blocks(124, 5, 3) == (44, 40, 40, 3, 120)


# every (M, T) with every N of the issue; the layout pairs, B, overlapping blocks and misaligned bases are dealt over the cases
# so that within each (M, T) every input layout meets both output layouts, and both B occur
PAIRS = [(li, lo) for li in LAYOUTS for lo in OUT_LAYOUTS]


def _deal(i):
    li, lo = PAIRS[i % 8]
    return li, lo, (1, 3)[(i // 3) % 2], i % 3 == 1, (i // 2) % 2


@pytest.mark.parametrize("M,T", MT)
def test_host_twin_within_the_bound_of_the_fp64_restatement(g, M, T):
    """|y - y64| <= (4Q + 4) 2^-24 sum_q |w_q| |z_q| per sample"""
    rng = np.random.default_rng(100 * M + T)
    Q, seen = M * T, set()
    sizes = sorted({T, T + 1, 2 * T - 1, 37, 257})
    for rep in range(2):
        for k, N in enumerate(sizes):
            li, lo, B, overlap, mis = _deal(k + len(sizes) * rep + M)
            seen.add((li, lo))
            J = (1, 3, 4, 5)[(k + rep) % 4]
            No = N - T + 1
            c = host_case(g, rng, li, lo, B, M, N, T, J, pad_in=3 * mis, pad_out=mis, off_in=mis, off_out=2 * mis, in_stride=No if overlap else None)
            w = random_weights(rng, J, Q)
            before = lay.guard_of(c["obuf"])
            assert g.spacetime_filter_host(c["idesc"], B, w, T, c["odesc"]) == 0
            want = ref.filt(c["x"], w, N, B, T, c["ibs"])
            lim = ref.bound(c["x"], w, N, B, T, c["ibs"])
            got = host_output(c)
            worst = float((np.abs(got - want) / lim).max())
            print(f"M {M} T {T} N {N} B {B} J {J} layouts {li}->{lo}: worst error over its bound {worst:.3f}")
            assert worst <= 1.0
            assert lay.unchanged_outside(c["obuf"], before, lo, c["oidx"])
    assert len(seen) == 8  # all four input layouts met both output layouts


def test_an_impulse_returns_the_conjugate_weights_and_small_integers_are_exact(g):
    rng = np.random.default_rng(3)
    M, T, N, J, m0, p = 3, 5, 40, 2, 1, 17
    Q = M * T
    w = (rng.integers(-8, 9, (J, Q)) + 1j * rng.integers(-8, 9, (J, Q))).astype(np.complex128)
    xr, xi = np.zeros((M, N), np.float32), np.zeros((M, N), np.float32)
    xr[m0, p] = 1.0
    No = N - T + 1
    o = [np.zeros((J, No), np.float32), np.zeros((J, No), np.float32)]
    assert g.spacetime_filter_host(g.spacetime.host_desc(xr, xi, PLANAR, M, N, N, N), 1, w, T, g.spacetime.host_desc(o[0], o[1], PLANAR, J, No, No, No)) == 0
    y = o[0] + 1j * o[1]
    want = np.zeros((J, No), np.complex128)
    for t in range(T):  # output n' holds the impulse at tap t = n' + T - 1 - p: the antenna's taps, newest tap first
        want[:, p - (T - 1) + t] = w[:, t * M + m0].conj()
    assert np.array_equal(y, want)
    # small integers, integer weights: every partial sum is an integer below 2^24
    for li in LAYOUTS:
        c = host_case(g, rng, li, CF32, 2, M, 33, T, J, small=True)
        assert g.spacetime_filter_host(c["idesc"], 2, w, T, c["odesc"]) == 0
        assert np.array_equal(host_output(c), ref.filt(c["x"], w, 33, 2, T, c["ibs"]))


def test_every_partition_of_a_stream_gives_the_same_bits(g):
    """one stream of 124 samples, 120 outputs, cut into 1, 3 and 8 overlap-save blocks by the geometry spacetime_stream uses"""
    rng = np.random.default_rng(4)
    M, T, J, total = 2, 5, 3, 124
    sr, si = lay.random_samples(rng, PLANAR, (M, total), special=False)
    w = random_weights(rng, J, M * T)
    outs = []
    for B in (1, 3, 8):
        N, stride, Qout, nb, total_out = g.spacetime.stream_blocks(total, T, B)
        assert total_out == 120 and nb == B
        o = [np.zeros((J, total_out), np.float32), np.zeros((J, total_out), np.float32)]
        idesc = g.spacetime.host_desc(sr, si, PLANAR, M, N, total, stride)
        odesc = g.spacetime.host_desc(o[0], o[1], PLANAR, J, Qout, total_out, Qout)
        assert g.spacetime_filter_host(idesc, B, w, T, odesc) == 0
        outs.append(o)
    for o in outs[1:]:
        assert lay.same_bits(o[0], outs[0][0]) and lay.same_bits(o[1], outs[0][1])
    assert np.abs(outs[0][0]).max() > 0


def test_refusals_leave_the_output_untouched(g):
    rng = np.random.default_rng(5)
    M, T, N, J, B = 2, 4, 30, 2, 2
    c = host_case(g, rng, PLANAR, PLANAR, B, M, N, T, J, pad_in=1, pad_out=1)
    w = random_weights(rng, J, M * T)
    w_re, w_im = np.ascontiguousarray(w.real), np.ascontiguousarray(w.imag)
    before = lay.guard_of(c["obuf"])

    def refused(code, desc=None, odesc=None, weights=(w_re, w_im), taps=T, beams=J, blocks=B):
        i = c["idesc"] if desc is None else desc
        o = c["odesc"] if odesc is None else odesc
        rc = g.spacetime_filter_host(None if i == "null" else i, blocks, weights, taps, None if o == "null" else o, num_beams=beams)
        assert rc == code, (rc, code)
        assert all(lay.same_bits(a, b) for a, b in zip(c["obuf"], before))

    def edit(d, **kw):
        e = type(d).from_buffer_copy(d)
        for k, v in kw.items():
            setattr(e, k, v)
        return e

    refused(ARG, desc="null")
    refused(ARG, odesc="null")
    refused(ARG, weights=(None, w_im))
    refused(ARG, weights=(w_re, None))
    refused(ARG, blocks=0)
    refused(ARG, beams=0)
    refused(RANGE, taps=0)
    refused(RANGE, taps=17)
    refused(RANGE, beams=65, odesc=edit(c["odesc"], num_ants=65))
    # M * T above 64: 5 antennas (a descriptor of the same memory with a smaller stride) x 13 taps
    refused(RANGE, desc=edit(c["idesc"], num_ants=5, ant_stride=1), taps=13, odesc=edit(c["odesc"], num_samples=N - 12))
    refused(ARG, desc=edit(c["idesc"], num_samples=T - 1), odesc=edit(c["odesc"], num_samples=1))  # N < T
    refused(ARG, odesc=edit(c["odesc"], num_samples=N - T + 2))
    refused(ARG, odesc=edit(c["odesc"], num_samples=N))
    refused(ARG, odesc=edit(c["odesc"], num_ants=J + 1))
    refused(ARG, odesc=edit(c["odesc"], im=None))
    refused(ARG, odesc=edit(c["odesc"], block_stride=-1))
    refused(ARG, odesc=edit(c["odesc"], ant_stride=0))
    refused(ARG, desc=edit(c["idesc"], layout=7))
    refused(ARG, desc=edit(c["idesc"], ant_stride=0))
    refused(UNSUPPORTED, odesc=edit(c["odesc"], layout=I16, im=None))
    refused(UNSUPPORTED, odesc=edit(c["odesc"], layout=I8, im=None))
    refused(UNSUPPORTED, desc=edit(c["idesc"], chan_stride=8))
    refused(UNSUPPORTED, odesc=edit(c["odesc"], chan_stride=8))
    refused(ARG, odesc=edit(c["odesc"], re=c["idesc"].re))  # the output overlaps the input
    # and the accepted call writes
    assert g.spacetime_filter_host(c["idesc"], B, (w_re, w_im), T, c["odesc"], num_beams=J) == 0
    assert not lay.same_bits(c["obuf"][0], before[0])


def test_nan_propagates(g):
    """one NaN sample reaches exactly the outputs whose snapshot holds it, on every beam; one NaN weight row makes that beam NaN"""
    rng = np.random.default_rng(6)
    M, T, N, J = 2, 4, 50, 3
    No = N - T + 1
    sr, si = lay.random_samples(rng, PLANAR, (M, N), special=False)
    w = random_weights(rng, J, M * T)

    def run(xr, xi, ww):
        o = [np.zeros((J, No), np.float32), np.zeros((J, No), np.float32)]
        assert g.spacetime_filter_host(g.spacetime.host_desc(xr, xi, PLANAR, M, N, N, N), 1, ww, T, g.spacetime.host_desc(o[0], o[1], PLANAR, J, No, No, No)) == 0
        return ~np.isfinite(o[0]) | ~np.isfinite(o[1])

    xr = sr.copy()
    xr[1, 20] = np.nan
    n = np.arange(No)
    hit = (n <= 20) & (20 <= n + T - 1)
    assert np.array_equal(run(xr, si, w), np.broadcast_to(hit, (J, No)))
    w2 = w.copy()
    w2[1, :] = np.nan
    bad = run(sr, si, w2)
    assert bad[1].all() and not bad[0].any() and not bad[2].any()


@pytest.mark.parametrize("M,li,lo", [(1, PLANAR, PLANAR), (4, CF32, PLANAR), (8, I16, CF32), (64, I8, CF32)])
def test_one_tap_is_the_beamformer(g, M, li, lo):
    """num_taps = 1 against the beamformer's restatement (tests/beam_ref.py), within its bound"""
    rng = np.random.default_rng(70 + M)
    B, N, J = 2, 37, 3
    c = host_case(g, rng, li, lo, B, M, N, 1, J, pad_in=2, pad_out=1, off_in=1, off_out=1)
    w = random_weights(rng, J, M)
    assert g.spacetime_filter_host(c["idesc"], B, w, 1, c["odesc"]) == 0
    err = np.abs(host_output(c) - beam_ref.beams(c["x"], w, N, B, c["ibs"]))
    assert (err <= beam_ref.bound(c["x"], w, N, B, c["ibs"])).all()


def test_restatement_equals_the_loop_written_sums():
    """the FP64 reference the other tests lean on, against the definitions written out as loops"""
    rng = np.random.default_rng(8)
    M, T, N, B, S, J = 3, 4, 9, 2, 11, 2
    x = rng.standard_normal((M, (B - 1) * S + N)) + 1j * rng.standard_normal((M, (B - 1) * S + N))
    w = random_weights(rng, J, M * T)
    y, R = ref.filt(x, w, N, B, T, S), ref.covariance(x, N, B, T, 2, S)
    Rl = np.zeros((M * T, M * T), np.complex128)
    for b in range(B):
        for n in range(T - 1, N):
            z = np.array([x[m, b * S + n - t] for t in range(T) for m in range(M)])
            Rl += np.outer(z, z.conj())
            for j in range(J):
                assert abs(y[b, j, n - (T - 1)] - np.vdot(w[j], z)) <= 1e-13 * (np.abs(w[j]) @ np.abs(z))
    assert R.shape == (1, M * T, M * T) and np.abs(R[0] - Rl).max() <= 1e-12 * np.abs(Rl).max()
    assert np.linalg.eigvalsh(R[0]).min() >= -1e-12 * np.abs(Rl).max()  # positive semi-definite by construction


def test_the_scene_in_fp64_and_with_the_twin(g):
    """Two antennas, two CW jammers 40 dB over the noise from two directions, a satellite 22 dB under it (st_ref.SCENE, noise seed
    17).  Behind spatial power inversion (one degree of freedom, two jammers) the satellite must NOT be detected at the default
    min_peak_ratio 2.0; behind five taps an antenna (power inversion referenced to tap 2, antenna 0, no loading) it must be, at the
    true code phase advanced by d = 2 samples within half a sample, with the output power within 3 dB of the noise.
    Measured with the FP64 restatement alone (weights by numpy.linalg.solve): peak / second 1.05 behind the spatial weights and
    7.14 behind the five-tap ones, against 2.0 -- factors 1.9 and 3.6 of room; output power 37.1 dB and 1.18 dB over the noise;
    code phase 417.398 chips for a truth of 417.402 (half a sample is 0.026 chips); covariance condition number 1.2e5.  The
    satellite alone in the noise of antenna 0 gives 7.25.  With the float32 twin behind weights from gat_array_weights_host on the
    float32-narrowed FP64 covariance the figures agree to their last printed digit."""
    s = ref.SCENE
    N, T, M, d = s["N"], s["T"], s["M"], s["T"] - 1 - s["ref_tap"]
    assert d == 2 and g.spacetime_delay(T, s["ref_tap"]) == d
    x, codes = ref.scene_stream(s)
    n_tot = N + T - 1
    noise = 2.0 * ref.scene_sigma(s) ** 2
    half_sample = 0.5 * ref.FC / s["fs"]

    def db(y):
        return 10.0 * np.log10((np.abs(y) ** 2).mean() / noise)

    # FP64 alone
    w1 = ref.weights(ref.covariance(x, n_tot, 1, 1, 1)[0], ref.steering([1, 0], 1, 0))
    y1 = ref.filt(x, w1[None], n_tot, 1, 1)[0, 0][:N]
    R5 = ref.covariance(x, n_tot, 1, T, 1)[0]
    w5 = ref.weights(R5, ref.steering([1, 0], T, s["ref_tap"]))
    y5 = ref.filt(x, w5[None], n_tot, 1, T)[0, 0]
    r1, r5 = ref.search(y1, codes, s["col"], s), ref.search(y5, codes, s["col"], s)
    print(f"FP64: spatial peak/second {r1['peak_to_second']:.2f} at {db(y1):.1f} dB; five taps {r5['peak_to_second']:.2f} at {db(y5):.2f} dB, "
          f"code phase {r5['code_phase_chips']:.3f} (truth {ref.scene_truth(s, d):.3f}), cond {np.linalg.cond(R5):.1e}")
    assert r1["peak_to_second"] * 1.3 < 2.0 < r5["peak_to_second"] / 1.3  # the restatement holds both verdicts with room
    assert not r1["detected"] and r5["detected"]

    # the library: the host solver on the narrowed covariance, the float32 twin on the float32 stream
    xr, xi = np.ascontiguousarray(x.real.astype(np.float32)), np.ascontiguousarray(x.imag.astype(np.float32))
    lib = g.load_library()

    def host_weights(R, a):
        Q = R.shape[0]
        c_re, c_im = np.ascontiguousarray(R.real.astype(np.float32)), np.ascontiguousarray(R.imag.astype(np.float32))
        a_re, a_im = np.ascontiguousarray(a.real), np.ascontiguousarray(a.imag)
        w_re, w_im = np.zeros(Q), np.zeros(Q)
        assert lib.gat_array_weights_host(c_re.ctypes.data, c_im.ctypes.data, Q, a_re.ctypes.data, a_im.ctypes.data, 1, 1, 0.0, w_re.ctypes.data,
                                          w_im.ctypes.data) == 0
        return w_re + 1j * w_im

    def twin(w, taps):
        No = n_tot - taps + 1
        o = [np.zeros((1, No), np.float32), np.zeros((1, No), np.float32)]
        assert g.spacetime_filter_host(g.spacetime.host_desc(xr, xi, PLANAR, M, n_tot, n_tot, n_tot), 1, w, taps,
                                       g.spacetime.host_desc(o[0], o[1], PLANAR, 1, No, No, No)) == 0
        return (o[0][0].astype(np.float64) + 1j * o[1][0].astype(np.float64))[:N]

    t1 = twin(host_weights(ref.covariance(x, n_tot, 1, 1, 1)[0], ref.steering([1, 0], 1, 0)), 1)
    t5 = twin(host_weights(R5, ref.steering([1, 0], T, s["ref_tap"])), T)
    q1, q5 = ref.search(t1, codes, s["col"], s), ref.search(t5, codes, s["col"], s)
    print(f"twin: spatial peak/second {q1['peak_to_second']:.2f} at {db(t1):.1f} dB; five taps {q5['peak_to_second']:.2f} at {db(t5):.2f} dB, "
          f"code phase {q5['code_phase_chips']:.3f}, Doppler {q5['carrier_doppler_hz']:.0f} Hz")
    assert not q1["detected"]
    assert q5["detected"]
    for r, y in ((r5, y5), (q5, t5)):
        err = (r["code_phase_chips"] - ref.scene_truth(s, d) + ref.LC / 2) % ref.LC - ref.LC / 2
        assert abs(err) <= half_sample, err
        assert abs(db(y)) <= 3.0
        assert abs(r["carrier_doppler_hz"] - s["dop"]) <= s["fs"] / (2.0 * N)
