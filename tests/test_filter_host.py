"""The sample filter's host twin (gat_filter_samples_host) and the tap design of gpuacceleratedtracking_amd/filtering.py, without a
device: the twin against the FP64 restatement (tests/fir_ref.py) within the documented bound, every refusal with the output
untouched, the identity filter, the invariance of the bits under the partition of a stream into overlap-save blocks, and the tap
helpers against mix-then-filter in FP64."""
import ctypes as C

import numpy as np
import pytest

from tests import fir_ref as ref
from tests.fir_ref import CF32, I8, I16, LAYOUTS, OUT_LAYOUTS, PLANAR

ARG, RANGE, UNSUPPORTED = 1, 2, 4


@pytest.fixture(scope="module")
def g():
    import gpuacceleratedtracking_amd as g
    g.load_library()
    return g


def host_case(g, rng, li, lo, B, M, N, taps, D, pad_in=0, pad_out=0, off_in=0, off_out=0, in_stride=None):
    """random samples [B, M, N] in layout li (blocks every in_stride samples: overlapping where in_stride < N, and then block b
    continues block b - 1), an output of layout lo full of sentinels, and the two descriptors"""
    T = len(taps)
    Q = ref.num_outputs(N, T, D)
    ibs = N + pad_in if in_stride is None else in_stride
    span = (B - 1) * ibs + N
    ias, obs = span + pad_in, Q + pad_out
    oas = B * obs + pad_out
    sr, si = ref.random_samples(rng, li, (M, span), special=False)
    ibuf = ref.make_buffers(li, 1, M, span, ias, 0, off_in)
    ref.put(ibuf, li, ref.index(1, M, span, ias, 0, off_in), sr[None], si[None])
    iidx = ref.index(B, M, N, ias, ibs, off_in)
    xr, xi = ref.get(ibuf, li, iidx)
    obuf = ref.make_buffers(lo, B, M, Q, oas, obs, off_out, fill=-3.25)
    oidx = ref.index(B, M, Q, oas, obs, off_out)
    idesc = g.filtering.host_desc(ibuf[0], ibuf[1] if li == PLANAR else None, li, M, N, ias, ibs, off_in)
    odesc = g.filtering.host_desc(obuf[0], obuf[1] if lo == PLANAR else None, lo, M, Q, oas, obs, off_out)
    return dict(xr=xr, xi=xi, ibuf=ibuf, obuf=obuf, oidx=oidx, idesc=idesc, odesc=odesc, Q=Q, ibs=ibs, B=B, lo=lo)


def host_output(c):
    yr, yi = ref.get(c["obuf"], c["lo"], c["oidx"])
    return yr.astype(np.float64) + 1j * yi.astype(np.float64)


def random_taps(rng, T):
    return (rng.standard_normal(T) + 1j * rng.standard_normal(T)) / np.sqrt(T)


CASES = [  # li, lo, B, M, N, T, D, step, phase, in_stride
    (PLANAR, PLANAR, 2, 2, 300, 7, 1, 0.0, 0.0, None),
    (CF32, CF32, 1, 3, 257, 64, 5, 0.125, 0.3, None),
    (I16, PLANAR, 3, 1, 1000, 255, 3, -0.2371, 7.25, 600),
    (I8, CF32, 2, 9, 700, 256, 64, 1e-3, 0.0, 1 << 20),
    (PLANAR, CF32, 3, 2, 90, 1, 2, 0.49999, 1e9 + 0.125, 40),
    (I8, PLANAR, 1, 2, 4099, 32, 8, 3.0 - 1e-7, -0.75, None),
]


@pytest.mark.parametrize("li,lo,B,M,N,T,D,step,phase,in_stride", CASES)
def test_host_twin_within_the_bound_of_the_fp64_restatement(g, li, lo, B, M, N, T, D, step, phase, in_stride):
    """|y - y64| <= [(2T + 8) 2^-24 + 2 pi 2^-53 (P/2 + 2)] S per component, S = sum_t (|g_re| + |g_im|)(|x_re| + |x_im|)"""
    rng = np.random.default_rng(1000 + T + D)
    taps = random_taps(rng, T)
    c = host_case(g, rng, li, lo, B, M, N, taps, D, pad_in=3, pad_out=1, off_in=1, off_out=2, in_stride=in_stride)
    before = ref.guard_of(c["obuf"])
    assert g.filter_samples_host(c["idesc"], B, taps, c["odesc"], D, step, phase) == 0
    want, S, P = ref.fir(c["xr"], c["xi"], taps, D, step, phase, c["ibs"])
    got = host_output(c)
    lim = ref.bound(T, S, P)
    worst = max(float((np.abs(got.real - want.real) / lim).max()), float((np.abs(got.imag - want.imag) / lim).max()))
    print(f"T {T} D {D}: worst error over its bound {worst:.3f}, P up to {P.max():.0f}")
    assert worst <= 1.0
    assert np.abs(want).max() > 1e3 * lim.max() or T == 1  # the bound is small next to the outputs: the check says something
    assert ref.unchanged_outside(c["obuf"], before, lo, c["oidx"])


def test_integer_samples_and_special_values(g):
    """an int16 stream and its float image give the same bits; NaN and inf propagate by the IEEE rules to exactly the outputs
    whose T samples hold them"""
    rng = np.random.default_rng(5)
    T, D, N = 9, 2, 200
    taps = random_taps(rng, T)
    a = host_case(g, rng, I16, PLANAR, 1, 2, N, taps, D)
    assert g.filter_samples_host(a["idesc"], 1, taps, a["odesc"], D, 0.1, 0.2) == 0
    fr, fi = a["xr"].astype(np.float32), a["xi"].astype(np.float32)
    fr[0, 0, 50], fi[0, 1, 120] = np.nan, np.inf
    for special in (False, True):
        xr, xi = (a["xr"].astype(np.float32), a["xi"].astype(np.float32)) if not special else (fr, fi)
        ib = [np.ascontiguousarray(xr.reshape(2, N)), np.ascontiguousarray(xi.reshape(2, N))]
        Q = a["Q"]
        ob = [np.zeros((2, Q), np.float32), np.zeros((2, Q), np.float32)]
        idesc = g.filtering.host_desc(ib[0], ib[1], PLANAR, 2, N, N, N)
        odesc = g.filtering.host_desc(ob[0], ob[1], PLANAR, 2, Q, Q, Q)
        assert g.filter_samples_host(idesc, 1, taps, odesc, D, 0.1, 0.2) == 0
        if not special:
            yr, yi = ref.get(a["obuf"], PLANAR, a["oidx"])
            assert ref.same_bits(ob[0], yr[0]) and ref.same_bits(ob[1], yi[0])
        else:
            q = np.arange(Q)
            for m, n in ((0, 50), (1, 120)):
                hit = (q * D <= n) & (n <= q * D + T - 1)
                bad = ~np.isfinite(ob[0][m]) | ~np.isfinite(ob[1][m])
                assert np.array_equal(bad, hit)


def test_identity_filter_reproduces_the_input_exactly(g):
    """T = 1, g = 1, D = 1, oscillator off: the output is the input, bit for bit, for all four input layouts"""
    rng = np.random.default_rng(11)
    for li in LAYOUTS:
        for lo in OUT_LAYOUTS:
            c = host_case(g, rng, li, lo, 2, 3, 37, [1.0], 1, pad_in=2, pad_out=3, off_in=1, off_out=1)
            before = ref.guard_of(c["obuf"])
            assert g.filter_samples_host(c["idesc"], 2, [1.0], c["odesc"]) == 0
            yr, yi = ref.get(c["obuf"], lo, c["oidx"])
            assert ref.same_bits(yr, c["xr"].astype(np.float32)) and ref.same_bits(yi, c["xi"].astype(np.float32))
            assert ref.unchanged_outside(c["obuf"], before, lo, c["oidx"])


@pytest.mark.parametrize("li,D,T,step", [(PLANAR, 1, 33, 0.0), (I8, 5, 64, 0.125), (CF32, 3, 20, -0.31830988), (I16, 2, 7, 0.25)])
def test_partition_invariance(g, li, D, T, step):
    """one stream as 1, 3 and 7 overlap-save blocks (input num_samples = Q D + T - 1, block_stride = Q D, output block_stride = Q)
    gives the same bits: the oscillator runs on the stream position"""
    rng = np.random.default_rng(21)
    taps = random_taps(rng, T)
    total_q, M = 21 * 11, 2
    span = total_q * D + T - 1
    sr, si = ref.random_samples(rng, li, (M, span), special=False)
    ibuf = ref.make_buffers(li, 1, M, span, span, 0)
    ref.put(ibuf, li, ref.index(1, M, span, span, 0), sr[None], si[None])
    outs = []
    for B in (1, 3, 7):
        Q = total_q // B
        ob = [np.zeros((M, total_q), np.float32), np.zeros((M, total_q), np.float32)]
        idesc = g.filtering.host_desc(ibuf[0], ibuf[1] if li == PLANAR else None, li, M, Q * D + T - 1, span, Q * D)
        odesc = g.filtering.host_desc(ob[0], ob[1], PLANAR, M, Q, total_q, Q)
        assert g.filter_samples_host(idesc, B, taps, odesc, D, step, 0.4 if step else 0.0) == 0
        outs.append(ob)
    for ob in outs[1:]:
        assert ref.same_bits(ob[0], outs[0][0]) and ref.same_bits(ob[1], outs[0][1])
    assert np.abs(outs[0][0]).max() > 0


def test_every_refusal_leaves_the_output_untouched(g):
    rng = np.random.default_rng(31)
    lib = g._lib.load()
    T, D, B, M, N = 5, 2, 2, 2, 64
    taps = random_taps(rng, T)
    g_re, g_im = g.filtering._tap_planes(taps)
    c = host_case(g, rng, CF32, PLANAR, B, M, N, taps, D)
    before = ref.guard_of(c["obuf"])
    FirConfig, SignalDesc = g._lib.FirConfig, g._lib.SignalDesc

    def cfg(**kw):
        f = FirConfig(C.sizeof(FirConfig), T, D, 0.0, 0.0)
        for k, v in kw.items():
            setattr(f, k, v)
        return f

    def clone(d, **kw):
        n = SignalDesc(d.re, d.im, d.layout, d.num_ants, d.num_samples, d.ant_stride, d.block_stride, d.chan_stride)
        for k, v in kw.items():
            setattr(n, k, v)
        return n

    def call(sig=c["idesc"], nb=B, re=g_re, im=g_im, f=None, out=c["odesc"], null=()):
        f = cfg() if f is None else f
        args = dict(sig=C.byref(sig), re=re.ctypes.data, im=im.ctypes.data, f=C.byref(f), out=C.byref(out))
        for k in null:
            args[k] = None
        return lib.gat_filter_samples_host(args["sig"], nb, args["re"], args["im"], args["f"], args["out"])

    assert call() == 0  # the valid call the refusals are made from
    for buf, b0 in zip(c["obuf"], before):
        buf[...] = b0
    i, o = c["idesc"], c["odesc"]
    in_bytes = ((B - 1) * i.block_stride + (M - 1) * i.ant_stride + N) * 8
    refusals = [
        (ARG, dict(null=("sig",))), (ARG, dict(null=("out",))), (ARG, dict(null=("re",))), (ARG, dict(null=("im",))), (ARG, dict(null=("f",))),
        (ARG, dict(f=cfg(struct_size=C.sizeof(FirConfig) - 4))), (ARG, dict(nb=0)),
        (ARG, dict(sig=clone(i, num_samples=0))), (ARG, dict(sig=clone(i, ant_stride=-1))), (ARG, dict(sig=clone(i, block_stride=0))),
        (ARG, dict(sig=clone(i, layout=7))), (ARG, dict(sig=clone(i, im=i.re))), (ARG, dict(out=clone(o, im=None))),
        (ARG, dict(out=clone(o, ant_stride=0))), (ARG, dict(out=clone(o, layout=-1))),
        (ARG, dict(sig=clone(i, num_samples=T - 1))),                                  # N < T
        (ARG, dict(out=clone(o, num_samples=c["Q"] + 1))), (ARG, dict(out=clone(o, num_samples=c["Q"] - 1))),
        (ARG, dict(out=clone(o, num_ants=M + 1))),
        (ARG, dict(f=cfg(nco_step=float("nan")))), (ARG, dict(f=cfg(nco_phase=float("inf")))), (ARG, dict(f=cfg(nco_step=-float("inf")))),
        (ARG, dict(out=clone(o, re=i.re + in_bytes - 1))), (ARG, dict(out=clone(o, im=i.re))),  # the output overlaps the input
        (RANGE, dict(f=cfg(num_taps=0))), (RANGE, dict(f=cfg(num_taps=257))), (RANGE, dict(f=cfg(decimation=0))), (RANGE, dict(f=cfg(decimation=65))),
        (RANGE, dict(sig=clone(i, num_ants=65), out=clone(o, num_ants=65))),
        (RANGE, dict(sig=clone(i, block_stride=(1 << 31) - N + 1))),                   # (B - 1) block_stride + N = 2^31 + 1
        (UNSUPPORTED, dict(out=clone(o, layout=I16, im=None))), (UNSUPPORTED, dict(out=clone(o, layout=I8, im=None))),
        (UNSUPPORTED, dict(sig=clone(i, chan_stride=8))), (UNSUPPORTED, dict(out=clone(o, chan_stride=8))),
    ]
    for code, kw in refusals:
        assert call(**kw) == code, kw
        assert all(ref.same_bits(buf, b0) for buf, b0 in zip(c["obuf"], before)), kw
    # the largest span a call may have is accepted as far as the plan goes: 2^31 exactly passes the range check (and would then read
    # memory nobody has, so it is asked of a call that is refused later, for its output's size)
    assert call(sig=clone(i, block_stride=(1 << 31) - N), out=clone(o, num_samples=c["Q"] + 1)) == ARG
    # the largest filter and decimation are accepted
    big = random_taps(rng, 256)
    cb = host_case(g, rng, I8, CF32, 1, 1, 256 + 64 * 2, big, 64)
    assert g.filter_samples_host(cb["idesc"], 1, big, cb["odesc"], 64) == 0 and cb["Q"] == 3


def test_tap_helpers(g):
    """shift_taps with nco_step = nu is mix-then-filter; channelize's taps are that; a notch has unit gain away from nu and a null there"""
    rng = np.random.default_rng(41)
    f = g.filtering
    h = f.lowpass_taps(101, 0.1)
    assert abs(h.sum() - 1.0) < 1e-12 and np.allclose(h, h[::-1])
    nu, n = 0.1234, np.arange(400)
    x = rng.standard_normal(400) + 1j * rng.standard_normal(400)
    mixed = x * np.exp(-2j * np.pi * nu * n)
    want = np.convolve(mixed, h, mode="valid")                                        # output q: newest sample p = q + T - 1
    got = np.convolve(x, f.shift_taps(h, nu), mode="valid") * np.exp(-2j * np.pi * nu * (np.arange(want.size) + h.size - 1))
    assert np.abs(got - want).max() < 1e-12 * np.abs(want).max() * 100
    # the restatement of the rule gives the same (float32 taps: 1e-7 of the outputs)
    y, _, _ = ref.fir(x.real[None, None], x.imag[None, None], f.shift_taps(h, nu), 1, nu, 0.0)
    assert np.abs(y[0, 0] - want).max() < 1e-6 * np.abs(want).max()
    # frequency responses
    w = np.linspace(-0.5, 0.5, 2001)
    resp = lambda taps: np.array([np.sum(taps * np.exp(-2j * np.pi * v * np.arange(len(taps)))) for v in w])  # noqa: E731
    H = np.abs(resp(h))
    assert (np.abs(H[np.abs(w) <= 0.05] - 1) < 1e-3).all() and (H[np.abs(w) >= 0.15] < 1e-3).all()
    notch = f.notch_taps(65, 0.2, 0.02)
    G = np.abs(resp(notch))
    assert abs(np.sum(notch * np.exp(-2j * np.pi * 0.2 * np.arange(65)))) < 1e-3      # the null at nu
    assert (np.abs(G[np.abs(w - 0.2) >= 0.08] - 1) < 1e-3).all()                       # unit gain away from it
    with pytest.raises(ValueError):
        f.notch_taps(64, 0.2, 0.02)
    N, stride, Q, B, total = f.stream_blocks(1000, 64, 5, 3)
    assert N == Q * 5 + 63 and stride == Q * 5 and total == 3 * Q and (B - 1) * stride + N <= 1000 < (B - 1) * stride + N + 5 * B
