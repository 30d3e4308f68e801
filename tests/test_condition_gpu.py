"""GPU tests of the sample conditioner (include/gat.h gat_condition_samples, gat_sample_stats, gat_agc_update; csrc/gat_cond.hip).

The conditioned stream is compared with the library's host twin BIT FOR BIT over the whole output allocation, sentinels
included (the twin itself is held to the numpy restatement by tests/test_condition_host.py on the CPU); gat_last_launch_info
says which kernel ran and every case asserts it.  The statistics are held to the FP64 restatement of tests/cond_ref.py:
counts and max_abs exactly, |sum - ref| <= 1e-5 sum |x| per component, sum_pow to a relative 1e-5."""
import ctypes as C

import numpy as np
import pytest

from tests import cond_ref as ref
from tests.cond_ref import CF32, I8, I16, LAYOUTS, PLANAR, records, same_bits

pytestmark = pytest.mark.gpu

OK, ERR_ARG, ERR_RANGE, ERR_UNSUPPORTED = 0, 1, 2, 4
STEP = {PLANAR: 4, CF32: 8, I16: 4, I8: 2}  # bytes per sample of a buffer


@pytest.fixture(scope="module")
def g():
    import gpuacceleratedtracking_amd as g
    g.load_library()
    return g


def to_dev(g, bufs):
    import torch
    return [torch.from_numpy(b).to(g.get_context().device) for b in bufs]


def dev_desc(g, tens, layout, M, N, ant_stride, block_stride, offset=0):
    off = offset * STEP[layout]
    return g._lib.SignalDesc(tens[0].data_ptr() + off, tens[1].data_ptr() + off if layout == PLANAR else None, layout, M, N, ant_stride, block_stride, 0)


def specials(li, vr, vi, T):
    """the rule's edge inputs at the first and last sample of a block, inside a lane's group and in the ragged tail"""
    N = vr.shape[-1]
    spots = sorted({0, 1, 5, N - 2, N - 1} & set(range(N)))
    if li in (PLANAR, CF32):
        vals = [np.nan, T, np.nextafter(np.float32(T), np.float32(np.inf)), np.inf, -T, 2.5, -0.0]
    else:
        vals = [int(T), int(T) + 1, -int(T), 3, -3, 1, -ref.LIMIT[li] - 1]  # threshold equality, ties under scale 0.5, the most negative code
    for k, n in enumerate(spots):
        vr[..., n] = vals[k % len(vals)]
        vi[..., n] = vals[(k + 3) % len(vals)]
        vi[:, 0, n] = 1  # antenna 0 trips only through its real part


def run_both(g, li, lo, vr, vi, p, blank_all=False, ant_pad=0, block_pad=0, offset=0, want_vec=None, out_block_pad=None, calls=2):
    """vr, vi [B, M, N] through the host twin and through the device from identical, sentinel-filled allocations; asserts the
    kernel that ran, identical bytes over the whole output allocation and exact counts, doubled by a second call without zeroing.
    Returns the device's logical output."""
    import torch
    fe = g.frontend
    ctx = g.get_context()
    B, M, N = vr.shape
    bs = N + block_pad
    as_ = B * bs + ant_pad
    obs = bs if out_block_pad is None else N + out_block_pad
    oas = B * obs + ant_pad
    ibuf = ref.make_buffers(li, B, M, N, as_, bs, offset)
    ref.put(ibuf, li, ref.index(B, M, N, as_, bs, offset), vr, vi)
    obuf = ref.make_buffers(lo, B, M, N, oas, obs, offset)
    d_in, d_out = to_dev(g, ibuf), to_dev(g, obuf)
    hcnt = np.zeros((M, 2), np.uint64)
    rc = fe.condition_samples_host(fe.host_desc(ibuf[0], ibuf[1] if li == PLANAR else None, li, M, N, as_, bs, offset), B, p,
                                   fe.host_desc(obuf[0], obuf[1] if lo == PLANAR else None, lo, M, N, oas, obs, offset), blank_all, hcnt)
    assert rc == OK
    prm = torch.from_numpy(p.view(np.float32).reshape(M, 4).copy()).to(ctx.device)
    cnt = torch.zeros((M, 2), dtype=torch.int64, device=ctx.device)
    idesc, odesc = dev_desc(g, d_in, li, M, N, as_, bs, offset), dev_desc(g, d_out, lo, M, N, oas, obs, offset)
    for k in range(1, calls + 1):
        ctx.check(ctx.lib.gat_condition_samples(ctx._h, C.byref(idesc), B, C.c_void_p(prm.data_ptr()), 1 if blank_all else 0, C.byref(odesc),
                                                C.c_void_p(cnt.data_ptr())), "gat_condition_samples")
        ctx.sync()
        info = ctx.last_launch_info()
        if want_vec is not None:
            assert info["vec"] == want_vec, (info, li, lo, M, N, B, offset)
        assert info["ant_tile"] == M and info["threads"] == 256
        for got, want in zip(d_out, obuf):
            assert same_bits(got.cpu().numpy(), want), f"device and host twin differ: layouts {li}->{lo} M={M} N={N} B={B} vec={info['vec']}"
        assert np.array_equal(cnt.cpu().numpy().astype(np.uint64), k * hcnt), (cnt.cpu().numpy(), hcnt)
    return ref.get([t.cpu().numpy() for t in d_out], lo, ref.index(B, M, N, oas, obs, offset)), hcnt


def case_inputs(rng, li, lo, B, M, N):
    vr, vi = ref.random_samples(rng, li, (B, M, N), special=False)
    T = 64.0 if li in (PLANAR, CF32) else float(ref.LIMIT[li] // 2)
    specials(li, vr, vi, T)
    level = 40.0 if li in (PLANAR, CF32) else ref.LIMIT[li] / 3.0
    target = 3.0 if lo in (PLANAR, CF32) else ref.LIMIT[lo] / 2.5  # some components clip
    p = np.zeros(M, dtype=np.dtype([("scale", "<f4"), ("dc_re", "<f4"), ("dc_im", "<f4"), ("threshold", "<f4")]))
    p["scale"] = (target / level) * rng.uniform(0.5, 1.5, M)
    p["dc_re"], p["dc_im"] = rng.uniform(-2, 2, M), rng.uniform(-2, 2, M)
    p["threshold"] = T
    p["scale"][0], p["dc_re"][0], p["dc_im"][0] = 0.5, 0.0, 0.0  # antenna 0: ties at every odd integer sample
    return vr, vi, p


def pad_to(n, to=8):
    return -(-n // to) * to - n


@pytest.mark.parametrize("lo", LAYOUTS)
@pytest.mark.parametrize("li", LAYOUTS)
def test_device_equals_host_twin(g, li, lo):
    rng = np.random.default_rng(1000 + 4 * li + lo)
    for N in (1, 7, 257, 2500):
        B = 3 if N in (257, 2500) else 1
        for M, offset, want in ((1, 0, 4), (4, 0, 4), (8, 0, 4), (3, 1, 1), (9, 0, 1), (64, 0, 1)):
            if M == 64 and N == 2500:
                B = 1
            vr, vi, p = case_inputs(rng, li, lo, B, M, N)
            # aligned cases: every block and antenna starts on a multiple of 8 samples (16 bytes in every layout)
            run_both(g, li, lo, vr, vi, p, blank_all=bool((M + N) % 2), ant_pad=8, block_pad=pad_to(N), offset=offset, want_vec=want)


@pytest.mark.parametrize("lo", LAYOUTS)
def test_unpadded_int8_blocks_fall_to_the_general_kernel(g, lo):
    """B = 3 blocks of N = 2500 int8 pairs back to back: block 1 starts 5000 bytes in, not on a 16-byte boundary, so the whole
    call runs the general kernel -- and still matches."""
    rng = np.random.default_rng(77 + lo)
    vr, vi, p = case_inputs(rng, I8, lo, 3, 4, 2500)
    run_both(g, I8, lo, vr, vi, p, blank_all=True, ant_pad=0, block_pad=0, want_vec=1)


@pytest.mark.parametrize("li,lo", [(PLANAR, I8), (CF32, I16), (I16, PLANAR), (I8, CF32), (I8, I8), (PLANAR, PLANAR)])
def test_streaming_and_general_kernel_give_the_same_bits(g, li, lo):
    rng = np.random.default_rng(5 + 4 * li + lo)
    vr, vi, p = case_inputs(rng, li, lo, 2, 4, 1029)
    (a_re, a_im), ca = run_both(g, li, lo, vr, vi, p, True, ant_pad=8, block_pad=pad_to(1029), offset=0, want_vec=4, calls=1)
    (b_re, b_im), cb = run_both(g, li, lo, vr, vi, p, True, ant_pad=8, block_pad=pad_to(1029), offset=1, want_vec=1, calls=1)
    assert same_bits(a_re, b_re) and same_bits(a_im, b_im) and np.array_equal(ca, cb)


@pytest.mark.parametrize("li,lo,offset,want", [(PLANAR, I8, 0, 4), (I16, CF32, 0, 4), (CF32, I8, 1, 1)])
def test_work_split(g, li, lo, offset, want):
    """more units than workgroups (300 blocks of 64 samples), and one block in many chunks with a ragged end (200 003 samples)"""
    rng = np.random.default_rng(31 + li)
    ctx = g.get_context()
    vr, vi, p = case_inputs(rng, li, lo, 300, 8, 64)
    run_both(g, li, lo, vr, vi, p, True, ant_pad=8, block_pad=0, offset=offset, want_vec=want, calls=1)
    assert ctx.last_launch_info()["splits"] == 1
    vr, vi, p = case_inputs(rng, li, lo, 2500, 1, 64)  # more units than the grid has workgroups on any device
    run_both(g, li, lo, vr, vi, p, False, ant_pad=8, block_pad=0, offset=offset, want_vec=want, calls=1)
    info = ctx.last_launch_info()
    assert info["workgroups"] <= 2500 and info["splits"] == 1
    vr, vi, p = case_inputs(rng, li, lo, 1, 2, 200003)
    run_both(g, li, lo, vr, vi, p, False, ant_pad=pad_to(200003), block_pad=0, offset=offset, want_vec=want, calls=1)
    info = ctx.last_launch_info()
    assert info["splits"] > 8 and info["workgroups"] == info["splits"]


def test_in_place_on_the_device(g):
    import torch
    rng = np.random.default_rng(9)
    ctx = g.get_context()
    for layout, offset, want in ((PLANAR, 0, 4), (I16, 0, 4), (CF32, 1, 1), (I8, 0, 4)):
        B, M, N = 2, 4, 1000
        vr, vi, p = case_inputs(rng, layout, layout, B, M, N)
        bufs = ref.make_buffers(layout, B, M, N, B * N + 8, N, offset)
        ref.put(bufs, layout, ref.index(B, M, N, B * N + 8, N, offset), vr, vi)
        dev = to_dev(g, bufs)
        hd = g.frontend.host_desc(bufs[0], bufs[1] if layout == PLANAR else None, layout, M, N, B * N + 8, N, offset)
        assert g.frontend.condition_samples_host(hd, B, p, hd, True) == OK
        dd = dev_desc(g, dev, layout, M, N, B * N + 8, N, offset)
        prm = torch.from_numpy(p.view(np.float32).reshape(M, 4).copy()).to(ctx.device)
        ctx.check(ctx.lib.gat_condition_samples(ctx._h, C.byref(dd), B, C.c_void_p(prm.data_ptr()), 1, C.byref(dd), None), "gat_condition_samples")
        ctx.sync()
        assert ctx.last_launch_info()["vec"] == want
        for got, exp in zip(dev, bufs):
            assert same_bits(got.cpu().numpy(), exp)


# ---- statistics --------------------------------------------------------------------------------------------------------------------
def run_stats(g, li, vr, vi, bpe, thresholds=None, blank_all=False, offset=0, pad=8, want_vec=None):
    """[B, M, N] samples -> the structured array [E, M] of the device; two calls, identical bits."""
    import torch
    ctx = g.get_context()
    B, M, N = vr.shape
    bs = N + (pad_to(N) if pad else 0)
    as_ = B * bs + pad
    ibuf = ref.make_buffers(li, B, M, N, as_, bs, offset)
    ref.put(ibuf, li, ref.index(B, M, N, as_, bs, offset), vr, vi)
    d_in = to_dev(g, ibuf)
    desc = dev_desc(g, d_in, li, M, N, as_, bs, offset)
    prm = None
    if thresholds is not None:
        p = records(g.frontend, M, threshold=thresholds)
        prm = torch.from_numpy(p.view(np.float32).reshape(M, 4).copy()).to(ctx.device)
    E = -(-B // bpe)
    outs = []
    for _ in range(2):
        st = torch.full((E, M, 48), 0x5A, dtype=torch.uint8, device=ctx.device)
        ctx.check(ctx.lib.gat_sample_stats(ctx._h, C.byref(desc), B, bpe, C.c_void_p(prm.data_ptr()) if prm is not None else None,
                                           1 if blank_all else 0, C.c_void_p(st.data_ptr())), "gat_sample_stats")
        ctx.sync()
        if want_vec is not None:
            assert ctx.last_launch_info()["vec"] == want_vec
        outs.append(st.cpu().numpy())
    assert outs[0].tobytes() == outs[1].tobytes(), "a repeat call gave other bits"
    return outs[0].view(g.frontend.SAMPLE_STATS_DTYPE).reshape(E, M)


def check_stats(got, vr, vi, bpe, thresholds=None, blank_all=False, exact=False):
    B = vr.shape[0]
    worst = 0.0
    for e in range(got.shape[0]):
        sl = slice(e * bpe, min(B, (e + 1) * bpe))
        want = ref.stats(vr[sl], vi[sl], thresholds, blank_all)
        assert np.array_equal(got[e]["kept"], want["kept"]) and np.array_equal(got[e]["blanked"], want["blanked"])
        assert same_bits(got[e]["max_abs"], want["max_abs"])
        assert not got[e]["pad_"].any()
        for name, ab in (("sum_re", "abs_re"), ("sum_im", "abs_im")):
            err = np.abs(got[e][name] - want[name])
            print(f"estimate {e} {name}: |err| / sum|x| = {np.max(err / np.maximum(want[ab], 1e-300)):.3e}")
            assert (err <= (0.0 if exact else 1e-5) * want[ab]).all(), (name, err, want[ab])
            worst = max(worst, float(np.max(err / np.maximum(want[ab], 1e-300))))
        err = np.abs(got[e]["sum_pow"] - want["sum_pow"])
        print(f"estimate {e} sum_pow: relative error {np.max(err / np.maximum(want['sum_pow'], 1e-300)):.3e}")
        assert (err <= (0.0 if exact else 1e-5) * want["sum_pow"]).all()
    return worst


@pytest.mark.parametrize("li", LAYOUTS)
def test_stats_against_the_fp64_restatement(g, li):
    rng = np.random.default_rng(200 + li)
    for N in (1, 63, 20000):
        for M, offset, want in ((1, 0, 4), (4, 0, 4), (3, 1, 1), (9, 0, 1)):
            vr, vi = ref.random_samples(rng, li, (4, M, N), special=N > 1)
            T = (90.0 if li in (PLANAR, CF32) else ref.LIMIT[li] * 0.8) * rng.uniform(0.8, 1.2, M)
            # without records +-inf would be kept and no sum would be finite: that case gets NaN (blanked at any threshold,
            # NULL records included) where the others have +-inf, so that its sums are asserted like theirs
            fr, fi = (np.where(np.isinf(v), np.float32(np.nan), v) for v in (vr, vi)) if li in (PLANAR, CF32) else (vr, vi)
            for thresholds, blank_all in ((None, False), (T, False), (T, True)):
                xr, xi = (fr, fi) if thresholds is None else (vr, vi)
                check_stats(run_stats(g, li, xr, xi, 2, thresholds, blank_all, offset, want_vec=want), xr, xi, 2, thresholds, blank_all)


def test_stats_int8_sums_are_exact(g):
    rng = np.random.default_rng(41)
    for N in (7, 256):
        vr, vi = ref.random_samples(rng, I8, (3, 4, N))
        check_stats(run_stats(g, I8, vr, vi, 2, want_vec=4), vr, vi, 2, exact=True)
        check_stats(run_stats(g, I8, vr, vi, 1, np.full(4, 100.0), True, offset=1, want_vec=1), vr, vi, 1, np.full(4, 100.0), True, exact=True)


def test_stats_dc_offset_over_a_long_block(g):
    """one block of 2^21 samples with a DC offset 100 times the noise: the case a single running float32 sum misses"""
    rng = np.random.default_rng(43)
    N = 1 << 21
    vr = (rng.standard_normal((1, 2, N)) + 100.0).astype(np.float32)
    vi = (rng.standard_normal((1, 2, N)) - 100.0).astype(np.float32)
    worst = check_stats(run_stats(g, PLANAR, vr, vi, 1, want_vec=4), vr, vi, 1)
    assert worst <= 1e-5


# ---- AGC, graph capture, refusals -----------------------------------------------------------------------------------------------
def test_agc_update_equals_its_host_twin(g):
    import torch
    fe = g.frontend
    ctx = g.get_context()
    rng = np.random.default_rng(51)
    M = 8
    vr = (rng.standard_normal((2, M, 5000)) * 10.0 ** rng.uniform(-2, 3, (1, M, 1)) + 3.0).astype(np.float32)
    vi = (rng.standard_normal((2, M, 5000)) * 10.0 ** rng.uniform(-2, 3, (1, M, 1)) - 1.0).astype(np.float32)
    vr[:, 5], vi[:, 5] = 0.0, 0.0   # no power
    vr[:, 6], vi[:, 6] = np.nan, 0  # nothing kept
    got = run_stats(g, PLANAR, vr, vi, 2)
    st = torch.from_numpy(got.view(np.uint8).reshape(1, M, 48).copy()).to(ctx.device)
    for target, factor, dc in ((16.0, 0.0, False), (16.0, 4.0, True), (2000.0, -1.0, True)):
        dev = fe.agc_params(fe.SampleStats(st), target, factor, dc, ctx).cpu().numpy()
        host = fe.agc_params_host(got[0], target, factor, dc)
        assert same_bits(dev, host.view(np.float32).reshape(M, 4)), (dev, host)
        assert dev[5, 0] == 0 and dev[6, 0] == 0 and np.isposinf(dev[5, 3]) and np.isposinf(dev[6, 3])
        assert (dev[:5, 0] > 0).all()


def test_the_iteration_is_capturable_in_a_stream_graph(g):
    """stats -> agc -> stats -> agc -> condition, captured once on the context's own stream and replayed twice: the eager bits"""
    import torch
    stream = torch.cuda.Stream()  # (the default stream cannot be captured)
    ctx = g.Context(stream=stream)
    rng = np.random.default_rng(61)
    B, M, N = 2, 4, 4096
    vr, vi = (rng.standard_normal((B, M, N)).astype(np.float32) * 5 for _ in range(2))
    pulse = rng.random((B, 1, N)) < 0.1
    vr = np.where(pulse, vr + 500.0, vr).astype(np.float32)
    ibuf = ref.make_buffers(PLANAR, B, M, N, B * N, N)
    ref.put(ibuf, PLANAR, ref.index(B, M, N, B * N, N), vr, vi)
    d_in = to_dev(g, ibuf)
    desc = dev_desc(g, d_in, PLANAR, M, N, B * N, N)
    out = torch.zeros((M, B * N, 2), dtype=torch.int8, device=ctx.device)
    odesc = g._lib.SignalDesc(out.data_ptr(), None, I8, M, N, B * N, N, 0)
    st = torch.zeros((1, M, 48), dtype=torch.uint8, device=ctx.device)
    prm = torch.zeros((M, 4), dtype=torch.float32, device=ctx.device)
    cnt = torch.zeros((M, 2), dtype=torch.int64, device=ctx.device)
    cfg = g.frontend._agc_config(16.0, 4.0, True)
    vp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    def sequence():
        ctx.check(ctx.lib.gat_sample_stats(ctx._h, C.byref(desc), B, B, None, 1, vp(st)), "gat_sample_stats")
        ctx.check(ctx.lib.gat_agc_update(ctx._h, vp(st), M, C.byref(cfg), vp(prm)), "gat_agc_update")
        ctx.check(ctx.lib.gat_sample_stats(ctx._h, C.byref(desc), B, B, vp(prm), 1, vp(st)), "gat_sample_stats")
        ctx.check(ctx.lib.gat_agc_update(ctx._h, vp(st), M, C.byref(cfg), vp(prm)), "gat_agc_update")
        ctx.check(ctx.lib.gat_condition_samples(ctx._h, C.byref(desc), B, vp(prm), 1, C.byref(odesc), vp(cnt)), "gat_condition_samples")

    torch.cuda.synchronize()  # the inputs were made on another stream
    sequence()  # eager: sizes the scratch, and is the reference
    ctx.sync()
    eager = [t.cpu().numpy().copy() for t in (out, st, prm, cnt)]
    assert eager[3][:, 0].min() > 0.05 * B * N and np.isfinite(eager[2]).all()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        sequence()
    for _ in range(2):
        for t in (out, st, prm, cnt):
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for t, want in zip((out, st, prm, cnt), eager):
            assert same_bits(t.cpu().numpy(), want)
    del graph
    ctx.close()


def test_refusals_on_the_device(g):
    import torch
    ctx = g.get_context()
    M, N, B = 2, 64, 2
    i_t = [torch.zeros(B * N * M + 16, dtype=torch.float32, device=ctx.device) for _ in range(2)]
    o_t = [torch.full((B * N * M + 16, 2), 77, dtype=torch.int8, device=ctx.device)]
    prm = torch.ones((M, 4), dtype=torch.float32, device=ctx.device)
    st = torch.full((1, M, 48), 0x5A, dtype=torch.uint8, device=ctx.device)
    good_i = dict(layout=PLANAR, M=M, N=N, ant_stride=B * N, block_stride=N)
    good_o = dict(layout=I8, M=M, N=N, ant_stride=B * N, block_stride=N)

    def call(ikw=None, okw=None, nb=B, params=prm, flags=0, null_in=False, null_out=False, chan=(0, 0), o_tens=None):
        i, o = dict(good_i, **(ikw or {})), dict(good_o, **(okw or {}))
        ot = o_tens or o_t
        di = g._lib.SignalDesc(i_t[0].data_ptr(), i.get("im", i_t[1].data_ptr()), i["layout"], i["M"], i["N"], i["ant_stride"], i["block_stride"], chan[0])
        do = g._lib.SignalDesc(ot[0].data_ptr() + o.get("shift", 0), o.get("im", None), o["layout"], o["M"], o["N"], o["ant_stride"], o["block_stride"], chan[1])
        return ctx.lib.gat_condition_samples(ctx._h, None if null_in else C.byref(di), nb, C.c_void_p(params.data_ptr()) if params is not None else None,
                                             flags, None if null_out else C.byref(do), None)

    assert call(null_in=True) == ERR_ARG and call(null_out=True) == ERR_ARG and call(params=None) == ERR_ARG
    assert call(nb=0) == ERR_ARG and call(ikw=dict(N=0), okw=dict(N=0)) == ERR_ARG and call(flags=4) == ERR_ARG
    assert call(ikw=dict(ant_stride=-1)) == ERR_ARG and call(okw=dict(block_stride=-1)) == ERR_ARG and call(okw=dict(ant_stride=0)) == ERR_ARG
    assert call(okw=dict(M=1)) == ERR_ARG and call(okw=dict(N=N - 1)) == ERR_ARG
    assert call(ikw=dict(im=None)) == ERR_ARG and call(okw=dict(im=i_t[1].data_ptr())) == ERR_ARG
    assert call(ikw=dict(layout=7)) == ERR_ARG and call(okw=dict(layout=-1)) == ERR_ARG
    assert call(chan=(4, 0)) == ERR_UNSUPPORTED and call(chan=(0, 4)) == ERR_UNSUPPORTED
    assert call(ikw=dict(M=65), okw=dict(M=65)) == ERR_RANGE
    # an int8 output inside the input's re plane: overlap without identity
    as_i8 = [i_t[0].view(torch.int8).view(-1, 2)]
    assert call(o_tens=as_i8, okw=dict(shift=16)) == ERR_ARG
    assert b"overlaps" in ctx.lib.gat_last_error(ctx._h)
    # gat_sample_stats shares the signal side's refusals
    di = g._lib.SignalDesc(i_t[0].data_ptr(), i_t[1].data_ptr(), PLANAR, M, N, B * N, N, 0)
    assert ctx.lib.gat_sample_stats(ctx._h, C.byref(di), B, 0, None, 0, C.c_void_p(st.data_ptr())) == ERR_ARG
    assert ctx.lib.gat_sample_stats(ctx._h, C.byref(di), B, 1, None, 2, C.c_void_p(st.data_ptr())) == ERR_ARG
    assert ctx.lib.gat_sample_stats(ctx._h, C.byref(di), B, 1, None, 0, None) == ERR_ARG
    di.chan_stride = 8
    assert ctx.lib.gat_sample_stats(ctx._h, C.byref(di), B, 1, None, 0, C.c_void_p(st.data_ptr())) == ERR_UNSUPPORTED
    bad = g.frontend._agc_config(float("nan"), 0.0, False)
    assert ctx.lib.gat_agc_update(ctx._h, C.c_void_p(st.data_ptr()), M, C.byref(bad), C.c_void_p(prm.data_ptr())) == ERR_ARG
    ctx.sync()
    assert (o_t[0].cpu().numpy() == 77).all() and (st.cpu().numpy() == 0x5A).all() and (i_t[0].cpu().numpy() == 0).all()
    assert call() == OK  # the harness itself is sound: the unmodified call runs
    ctx.sync()


def test_python_layer_round_trip(g):
    """requantize on a planar float stream: the int8 image has the target level, its descriptor is padded to 16 bytes and it is
    what condition_samples_host makes of the same records"""
    import torch
    ctx = g.get_context()
    rng = np.random.default_rng(71)
    M, N, B, S = 2, 1001, 3, 1004  # input blocks 1004 floats apart: on 16-byte boundaries
    re = torch.from_numpy((rng.standard_normal((M, B * S)) * 7.0).astype(np.float32)).to(ctx.device)
    im = torch.from_numpy((rng.standard_normal((M, B * S)) * 7.0).astype(np.float32)).to(ctx.device)
    out, desc, counts, params = g.requantize((re, im), N, B, target_rms=16.0, blank_factor=0.0, block_stride=S)
    ctx.sync()
    assert out.dtype == torch.int8 and tuple(out.shape) == (M, B * 1008, 2) and desc.block_stride == 1008 and desc.layout == I8
    assert ctx.last_launch_info()["vec"] == 4
    o = out.cpu().numpy().reshape(M, B, 1008, 2)
    assert not o[:, :, N:].any()
    rms = np.sqrt((o[:, :, :N].astype(np.float64) ** 2).mean(axis=(1, 2, 3)))
    assert np.all(np.abs(rms - 16.0) < 0.5), rms
    assert counts.cpu().numpy().sum() == 0
    vr = re.cpu().numpy().reshape(M, B, S)[:, :, :N].transpose(1, 0, 2)
    vi = im.cpu().numpy().reshape(M, B, S)[:, :, :N].transpose(1, 0, 2)
    p = params.cpu().numpy().copy().view(g.frontend.COND_PARAMS_DTYPE).reshape(M)
    er, ei, _ = ref.condition(vr, vi, p, I8)
    assert np.array_equal(o[:, :, :N, 0].transpose(1, 0, 2), er) and np.array_equal(o[:, :, :N, 1].transpose(1, 0, 2), ei)
    st = g.sample_stats((re, im), N, B, blocks_per_estimate=2, block_stride=S).numpy()
    assert st.shape == (2, M) and st["kept"].tolist() == [[2 * N] * M, [N] * M]
