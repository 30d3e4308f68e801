"""GPU tests of the sample filter (include/gat.h gat_filter_samples; csrc/gat_fir.hip).

The filtered stream is compared with the library's host twin BIT FOR BIT over the whole output allocation, sentinels included --
so every guard cell around every output region is checked by every case -- (the twin itself is held to the FP64 restatement by
tests/test_filter_host.py on the CPU); gat_last_launch_info says which kernel ran and every case asserts that it is the tiled
one exactly when the fast-path rule holds.  Shapes are the smallest that take every path: one tap and the most, every decimation
class, antennas beyond a power of two, one and several blocks, a single output, a ragged wave and a second round of the workgroup."""
import ctypes as C

import numpy as np
import pytest

from tests import fir_ref as ref
from tests.fir_ref import CF32, I8, I16, LAYOUTS, OUT_LAYOUTS, PLANAR, VEC_SAMPLES, same_bits

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


def fast_path(desc, B):
    """the rule of gat.h: every block of every antenna starts on a 16-byte boundary"""
    vs = VEC_SAMPLES[desc.layout]
    return (desc.re % 16 == 0 and (desc.layout != PLANAR or desc.im % 16 == 0) and (desc.num_ants == 1 or desc.ant_stride % vs == 0) and
            (B == 1 or desc.block_stride % vs == 0))


def up(n, to):
    return -(-n // to) * to


def geometry(li, lo, B, M, N, T, D, mode):
    """strides and offsets of a case: mode "padded" (every block on a 16-byte boundary), "overlap" (overlap-save: block_stride =
    Q D, output blocks back to back; aligned only where that happens to be) or "misaligned" (the padded case one sample on)"""
    Q = ref.num_outputs(N, T, D)
    vi, vo = VEC_SAMPLES[li], VEC_SAMPLES[lo]
    if mode == "overlap":
        ibs, obs = Q * D, Q
    else:
        ibs, obs = up(N + 3, vi), up(Q + 1, vo)
    ias, oas = up((B - 1) * ibs + N + 5, vi), up(B * obs + 3, vo)
    off = 1 if mode == "misaligned" else 0
    return Q, ibs, obs, ias, oas, off


def run_both(g, li, lo, B, M, N, T, D, step, phase, mode, seed, calls=2):
    """random samples through the host twin and through the device from identical, sentinel-filled allocations; asserts the kernel
    that ran against the fast-path rule and identical bytes over the whole output allocation, on every one of `calls` calls.
    Returns (logical device output (re, im) [B, M, Q], launch info)."""
    import torch
    f = g.filtering
    ctx = g.get_context()
    rng = np.random.default_rng(seed)
    Q, ibs, obs, ias, oas, off = geometry(li, lo, B, M, N, T, D, mode)
    span = (B - 1) * ibs + N
    taps = (rng.standard_normal(T) + 1j * rng.standard_normal(T)) / np.sqrt(T)
    g_re, g_im = f._tap_planes(taps)
    sr, si = ref.random_samples(rng, li, (M, span), special=False)
    ibuf = ref.make_buffers(li, 1, M, span, ias, 0, off)
    ref.put(ibuf, li, ref.index(1, M, span, ias, 0, off), sr[None], si[None])
    obuf = ref.make_buffers(lo, B, M, Q, oas, obs, off, fill=-3.25)
    d_in, d_out = to_dev(g, ibuf), to_dev(g, obuf)
    rc = f.filter_samples_host(f.host_desc(ibuf[0], ibuf[1] if li == PLANAR else None, li, M, N, ias, ibs, off), B, (g_re, g_im),
                               f.host_desc(obuf[0], obuf[1] if lo == PLANAR else None, lo, M, Q, oas, obs, off), D, step, phase)
    assert rc == OK
    t_re, t_im = torch.from_numpy(g_re).to(ctx.device), torch.from_numpy(g_im).to(ctx.device)
    idesc, odesc = dev_desc(g, d_in, li, M, N, ias, ibs, off), dev_desc(g, d_out, lo, M, Q, oas, obs, off)
    cfg = f._config(T, D, step, phase)
    info = None
    for _ in range(calls):
        ctx.check(ctx.lib.gat_filter_samples(ctx._h, C.byref(idesc), B, C.c_void_p(t_re.data_ptr()), C.c_void_p(t_im.data_ptr()), C.byref(cfg),
                                             C.byref(odesc)), "gat_filter_samples")
        ctx.sync()
        info = ctx.last_launch_info()
        rule = fast_path(idesc, B) and fast_path(odesc, B)
        assert (info["vec"] > 1) == rule and info["vec"] == (VEC_SAMPLES[li] if rule else 1), (info, li, lo, mode)
        assert info["threads"] == 256 and info["ant_tile"] == 1 and info["workgroups"] >= 1
        for got, want in zip(d_out, obuf):
            assert same_bits(got.cpu().numpy(), want), f"device and host twin differ: layouts {li}->{lo} B={B} M={M} N={N} T={T} D={D} {mode} vec={info['vec']}"
    return ref.get([t.cpu().numpy() for t in d_out], lo, ref.index(B, M, Q, oas, obs, off)), info


TS, DS, MS, BS, QS = (1, 2, 7, 64, 255, 256), (1, 2, 3, 5, 8, 64), (1, 3, 8, 9), (1, 3), (1, 63, 257)
MODES = ("padded", "overlap", "misaligned")


def subset():
    """24 cases that between them hold every input and output layout, every T, D, M, B, Q and mode of the lists above, the
    oscillator on and off"""
    out = []
    for k in range(24):
        li, lo = LAYOUTS[k % 4], OUT_LAYOUTS[(k // 4) % 2]
        T, D = TS[(5 * k) % 6], DS[(5 * k + k // 6) % 6]
        M, B, Q = MS[(k + k // 4) % 4], BS[(k + k // 8) % 2], QS[(k + k // 3) % 3]
        out.append((li, lo, T, D, M, B, Q, MODES[k % 3], (k // 2) % 2 == 1, k))
    for vals, col in ((LAYOUTS, 0), (OUT_LAYOUTS, 1), (TS, 2), (DS, 3), (MS, 4), (BS, 5), (QS, 6), (MODES, 7), ((False, True), 8)):
        assert {c[col] for c in out} == set(vals), col
    return out


@pytest.mark.parametrize("li,lo,T,D,M,B,Q,mode,nco,k", subset())
def test_device_equals_host_twin(g, li, lo, T, D, M, B, Q, mode, nco, k):
    N = Q * D + T - 1 + (k % D if mode != "overlap" else 0)  # (N - T) not always a multiple of D
    step, phase = ((-1) ** k * (0.013 + 0.0371 * k), 0.1 * k - 1.0) if nco else (0.0, 0.0)
    run_both(g, li, lo, B, M, N, T, D, step, phase, mode, 100 + k)


@pytest.mark.parametrize("T,D,li", [(1, 3, I16), (2, 64, PLANAR), (7, 2, I8), (64, 8, CF32), (255, 5, I8), (256, 1, PLANAR)])
def test_every_tap_count_runs_the_tiled_kernel(g, T, D, li):
    """the subset above aligns its cases by mode, not by T: here every T of the list goes through the tiled kernel, several blocks
    and antennas, a second round of the workgroup (Q = 300), the oscillator on"""
    _, info = run_both(g, li, OUT_LAYOUTS[T % 2], 3, 3, 300 * D + T - 1 + D // 2, T, D, 0.0731, 0.25, "padded", 300 + T, calls=1)
    assert info["vec"] > 1


@pytest.mark.parametrize("li,lo,T,D,Q", [(PLANAR, PLANAR, 7, 1, 3 * 4096 + 777), (I8, CF32, 64, 5, 3 * 3072 + 500), (I16, PLANAR, 33, 2, 3 * 4096 + 1)])
def test_one_long_block_is_cut_into_chunks(g, li, lo, T, D, Q):
    """one (block, antenna) pair long enough for three chunks of whole tiles and a ragged last one"""
    _, info = run_both(g, li, lo, 1, 1, Q * D + T - 1, T, D, 0.0625, 0.5, "padded", 7, calls=1)
    assert info["vec"] > 1 and info["splits"] >= 3 and info["workgroups"] == info["splits"]
    _, info = run_both(g, li, lo, 1, 1, Q * D + T - 1, T, D, 0.0625, 0.5, "misaligned", 7, calls=1)
    assert info["vec"] == 1 and info["splits"] >= 3


@pytest.mark.parametrize("li", LAYOUTS)
def test_both_kernels_give_the_same_bits(g, li):
    """the same values (the same seed) through the tiled kernel and, one sample off its alignment, through the general one"""
    for lo in OUT_LAYOUTS:
        args = (g, li, lo, 2, 3, 700, 20, 3, 0.21, 0.3)
        (ar, ai), a = run_both(*args, "padded", 55, calls=1)
        (br, bi), b = run_both(*args, "misaligned", 55, calls=1)
        assert a["vec"] > 1 and b["vec"] == 1
        assert same_bits(ar, br) and same_bits(ai, bi)


def test_partition_invariance_on_the_device(g):
    """filter_stream over one stream as 1, 3 and 7 overlap-save blocks: one seamless output, the same bits"""
    import torch
    ctx = g.get_context()
    rng = np.random.default_rng(9)
    D, T, M, total_q = 5, 64, 2, 231
    total = total_q * D + T - 1
    W = up(total, 8)  # antennas on 16 bytes: one block runs the tiled kernel, blocks every Q D = 385 or 165 samples the general one
    x = torch.from_numpy(rng.integers(-100, 100, (M, W, 2)).astype(np.int8)).to(ctx.device)
    taps = g.shift_taps(g.lowpass_taps(T, 0.08), 0.125)
    outs = []
    for B in (1, 3, 7):
        (yr, yi), desc = g.filter_stream(x, taps, total, D, nco_step=0.125, nco_phase=0.3, num_blocks=B)
        ctx.sync()
        assert (ctx.last_launch_info()["vec"] > 1) == (B == 1)
        assert desc.num_samples == total_q and tuple(yr.shape) == (M, total_q)
        outs.append((yr.cpu().numpy(), yi.cpu().numpy()))
    for yr, yi in outs[1:]:
        assert same_bits(yr, outs[0][0]) and same_bits(yi, outs[0][1])
    # and they are the host twin's
    h = x.cpu().numpy()
    o = [np.zeros((M, total_q), np.float32), np.zeros((M, total_q), np.float32)]
    f = g.filtering
    assert f.filter_samples_host(f.host_desc(h, None, I8, M, total, W, total), 1, taps, f.host_desc(o[0], o[1], PLANAR, M, total_q, total_q, total_q),
                                 D, 0.125, 0.3) == OK
    assert same_bits(o[0], outs[0][0]) and same_bits(o[1], outs[0][1])


def test_filter_samples_allocates_padded_blocks(g):
    """the Python call: blocks padded to 16 bytes (the tiled kernel runs), zeros between them, planar and interleaved alike"""
    import torch
    ctx = g.get_context()
    rng = np.random.default_rng(13)
    M, N, B, T, D = 2, 203, 3, 9, 2
    xr, xi = (torch.from_numpy(rng.standard_normal((M, B * N)).astype(np.float32)).to(ctx.device) for _ in range(2))
    taps = rng.standard_normal(T)
    Q = ref.num_outputs(N, T, D)
    (yr, yi), desc = g.filter_samples((xr, xi), taps, N, B, D)
    ctx.sync()
    assert ctx.last_launch_info()["vec"] == 1  # a block_stride of 203 floats is not on 16 bytes
    y2, desc2 = g.filter_samples((xr, xi), taps, N, B, D, interleaved=True)
    ctx.sync()
    assert desc.num_samples == Q and desc.block_stride == up(Q, 4) and desc2.block_stride == up(Q, 2) and desc.num_ants == M
    want, _, _ = ref.fir(xr.cpu().numpy().reshape(M, B, N).transpose(1, 0, 2), xi.cpu().numpy().reshape(M, B, N).transpose(1, 0, 2), taps, D)
    for b in range(B):
        a = yr.cpu().numpy()[:, b * desc.block_stride:][:, :Q] + 1j * yi.cpu().numpy()[:, b * desc.block_stride:][:, :Q]
        c = y2.cpu().numpy()[:, b * desc2.block_stride:][:, :Q]
        assert np.abs(a - want[b]).max() <= 1e-5 * np.abs(want).max()
        assert same_bits(np.ascontiguousarray(c[..., 0]), np.ascontiguousarray(a.real.astype(np.float32)))
        assert same_bits(np.ascontiguousarray(c[..., 1]), np.ascontiguousarray(a.imag.astype(np.float32)))
        assert (yr.cpu().numpy()[:, b * desc.block_stride + Q:(b + 1) * desc.block_stride] == 0).all()
    with pytest.raises(g.GatError):
        g.filter_samples((xr, xi), np.ones(257), 300, 1)


def test_refusals_leave_the_output_untouched(g):
    import torch
    ctx = g.get_context()
    f = g.filtering
    M, N, B, T, D = 2, 64, 2, 5, 2
    Q = ref.num_outputs(N, T, D)
    x = torch.zeros((M, B * N, 2), dtype=torch.float32, device=ctx.device)
    y = torch.full((M, B * Q + 4, 2), -3.25, dtype=torch.float32, device=ctx.device)
    taps = torch.ones(T, dtype=torch.float32, device=ctx.device)
    SignalDesc = g._lib.SignalDesc
    i = SignalDesc(x.data_ptr(), None, CF32, M, N, B * N, N, 0)
    o = SignalDesc(y.data_ptr(), None, CF32, M, Q, B * Q + 4, Q, 0)

    def clone(d, **kw):
        n = SignalDesc(d.re, d.im, d.layout, d.num_ants, d.num_samples, d.ant_stride, d.block_stride, d.chan_stride)
        for k, v in kw.items():
            setattr(n, k, v)
        return n

    def call(sig=i, nb=B, cfg=None, out=o, taps_im=taps.data_ptr()):
        cfg = f._config(T, D, 0.0, 0.0) if cfg is None else cfg
        return ctx.lib.gat_filter_samples(ctx._h, C.byref(sig), nb, C.c_void_p(taps.data_ptr()), C.c_void_p(taps_im), C.byref(cfg), C.byref(out))

    cases = [(ERR_ARG, dict(nb=0)), (ERR_ARG, dict(taps_im=None)), (ERR_ARG, dict(cfg=f._config(T, D, float("nan"), 0.0))),
             (ERR_ARG, dict(sig=clone(i, num_samples=T - 1))), (ERR_ARG, dict(out=clone(o, num_samples=Q + 1))), (ERR_ARG, dict(out=clone(o, num_ants=1))),
             (ERR_ARG, dict(out=clone(o, re=x.data_ptr() + 8))), (ERR_RANGE, dict(cfg=f._config(257, D, 0.0, 0.0))), (ERR_RANGE, dict(cfg=f._config(T, 65, 0.0, 0.0))),
             (ERR_RANGE, dict(sig=clone(i, block_stride=(1 << 31)))), (ERR_UNSUPPORTED, dict(out=clone(o, layout=I8))),
             (ERR_UNSUPPORTED, dict(sig=clone(i, chan_stride=4)))]
    for code, kw in cases:
        assert call(**kw) == code, kw
        assert ctx.lib.gat_last_error(ctx._h)
    ctx.sync()
    assert (y.cpu().numpy() == -3.25).all()
    assert call() == OK
    ctx.sync()
    assert (y.cpu().numpy()[:, :B * Q] == 0).all() and (y.cpu().numpy()[:, B * Q:] == -3.25).all()
