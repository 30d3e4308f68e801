"""GPU tests of the sample spectrum (include/gat.h gat_sample_spectrum; csrc/gat_spec.hip).

The device's sums are compared with the library's host twin BIT FOR BIT over the whole output allocation, a canary border
included (the twin itself is held to the FP64 restatement by tests/test_spectrum_host.py on the CPU); gat_last_launch_info says
which load path ran and every case asserts that it is the aligned one exactly when the rule of gat.h holds.  Shapes are the
smallest that take every path: every number of points a lane keeps (F = 64 .. 1024: 4, with 16, 4 and 1 transforms a workgroup;
F = 4096: 16), a first pass of one stage (F = 128, 512) and of two, one segment and several with unused tail samples, a round of
teams that is not full, and more rounds than workgroups."""
import ctypes as C

import numpy as np
import pytest

from tests import spec_ref as ref
from tests.spec_ref import CF32, I8, I16, LAYOUTS, PLANAR, VEC_SAMPLES, same_bits

pytestmark = pytest.mark.gpu

OK, ERR_ARG, ERR_RANGE, ERR_UNSUPPORTED = 0, 1, 2, 4
STEP = {PLANAR: 4, CF32: 8, I16: 4, I8: 2}  # bytes per sample of a buffer
BORDER = 64                                  # canary floats on either side of the output


@pytest.fixture(scope="module")
def g():
    import gpuacceleratedtracking_amd as g
    g.load_library()
    return g


def up(n, to):
    return -(-n // to) * to


def geometry(layout, B, N, H, mode):
    """(ant_stride, block_stride, offset) of a case.  "aligned": every block of every antenna on a 16-byte boundary; "off": the
    same one sample on; "odd": an odd block_stride (ant_stride where there is one block); "overlap": blocks every H samples"""
    vs = VEC_SAMPLES[layout]
    bs = up(N + 3, vs)
    if mode == "overlap":
        bs = H
    elif mode == "odd" and B > 1:
        bs = N + 1 + (N % 2)
    a_s = up((B - 1) * bs + N + 5, vs)
    if mode == "odd" and B == 1:
        a_s += 1
    return a_s, bs, 1 if mode == "off" else 0


def aligned_rule(desc, B, H):
    vs = VEC_SAMPLES[desc.layout]
    return (desc.re % 16 == 0 and (desc.layout != PLANAR or desc.im % 16 == 0) and (desc.num_ants == 1 or desc.ant_stride % vs == 0) and
            (B == 1 or desc.block_stride % vs == 0) and H % vs == 0)


def run_both(g, layout, B, M, F, H, S, mode, seed, window="hann", calls=2):
    """random samples through the host twin and through the device; asserts the load path against the rule and identical bytes
    over the whole output allocation on every one of `calls` calls.  Returns (float32 [B, M, F], launch info)."""
    import torch
    sp, fe = g.spectrum, g.frontend
    ctx = g.get_context()
    rng = np.random.default_rng(seed)
    N = (S - 1) * H + F + min(3, H - 1)  # tail samples no segment uses
    a_s, bs, off = geometry(layout, B, N, H, mode)
    span = (B - 1) * bs + N
    sr, si = ref.random_samples(rng, layout, (M, span), special=False)
    buf = ref.make_buffers(layout, 1, M, span, a_s, 0, off)
    ref.put(buf, layout, ref.index(1, M, span, a_s, 0, off), sr[None], si[None])
    w = ref.window(window, F) if isinstance(window, str) else window
    want = np.full(B * M * F + 2 * BORDER, -3.25, np.float32)
    rc = sp.sample_spectrum_host(fe.host_desc(buf[0], buf[1] if layout == PLANAR else None, layout, M, N, a_s, bs, off), B, w, F, H,
                                 want[BORDER:BORDER + B * M * F])
    assert rc == OK
    dev = [torch.from_numpy(b).to(ctx.device) for b in buf]
    o = off * STEP[layout]
    desc = g._lib.SignalDesc(dev[0].data_ptr() + o, dev[1].data_ptr() + o if layout == PLANAR else None, layout, M, N, a_s, bs, 0)
    w_dev = torch.from_numpy(w).to(ctx.device)
    out = torch.full((B * M * F + 2 * BORDER,), -3.25, dtype=torch.float32, device=ctx.device)
    cfg = sp._config(F, H)
    info = None
    for _ in range(calls):
        ctx.check(ctx.lib.gat_sample_spectrum(ctx._h, C.byref(desc), B, C.c_void_p(w_dev.data_ptr()), C.byref(cfg),
                                              C.c_void_p(out.data_ptr() + 4 * BORDER)), "gat_sample_spectrum")
        ctx.sync()
        info = ctx.last_launch_info()
        rule = aligned_rule(desc, B, H)
        assert info["vec"] == (VEC_SAMPLES[layout] if rule else 1), (info, layout, mode)
        assert info["threads"] == 256 and info["splits"] == 1 and info["ant_tile"] == 1 and info["workgroups"] >= 1
        assert info["channels_per_wg"] == 256 // (F // max(4, F // 256))
        got = out.cpu().numpy()
        assert same_bits(got, want), f"device and host twin differ: layout {layout} B={B} M={M} F={F} H={H} S={S} {mode} vec={info['vec']}"
    return got[BORDER:BORDER + B * M * F].reshape(B, M, F), info


FS, MS, BS, SS = (64, 256, 1024, 4096), (1, 3), (1, 5), (1, 2, 5)
HOPS = ("F", "F/2", "F/4+8", "7")
MODES = ("aligned", "off", "odd", "overlap")


def hop_of(name, F):
    return {"F": F, "F/2": F // 2, "F/4+8": F // 4 + 8, "7": 7}[name]


def subset():
    """16 cases that between them hold every layout, F, M, B, S, hop and mode of the lists above -- and every (F, layout) pair:
    the kernel's instances are (layout, load path, points a lane), and F = 64 .. 1024 share the instances of four points
    (those of eight, F = 2048 alone, run in test_the_sizes_between)"""
    out = []
    for k in range(16):
        F, layout = FS[k % 4], LAYOUTS[(k + k // 4) % 4]
        out.append((layout, F, MS[(k + k // 4) % 2], BS[(k // 2 + k // 8) % 2], SS[(k + k // 3) % 3], HOPS[(k + k // 4 + k // 8) % 4], MODES[(k // 4 + k) % 4], k))
    for vals, col in ((LAYOUTS, 0), (FS, 1), (MS, 2), (BS, 3), (SS, 4), (HOPS, 5), (MODES, 6)):
        assert {c[col] for c in out} == set(vals), col
    assert {(c[0], c[1]) for c in out} == {(la, F) for la in LAYOUTS for F in FS}
    return out


@pytest.mark.parametrize("layout,F,M,B,S,hop,mode,k", subset())
def test_device_equals_host_twin(g, layout, F, M, B, S, hop, mode, k):
    run_both(g, layout, B, M, F, hop_of(hop, F), S, mode, 500 + k)


@pytest.mark.parametrize("F,layout", [(128, I8), (512, PLANAR), (2048, PLANAR), (2048, CF32), (2048, I16), (2048, I8)])
def test_the_sizes_between(g, F, layout):
    """F = 128 and 512: a first pass of one stage; F = 2048: eight points a lane, the only size that runs those instances, so
    every layout on both paths.  Aligned and one sample off give the same bits."""
    a, ia = run_both(g, layout, 3, 2, F, F // 2, 3, "aligned", 40 + F, calls=1)
    b, ib = run_both(g, layout, 3, 2, F, F // 2, 3, "off", 40 + F, calls=1)
    assert ia["vec"] > 1 and ib["vec"] == 1 and same_bits(a, b)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_every_layout_on_both_paths_at_every_lane_size(g, layout):
    for F in (256, 4096):
        a, ia = run_both(g, layout, 2, 3, F, F // 4 + 8, 2, "aligned", 77, calls=1)
        b, ib = run_both(g, layout, 2, 3, F, F // 4 + 8, 2, "off", 77, calls=1)
        assert ia["vec"] == VEC_SAMPLES[layout] and ib["vec"] == 1 and same_bits(a, b)


def test_more_rounds_than_workgroups(g):
    """3 x 900 one-segment blocks every 8 samples of a short stream: 2700 work units of F = 1024, one to a workgroup's round --
    more than the eight workgroups a compute unit the call launches, so workgroups walk several rounds"""
    _, info = run_both(g, I8, 900, 3, 1024, 8, 1, "overlap", 5, calls=1)
    assert info["vec"] == 8 and info["workgroups"] < 2700
    _, info = run_both(g, PLANAR, 700, 3, 64, 7, 2, "overlap", 6, calls=1)
    assert info["vec"] == 1 and info["channels_per_wg"] == 16 and info["workgroups"] == -(-2100 // 16)


def test_refusals_launch_nothing(g):
    """one refusal of each class on the device entry point: the status, a message, the output and the launch info untouched"""
    import torch
    ctx = g.get_context()
    sp = g.spectrum
    F, H, M, B = 64, 32, 2, 2
    N = F + H
    run_both(g, CF32, 1, 1, 64, 64, 1, "aligned", 1, calls=1)  # a launch whose info the refusals must leave
    before = ctx.last_launch_info()
    x = torch.zeros((M, B * N, 2), dtype=torch.float32, device=ctx.device)
    y = torch.full((B * M * F,), -3.25, dtype=torch.float32, device=ctx.device)
    w = torch.ones(F, dtype=torch.float32, device=ctx.device)
    SignalDesc = g._lib.SignalDesc

    def call(nb=B, cfg=None, chan=0, N=N, out=None, window=w.data_ptr()):
        d = SignalDesc(x.data_ptr(), None, CF32, M, N, B * (F + H), F + H, chan)
        cfg = sp._config(F, H) if cfg is None else cfg
        return ctx.lib.gat_sample_spectrum(ctx._h, C.byref(d), nb, C.c_void_p(window), C.byref(cfg), C.c_void_p(y.data_ptr() if out is None else out))

    cases = [(ERR_ARG, dict(nb=0)), (ERR_ARG, dict(window=None)), (ERR_ARG, dict(cfg=sp._config(F, H, flags=1))), (ERR_ARG, dict(N=F - 1)),
             (ERR_ARG, dict(out=x.data_ptr() + 16)), (ERR_RANGE, dict(cfg=sp._config(96, H))), (ERR_RANGE, dict(cfg=sp._config(F, F + 1))),
             (ERR_RANGE, dict(cfg=sp._config(8192, H))), (ERR_UNSUPPORTED, dict(chan=4))]
    for code, kw in cases:
        assert call(**kw) == code, kw
        assert ctx.lib.gat_last_error(ctx._h)
        assert ctx.last_launch_info() == before
    ctx.sync()
    assert (y.cpu().numpy() == -3.25).all()
    assert call() == OK
    ctx.sync()
    assert (y.cpu().numpy() == 0).all()


def test_spectrum_stream_is_the_float64_sum_of_the_twins_blocks(g):
    """the stream wrapper cuts 30011 samples of 3 antennas into overlapping blocks by descriptor; its mean is the float64 sum, in
    block order, of the host twin's sums over the same blocks, divided by the segment count -- to the last bit"""
    import torch
    sp, fe = g.spectrum, g.frontend
    ctx = g.get_context()
    rng = np.random.default_rng(21)
    M, total, F, H, start = 3, 30011, 256, 96, 5
    h = rng.integers(-100, 100, (M, total + 9, 2)).astype(np.int8)
    x = torch.from_numpy(h).to(ctx.device)
    for units in (2048, 40, 1):
        psd, S = sp.spectrum_stream(x, F, total, H, "hamming", start, units_wanted=units)
        S_total, S_block, B, S_rest = sp.stream_partition(total, F, H, M, units)
        assert S == S_total == (total - F) // H + 1 and B * S_block + S_rest == S_total
        w = ref.window("hamming", F)
        blocks = np.zeros((B, M, F), np.float32)
        assert sp.sample_spectrum_host(fe.host_desc(h, None, I8, M, (S_block - 1) * H + F, total + 9, S_block * H, start), B, w, F, H, blocks) == OK
        acc = np.zeros((M, F))
        for b in range(B):
            acc = acc + blocks[b].astype(np.float64)
        if S_rest:
            rest = np.zeros((1, M, F), np.float32)
            assert sp.sample_spectrum_host(fe.host_desc(h, None, I8, M, (S_rest - 1) * H + F, total + 9, 0, start + B * S_block * H), 1, w, F, H, rest) == OK
            acc = acc + rest[0].astype(np.float64)
        assert psd.dtype == np.float64 and psd.shape == (M, F) and same_bits(psd, acc / S_total)
    assert (units, B, S_rest > 0) == (1, 1, False)  # the last partition: one block of every segment


def test_sample_spectrum_takes_what_filter_samples_takes(g):
    """the Python call on a planar pair and on an int16 tensor, a named window and a caller's, against the FP64 restatement"""
    import torch
    sp = g.spectrum
    ctx = g.get_context()
    rng = np.random.default_rng(8)
    M, N, B, F = 2, 700, 2, 128
    xr, xi = (rng.standard_normal((M, B * N)).astype(np.float32) for _ in range(2))
    got, S = sp.sample_spectrum((torch.from_numpy(xr).to(ctx.device), torch.from_numpy(xi).to(ctx.device)), F, N, B)
    assert S == (N - F) // 64 + 1 and tuple(got.shape) == (B, M, F) and got.dtype == torch.float32
    lr, li = (a.reshape(M, B, N).transpose(1, 0, 2) for a in (xr, xi))
    want, _, A = ref.spectrum(lr, li, ref.window("hann", F), F, 64)
    assert (np.abs(got.cpu().numpy() - want) <= ref.bound_power(F, A)[..., None]).all()
    wv = rng.uniform(-1, 1, F).astype(np.float32)
    x16 = rng.integers(-3000, 3000, (M, N, 2)).astype(np.int16)
    got, S = sp.sample_spectrum(torch.from_numpy(x16).to(ctx.device), F, N - 3, 1, hop=50, window=wv, start=3)
    want, _, A = ref.spectrum(x16[None, :, 3:, 0], x16[None, :, 3:, 1], wv, F, 50)
    assert S == (N - 3 - F) // 50 + 1 and (np.abs(got.cpu().numpy() - want) <= ref.bound_power(F, A)[..., None]).all()
    with pytest.raises(g.GatError):
        sp.sample_spectrum(torch.from_numpy(x16).to(ctx.device), 96, N)
    with pytest.raises(ValueError):
        sp.sample_spectrum(torch.from_numpy(x16).to(ctx.device), F, N, window="kaiser")


def test_auto_notch_without_a_tone_returns_the_input(g):
    import torch
    ctx = g.get_context()
    rng = np.random.default_rng(3)
    M, total = 2, 20000
    re, im = (torch.from_numpy((14.13 * rng.standard_normal((M, total))).astype(np.float32)).to(ctx.device) for _ in range(2))
    out, desc, tones = g.auto_notch((re, im), total)
    assert tones == [] and out[0] is re and out[1] is im
    assert desc.num_samples == total and desc.num_ants == M and desc.re == re.data_ptr() and desc.im == im.data_ptr()
