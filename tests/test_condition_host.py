"""CPU tests of the sample conditioner's host twins (include/gat.h gat_condition_samples_host, gat_agc_update_host) against the
numpy restatement tests/cond_ref.py: the rule bit for bit over the 4 x 4 layout pairs, antenna counts, lengths and strides,
every edge of the rule by name, counts, sentinels, in-place and overlap, and the AGC's record against the FP64 formula."""
import ctypes as C

import numpy as np
import pytest

from tests import cond_ref as ref
from tests.cond_ref import CF32, I8, I16, LAYOUTS, PLANAR, records, same_bits

GAT_OK, GAT_ERR_ARG, GAT_ERR_RANGE, GAT_ERR_UNSUPPORTED = 0, 1, 2, 4


@pytest.fixture(scope="module")
def fe():
    from gpuacceleratedtracking_amd import frontend
    return frontend


def run_host(fe, li, lo, vr, vi, params, blank_all=False, ant_pad=0, block_pad=0, offset=0, counts=None):
    """vr, vi [B, M, N] in the input layout's dtype through the host twin; returns (yr, yi, counts, out buffers, out index, rc)."""
    B, M, N = vr.shape
    bs = N + block_pad
    as_ = B * bs + ant_pad
    ibuf = ref.make_buffers(li, B, M, N, as_, bs, offset)
    idx = ref.index(B, M, N, as_, bs, offset)
    ref.put(ibuf, li, idx, vr, vi)
    obuf = ref.make_buffers(lo, B, M, N, as_, bs, offset)
    idesc = fe.host_desc(ibuf[0], ibuf[1] if li == PLANAR else None, li, M, N, as_, bs, offset)
    odesc = fe.host_desc(obuf[0], obuf[1] if lo == PLANAR else None, lo, M, N, as_, bs, offset)
    cnt = np.zeros((M, 2), np.uint64) if counts is None else counts
    rc = fe.condition_samples_host(idesc, B, params, odesc, blank_all, cnt)
    yr, yi = ref.get(obuf, lo, idx)
    return yr, yi, cnt, obuf, idx, rc


def check_against_ref(fe, li, lo, vr, vi, params, blank_all=False, **kw):
    yr, yi, cnt, obuf, idx, rc = run_host(fe, li, lo, vr, vi, params, blank_all, **kw)
    assert rc == GAT_OK
    er, ei, ecnt = ref.condition(vr, vi, params, lo, blank_all)
    assert same_bits(yr, er) and same_bits(yi, ei), (li, lo, vr.shape)
    assert np.array_equal(cnt, ecnt)
    # nothing outside the described elements was written
    mask = np.ones(obuf[0].shape[0], bool)
    mask[idx.reshape(-1)] = False
    fresh = ref.make_buffers(lo, 1, 1, obuf[0].shape[0] - 3, 0, 0)
    for got, want in zip(obuf, fresh):
        assert same_bits(got[mask], want[mask])
    return yr, yi, cnt


@pytest.mark.parametrize("lo", LAYOUTS)
@pytest.mark.parametrize("li", LAYOUTS)
def test_host_twin_equals_the_restatement(fe, li, lo):
    rng = np.random.default_rng(100 + 4 * li + lo)
    for M in (1, 3, 8, 9):
        for N in (1, 7, 64, 257):
            vr, vi = ref.random_samples(rng, li, (1, M, N))
            p = records(fe, M)
            level = 40.0 if li in (PLANAR, CF32) else ref.LIMIT[li] / 3.0
            target = 3.0 if lo in (PLANAR, CF32) else ref.LIMIT[lo] / 2.5  # some components clip
            p["scale"] = (target / level) * rng.uniform(0.5, 1.5, M)
            p["dc_re"], p["dc_im"] = rng.uniform(-2, 2, M), rng.uniform(-2, 2, M)
            p["threshold"] = level * rng.uniform(1.0, 3.0, M)
            for blank_all in (False, True):
                check_against_ref(fe, li, lo, vr, vi, p, blank_all)


@pytest.mark.parametrize("lo", LAYOUTS)
@pytest.mark.parametrize("li", LAYOUTS)
def test_two_blocks_with_padded_strides_and_an_offset_base(fe, li, lo):
    rng = np.random.default_rng(7 + 4 * li + lo)
    vr, vi = ref.random_samples(rng, li, (2, 3, 37))
    p = records(fe, 3, scale=0.7, dc_re=0.25, threshold=60.0)
    check_against_ref(fe, li, lo, vr, vi, p, True, ant_pad=5, block_pad=11, offset=1)


def test_ties_go_to_even(fe):
    odd = np.array([1, 3, 5, 7, -1, -3, -5, -7, 253, -253], np.int16).reshape(1, 1, -1)
    yr, yi, cnt = check_against_ref(fe, I16, I8, odd, odd[..., ::-1].copy(), records(fe, 1, scale=0.5))
    assert yr.reshape(-1).tolist() == [0, 2, 2, 4, 0, -2, -2, -4, 126, -126]
    assert cnt[0].tolist() == [0, 0]


def test_limits_reached_and_exceeded_and_the_most_negative_code(fe):
    x8 = np.array([127, -127, 127.49, -127.49, 127.5, -127.5, 128, -128, 1e9, -1e9, np.inf, -np.inf], np.float32).reshape(1, 1, -1)
    zero = np.zeros_like(x8)
    yr, _, cnt = check_against_ref(fe, PLANAR, I8, x8, zero, records(fe, 1))
    assert yr.reshape(-1).tolist() == [127, -127, 127, -127, 127, -127, 127, -127, 127, -127, 127, -127]
    assert cnt[0].tolist() == [0, 8]  # 127.5 rounds to 128: from there on every component is clipped
    x16 = np.array([32767, -32767, 32767.4, 32767.5, -32767.5, 32768, -32768, -40000], np.float32).reshape(1, 1, -1)
    yr, _, cnt = check_against_ref(fe, CF32, I16, x16, np.zeros_like(x16), records(fe, 1))
    assert yr.reshape(-1).tolist() == [32767, -32767, 32767, 32767, -32767, 32767, -32767, -32767]
    assert cnt[0].tolist() == [0, 5]  # 32767.4 rounds down: not clipped; the tie 32767.5 goes to the even 32768: clipped
    # an integer input's most negative code passes through a unit gain as -127 / -32767
    for li, lo, v in ((I8, I8, -128), (I16, I16, -32768)):
        x = np.full((1, 1, 5), v, ref.DTYPE[li])
        yr, yi, cnt = check_against_ref(fe, li, lo, x, x, records(fe, 1))
        assert (yr == v + 1).all() and (yi == v + 1).all() and cnt[0].tolist() == [0, 10]
    rng = np.random.default_rng(5)
    for lo in (I8, I16):
        big = (rng.standard_normal((1, 2, 500)) * 1e6).astype(np.float32)
        yr, yi, _ = check_against_ref(fe, PLANAR, lo, big, -big, records(fe, 2))
        assert yr.min() == -ref.LIMIT[lo] and yi.min() == -ref.LIMIT[lo]


def test_threshold_equality_is_kept_and_the_next_float_is_blanked(fe):
    T = np.float32(3.25)
    up = np.nextafter(T, np.float32(np.inf))
    x = np.array([T, -T, up, -up, 1.0, 1.0], np.float32).reshape(1, 1, -1)
    y = np.array([1.0, 1.0, 1.0, 1.0, T, up], np.float32).reshape(1, 1, -1)
    yr, yi, cnt = check_against_ref(fe, PLANAR, PLANAR, x, y, records(fe, 1, threshold=T))
    assert yr.reshape(-1).tolist() == [T, -T, 0, 0, 1, 0] and cnt[0].tolist() == [3, 0]


def test_nan_and_inf_components_without_a_threshold(fe):
    x = np.array([np.nan, 1.0, np.inf, -np.inf, 2.0], np.float32).reshape(1, 1, -1)
    y = np.array([1.0, np.nan, 1.0, 1.0, 2.0], np.float32).reshape(1, 1, -1)
    yr, yi, cnt = check_against_ref(fe, CF32, CF32, x, y, records(fe, 1))
    # a NaN component blanks its sample even at T = +inf; an infinite one is kept (|inf| <= inf)
    assert yr.reshape(-1).tolist() == [0, 0, np.inf, -np.inf, 2] and yi.reshape(-1).tolist() == [0, 0, 1, 1, 2]
    assert cnt[0].tolist() == [2, 0]
    yr, yi, cnt = check_against_ref(fe, CF32, I8, x, y, records(fe, 1))
    assert yr.reshape(-1).tolist() == [0, 0, 127, -127, 2] and cnt[0].tolist() == [2, 2]
    # NaN parameters: a kept sample's y is NaN, which writes 0 and counts as clipped
    yr, yi, cnt = check_against_ref(fe, CF32, I16, x, y, records(fe, 1, scale=np.nan))
    assert not yr.any() and not yi.any() and cnt[0].tolist() == [2, 6]


def test_blank_all_antennas_with_one_tripping_antenna(fe):
    rng = np.random.default_rng(3)
    vr, vi = (rng.standard_normal((1, 4, 50)).astype(np.float32) for _ in range(2))
    vr[0, 2, 10], vi[0, 2, 31] = 100.0, -100.0
    p = records(fe, 4, threshold=10.0)
    yr, yi, cnt = check_against_ref(fe, PLANAR, CF32, vr, vi, p, True)
    assert cnt[:, 0].tolist() == [2, 2, 2, 2] and not yr[0, :, [10, 31]].any() and not yi[0, :, [10, 31]].any()
    yr, yi, cnt = check_against_ref(fe, PLANAR, CF32, vr, vi, p, False)
    assert cnt[:, 0].tolist() == [0, 0, 2, 0]


def test_zero_scale_and_the_sign_of_blanked_samples(fe):
    x = np.array([-5.0, 5.0, -50.0, 50.0], np.float32).reshape(1, 1, -1)
    for lo in (PLANAR, CF32):
        yr, yi, cnt = check_against_ref(fe, PLANAR, lo, x, -x, records(fe, 1, scale=0.0, threshold=10.0))
        # kept: -5 * 0 = -0.0, as float32 arithmetic has it; blanked: +0.0 whatever the sample's sign
        assert np.signbit(yr.reshape(-1)).tolist() == [True, False, False, False]
        assert np.signbit(yi.reshape(-1)).tolist() == [False, True, False, False]
        assert cnt[0].tolist() == [2, 0]
    yr, yi, cnt = check_against_ref(fe, PLANAR, I8, x, -x, records(fe, 1, scale=0.0))
    assert not yr.any() and not yi.any() and cnt[0].tolist() == [0, 0]


def test_counts_are_added_to_what_is_there(fe):
    rng = np.random.default_rng(11)
    vr, vi = ref.random_samples(rng, PLANAR, (2, 3, 100), special=False)
    p = records(fe, 3, scale=4.0, threshold=50.0)
    _, _, want = ref.condition(vr, vi, p, I8)
    cnt = np.zeros((3, 2), np.uint64)
    for k in (1, 2):
        assert run_host(fe, PLANAR, I8, vr, vi, p, counts=cnt)[5] == GAT_OK
        assert np.array_equal(cnt, k * want)
    assert want[:, 0].min() > 0 and want[:, 1].min() > 0


def test_in_place_is_allowed_and_partial_overlap_refused(fe):
    rng = np.random.default_rng(13)
    M, N, B = 3, 41, 2
    for layout in LAYOUTS:
        vr, vi = ref.random_samples(rng, layout, (B, M, N))
        p = records(fe, M, scale=0.5, dc_re=1.0, threshold=70.0)
        bufs = ref.make_buffers(layout, B, M, N, B * N, N)
        idx = ref.index(B, M, N, B * N, N)
        ref.put(bufs, layout, idx, vr, vi)
        d = fe.host_desc(bufs[0], bufs[1] if layout == PLANAR else None, layout, M, N, B * N, N)
        assert fe.condition_samples_host(d, B, p, d, True) == GAT_OK
        er, ei, _ = ref.condition(vr, vi, p, layout, True)
        yr, yi = ref.get(bufs, layout, idx)
        assert same_bits(yr, er) and same_bits(yi, ei)
        # the same memory one sample further on, another stride, or another layout: refused, nothing written
        before = [b.copy() for b in bufs]
        shifted = fe.host_desc(bufs[0], bufs[1] if layout == PLANAR else None, layout, M, N, B * N, N, 1)
        assert fe.condition_samples_host(d, B, p, shifted) == GAT_ERR_ARG
        restrided = fe.host_desc(bufs[0], bufs[1] if layout == PLANAR else None, layout, M, N, B * N, N - 1)
        assert fe.condition_samples_host(d, B, p, restrided) == GAT_ERR_ARG
        if layout in (I16, I8):
            other = fe.host_desc(bufs[0], None, I8 if layout == I16 else I16, M, N, B * N, N)
            assert fe.condition_samples_host(d, B, p, other) == GAT_ERR_ARG
        assert all(same_bits(a, b) for a, b in zip(bufs, before))


def test_refusals(fe):
    M, N, B = 2, 16, 2
    a = ref.make_buffers(PLANAR, B, M, N, B * N, N)
    o = ref.make_buffers(I8, B, M, N, B * N, N)
    p = records(fe, M)

    def call(ikw=None, okw=None, nb=B, prm=p, flags=False, idesc="x", odesc="x"):
        i = dict(layout=PLANAR, M=M, N=N, ant_stride=B * N, block_stride=N)
        i.update(ikw or {})
        d = dict(layout=I8, M=M, N=N, ant_stride=B * N, block_stride=N)
        d.update(okw or {})
        im = i.pop("im", a[1])
        idsc = fe.host_desc(a[0], im, i["layout"], i["M"], i["N"], i["ant_stride"], i["block_stride"]) if idesc else None
        oim = d.pop("im", None)
        odsc = fe.host_desc(o[0], oim, d["layout"], d["M"], d["N"], d["ant_stride"], d["block_stride"]) if odesc else None
        for k, dsc in (("chan_stride", idsc), ("out_chan_stride", odsc)):
            if dsc is not None and k in (ikw or {}) | (okw or {}):
                dsc.chan_stride = ((ikw or {}) | (okw or {}))[k]
        return fe.condition_samples_host(idsc, nb, prm, odsc, flags)

    before = o[0].copy()
    assert call() == GAT_OK
    o[0][:] = before
    assert call(idesc=None) == GAT_ERR_ARG and call(odesc=None) == GAT_ERR_ARG and call(prm=None) == GAT_ERR_ARG
    assert call(nb=0) == GAT_ERR_ARG and call(ikw=dict(N=0), okw=dict(N=0)) == GAT_ERR_ARG
    assert call(ikw=dict(ant_stride=-1)) == GAT_ERR_ARG and call(okw=dict(block_stride=-1)) == GAT_ERR_ARG
    assert call(ikw=dict(ant_stride=0)) == GAT_ERR_ARG and call(okw=dict(block_stride=0)) == GAT_ERR_ARG
    assert call(okw=dict(M=M + 1)) == GAT_ERR_ARG and call(okw=dict(N=N - 1)) == GAT_ERR_ARG
    assert call(ikw=dict(im=None)) == GAT_ERR_ARG  # planar without im
    assert call(okw=dict(im=a[1])) == GAT_ERR_ARG  # interleaved with im
    assert call(ikw=dict(layout=4)) == GAT_ERR_ARG and call(okw=dict(layout=-1)) == GAT_ERR_ARG
    assert call(flags=2) == GAT_ERR_ARG
    assert call(ikw=dict(chan_stride=8)) == GAT_ERR_UNSUPPORTED and call(okw=dict(out_chan_stride=8)) == GAT_ERR_UNSUPPORTED
    assert call(ikw=dict(M=65), okw=dict(M=65)) == GAT_ERR_RANGE
    assert np.array_equal(o[0], before)


def test_agc_record_against_the_fp64_formula(fe):
    rng = np.random.default_rng(17)
    M = 6
    st = np.zeros(M, fe.SAMPLE_STATS_DTYPE)
    st["kept"] = [1000, 1, 0, 123456789, 50, 7]
    st["sum_pow"] = [2.0e5, 3.0, 0.0, 1.0e13, 0.0, np.inf]
    st["sum_re"], st["sum_im"] = rng.standard_normal(M) * 100, rng.standard_normal(M) * 100
    for target, factor, dc in ((16.0, 0.0, False), (16.0, 4.5, True), (1000.0, -1.0, True), (0.0, 3.0, False)):
        got = fe.agc_params_host(st, target, factor, dc)
        want = ref.agc(st, target, factor, dc)
        for j, name in enumerate(("scale", "dc_re", "dc_im", "threshold")):
            g, w = got[name].astype(np.float64), want[:, j]
            assert same_bits(got[name], w.astype(np.float32)), (name, g, w)  # narrowed once
            fin = np.isfinite(w)
            assert np.array_equal(np.isfinite(g), fin)
            # the float32 record is within half a float32 ulp of the FP64 value, which itself is the formula to 1e-15
            assert np.all(np.abs(g[fin] - w[fin]) <= 2.0 ** -24 * np.abs(w[fin]) + 1e-15 * np.abs(w[fin]))
        # kept == 0, no power, or an unusable sigma: no gain, no blanking
        for m in (2, 4, 5):
            assert got[m]["scale"] == 0 and got[m]["dc_re"] == 0 and got[m]["dc_im"] == 0 and np.isposinf(got[m]["threshold"])
    bad = fe._agc_config(16.0, 0.0, False)
    bad.struct_size = 8
    out = np.zeros(M, fe.COND_PARAMS_DTYPE)
    from gpuacceleratedtracking_amd import _lib
    assert _lib.load().gat_agc_update_host(st.ctypes.data, M, C.byref(bad), out.ctypes.data) == GAT_ERR_ARG


def test_python_surface_is_exported():
    import gpuacceleratedtracking_amd as g
    for name in ("sample_stats", "agc_params", "condition_samples", "requantize", "GAT_COND_BLANK_ALL_ANTS"):
        assert hasattr(g, name), name
