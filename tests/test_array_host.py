"""CPU tests of the antenna-array host entry points (include/gat.h gat_array_weights_host, gat_tracking_update_host_weighted)
against the FP64 numpy reference (tests/array_ref.py).  No device.

Where the weights' tolerance comes from: a hand-written FP64 Cholesky against numpy.linalg.solve on covariances of
M in {2, 4, 16, 64}, noise plus one jammer at 0 to 60 dB, differed by about 2e-17 * cond, 2.2e-10 at cond 8e6.  The tests keep
cond <= 1e7 (asserted) with jammers up to 50 dB over the noise, and ask for 1e-8 in the relative 2-norm: 50 x that measurement."""
import ctypes as C

import numpy as np
import pytest

import oracle
from tests import array_ref

VP = C.c_void_p


@pytest.fixture(scope="module")
def g():
    import gpuacceleratedtracking_amd as g
    g.load_library()
    return g


def _vp(a):
    return VP(a.ctypes.data) if a is not None else None


def host_weights(g, R, a, mode, loading=0.0, K=None):
    """gat_array_weights_host on a covariance rounded to float32 planes; returns (status, w complex128 [K, M])."""
    lib = g.load_library()
    M = R.shape[0] if R is not None else a.shape[1]
    c_re = np.ascontiguousarray(R.real, dtype=np.float32) if R is not None else None
    c_im = np.ascontiguousarray(R.imag, dtype=np.float32) if R is not None else None
    a_re = np.ascontiguousarray(a.real, dtype=np.float64) if a is not None else None
    a_im = np.ascontiguousarray(a.imag, dtype=np.float64) if a is not None else None
    K = (a.shape[0] if a is not None else 1) if K is None else K
    w_re, w_im = np.full((K, M), 7.0), np.full((K, M), 7.0)
    rc = lib.gat_array_weights_host(_vp(c_re), _vp(c_im), M, _vp(a_re), _vp(a_im), K, mode, loading, _vp(w_re), _vp(w_im))
    return rc, w_re + 1j * w_im


def f32_cov(R):
    """what the library is handed: the covariance rounded to float32 planes, as complex128 (the reference sees the same)"""
    return R.real.astype(np.float32).astype(np.float64) + 1j * R.imag.astype(np.float32).astype(np.float64)


CASES = [(M, jnr, sample) for M in (1, 2, 3, 4, 5, 8, 9, 16, 33, 63, 64) for jnr, sample in ((0.0, False), (30.0, False), (50.0, False), (40.0, True))]


@pytest.mark.parametrize("M,jnr,sample", CASES)
def test_weights_match_numpy_solve(g, M, jnr, sample):
    rng = np.random.default_rng(1000 + M + int(jnr))
    R, _ = array_ref.jammer_covariance(M, jnr, rng, snapshots=4000 if sample else None)
    R = f32_cov(R)
    cond = np.linalg.cond(R)
    assert cond <= 1e7, cond
    K = 3
    a = np.exp(2j * np.pi * rng.uniform(0, 1, (K, M)))
    for mode in (g.GAT_BF_MVDR, g.GAT_BF_POWER_INVERSION, g.GAT_BF_CONVENTIONAL):
        for loading in (0.0, 1e-3):
            rc, w = host_weights(g, R, a, mode, loading)
            assert rc == 0, (mode, rc)
            ref = array_ref.weights(R, a, mode, loading)
            err = np.linalg.norm(w - ref, axis=1) / np.linalg.norm(ref, axis=1)
            print(f"M {M} jammer {jnr} dB sample {sample} mode {mode} loading {loading}: cond {cond:.3g} rel err {err.max():.3e}")
            assert err.max() <= 1e-8, (mode, loading, err)
            if mode == g.GAT_BF_MVDR:
                assert np.abs(np.sum(np.conj(w) * a, axis=1) - 1.0).max() <= 1e-12
            if mode == g.GAT_BF_POWER_INVERSION:
                assert (w[:, 0] == 1.0).all()
                assert (w == w[0]).all()  # no steering vector: every channel gets the same weights


@pytest.mark.parametrize("K", (1, 65, 1000))
def test_weights_for_many_channels(g, K):
    """K steering vectors on one factor: every row against numpy.linalg.solve at the tolerance and condition cap above"""
    M = 8
    rng = np.random.default_rng(2000 + K)
    R = f32_cov(array_ref.jammer_covariance(M, 50.0, rng)[0])
    assert np.linalg.cond(R) <= 1e7
    a = np.exp(2j * np.pi * rng.uniform(0, 1, (K, M)))
    for mode in (g.GAT_BF_MVDR, g.GAT_BF_POWER_INVERSION, g.GAT_BF_CONVENTIONAL):
        for loading in (0.0, 1e-3):
            rc, w = host_weights(g, R, a, mode, loading)
            assert rc == 0 and w.shape == (K, M), (mode, rc)
            ref = array_ref.weights(R, a, mode, loading)
            err = np.linalg.norm(w - ref, axis=1) / np.linalg.norm(ref, axis=1)
            assert err.max() <= 1e-8, (mode, loading, err.max())
            if mode == g.GAT_BF_MVDR:
                assert np.abs(np.sum(np.conj(w) * a, axis=1) - 1.0).max() <= 1e-12


def test_power_inversion_needs_no_steering_and_conventional_no_covariance(g):
    rng = np.random.default_rng(5)
    R = f32_cov(array_ref.jammer_covariance(4, 30.0, rng)[0])
    rc, w = host_weights(g, R, None, g.GAT_BF_POWER_INVERSION, K=2)
    assert rc == 0 and np.allclose(w, array_ref.weights(R, None, 2), rtol=1e-9, atol=0) and (w[0] == w[1]).all()
    a = np.exp(2j * np.pi * rng.uniform(0, 1, (2, 4)))
    rc, w = host_weights(g, None, a, g.GAT_BF_CONVENTIONAL)
    assert rc == 0 and np.allclose(w, a / 4.0, rtol=1e-15, atol=0)


def test_weights_error_codes(g):
    lib = g.load_library()
    rng = np.random.default_rng(6)
    M = 4
    R = f32_cov(array_ref.jammer_covariance(M, 20.0, rng)[0])
    a = np.exp(2j * np.pi * rng.uniform(0, 1, (1, M)))
    # not positive definite: indefinite, singular, NaN
    bad = R.copy()
    bad[2, 2] = -1.0
    assert host_weights(g, bad, a, g.GAT_BF_MVDR)[0] == 2
    v = np.ones(M, dtype=np.complex128)
    assert host_weights(g, np.outer(v, v.conj()), a, g.GAT_BF_MVDR)[0] == 2
    assert host_weights(g, np.outer(v, v.conj()), a, g.GAT_BF_MVDR, loading=0.1)[0] == 0  # loading makes it definite
    nanm = R.copy()
    nanm[1, 1] = np.nan
    assert host_weights(g, nanm, a, g.GAT_BF_POWER_INVERSION)[0] == 2
    assert host_weights(g, None, np.zeros((1, M), dtype=np.complex128), g.GAT_BF_CONVENTIONAL)[0] == 2  # a steering vector of zeros
    # bad arguments
    assert host_weights(g, R, a, 3)[0] == 1 and host_weights(g, R, a, -1)[0] == 1  # mode
    assert host_weights(g, R, None, g.GAT_BF_MVDR)[0] == 1  # MVDR without steering
    assert host_weights(g, None, a, g.GAT_BF_MVDR)[0] == 1  # MVDR without covariance
    assert host_weights(g, R, a, g.GAT_BF_MVDR, loading=-1e-3)[0] == 1
    assert host_weights(g, R, a, g.GAT_BF_MVDR, loading=float("nan"))[0] == 1
    assert host_weights(g, R, a, g.GAT_BF_MVDR, K=0)[0] == 1
    big = np.eye(65, dtype=np.complex128)
    assert host_weights(g, big, np.ones((1, 65), dtype=np.complex128), g.GAT_BF_MVDR)[0] == 2  # more than 64 antennas
    c_re, c_im = np.ascontiguousarray(R.real, np.float32), np.ascontiguousarray(R.imag, np.float32)
    a_re, a_im = np.ascontiguousarray(a.real), np.ascontiguousarray(a.imag)
    w = np.zeros((1, M))
    assert lib.gat_array_weights_host(_vp(c_re), _vp(c_im), M, _vp(a_re), _vp(a_im), 1, 1, 0.0, None, _vp(w)) == 1  # null output


def _loop_case(g, seed=4, K=5, M=3, L=3, taps=(0, 1, 2)):
    """taps: (early, prompt, late) indices into the L taps"""
    L_ = g._lib
    rng = np.random.default_rng(seed)
    cfg = L_.LoopConfig(1e-3, 18.0, 2.0, 1.023e6, 1575.42e6, 1.0e5, 1.0, 1023, L, *taps)
    dop = rng.uniform(-3e3, 3e3, K)
    cur = g.make_params(np.arange(K) % 32, 1.023e6 + dop * 1.023e6 / 1575.42e6, 1.0e5 + dop, rng.uniform(0, 1023, K), rng.uniform(0, 1, K), shape=(K,))
    st = np.zeros(K, dtype=L_.LOOP_STATE_DTYPE)
    st["init_carrier_doppler_hz"] = dop
    st["carrier_doppler_hz"] = dop
    return K, M, L, rng, cfg, cur, st


def test_host_weighted_update_with_null_weights_is_the_unweighted_update(g):
    lib = g.load_library()
    K, M, L, rng, cfg, cur, st = _loop_case(g)
    cur2, st2 = cur.copy(), st.copy()
    nxt, nxt2 = cur.copy(), cur.copy()
    for it in range(5):
        acc = (rng.standard_normal((K, L, M)) + 1j * rng.standard_normal((K, L, M))).astype(np.complex64) * 1000
        re, im = np.ascontiguousarray(acc.real), np.ascontiguousarray(acc.imag)
        assert lib.gat_tracking_update_host(_vp(re), _vp(im), K, M, C.byref(cfg), _vp(st), _vp(cur), _vp(nxt)) == 0
        assert lib.gat_tracking_update_host_weighted(_vp(re), _vp(im), K, M, C.byref(cfg), _vp(st2), _vp(cur2), _vp(nxt2), None, None) == 0
        cur, nxt, cur2, nxt2 = nxt, cur, nxt2, cur2
        assert cur.tobytes() == cur2.tobytes() and st.tobytes() == st2.tobytes(), it


LOOP_SHAPES = ((5, 3, 5, (4, 1, 0)), (200, 3, 3, (0, 1, 2)), (200, 16, 5, (3, 0, 2)), (1, 1, 5, (2, 4, 1)))


@pytest.mark.parametrize("K,M,L,taps", LOOP_SHAPES)
def test_host_weighted_update_tap_orders_and_channel_counts(g, K, M, L, taps):
    """five taps with early, prompt and late out of order, 200 channels, one antenna: against the numpy restatement over
    five updates, at the tolerances of the test below"""
    lib = g.load_library()
    _, _, _, rng, cfg, cur, st = _loop_case(g, seed=40 + K + L, K=K, M=M, L=L, taps=taps)
    cfgd = {n: getattr(cfg, n) for n, _ in cfg._fields_}
    nxt = cur.copy()
    ostate = {n: st[n].copy() for n in st.dtype.names}
    ocur = oracle.make_params(cur["prn"], cur["code_freq_hz"], cur["carrier_freq_hz"], cur["code_phase_chips"], cur["carrier_phase_cycles"])
    w = (rng.standard_normal((K, M)) + 1j * rng.standard_normal((K, M))) / M
    w_re, w_im = np.ascontiguousarray(w.real), np.ascontiguousarray(w.imag)
    for it in range(5):
        acc = (rng.standard_normal((K, L, M)) + 1j * rng.standard_normal((K, L, M))).astype(np.complex64) * 1000
        re, im = np.ascontiguousarray(acc.real), np.ascontiguousarray(acc.imag)
        assert lib.gat_tracking_update_host_weighted(_vp(re), _vp(im), K, M, C.byref(cfg), _vp(st), _vp(cur), _vp(nxt), _vp(w_re), _vp(w_im)) == 0
        cur, nxt = nxt, cur
        ocur, ostate = array_ref.tracking_update_weighted(acc, w, cfgd, ostate, ocur)
        for f in ("code_freq_hz", "carrier_freq_hz", "code_phase_chips", "carrier_phase_cycles"):
            assert np.allclose(cur[f], ocur[f], rtol=1e-12, atol=1e-9), (it, f)
        for name in ostate:
            assert np.allclose(st[name], ostate[name], rtol=1e-10, atol=1e-9), (it, name)


def test_host_weighted_update_matches_numpy_restatement(g):
    """With weights: the oracle's restatement of the loop equations on the beamformed taps, at the tolerances
    test_abi_and_host.py uses for the unweighted update; error codes."""
    lib = g.load_library()
    K, M, L, rng, cfg, cur, st = _loop_case(g, seed=14)
    cfgd = {n: getattr(cfg, n) for n, _ in cfg._fields_}
    nxt = cur.copy()
    ostate = {n: st[n].copy() for n in st.dtype.names}
    ocur = oracle.make_params(cur["prn"], cur["code_freq_hz"], cur["carrier_freq_hz"], cur["code_phase_chips"], cur["carrier_phase_cycles"])
    w = (rng.standard_normal((K, M)) + 1j * rng.standard_normal((K, M))) / M
    w_re, w_im = np.ascontiguousarray(w.real), np.ascontiguousarray(w.imag)
    for it in range(5):
        acc = (rng.standard_normal((K, L, M)) + 1j * rng.standard_normal((K, L, M))).astype(np.complex64) * 1000
        re, im = np.ascontiguousarray(acc.real), np.ascontiguousarray(acc.imag)
        assert lib.gat_tracking_update_host_weighted(_vp(re), _vp(im), K, M, C.byref(cfg), _vp(st), _vp(cur), _vp(nxt), _vp(w_re), _vp(w_im)) == 0
        cur, nxt = nxt, cur
        ocur, ostate = array_ref.tracking_update_weighted(acc, w, cfgd, ostate, ocur)
        for f in ("code_freq_hz", "carrier_freq_hz", "code_phase_chips", "carrier_phase_cycles"):
            assert np.allclose(cur[f], ocur[f], rtol=1e-12, atol=1e-9), (it, f)
        for name in ostate:
            assert np.allclose(st[name], ostate[name], rtol=1e-10, atol=1e-9), (it, name)
    # unit weights on every antenna are the plain sum (up to the order of the FP64 additions)
    K2, M2, L2, rng2, cfg2, cur_a, st_a = _loop_case(g, seed=15)
    cur_b, st_b, n_a, n_b = cur_a.copy(), st_a.copy(), cur_a.copy(), cur_a.copy()
    ones, zeros = np.ones((K2, M2)), np.zeros((K2, M2))
    acc = (rng2.standard_normal((K2, L2, M2)) + 1j * rng2.standard_normal((K2, L2, M2))).astype(np.complex64) * 1000
    re, im = np.ascontiguousarray(acc.real), np.ascontiguousarray(acc.imag)
    assert lib.gat_tracking_update_host(_vp(re), _vp(im), K2, M2, C.byref(cfg2), _vp(st_a), _vp(cur_a), _vp(n_a)) == 0
    assert lib.gat_tracking_update_host_weighted(_vp(re), _vp(im), K2, M2, C.byref(cfg2), _vp(st_b), _vp(cur_b), _vp(n_b), _vp(ones), _vp(zeros)) == 0
    for f in ("code_freq_hz", "carrier_freq_hz", "code_phase_chips", "carrier_phase_cycles"):
        assert np.allclose(n_a[f], n_b[f], rtol=1e-13, atol=1e-10), f
    bad = g._lib.LoopConfig(1e-3, 18.0, 2.0, 1.023e6, 1575.42e6, 0.0, 1.0, 1023, L, 0, 1, 7)  # late tap outside the list
    assert lib.gat_tracking_update_host_weighted(_vp(re), _vp(im), K, M, C.byref(bad), _vp(st), _vp(cur), _vp(nxt), _vp(w_re), _vp(w_im)) == 2
    assert lib.gat_tracking_update_host_weighted(None, _vp(im), K, M, C.byref(cfg), _vp(st), _vp(cur), _vp(nxt), _vp(w_re), _vp(w_im)) == 1
    assert lib.gat_tracking_update_host_weighted(_vp(re), _vp(im), K, M, C.byref(cfg), _vp(st), _vp(cur), _vp(nxt), _vp(w_re), None) == 1
