"""The FP64 reference of the sample beamformer (tests/beam_ref.py) against a sum written out as loops, so that the reference the
GPU tests lean on is itself pinned; and the bound against a float32 emulation of the kernels' sum."""
import numpy as np

from tests import beam_ref


def _case(seed, M=3, J=2, N=5, B=2, S=7):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((M, B * S)) + 1j * rng.standard_normal((M, B * S))
    w = rng.standard_normal((J, M)) + 1j * rng.standard_normal((J, M))
    return x, w, N, B, S


def test_beams_equal_the_loop_written_sum():
    x, w, N, B, S = _case(1)
    y = beam_ref.beams(x, w, N, B, S)
    assert y.shape == (B, w.shape[0], N) and y.dtype == np.complex128
    for b in range(B):
        for j in range(w.shape[0]):
            for n in range(N):
                acc = 0j
                for m in range(x.shape[0]):
                    acc += (w[j, m].real - 1j * w[j, m].imag) * x[m, b * S + n]
                assert abs(y[b, j, n] - acc) <= 1e-14 * (np.abs(w[j]) @ np.abs(x[:, b * S + n]))
    # the default stride is the block length
    assert np.array_equal(beam_ref.beams(x[:, :B * N], w, N, B), beam_ref.beams(x[:, :B * N], w, N, B, N))


def test_bound_is_the_stated_formula_and_holds_for_a_float32_sum():
    x, w, N, B, S = _case(2, M=16, J=3, N=64, B=2, S=64)
    bd = beam_ref.bound(x, w, N, B, S)
    M = x.shape[0]
    for b, j, n in ((0, 0, 0), (1, 2, 63), (1, 1, 17)):
        want = (4 * M + 4) * 2.0 ** -24 * sum(abs(w[j, m]) * abs(x[m, b * S + n]) for m in range(M))
        assert abs(bd[b, j, n] - want) <= 1e-12 * want
    # the kernels' arithmetic in numpy: float32 weights, float32 running sums in antenna order (products rounded as well:
    # more roundings than the FMA chain has)
    x32r, x32i = x.real.astype(np.float32), x.imag.astype(np.float32)
    xs = x32r.astype(np.float64) + 1j * x32i.astype(np.float64)
    wr, wi = w.real.astype(np.float32), w.imag.astype(np.float32)
    yr = np.zeros((B, w.shape[0], N), dtype=np.float32)
    yi = np.zeros_like(yr)
    for b in range(B):
        for m in range(M):
            xr, xi = x32r[m, b * S:b * S + N][None, :], x32i[m, b * S:b * S + N][None, :]
            yr[b] = yr[b] + wr[:, m, None] * xr
            yr[b] = yr[b] + wi[:, m, None] * xi
            yi[b] = yi[b] + wr[:, m, None] * xi
            yi[b] = yi[b] - wi[:, m, None] * xr
    err = np.abs((yr.astype(np.float64) + 1j * yi.astype(np.float64)) - beam_ref.beams(xs, w, N, B, S))
    # one more rounding per term than an FMA has: first order (2 M + 1) u + u for the weights, still inside (4 M + 4) u
    assert (err <= beam_ref.bound(xs, w, N, B, S)).all()
