"""FP64 numpy reference of the antenna-array maths (include/gat.h, "antenna-array processing"): spatial covariance,
beamformer weights, beamformed accumulators and the weighted loop update.  Nothing here calls the library."""
import numpy as np

import oracle


def block_view(x, N, B, block_stride=None):
    """x [M, ld] -> the B blocks of N samples, block_stride apart, as a read-only view [B, M, N]"""
    S = N if block_stride is None else block_stride
    assert x.ndim == 2 and (B - 1) * S + N <= x.shape[1], (x.shape, N, B, S)
    return np.lib.stride_tricks.as_strided(x, shape=(B, x.shape[0], N), strides=(S * x.strides[1], x.strides[0], x.strides[1]), writeable=False)


def _block_products(x, N, B, bpe, block_stride):
    """one matrix product x_b x_b^H per block in x's own precision, the blocks of an estimate added in order"""
    xb = block_view(x, N, B, block_stride)
    R = xb @ xb.conj().transpose(0, 2, 1)
    return R if bpe == 1 else np.add.reduceat(R, np.arange(0, B, bpe), axis=0)


def covariance(x, N, B, bpe, block_stride=None):
    """x complex128 [M, ld]: R_e[i, j] = sum_{b in e} sum_{n < N} x[i, b S + n] conj(x[j, b S + n]), [E, M, M]."""
    return _block_products(np.asarray(x, dtype=np.complex128), N, B, bpe, block_stride)


def covariance_error(got, ref):
    """Per estimate, max_ij |got_ij - ref_ij| / sqrt(ref_ii ref_jj): every element on its own natural scale (what bounds
    both |R_ij| and its float32 summation error), so that an error confined to a weak antenna's sub-matrix counts as much
    as one on the strongest.  got, ref complex [E, M, M]; returns float64 [E].  Where a diagonal element of ref is exactly
    0 (an antenna of zeros) that row and column of got must be exactly 0 (asserted); they take no part in the maximum.
    Elements that are not finite in got or ref give NaN (or inf), which no bound passes."""
    got = np.asarray(got, dtype=np.complex128)
    ref = np.asarray(ref, dtype=np.complex128)
    assert got.shape == ref.shape and got.ndim == 3 and got.shape[1] == got.shape[2], (got.shape, ref.shape)
    E, M = ref.shape[:2]
    d = ref[:, np.arange(M), np.arange(M)].real  # [E, M]
    zero = d == 0
    dead = zero[:, :, None] | zero[:, None, :]
    assert (got[dead] == 0).all(), "an antenna of zeros has a nonzero row or column"
    scale = np.sqrt(np.where(zero, 1.0, d))
    err = np.abs(got - ref) / (scale[:, :, None] * scale[:, None, :])
    err = np.where(dead, 0.0, err)
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(err).any(axis=(1, 2)), np.nan, np.nanmax(err, axis=(1, 2)))


def covariance_f32(x, N, B, bpe, block_stride=None):
    """covariance() by numpy's complex64 product x32 @ x32.conj().T of the same samples, block by block, the block sums added
    in complex64: a float32 reference, whose own covariance_error against covariance() is what float32 summation costs on
    these samples."""
    return _block_products(np.asarray(x).astype(np.complex64), N, B, bpe, block_stride)


def loaded(R, loading):
    M = R.shape[0]
    return np.asarray(R, dtype=np.complex128) + loading * np.trace(R).real / M * np.eye(M)


def weights(R, a, mode, loading=0.0):
    """mode 0: a / (a^H a); 1: R'^-1 a / (a^H R'^-1 a); 2: R'^-1 e0 / (e0^H R'^-1 e0).  a: [K, M] (ignored for mode 2: one row
    per row of a, or one row).  numpy.linalg.solve in FP64."""
    a = None if a is None else np.atleast_2d(np.asarray(a, dtype=np.complex128))
    if mode == 0:
        return a / np.sum(np.abs(a) ** 2, axis=1, keepdims=True)
    Rl = loaded(R, loading)
    M = Rl.shape[0]
    if mode == 2:
        e0 = np.zeros(M, dtype=np.complex128)
        e0[0] = 1.0
        K = 1 if a is None else a.shape[0]
        a = np.tile(e0, (K, 1))
    z = np.linalg.solve(Rl, a.T).T  # [K, M]
    return z / np.sum(a.conj() * z, axis=1, keepdims=True)


def beamform(acc, w):
    """acc complex [B, K, L, M], w complex [K, M]: y[b, k, l] = sum_m conj(w[k, m]) acc[b, k, l, m]."""
    return np.einsum("km,bklm->bkl", np.conj(w), acc)


def tracking_update_weighted(acc, w, cfg, state, cur):
    """oracle.np_tracking_update on the beamformed taps: its antenna sum over ONE antenna that carries
    sum_m conj(w[k, m]) acc[k, l, m]."""
    y = beamform(np.asarray(acc, dtype=np.complex128)[None], w)[0]  # [K, L]
    return oracle.np_tracking_update(y[:, :, None], cfg, state, cur)


def jammer_covariance(M, jnr_db, rng, snapshots=None):
    """Unit noise plus one jammer of power 10^(jnr_db / 10) from a random direction: the exact covariance, or (snapshots) a
    sample covariance sum of that many draws.  Returns (R complex128 [M, M], jammer steering vector)."""
    v = np.exp(2j * np.pi * rng.uniform(0, 1, M))
    p = 10.0 ** (jnr_db / 10.0)
    if snapshots is None:
        return np.eye(M, dtype=np.complex128) + p * np.outer(v, v.conj()), v
    n = (rng.standard_normal((M, snapshots)) + 1j * rng.standard_normal((M, snapshots))) / np.sqrt(2.0)
    j = np.sqrt(p / 2.0) * (rng.standard_normal(snapshots) + 1j * rng.standard_normal(snapshots))
    x = n + v[:, None] * j[None, :]
    return x @ x.conj().T, v
