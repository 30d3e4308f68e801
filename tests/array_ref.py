"""FP64 numpy reference of the antenna-array maths (include/gat.h, "antenna-array processing"): spatial covariance,
beamformer weights, beamformed accumulators and the weighted loop update.  Nothing here calls the library."""
import numpy as np

import oracle


def covariance(x, N, B, bpe, block_stride=None):
    """x complex128 [M, ld]: R_e[i, j] = sum_{b in e} sum_{n < N} x[i, b S + n] conj(x[j, b S + n]), [E, M, M]."""
    S = N if block_stride is None else block_stride
    M = x.shape[0]
    E = -(-B // bpe)
    R = np.zeros((E, M, M), dtype=np.complex128)
    for b in range(B):
        xb = x[:, b * S:b * S + N]
        R[b // bpe] += xb @ xb.conj().T
    return R


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
