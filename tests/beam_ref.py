"""FP64 restatement of gat_beamform_samples (include/gat.h): y[b, j, n] = sum_m conj(w[j, m]) x[m, b * block_stride + n], and the
error bound the float32 kernels are held to."""
import numpy as np

U = 2.0 ** -24  # unit roundoff of float32


def beams(x, w, N, B, block_stride=None):
    """x complex128 [M, ld] holding B blocks of N samples block_stride apart, w complex128 [J, M].  complex128 [B, J, N]."""
    S = N if block_stride is None else block_stride
    w = np.asarray(w, dtype=np.complex128)
    return np.stack([np.einsum('jm,mn->jn', w.conj(), x[:, b * S:b * S + N]) for b in range(B)])


def bound(x, w, N, B, block_stride=None):
    """Per-sample bound on |y - y64|, float64 [B, J, N].  A complex dot product of length M is two real FMA chains of length
    2 M on weights rounded once to float32: first order (2 M + 2) u sum_m |w_m| |x_m|; the kernels are held to twice that,
    (4 M + 4) 2^-24 sum_m |w_m| |x_m|."""
    S = N if block_stride is None else block_stride
    M = x.shape[0]
    aw = np.abs(np.asarray(w, dtype=np.complex128))
    return (4 * M + 4) * U * np.stack([aw @ np.abs(x[:, b * S:b * S + N]) for b in range(B)])
