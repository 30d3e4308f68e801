"""What the subspace tests share: the covariance's shapes and calls, output buffers between canaries, raw calls of the host twins,
and the eigensolver's batches.  No device is needed here."""
import numpy as np

from tests import eig_ref as er
from tests.mon_cases import make_acc  # float32 accumulators with NaN between padded blocks

CANARY = -7.25e77
GUARD = 16
COV_SHAPES = [(1, 1, 1, 1), (5, 3, 3, 4), (255, 2, 3, 3), (256, 2, 3, 16), (257, 1, 5, 33), (700, 2, 3, 64)]
BPES = (None, 1, 256, 300)


def estimates(B, bpe):
    bpe = B if bpe is None or bpe <= 0 or bpe > B else bpe
    return (B + bpe - 1) // bpe


def guarded(parts, dtype=np.float64):
    """one flat buffer of CANARY holding the parts (name -> elements) with GUARD canaries around each: (buffer, name -> slice)"""
    at, pos = {}, GUARD
    for name, n in parts.items():
        at[name] = slice(pos, pos + n)
        pos += n + GUARD
    return np.full(pos, CANARY, dtype), at


def canaries_intact(buf, at):
    keep = np.ones(buf.shape, bool)
    for s in at.values():
        keep[s] = False
    return bool((buf[keep] == CANARY).all())


def cov_host(lib, acc_re, acc_im, stride, B, K, L, M, tap, bpe):
    """gat_accumulator_covariance_host on flat accumulators: (status, buffer, layout)"""
    n = estimates(B, bpe) * K * M * M
    buf, at = guarded({"cov_re": n, "cov_im": n})
    base = buf.ctypes.data
    rc = lib.gat_accumulator_covariance_host(acc_re.ctypes.data, acc_im.ctypes.data, stride, B, K, L, M, tap, 0 if bpe is None else bpe,
                                             base + 8 * at["cov_re"].start, base + 8 * at["cov_im"].start)
    return rc, buf, at


def eig_layout(n, Q, R, want=("eigenvalues", "vec", "status")):
    """doubles of a flat float64 buffer: eigenvalues [n, Q], vec_re, vec_im [n, R, Q] and the status as n int32 in ceil(n / 2) doubles"""
    parts = {}
    if "eigenvalues" in want:
        parts["eigenvalues"] = n * Q
    if "vec" in want:
        parts["vec_re"], parts["vec_im"] = n * R * Q, n * R * Q
    if "status" in want:
        parts["status"] = (n + 1) // 2
    return guarded(parts)


def eig_pointers(base, at):
    p = lambda name: base + 8 * at[name].start if name in at else None  # noqa: E731
    return p("eigenvalues"), p("vec_re"), p("vec_im"), p("status")


def eig_planes(batch):
    """the planes of a batch [n, Q, Q], float32 for complex64"""
    part = np.float32 if batch.dtype == np.complex64 else np.float64
    return np.ascontiguousarray(batch.real, dtype=part), np.ascontiguousarray(batch.imag, dtype=part), int(batch.dtype == np.complex64)


def eig_host(lib, batch, R, want=("eigenvalues", "vec", "status")):
    n, Q = batch.shape[0], batch.shape[-1]
    a_re, a_im, flags = eig_planes(batch)
    buf, at = eig_layout(n, Q, R, want)
    if "status" in at and n % 2:
        buf[at["status"]].view(np.int32)[n:] = 0  # the spare half of the last double is nobody's
    rc = lib.gat_hermitian_eig_host(a_re.ctypes.data, a_im.ctypes.data, n, Q, R, flags, *eig_pointers(buf.ctypes.data, at))
    return rc, buf, at


def status_of(buf, at, n):
    return buf[at["status"]].view(np.int32)[:n].copy()


def mixed_batch(Q, n, rng, f32=False):
    """n matrices of order Q drawn over the families in turn"""
    names = er.FAMILIES
    batch = np.stack([er.family(names[(i + Q) % len(names)], Q, rng) for i in range(n)])
    return batch.astype(np.complex64) if f32 else batch
