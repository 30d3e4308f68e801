"""FP64 numpy restatements of the subspace rules of include/gat.h (csrc/gat_eig.h), the matrix families the eigensolver is tested
on and the tolerance its results are held to.  numpy evaluates every elementwise expression as written (no contraction) and its
sqrt and / are IEEE, so the restatements give the bits of the library's twins.

EIG_C[Q], the constant of the three error bounds ``c * eps * ||A||_F`` (eigenvalues against numpy.linalg.eigh, the residual
||A V - V diag(lambda)||_F and ||A||_F ||V^H V - I||_F) at order Q: 4 x the largest of the three the host twin shows on ``cases()``
-- FAMILIES x SIZES and the float32 inputs -- at that order, rounded up.  Measured with ``python -m tests.eig_ref``, in eps ||A||_F
(the orthogonality in eps), eps = 2^-52:

      Q   eigenvalues   residual   orthogonality   sweeps      c    64 Q
      1       0.58         0.00         0.00          0        2.5     64
      2       1.75         1.78         2.83          1       12      128
      3       2.82         3.98         6.29          4       26      192
      4       5.65         4.83         7.39          4       30      256
      5       5.55        51.90         9.82          5      208      320
      8      12.14        72.22        20.49          6      289      512
     16      27.65        52.30        56.90         10      228     1024
     17      17.45        77.21        61.35         11      309     1088
     33      62.03        61.40       147.30         14      590     2112
     64     107.94       108.59       512.91         18     2052     4096

The residuals of 50 - 80 at small orders are the matrices scaled by 1e-150: the squares of their small off-diagonal elements
underflow, and so does the threshold.  No c exceeds 64 Q: above that the rule would be wrong, not the tolerance."""
import numpy as np

EPS = 2.0 ** -52
CHUNK = 256
MAX_SWEEPS = 60
SIZES = (1, 2, 3, 4, 5, 8, 16, 17, 33, 64)
FAMILIES = ("wishart", "rank_one", "rank_one_noise", "identity", "zero", "scaled_up", "scaled_down", "indefinite", "graded")
EIG_C = {1: 2.5, 2: 12.0, 3: 26.0, 4: 30.0, 5: 208.0, 8: 289.0, 16: 228.0, 17: 309.0, 33: 590.0, 64: 2052.0}
assert all(c <= 64 * q for q, c in EIG_C.items())


# ---- accumulator covariance --------------------------------------------------------------------------------------------------------
def _estimates(B, bpe):
    bpe = B if bpe is None or bpe <= 0 or bpe > B else int(bpe)
    return [(b0, min(bpe, B - b0)) for b0 in range(0, B, bpe)]


def acc_cov_chunked(acc_re, acc_im, tap, bpe=None):
    """The rule: per estimate, chunks of 256 blocks summed in block order from +0, the chunk sums added in chunk order from +0;
    the lower triangle computed, the upper its conjugate, the diagonal's imaginary part +0.  complex128 [E, K, M, M]."""
    xr, xi = acc_re[:, :, tap, :].astype(np.float64), acc_im[:, :, tap, :].astype(np.float64)  # [B, K, M]
    B, K, M = xr.shape
    out = []
    low = np.tril(np.ones((M, M), bool))
    for b0, n in _estimates(B, bpe):
        tr, ti = np.zeros((K, M, M)), np.zeros((K, M, M))
        for c0 in range(0, n, CHUNK):
            sr, si = np.zeros((K, M, M)), np.zeros((K, M, M))
            for b in range(b0 + c0, b0 + min(c0 + CHUNK, n)):
                ri, rj, ii, ij = xr[b][:, :, None], xr[b][:, None, :], xi[b][:, :, None], xi[b][:, None, :]
                sr = sr + (ri * rj + ii * ij)
                si = si + (ii * rj - ri * ij)
            tr, ti = tr + sr, ti + si
        re = np.where(low, tr, np.swapaxes(tr, -1, -2))
        im = np.where(low, ti, -np.swapaxes(ti, -1, -2))
        im[:, np.arange(M), np.arange(M)] = 0.0
        cov = np.empty(re.shape, np.complex128)
        cov.real, cov.imag = re, im  # (no complex arithmetic: it would lose the zeros' signs)
        out.append(cov)
    return np.stack(out)


def acc_cov_plain(acc_re, acc_im, tap, bpe=None):
    """The plain sum by einsum, complex128 [E, K, M, M]."""
    x = acc_re[:, :, tap, :].astype(np.float64) + 1j * acc_im[:, :, tap, :].astype(np.float64)
    return np.stack([np.einsum("bki,bkj->kij", x[b0:b0 + n], x[b0:b0 + n].conj()) for b0, n in _estimates(x.shape[0], bpe)])


# ---- eigensolver -------------------------------------------------------------------------------------------------------------------
def round_pairs(Q, r):
    """The pairs (p, q), p < q, of round r of a sweep, in slot order; the slot with the dummy index is left out."""
    n = (Q + 1) & ~1
    idx = [0] + [1 + (i - 1 - r) % (n - 1) for i in range(1, n)]
    pairs = [(idx[i], idx[n - 1 - i]) for i in range(n // 2)]
    return [(min(a, b), max(a, b)) for a, b in pairs if a < Q and b < Q]


def round_pairs_by_shifting(Q, rounds):
    """The same ordering as the rule words it: idx <- [idx[0], idx[n'-1], idx[1], .., idx[n'-2]] after every round."""
    n = (Q + 1) & ~1
    idx, out = list(range(n)), []
    for _ in range(rounds):
        out.append([(min(idx[i], idx[n - 1 - i]), max(idx[i], idx[n - 1 - i])) for i in range(n // 2) if idx[i] < Q and idx[n - 1 - i] < Q])
        idx = [idx[0], idx[n - 1]] + idx[1:n - 1]
    return out


def jacobi_eig(a, num_vectors=None):
    """The rule on one matrix (complex [Q, Q]; the lower triangle and the diagonal's real part are read): (eigenvalues [Q],
    vectors [R, Q], status)."""
    a = np.asarray(a)
    Q = a.shape[0]
    R = Q if num_vectors is None else num_vectors
    low = np.tril(np.ones((Q, Q), bool))
    are = np.where(low, a.real, a.real.T).astype(np.float64)
    aim = np.where(low, a.imag, -a.imag.T).astype(np.float64)
    aim[np.arange(Q), np.arange(Q)] = 0.0
    F = 0.0
    for v in (are * are + aim * aim).reshape(-1):
        F = F + v
    if not F <= np.finfo(np.float64).max:
        return np.full(Q, np.nan), np.full((R, Q), np.nan + 1j * np.nan), -2
    limit = 2.0 ** -104 * F
    vre, vim = np.eye(Q), np.zeros((Q, Q))
    sweeps, converged = 0, False
    with np.errstate(all="ignore"):
        while sweeps < MAX_SWEEPS:
            rotated = False
            for r in range(((Q + 1) & ~1) - 1):
                pairs = round_pairs(Q, r)
                if not pairs:
                    continue
                p, q = np.array([x[0] for x in pairs]), np.array([x[1] for x in pairs])
                br, bi = are[p, q], aim[p, q]
                b2 = br * br + bi * bi
                live = b2 > limit
                if not live.any():
                    continue
                rotated = True
                p, q, br, bi, b2 = p[live], q[live], br[live], bi[live], b2[live]
                ab = np.sqrt(b2)
                ur, ui = br / ab, bi / ab
                tau = (are[q, q] - are[p, p]) / (2.0 * ab)
                d = np.abs(tau) + np.sqrt(1.0 + tau * tau)
                t = np.where(tau < 0.0, -1.0 / d, 1.0 / d)
                c = 1.0 / np.sqrt(1.0 + t * t)
                s = t * c
                gr, gi = s * ur, s * ui
                for mr, mi in ((are, aim), (vre, vim)):  # A <- A J, V <- V J
                    xpr, xpi, xqr, xqi = mr[:, p], mi[:, p], mr[:, q], mi[:, q]
                    npr, npi = c * xpr - (gr * xqr + gi * xqi), c * xpi - (gr * xqi - gi * xqr)
                    nqr, nqi = (gr * xpr - gi * xpi) + c * xqr, (gr * xpi + gi * xpr) + c * xqi
                    mr[:, p], mi[:, p], mr[:, q], mi[:, q] = npr, npi, nqr, nqi
                c, gr, gi = c[:, None], gr[:, None], gi[:, None]  # A <- J^H A
                ypr, ypi, yqr, yqi = are[p, :], aim[p, :], are[q, :], aim[q, :]
                npr, npi = c * ypr - (gr * yqr - gi * yqi), c * ypi - (gr * yqi + gi * yqr)
                nqr, nqi = (gr * ypr + gi * ypi) + c * yqr, (gr * ypi - gi * ypr) + c * yqi
                are[p, :], aim[p, :], are[q, :], aim[q, :] = npr, npi, nqr, nqi
                are[p, q] = aim[p, q] = are[q, p] = aim[q, p] = 0.0
                aim[p, p] = aim[q, q] = 0.0
            if not rotated:
                converged = True
                break
            sweeps += 1
        d = are[np.arange(Q), np.arange(Q)].copy()
        order = np.argsort(-d, kind="stable")  # descending, ties to the lower index
        vec = np.zeros((R, Q), np.complex128)
        for r_ in range(R):
            col = order[r_]
            wr, wi = vre[:, col], vim[:, col]
            m = int(np.argmax(wr * wr + wi * wi))  # the first of the largest
            mod = np.sqrt(wr[m] * wr[m] + wi[m] * wi[m])
            fr, fi = (wr[m] / mod, -wi[m] / mod) if mod > 0.0 else (1.0, 0.0)
            vec[r_].real, vec[r_].imag = wr * fr - wi * fi, wr * fi + wi * fr  # (no complex arithmetic: it would lose the zeros' signs)
            if mod > 0.0:
                vec[r_, m] = mod
    return d[order], vec, sweeps if converged else -1


def family(name, Q, rng):
    """One Hermitian test matrix, complex128 [Q, Q]."""
    def cplx(*shape):
        return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)

    big = 1e140 if Q == 64 else 1e150
    if name == "wishart":
        x = cplx(Q, 3 * Q + 2)
        a = x @ x.conj().T
    elif name == "rank_one":
        v = cplx(Q)
        a = np.outer(v, v.conj())
    elif name == "rank_one_noise":
        v, x = cplx(Q), cplx(Q, 4 * Q)
        a = 100.0 * np.outer(v, v.conj()) + x @ x.conj().T / (4 * Q)
    elif name == "identity":
        a = np.eye(Q, dtype=np.complex128)
    elif name == "zero":
        a = np.zeros((Q, Q), np.complex128)
    elif name in ("scaled_up", "scaled_down"):
        x = cplx(Q, 2 * Q + 1)
        a = (x @ x.conj().T) * (big if name == "scaled_up" else 1.0 / big)
    elif name == "indefinite":
        x = cplx(Q, Q)
        a = x + x.conj().T
    elif name == "graded":
        q, _ = np.linalg.qr(cplx(Q, Q))
        a = (q * np.logspace(0, -12, Q)) @ q.conj().T
    else:
        raise ValueError(name)
    a = np.tril(a) + np.tril(a, -1).conj().T
    a[np.arange(Q), np.arange(Q)] = a.diagonal().real
    return a


def errors(a, lam, vec):
    """(eigenvalue error, residual) in eps ||A||_F and the orthogonality error in eps, of a full decomposition (vec [Q, Q], rows)."""
    a = np.asarray(a, np.complex128)
    Q = a.shape[0]
    norm = np.linalg.norm(a)
    unit = norm if norm > 0.0 else 1.0
    s = 1.0 / unit  # scale first: the products of a matrix at 1e150 overflow
    V = vec.T  # columns
    val = np.abs(lam - np.linalg.eigvalsh(a * s)[::-1] * unit).max() / (EPS * unit)
    res = np.linalg.norm((a * s) @ V - V * (lam * s)) / EPS
    ort = np.linalg.norm(V.conj().T @ V - np.eye(Q)) / EPS
    return val, res, ort


def cases(seed=7):
    """(name, Q, matrix) over FAMILIES x SIZES, and complex64 inputs."""
    rng = np.random.default_rng(seed)
    for Q in SIZES:
        for name in FAMILIES:
            yield name, Q, family(name, Q, rng)
        for name in ("wishart", "rank_one_noise", "indefinite"):
            yield name + "_f32", Q, family(name, Q, rng).astype(np.complex64)


if __name__ == "__main__":
    from gpuacceleratedtracking_amd import hermitian_eig_host

    worst = {}
    for name, Q, a in cases():
        lam, vec, status = hermitian_eig_host(a)
        val, res, ort = errors(a, lam, vec)
        w = worst.setdefault(Q, [0.0, 0.0, 0.0, 0])
        worst[Q] = [max(w[0], val), max(w[1], res), max(w[2], ort), max(w[3], int(status))]
    for Q, w in worst.items():
        print(f"Q {Q:3d}: value {w[0]:8.2f}  residual {w[1]:8.2f}  orthogonality {w[2]:8.2f}  sweeps {w[3]}")
    print("largest:", [max(w[i] for w in worst.values()) for i in range(4)])
