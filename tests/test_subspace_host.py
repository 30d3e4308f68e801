"""The subspace layer without a device: the package's surface; the covariance's host twin (gat_accumulator_covariance_host) against
the FP64 restatement (tests/eig_ref.py) bit for bit and against the plain sum; the eigensolver's twin (gat_hermitian_eig_host)
against numpy.linalg.eigh over the matrix families and sizes of tests/eig_ref.py within EIG_C[Q] * eps * ||A||_F, and against the
restatement of the rule bit for bit; the exact cases; every refusal with nothing written; source_count."""
import numpy as np
import pytest

from tests import eig_ref as er
from tests import sub_cases as sc

ARG, RANGE = 1, 2


@pytest.fixture(scope="module")
def g():
    import gpuacceleratedtracking_amd as g
    g.load_library()
    return g


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64)


def test_the_surface(g):
    """declared, bound and exported (on the parent commit none of it exists)"""
    from gpuacceleratedtracking_amd import _lib
    lib = g.load_library()
    for name in ("gat_accumulator_covariance", "gat_accumulator_covariance_host", "gat_hermitian_eig", "gat_hermitian_eig_host", "gat_subspace_plan"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    for name in ("accumulator_covariance", "accumulator_covariance_host", "hermitian_eig", "hermitian_eig_host", "steering_from_accumulators",
                 "source_count", "subspace_plan"):
        assert callable(getattr(g, name))
    assert callable(g.TrackingLoop.steering)
    assert (_lib.GAT_ACC_COV_CHUNK, _lib.GAT_EIG_MAX_SWEEPS, _lib.GAT_EIG_INPUT_F32) == (er.CHUNK, er.MAX_SWEEPS, 1)
    p = g.subspace_plan(700, 2, 3, 64, 1, eig_matrices=6, eig_order=64, eig_vectors=1)
    assert (p["num_estimates"], p["chunks_per_estimate"], p["cov_split"], p["cov_workgroups"]) == (1, 3, 1, 6)
    assert p["scratch_bytes"] >= 2 * 6 * 2080 * 8 and p["eig_workgroups"] == 6 and 128 * 1024 < p["eig_lds_bytes"] <= 160 * 1024
    p = g.subspace_plan(700, 600, 1, 2, 0)
    assert (p["cov_split"], p["cov_workgroups"], p["cov_reduce_workgroups"], p["scratch_bytes"], p["eig_workgroups"]) == (0, 600, 0, 0, 0)
    with pytest.raises(g.GatError):
        g.subspace_plan()


# ---- covariance --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,K,L,M", sc.COV_SHAPES)
def test_covariance_twin_against_the_restatement(g, B, K, L, M):
    lib = g.load_library()
    rng = np.random.default_rng(B * 7 + M)
    for pad in (0, 5):
        acc_re, acc_im, dre, dim, stride = sc.make_acc(rng, B, K, L, M, pad)
        for tap in sorted({0, L - 1}):
            for bpe in sc.BPES:
                if bpe == 1 and B > 300:
                    continue  # (700 estimates of 64 x 64: the restatement's time, not another path)
                rc, buf, at = sc.cov_host(lib, acc_re, acc_im, stride, B, K, L, M, tap, bpe)
                assert rc == 0 and sc.canaries_intact(buf, at), (pad, tap, bpe)
                E = sc.estimates(B, bpe)
                cov = np.empty((E, K, M, M), np.complex128)
                cov.real, cov.imag = buf[at["cov_re"]].reshape(E, K, M, M), buf[at["cov_im"]].reshape(E, K, M, M)
                want = er.acc_cov_chunked(dre, dim, tap, bpe)
                assert np.array_equal(bits(cov.real), bits(want.real)) and np.array_equal(bits(cov.imag), bits(want.imag)), (pad, tap, bpe)
                assert np.array_equal(cov.real, np.swapaxes(cov.real, -1, -2)) and np.array_equal(cov.imag, -np.swapaxes(cov.imag, -1, -2))
                d = np.diagonal(cov.imag, axis1=-2, axis2=-1)
                assert not d.any() and not np.signbit(d).any()
                plain = er.acc_cov_plain(dre, dim, tap, bpe)
                x = np.abs(dre[:, :, tap, :].astype(np.float64) + 1j * dim[:, :, tap, :].astype(np.float64))
                bpe_ = B if bpe is None or bpe > B else bpe
                scale = np.stack([np.einsum("bki,bkj->kij", x[b0:b0 + bpe_], x[b0:b0 + bpe_]) for b0 in range(0, B, bpe_)])
                assert (np.abs(cov - plain) <= B * er.EPS * scale).all(), (pad, tap, bpe)  # B eps sum_b |x_i| |x_j|
                if pad == 0 and K * L * M * B < 200000:
                    assert np.array_equal(bits(g.accumulator_covariance_host(dre, dim, tap_index=tap, blocks_per_estimate=bpe).real), bits(cov.real))


def test_covariance_nan_is_not_an_error(g):
    rng = np.random.default_rng(3)
    re, im = rng.standard_normal((6, 2, 3, 3)).astype(np.float32), rng.standard_normal((6, 2, 3, 3)).astype(np.float32)
    re[4, 1, 2, 1] = np.nan
    cov = g.accumulator_covariance_host(re, im, tap_index=2)
    bad = np.isnan(cov)
    assert bad[0, 1, 1, :].all() and bad[0, 1, :, 1].all() and not bad[0, 0].any() and not bad[0, 1, 0, 0] and not bad[0, 1, 2, 0]
    assert not np.isnan(g.accumulator_covariance_host(re, im, tap_index=0)).any()


def test_covariance_refusals_write_nothing(g):
    lib = g.load_library()
    rng = np.random.default_rng(5)
    B, K, L, M = 24, 2, 3, 2
    acc_re, acc_im, _, _, stride = sc.make_acc(rng, B, K, L, M, 0)
    n = K * M * M

    def call(re=acc_re, im=acc_im, stride=stride, B=B, K=K, L=L, M=M, tap=1, bpe=0, null_out=None):
        buf, at = sc.guarded({"cov_re": 4 * n, "cov_im": 4 * n})
        base = buf.ctypes.data
        rc = lib.gat_accumulator_covariance_host(None if re is None else re.ctypes.data, None if im is None else im.ctypes.data, stride, B, K, L, M, tap, bpe,
                                                 None if null_out == "re" else base + 8 * at["cov_re"].start,
                                                 None if null_out == "im" else base + 8 * at["cov_im"].start)
        assert (buf == sc.CANARY).all() or rc == 0
        return rc

    assert call() == 0
    assert call(re=None) == ARG and call(im=None) == ARG and call(null_out="re") == ARG and call(null_out="im") == ARG
    assert call(B=0) == ARG and call(K=0) == ARG and call(L=0, tap=0) == ARG and call(M=0) == ARG
    assert call(M=65) == RANGE and call(B=(1 << 20) + 1) == RANGE and call(K=4097) == RANGE
    assert call(tap=3) == RANGE and call(tap=-1) == RANGE
    assert call(stride=stride - 1) == ARG and call(stride=-stride) == ARG
    assert call(B=1 << 20, K=511, L=1, M=64, tap=0, stride=511 * 64) == RANGE  # 34 GB of chunk sums
    with pytest.raises(g.GatError):
        g.accumulator_covariance_host(np.zeros((3, 1, 2, 2), np.float32), np.zeros((3, 1, 2, 2), np.float32), tap_index=2)
    with pytest.raises(ValueError):
        g.accumulator_covariance_host(np.zeros((3, 1, 2, 2), np.float32), np.zeros((3, 1, 2, 2), np.float32), tap_index=0, blocks_per_estimate=0)


# ---- eigensolver -------------------------------------------------------------------------------------------------------------------
def test_the_pairing_is_the_rule_s_shifting():
    for Q in er.SIZES + (6, 7):
        n = (Q + 1) & ~1
        shifted = er.round_pairs_by_shifting(Q, 2 * (n - 1))
        assert [er.round_pairs(Q, r % (n - 1)) for r in range(2 * (n - 1))] == shifted
        met = sorted(p for r in shifted[:n - 1] for p in r)
        assert met == [(a, b) for a in range(Q) for b in range(a + 1, Q)]


def test_eigen_twin_against_eigh(g):
    worst, seen = {}, 0
    for name, Q, a in er.cases():
        lam, vec, status = g.hermitian_eig_host(a)
        val, res, ort = er.errors(a, lam, vec)
        c = er.EIG_C[Q]
        w = worst.setdefault(Q, [0.0, 0.0, 0.0, 0])
        worst[Q] = [max(w[0], val), max(w[1], res), max(w[2], ort), max(w[3], int(status))]
        assert val <= c and res <= c and ort <= c, (name, Q, val, res, ort, c)
        assert 0 <= status <= 30, (name, Q, status)
        assert (np.diff(lam) <= 0).all()
        big = np.argmax(np.abs(vec) ** 2, axis=1)
        top = vec[np.arange(Q), big]
        assert (top.imag == 0).all() and (top.real > 0).all(), (name, Q)
        seen += 1
    print({Q: [round(float(v), 2) for v in w[:3]] + [w[3]] for Q, w in worst.items()})
    assert seen == len(er.SIZES) * (len(er.FAMILIES) + 3)


@pytest.mark.parametrize("Q", [q for q in er.SIZES if q <= 33])
def test_eigen_twin_is_the_restated_rule_bit_for_bit(g, Q):
    lib = g.load_library()
    rng = np.random.default_rng(100 + Q)
    for f32 in (False, True):
        with np.errstate(over="ignore"):
            batch = sc.mixed_batch(Q, 9 if Q <= 17 else 3, rng, f32)
        for R in sorted({0, 1, Q}):
            rc, buf, at = sc.eig_host(lib, batch, R)
            assert rc == 0 and sc.canaries_intact(buf, at)
            st = sc.status_of(buf, at, len(batch))
            for i, a in enumerate(batch):
                lam, vec, status = er.jacobi_eig(a, R)
                assert status == st[i], (Q, f32, R, i)
                assert np.array_equal(bits(buf[at["eigenvalues"]].reshape(len(batch), Q)[i]), bits(lam)), (Q, f32, R, i)
                assert np.array_equal(bits(buf[at["vec_re"]].reshape(len(batch), R, Q)[i]), bits(vec.real)), (Q, f32, R, i)
                assert np.array_equal(bits(buf[at["vec_im"]].reshape(len(batch), R, Q)[i]), bits(vec.imag)), (Q, f32, R, i)
        if f32 and len(batch) == 9:
            assert (st == -2).any()  # the family scaled by 1e150 is infinite in float32


def test_exact_cases(g):
    for Q in (1, 2, 5, 16):
        lam, vec, status = g.hermitian_eig_host(np.eye(Q, dtype=np.complex128))
        assert status == 0 and (lam == 1).all() and np.array_equal(vec, np.eye(Q))
        lam, vec, status = g.hermitian_eig_host(np.zeros((Q, Q), np.complex128))
        assert status == 0 and not lam.any() and np.array_equal(vec, np.eye(Q))
    # descending, equal eigenvalues in index order: the eigenvectors of a diagonal matrix are unit vectors
    d = np.array([2.0, 5.0, 2.0, -1.0, 5.0, 2.0])
    lam, vec, status = g.hermitian_eig_host(np.diag(d).astype(np.complex128))
    assert status == 0 and np.array_equal(lam, [5, 5, 2, 2, 2, -1])
    assert np.array_equal(np.argmax(np.abs(vec), axis=1), [1, 4, 0, 2, 5, 3]) and np.array_equal(np.abs(vec).sum(axis=1), np.ones(6))
    # only the lower triangle and the diagonal's real part are read
    rng = np.random.default_rng(9)
    a = er.family("wishart", 7, rng)
    junk = np.tril(a) + np.triu(rng.standard_normal((7, 7)) + 1j * rng.standard_normal((7, 7)), 1) + 1j * np.diag(rng.standard_normal(7))
    for x, y in zip(g.hermitian_eig_host(a), g.hermitian_eig_host(junk)):
        assert np.array_equal(x, y)
    # a batch keeps its leading dimensions; R rows
    lam, vec, status = g.hermitian_eig_host(np.stack([a, 2 * a, 3 * a, a, a, a]).reshape(2, 3, 7, 7), num_vectors=2)
    assert lam.shape == (2, 3, 7) and vec.shape == (2, 3, 2, 7) and status.shape == (2, 3) and np.array_equal(lam[0, 1], 2 * lam[0, 0])
    # a rank-one matrix: the principal eigenvector is the vector
    v = rng.standard_normal(4) + 1j * rng.standard_normal(4)
    lam, vec, _ = g.hermitian_eig_host(np.outer(v, v.conj()), num_vectors=1)
    assert abs(lam[0] - np.vdot(v, v).real) < 1e-14 * lam[0] and abs(abs(np.vdot(vec[0], v)) - np.linalg.norm(v)) < 1e-14


def test_a_nan_entry_gives_status_minus_two_and_nan_outputs(g):
    rng = np.random.default_rng(4)
    batch = np.stack([er.family("wishart", 5, rng) for _ in range(3)])
    for bad in (np.nan, np.inf):
        b = batch.copy()
        b[1, 3, 2] = bad
        lam, vec, status = g.hermitian_eig_host(b, num_vectors=2)
        assert list(status) == [status[0], -2, status[2]] and status[0] > 0 and status[2] > 0
        assert np.isnan(lam[1]).all() and np.isnan(vec[1].real).all() and np.isnan(vec[1].imag).all()
        assert np.isfinite(lam[[0, 2]]).all() and np.isfinite(vec[[0, 2]]).all()
        b = batch.copy()
        b[1, 2, 3] = bad  # the upper triangle is not read
        assert (g.hermitian_eig_host(b)[2] > 0).all()


def test_eigen_refusals_write_nothing(g):
    lib = g.load_library()
    rng = np.random.default_rng(6)
    batch = np.stack([er.family("wishart", 5, rng) for _ in range(3)])
    a_re, a_im, _ = sc.eig_planes(batch)

    def call(re=a_re, im=a_im, n=3, Q=5, R=2, flags=0, want=("eigenvalues", "vec", "status"), drop=None):
        buf, at = sc.eig_layout(3, 5, 5, want)
        ptr = list(sc.eig_pointers(buf.ctypes.data, at))
        if drop is not None:
            ptr[drop] = None
        rc = lib.gat_hermitian_eig_host(None if re is None else re.ctypes.data, None if im is None else im.ctypes.data, n, Q, R, flags, *ptr)
        assert (buf == sc.CANARY).all() or rc == 0
        return rc

    assert call() == 0 and call(want=("status",)) == 0 and call(want=("eigenvalues",)) == 0 and call(want=("vec",)) == 0 and call(R=0) == 0
    assert call(re=None) == ARG and call(im=None) == ARG and call(want=()) == ARG and call(n=0) == ARG and call(n=-1) == ARG
    assert call(Q=0, R=0) == RANGE and call(Q=65) == RANGE and call(R=-1) == RANGE and call(R=6) == RANGE
    assert call(drop=1) == ARG and call(drop=2) == ARG and call(flags=2) == ARG
    with pytest.raises(ValueError):
        g.hermitian_eig_host(np.zeros((3, 4), np.complex128))
    with pytest.raises(ValueError):
        g.hermitian_eig_host(np.zeros((3, 3)))
    with pytest.raises(g.GatError):
        g.hermitian_eig_host(np.zeros((3, 3), np.complex128), num_vectors=4)


# ---- source count ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["mdl", "aic"])
def test_source_count(g, method):
    rng = np.random.default_rng(12)
    Q, N = 8, 2000

    def eigenvalues(powers):
        """of a sample covariance of N snapshots: unit noise and sources of the given powers in random directions"""
        x = (rng.standard_normal((Q, N)) + 1j * rng.standard_normal((Q, N))) / np.sqrt(2.0)
        for p in powers:
            v = rng.standard_normal(Q) + 1j * rng.standard_normal(Q)
            s = (rng.standard_normal(N) + 1j * rng.standard_normal(N)) / np.sqrt(2.0)
            x = x + np.sqrt(p) * np.outer(v / np.linalg.norm(v), s)
        return g.hermitian_eig_host(x @ x.conj().T / N, num_vectors=0)[0]

    sets = [eigenvalues(()), eigenvalues((30.0,)), eigenvalues((100.0, 30.0, 10.0))]
    if method == "mdl":  # MDL is consistent; AIC tends to overestimate, so it is held to the cases with sources only
        assert g.source_count(sets[0], N, "mdl") == 0
    assert g.source_count(sets[1], N, method) == 1 and g.source_count(sets[2], N, method) == 3
    assert list(g.source_count(np.stack(sets[1:]), N, method)) == [1, 3]
    assert g.source_count(sets[2][::-1], N, method) == 3  # any order
    assert g.source_count(np.ones(5), 100, method) == 0 and g.source_count([4.0, 1.0, 1.0, 1.0], 1000, method) == 1
    with pytest.raises(ValueError):
        g.source_count(sets[0], N, "bic")
    with pytest.raises(ValueError):
        g.source_count(sets[0], 0, method)
