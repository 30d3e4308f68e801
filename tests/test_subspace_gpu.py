"""GPU tests of the subspace layer (include/gat.h gat_accumulator_covariance, gat_hermitian_eig; csrc/gat_eig.hip).

Every output of a device call lies in ONE flat buffer between canaries (tests/sub_cases.py) and is compared with the host twin's
buffer as integer views: every output bit for bit and every canary intact in one comparison (tests/test_subspace_host.py holds the
twins to the FP64 restatement and to numpy.linalg.eigh on the CPU).  The accumulators carry NaN between padded blocks, so a finite
result shows the padding is not read.  The calls do not synchronise: results are read after ctx.sync() only."""
import numpy as np
import pytest

from tests import eig_ref as er
from tests import sub_cases as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g():
    import gpuacceleratedtracking_amd as g
    g.load_library()
    return g


def same_bits(dev_buf, host_buf):
    a = dev_buf.cpu().numpy()
    return a.shape == host_buf.shape and np.array_equal(a.view(np.int64), host_buf.view(np.int64))


def cov_device(g, ctx, d_re, d_im, stride, B, K, L, M, tap, bpe):
    """the device call on flat device accumulators, not synchronised: (status, device buffer, layout)"""
    import torch
    n = sc.estimates(B, bpe) * K * M * M
    host, at = sc.guarded({"cov_re": n, "cov_im": n})
    buf = torch.from_numpy(host).to(ctx.device)
    base = buf.data_ptr()
    rc = ctx.lib.gat_accumulator_covariance(ctx._h, d_re.data_ptr(), d_im.data_ptr(), stride, B, K, L, M, tap, 0 if bpe is None else bpe,
                                            base + 8 * at["cov_re"].start, base + 8 * at["cov_im"].start)
    return rc, buf, at


def check_covariance(g, B, K, L, M, pads=(0, 5), bpes=sc.BPES, seed=0):
    import torch
    lib, ctx = g.load_library(), g.get_context()
    rng = np.random.default_rng(seed + B * 7 + M)
    calls = 0
    for pad in pads:
        acc_re, acc_im, _, _, stride = sc.make_acc(rng, B, K, L, M, pad)
        d_re, d_im = torch.from_numpy(acc_re).to(ctx.device), torch.from_numpy(acc_im).to(ctx.device)
        pending = []
        for tap in sorted({0, L - 1}):
            for bpe in bpes:
                for again in range(2 if bpe in (None, 300) else 1):  # a repeat call gives the same bits
                    rc, buf, at = cov_device(g, ctx, d_re, d_im, stride, B, K, L, M, tap, bpe)
                    assert rc == 0, (pad, tap, bpe)
                    pending.append((tap, bpe, buf))
        ctx.sync()
        for tap, bpe, buf in pending:
            rc, host, at = sc.cov_host(lib, acc_re, acc_im, stride, B, K, L, M, tap, bpe)
            assert rc == 0 and sc.canaries_intact(host, at) and np.isfinite(host).all(), (pad, tap, bpe)
            assert same_bits(buf, host), (B, K, L, M, pad, tap, bpe)
            calls += 1
    return calls


@pytest.mark.parametrize("B,K,L,M", sc.COV_SHAPES)
def test_covariance_equals_the_twin_bit_for_bit(g, B, K, L, M):
    assert check_covariance(g, B, K, L, M) == 2 * len({0, L - 1}) * 6


def test_covariance_through_each_work_split(g):
    """the plan says which: chunk sums through the scratch to a second kernel where (estimate, channel) pairs are few, one workgroup
    walking its chunks where they are many -- and one chunk an estimate leaves nothing to split"""
    split = g.subspace_plan(700, 2, 3, 64, 0)
    assert (split["cov_split"], split["chunks_per_estimate"], split["cov_workgroups"]) == (1, 3, 6) and split["cov_reduce_workgroups"] == 17
    assert g.subspace_plan(700, 2, 3, 64, 0, blocks_per_estimate=300)["cov_split"] == 1  # the last estimate has one chunk of two
    direct = g.subspace_plan(600, 520, 1, 2, 0)
    assert (direct["cov_split"], direct["chunks_per_estimate"], direct["cov_workgroups"], direct["scratch_bytes"]) == (0, 3, 520, 0)
    assert g.subspace_plan(600, 520, 1, 2, 0, blocks_per_estimate=256)["chunks_per_estimate"] == 1
    assert check_covariance(g, 600, 520, 1, 2, pads=(3,), bpes=(None, 256, 300, 599), seed=1) == 6
    # split again right after a direct call: the scratch is the context's
    assert check_covariance(g, 513, 3, 2, 5, pads=(1,), bpes=(None, 257), seed=2) == 6


def eig_device(g, ctx, batch, R, want=("eigenvalues", "vec", "status")):
    import torch
    n, Q = batch.shape[0], batch.shape[-1]
    a_re, a_im, flags = sc.eig_planes(batch)
    d_re, d_im = torch.from_numpy(a_re).to(ctx.device), torch.from_numpy(a_im).to(ctx.device)
    host, at = sc.eig_layout(n, Q, R, want)
    if "status" in at and n % 2:
        host[at["status"]].view(np.int32)[n:] = 0
    buf = torch.from_numpy(host).to(ctx.device)
    rc = ctx.lib.gat_hermitian_eig(ctx._h, d_re.data_ptr(), d_im.data_ptr(), n, Q, R, flags, *sc.eig_pointers(buf.data_ptr(), at))
    return rc, buf, (d_re, d_im)


@pytest.mark.parametrize("Q", er.SIZES)
def test_eigensolver_equals_the_twin_bit_for_bit(g, Q):
    """values, vectors and status; batches that mix the families, float64 and float32 inputs"""
    lib, ctx = g.load_library(), g.get_context()
    rng = np.random.default_rng(500 + Q)
    if Q <= 17:
        combos = [(n, R) for n in (1, 3, 70) for R in sorted({0, 1, Q})]
    else:  # (the twin's time: every n and every R, not their product)
        combos = [(1, Q), (3, 0), (3, Q), (70 if Q == 33 else 18, 1)] + ([(70, 0)] if Q == 64 else [])
    pending = []
    for n, R in combos:
        for f32 in (False, True):
            if f32 and (n, R) != combos[-1] and Q > 17:
                continue
            with np.errstate(over="ignore"):
                batch = sc.mixed_batch(Q, n, rng, f32)
            rc, buf, keep = eig_device(g, ctx, batch, R)
            assert rc == 0, (n, R, f32)
            pending.append((batch, R, buf, keep))
    ctx.sync()
    seen = set()
    for batch, R, buf, _ in pending:
        rc, host, at = sc.eig_host(lib, batch, R)
        assert rc == 0 and sc.canaries_intact(host, at)
        assert same_bits(buf, host), (Q, len(batch), R, batch.dtype)
        seen.update(int(s) for s in sc.status_of(host, at, len(batch)))
    assert min(seen) >= -2 and -1 not in seen and max(seen) <= 30 and (Q == 1 or max(seen) >= 1)


def test_eigensolver_subsets_of_the_outputs(g):
    lib, ctx = g.load_library(), g.get_context()
    rng = np.random.default_rng(77)
    batch = sc.mixed_batch(17, 5, rng)
    pending = []
    for want in (("eigenvalues",), ("vec",), ("status",), ("eigenvalues", "status"), ("vec", "status")):
        for R in (0, 3):
            rc, buf, keep = eig_device(g, ctx, batch, R, want)
            assert rc == 0
            pending.append((want, R, buf, keep))
    ctx.sync()
    for want, R, buf, _ in pending:
        rc, host, at = sc.eig_host(lib, batch, R, want)
        assert rc == 0 and same_bits(buf, host), (want, R)


def test_eigensolver_takes_the_spatial_covariance_as_it_is(g):
    """float32 planes straight from gat_spatial_covariance, several estimates in one batch"""
    import torch
    ctx = g.get_context()
    gen = torch.Generator().manual_seed(5)
    M, N, B = 6, 500, 9
    x = torch.randn((2, M, B * N), generator=gen, dtype=torch.float32)
    mix = torch.randn((M, M), generator=gen, dtype=torch.float32)
    re, im = (mix @ x[0]).to(ctx.device).contiguous(), (mix @ x[1]).to(ctx.device).contiguous()
    cov = g.spatial_covariance((re, im), N, B, blocks_per_estimate=2)
    assert cov.dtype == torch.complex64 and tuple(cov.shape) == (5, M, M)
    lam, vec, status = g.hermitian_eig(cov)
    ctx.sync()
    h_lam, h_vec, h_status = g.hermitian_eig_host(cov.cpu().numpy())
    assert np.array_equal(lam.cpu().numpy().view(np.int64), h_lam.view(np.int64)) and np.array_equal(status.cpu().numpy(), h_status)
    v = vec.cpu().numpy()
    assert np.array_equal(v.real.copy().view(np.int64), h_vec.real.copy().view(np.int64))
    assert np.array_equal(v.imag.copy().view(np.int64), h_vec.imag.copy().view(np.int64))
    assert (h_status > 0).all() and (h_lam[:, -1] > 0).all()
    c = cov.cpu().numpy().astype(np.complex128)
    for e in range(5):
        val, res, ort = er.errors(c[e], h_lam[e], h_vec[e])
        assert max(val, res, ort) <= er.EIG_C[8], (e, val, res, ort)


def test_python_surface_and_errors(g):
    import torch
    ctx = g.get_context()
    rng = np.random.default_rng(21)
    B, K, L, M = 300, 3, 3, 4
    # a rank-one signal per channel under noise, every block with a random sign (data bits) and a common random phase (the loop's)
    a = np.exp(2j * np.pi * rng.uniform(0, 1, (K, M)))
    a[:, 0] = np.exp(2j * np.pi * 0.3)
    sym = rng.choice([-1.0, 1.0], (B, K, 1)) * np.exp(2j * np.pi * rng.uniform(0, 1, (B, K, 1)))
    x = np.zeros((B, K, L, M), np.complex128)
    x[:, :, 1, :] = 50.0 * sym * a[None] + (rng.standard_normal((B, K, M)) + 1j * rng.standard_normal((B, K, M)))
    x[:, :, 0, :] = rng.standard_normal((B, K, M))
    h_re, h_im = x.real.astype(np.float32), x.imag.astype(np.float32)
    padded = torch.full((B, K * L * M + 7), float("nan"), dtype=torch.float32, device=ctx.device)
    views = []
    for h in (h_re, h_im):
        t = padded.clone()
        t[:, :K * L * M] = torch.from_numpy(h.reshape(B, -1)).to(ctx.device)
        views.append(t[:, :K * L * M].view(B, K, L, M))
    acc_re, acc_im = views
    assert acc_re.stride(0) == K * L * M + 7
    for bpe in (None, 128):
        cov = g.accumulator_covariance(acc_re, acc_im, tap_index=1, blocks_per_estimate=bpe)
        ctx.sync()
        want = g.accumulator_covariance_host(h_re, h_im, tap_index=1, blocks_per_estimate=bpe)
        got = cov.cpu().numpy()
        assert got.shape == want.shape == (1 if bpe is None else 3, K, M, M) and cov.dtype == torch.complex128
        assert np.array_equal(got.real.copy().view(np.int64), want.real.copy().view(np.int64))
        assert np.array_equal(got.imag.copy().view(np.int64), want.imag.copy().view(np.int64))
    lam, vec, status = g.hermitian_eig(cov, num_vectors=2)
    assert tuple(lam.shape) == (3, K, M) and tuple(vec.shape) == (3, K, 2, M) and tuple(status.shape) == (3, K) and status.dtype == torch.int32
    steer, lam1 = g.steering_from_accumulators(acc_re, acc_im, tap_index=1, ref_ant=0)
    steer2, _ = g.steering_from_accumulators(acc_re, acc_im, tap_index=1, ref_ant=2, blocks_per_estimate=128)
    ctx.sync()
    s, s2 = steer.cpu().numpy(), steer2.cpu().numpy()
    assert s.shape == (1, K, M) and s2.shape == (3, K, M) and steer.dtype == torch.complex128 and tuple(lam1.shape) == (1, K, M)
    assert np.abs(s[..., 0].imag).max() <= 1e-15 and (s[..., 0].real > 0).all() and np.abs(s2[..., 2].imag).max() <= 1e-15 and (s2[..., 2].real > 0).all()
    assert np.abs(np.linalg.norm(s, axis=-1) - 1).max() < 1e-12
    # the estimate is the channel's steering vector: 1 - |a^H s|^2 / (M |s|^2) of the order of (M - 1) / (M B SNR), SNR = 50^2 / 2
    miss = 1 - np.abs(np.einsum("km,ekm->ek", a.conj(), s)) ** 2 / M
    assert miss.max() < 8 * (M - 1) / (M * B * 1250.0), miss
    w = g.beamformer_weights(None, steer[0], "conventional")
    ctx.sync()
    assert np.abs(np.einsum("km,km->k", w.cpu().numpy().conj(), s[0]) - 1).max() < 1e-12
    # errors
    with pytest.raises(g.GatError):
        g.accumulator_covariance(acc_re, acc_im, tap_index=L)
    with pytest.raises(ValueError):
        g.accumulator_covariance(acc_re, acc_im.double(), tap_index=0)
    with pytest.raises(ValueError):
        g.accumulator_covariance(acc_re.transpose(1, 2), acc_im.transpose(1, 2), tap_index=0)
    with pytest.raises(ValueError):
        g.accumulator_covariance(acc_re, acc_im, tap_index=0, blocks_per_estimate=0)
    with pytest.raises(ValueError):
        g.steering_from_accumulators(acc_re, acc_im, tap_index=1, ref_ant=M)
    with pytest.raises(ValueError):
        g.hermitian_eig(cov.real)
    with pytest.raises(ValueError):
        g.hermitian_eig(cov[..., :3])
    with pytest.raises(g.GatError):
        g.hermitian_eig(cov, num_vectors=M + 1)
