"""Every kernel across the whole domain of the channel record (include/gat.h gat_channel_params) and at its bounds.

The parity tests draw records from a narrow, realistic box (code phase in [0, Lc), carrier IF +- 5 kHz, carrier phase in
[0, 1), nearly equal code rates).  The library accepts far more, and its kernels switch arithmetic per channel on the
record's values: the chip walk or the exact evaluation of every entry, the replica fill by quads, the split-bf16 kernel's
code-index increment or re-anchor, the float-reciprocal modulo.  Here every path of the correlator runs records on both
sides of each switch, mixed in one launch:

A. chip edges across the code domain, bit-exact: an all-ones signal at zero carrier makes every output an integer sum of
   chips, compared exactly with the FP64 oracle (and the replica generators bit for bit);
B. the carrier across its domain -- above Nyquist, many times fs, phases up to 0.99e15 cycles -- against a reference built
   on the exactly reduced step and phase, with the identities R(f, phi) = R(f, phi + 2^10) = R(f + k fs, phi);
C. one poison predicate: device records at each bound and one step past it give NaN for exactly the offending channel on
   every path, and the host entry points reject exactly those records without touching the outputs.

Run with -m gpu."""
import numpy as np
import pytest

import oracle
from tests.helpers import (PATHS, RTOL, channel_errors, check_close, code_table, configure, correlate, correlate_reduced,
                           floormod_hard_taus, geometry, reset, span_bound_tau, standard_codes_after)  # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu

FS_A = 16777216.0  # 2^24 Hz: code rate / fs is exactly the ratio the test asks for
FC = 1.023e6
SENTINEL = 7.0


@pytest.fixture(scope="module")
def g():
    import gpuacceleratedtracking_amd as g
    g.load_library()
    return g


@pytest.fixture()
def ctx(g, standard_codes_after):
    """The default context, its kernel selection, tiling and options restored after the test."""
    c = g.get_context()
    yield c
    reset(g, c)


def as_oracle(prm):
    return prm.view(oracle.PARAMS_DTYPE)


def nxt(x, d=np.inf):
    return float(np.nextafter(np.float64(x), d))


# ---- A. chip edges across the code domain, bit-exact --------------------------------------------------------------------------
TABLES = ["GPSL1", "GPSL5", "caller-101"]
SHIFTS_A = np.array([-8, 0, 8], dtype=np.int32)  # even tap distances: the 2 x 2 tile may fill by quads


def table(name):
    if name == "caller-101":
        return code_table(101, 4, 101, "pm1")
    return oracle.codes(name, 32)


def chip_channels(lc, P, reach, matrix_core=False):
    """(prn, code rate / fs, tau) of the channels of one launch: each regime switch straddled, code phases over the whole
    accepted domain.  matrix_core: leave out code rates the matrix-core kernels poison (ratio * 32 >= Lc: part C)."""
    ratios = [1.0, 2.5, 7.3]
    for rpc in (256, 128, 64):  # chip walk -> exact evaluation of every entry: ratio * (RPC + 1) + 2 >= Lc
        t = (lc - 2.0) / (rpc + 1)
        ratios += [nxt(t, 0), t, nxt(t), (lc - 1.0) / (rpc + 1)]
        t = (lc - 2.0) / (4 * rpc + 1)  # quads need ratio * (4 RPC + 1) + 2 < Lc
        if t < 0.34:
            ratios += [nxt(t, 0), t, nxt(t)]
    q = 0x55000000 / 2 ** 32  # quads need floor(ratio * 2^32) < 0x55000000
    ratios += [nxt(q, 0), q, nxt(q), 1.0 / 3.0, nxt(1.0 / 3.0), 0x55ffffff / 2 ** 32]
    for T in (32, 64, 128, 256):  # split-bf16 kernel: code-index increment while ratio * (T + 2) < Lc
        t = lc / (T + 2.0)
        ratios += [nxt(t, 0), t, nxt(t)]
    ratios += [nxt(lc / 32.0, 0)]
    if matrix_core:
        ratios = [r for r in ratios if r * 32.0 < lc]
    far = -3.7e8 if 3.7e8 < 0.4 * min(2.0 ** 30, 2097152.0 * lc) else -0.35 * 2097152.0 * lc
    taus = [0.0, lc - 1e-9, -0.25, -lc - 0.5, far, 3.0 * lc, nxt(3.0 * lc, 0), nxt(3.0 * lc), 12345.0 * lc,
            nxt(12345.0 * lc, 0), 0.999999999]
    ch = [((i * 7) % P, r, taus[i % len(taus)]) for i, r in enumerate(ratios)]
    # code rate 0: one chip for the whole block -- tau an integer, one ulp either side, multiples of Lc
    for t in (5.0, nxt(5.0, 0), nxt(5.0), float(lc), nxt(lc, 0), nxt(lc), -float(lc), nxt(-lc, 0), nxt(-lc)):
        ch.append((P - 1, 0.0, t))
    # the float-reciprocal modulo one quotient off, both signs; code rate 0 (every sample on that index) and 1
    hi = min(2.0 ** 30, 2097152.0 * lc) - reach - 2
    for sgn in (1, -1):
        for t in floormod_hard_taus(lc, int(hi // 2), int(hi), 17 + lc, count=2) if sgn > 0 else \
                floormod_hard_taus(lc, -int(hi), -int(hi // 2), 19 + lc, count=2):
            ch += [(P - 1, 0.0, t + 0.5), (0, 1.0, t - reach if sgn > 0 else t + reach)]
    # just inside the span bound (2^30 binds for the ICD tables, 2^21 Lc for the short caller table), both signs
    for r in (0.0, 1.0, 2.5):
        t_in, _ = span_bound_tau(r, reach, lc)
        ch += [(1 % P, r, t_in), (2 % P, r, -t_in)]
    return ch


def ones_case(codes, channels, N, M, fs, S=None):
    P, lc = codes.shape
    S = S or (N + 7) // 8 * 8
    import gpuacceleratedtracking_amd as g
    prn = np.array([c[0] for c in channels])
    prm = g.make_params(prn, np.array([c[1] for c in channels]) * fs, 0.0, np.array([c[2] for c in channels]), 0.0)[None, :]
    re = np.ones((M, S), dtype=np.float32)
    im = np.zeros_like(re)
    return prm, re, im


@pytest.mark.parametrize("tab", TABLES)
@pytest.mark.parametrize("path", list(PATHS))
def test_chip_edges_bit_exact(g, ctx, path, tab):
    codes = table(tab)
    ctx.set_codes(codes)
    configure(g, ctx, path)
    N, M, _ = geometry(path, 32768, 4, 1)
    P, lc = codes.shape
    reach = N + int(np.abs(SHIFTS_A).max())
    channels = chip_channels(lc, P, reach, matrix_core=path.startswith("mc-"))
    prm, re, im = ones_case(codes, channels, N, M, FS_A)
    ref = oracle.correlate_f64(re, im, codes, as_oracle(prm), FS_A, SHIFTS_A, N=N, blk_stride=re.shape[1])
    assert np.array_equal(ref.real, np.rint(ref.real)) and np.abs(ref.real).max() < 2 ** 24
    # (the split-bf16 kernel and one-wave workgroups take chip rows of up to 2048 bytes: GPS L5 runs on four-wave workgroups)
    got, info = correlate(g, ctx, path, re, im, prm, N, FS_A, SHIFTS_A,
                          check_want=not ((path.startswith("mc-bf16") or path == "one-wave") and lc > 2032))
    bad = [(k, channels[k], got[0, k, :, 0].real, ref[0, k, :, 0].real) for k in range(len(channels))
           if not (np.array_equal(got[0, k].real, ref[0, k].real) and np.all(got[0, k].imag == 0))]
    assert not bad, f"{path} {tab} {info}: {len(bad)} channels differ: {bad[:6]}"


@pytest.mark.parametrize("tab", TABLES)
def test_chip_edges_bit_exact_host_records_and_resident(g, ctx, tab):
    """The same channels as host records: through gat_downconvert_and_correlate (default planner) and through the resident
    correlator (at most 16 channels per call)."""
    import torch
    codes = table(tab)
    ctx.set_codes(codes)
    N, M = 32768, 4
    P, lc = codes.shape
    channels = chip_channels(lc, P, N + 8)
    prm, re, im = ones_case(codes, channels, N, M, FS_A)
    ref = oracle.correlate_f64(re, im, codes, as_oracle(prm), FS_A, SHIFTS_A, N=N)
    got, info = correlate(g, ctx, "default-planar", re, im, prm, N, FS_A, SHIFTS_A, host=True)
    assert np.array_equal(got, ref), (tab, info)
    d_re, d_im = torch.from_numpy(re).to(ctx.device), torch.from_numpy(im).to(ctx.device)
    torch.cuda.synchronize()
    for k0 in range(0, len(channels), 16):
        part = np.ascontiguousarray(prm[0, k0:k0 + 16])
        desc = g._lib.SignalDesc(d_re.data_ptr(), d_im.data_ptr(), g.GAT_LAYOUT_PLANAR, M, N, N, N, 0)
        with ctx.open_resident(desc, part.size, SHIFTS_A, FS_A) as res:
            o_re, o_im = res.correlate(part)
            assert np.array_equal(o_re.astype(np.float64), ref[0, k0:k0 + 16].real) and np.all(o_im == 0), (tab, k0)


@pytest.mark.parametrize("tab", TABLES)
def test_code_replica_bit_exact_across_the_code_domain(g, ctx, tab):
    """gat_gen_code_replica (host records) and gat_gen_code_replica_multi (device records, every channel at once) bit for bit
    against oracle.gen_code_replica on the same channels, taps in front of the block."""
    import torch
    codes = table(tab)
    ctx.set_codes(codes)
    P, lc = codes.shape
    count, first = 20011, -8
    channels = chip_channels(lc, P, 32768 + 8)  # (a longer reach: every code phase is inside the replica's span bound too)
    want = np.stack([oracle.gen_code_replica(codes, p, r * FS_A, FS_A, t, first, count) for p, r, t in channels])
    rep = torch.full((len(channels), count + 8), SENTINEL, device=ctx.device)
    prm = g.make_params(np.array([c[0] for c in channels]), np.array([c[1] for c in channels]) * FS_A, 0.0,
                        np.array([c[2] for c in channels]), 0.0)
    ctx.gen_code_replica_multi(rep, count, ctx.params_to_device(prm), len(channels), FS_A, first)
    got = rep.cpu().numpy()
    diff = [k for k in range(len(channels)) if not np.array_equal(got[k, :count], want[k])]
    assert not diff, (tab, [channels[k] for k in diff[:6]])
    assert (got[:, count:] == SENTINEL).all()
    one = torch.full((count + 8,), SENTINEL, device=ctx.device)
    for k, (p, r, t) in enumerate(channels):
        ctx.gen_code_replica(one, count, p, r * FS_A, FS_A, t, first)
        assert np.array_equal(one.cpu().numpy()[:count], want[k]), (tab, channels[k])


# ---- B. the carrier across its domain, against the exactly reduced reference -----------------------------------------------
FS_B = 16.368e6
N_B = 16384
DELTA = 1234.5
CARRIERS = [0.0, FS_B / 2 - DELTA, FS_B / 2 + DELTA, -FS_B / 2 + DELTA, -FS_B / 2 - DELTA, 1.3 * FS_B, -2.7 * FS_B, 37 * FS_B]
PHASES = [-0.7, -3e5, 1e6, 1e9, 1e10, 1e11, 1e12, 1e13, 1e14, 0.99e15]
PHASE_FRAC = 0.3719
SHIFTS_B = np.array([-3, 0, 3], dtype=np.int32)


def carrier_case(codes, N, M, B, seed, noise, quantize=None, S=None):
    """B blocks of K = len(CARRIERS) channels: block b carries phase PHASES[b] + PHASE_FRAC on every channel, channel k
    carrier CARRIERS[k].  The signal holds every channel (its chips times its carrier, from the reduced step and phase)
    with per-antenna steering and noise.  Returns library records [B, K], re, im [M, B * S]."""
    import gpuacceleratedtracking_amd as g
    rng = np.random.default_rng(seed)
    P, lc = codes.shape
    K = len(CARRIERS)
    S = S or (N + 7) // 8 * 8
    prn = rng.permutation(P)[:K]
    tau = rng.uniform(0, lc, (B, K))
    phi = (np.array(PHASES[:B]) + PHASE_FRAC)[:, None] * np.ones((1, K))
    prm = g.make_params(np.broadcast_to(prn, (B, K)), FC, np.broadcast_to(np.array(CARRIERS), (B, K)), tau, phi)
    n = np.arange(N, dtype=np.float64)
    steer = np.exp(2j * np.pi * rng.uniform(0, 1, M))
    re = np.zeros((M, B * S), dtype=np.float32)
    im = np.zeros_like(re)
    for b in range(B):
        acc = noise * (rng.standard_normal(N) + 1j * rng.standard_normal(N))
        for k in range(K):
            s0 = CARRIERS[k] / FS_B - np.rint(CARRIERS[k] / FS_B)
            phi0 = phi[b, k] - np.floor(phi[b, k])
            idx = np.mod(np.floor(FC / FS_B * n + tau[b, k]).astype(np.int64), lc)
            acc = acc + codes[prn[k]][idx] * np.exp(2j * np.pi * (n * s0 + phi0))
        x = steer[:, None] * acc[None, :]
        if quantize:
            x = np.rint(x * (quantize / max(np.abs(x.real).max(), np.abs(x.imag).max())))
        re[:, b * S:b * S + N] = x.real
        im[:, b * S:b * S + N] = x.imag
    return prm, re, im


def shifted(prm, dphi=0.0, kfs=None):
    out = prm.copy()
    out["carrier_phase_cycles"] += dphi
    if kfs is not None:
        out["carrier_freq_hz"] += np.asarray(kfs)[None, :] * FS_B
    return out


K_SHIFT = np.array([1, -1, 2, -2, 1, 3, -1, 1])  # (37 fs + fs: a step of 38 cycles per sample)


def judge(path, got, ref, prm, what):
    e_n, e_e = channel_errors(got, ref)
    phis = prm["carrier_phase_cycles"]
    # (the worst error per phase, for the record: pytest -s shows it)
    print(f"\nB worst error {path} {what.split(' {')[0]}: " +
          " ".join(f"phi={PHASES[b]:.3g}:{max(e_n[b].max(), e_e[b].max()):.2e}" for b in range(prm.shape[0])))
    bad = [(float(phis[b, k]), float(prm["carrier_freq_hz"][b, k] / FS_B), float(e_n[b, k]), float(e_e[b, k]))
           for b in range(prm.shape[0]) for k in range(prm.shape[1]) if not (e_n[b, k] <= RTOL and e_e[b, k] <= RTOL)]
    assert not bad, f"{path} {what}: {len(bad)} channels miss {RTOL} (phi, f/fs, norm-wise, element-wise): {bad[:8]}"


@pytest.mark.parametrize("path", list(PATHS))
def test_carrier_across_its_domain(g, ctx, path):
    """Carriers 0, +-fs/2 +- delta, 1.3 fs, -2.7 fs, 37 fs at phases -0.7 .. 0.99e15 cycles (plus a fraction), in noise,
    against correlate_reduced at 1e-5; then the same signal with every phase + 2^10 and every carrier + k fs."""
    codes = oracle.codes("GPSL1", 32)
    ctx.set_codes(codes)
    configure(g, ctx, path)
    N, M, B = geometry(path, N_B, 4, len(PHASES))
    if B < len(PHASES):
        B = len(PHASES)  # (every phase; the split path splits these blocks as well)
    layout = PATHS[path].get("layout", 0)
    prm, re, im = carrier_case(codes, N, M, B, seed=5 + layout, noise=0.5,
                               quantize={2: 3000.0, 3: 100.0}.get(layout))
    S = re.shape[1] // B
    base = None
    for what, p in (("base", prm), ("phi + 2^10", shifted(prm, dphi=1024.0)), ("f + k fs", shifted(prm, kfs=K_SHIFT))):
        ref = correlate_reduced(re, im, codes, as_oracle(p), FS_B, SHIFTS_B, N, blk_stride=S)
        got, info = correlate(g, ctx, path, re, im, p, N, FS_B, SHIFTS_B)
        judge(path, got, ref, p, f"{what} {info}")
        if base is None:
            base = got
        else:  # the identities: each record's outputs within the tolerance of the unshifted record's
            check_close(got, base, rtol=2 * RTOL, what=f"{path} {what} vs base")


def test_carrier_across_its_domain_resident_and_host_records(g, ctx):
    """The same carriers as host records: gat_downconvert_and_correlate and the resident correlator, block by block."""
    import torch
    codes = oracle.codes("GPSL1", 32)
    ctx.set_codes(codes)
    N, M, B = N_B, 4, len(PHASES)
    prm, re, im = carrier_case(codes, N, M, B, seed=9, noise=0.5)
    for what, p in (("base", prm), ("phi + 2^10", shifted(prm, dphi=1024.0)), ("f + k fs", shifted(prm, kfs=K_SHIFT))):
        ref = correlate_reduced(re, im, codes, as_oracle(p), FS_B, SHIFTS_B, N)
        got, info = correlate(g, ctx, "default-planar", re, im, p, N, FS_B, SHIFTS_B, host=True)
        judge("host-records", got, ref, p, f"{what} {info}")
        d_re, d_im = torch.from_numpy(re).to(ctx.device), torch.from_numpy(im).to(ctx.device)
        torch.cuda.synchronize()
        desc = g._lib.SignalDesc(d_re.data_ptr(), d_im.data_ptr(), g.GAT_LAYOUT_PLANAR, M, N, B * N, N, 0)
        with ctx.open_resident(desc, len(CARRIERS), SHIFTS_B, FS_B) as res:
            out = np.empty_like(ref)
            for b in range(B):
                o_re, o_im = res.correlate(np.ascontiguousarray(p[b]), block_offset=b * N)
                out[b] = o_re.astype(np.float64) + 1j * o_im.astype(np.float64)
        judge("resident", out, ref, p, what)


# ---- C. one poison predicate ---------------------------------------------------------------------------------------------
def bound_records(lc, P, reach, fs):
    """(name, prn, code rate, carrier, code phase, carrier phase, poisoned) at each bound of the accepted domain and one step
    past it.  Valid records at a bound must match the reference; poisoned ones give NaN (device) / an error (host)."""
    r = FC / fs
    t_in, t_out = span_bound_tau(r, reach, lc)
    big = 1e15
    rec = [
        ("prn -1", -1, FC, 0.0, 1.0, 0.0, True), (f"prn {P}", P, FC, 0.0, 1.0, 0.0, True),
        ("prn P - 1", P - 1, FC, 0.0, 1.0, 0.0, False),
        ("code rate -1e-300", 0, -1e-300, 0.0, 1.0, 0.0, True), ("code rate nan", 0, np.nan, 0.0, 1.0, 0.0, True),
        ("code rate +inf", 0, np.inf, 0.0, 1.0, 0.0, True), ("code rate -inf", 0, -np.inf, 0.0, 1.0, 0.0, True),
        ("code rate 0", 1, 0.0, 0.0, 3.5, 0.0, False),
        ("tau +bound", 2, FC, 0.0, t_in, 0.0, False), ("tau -bound", 3, FC, 0.0, -t_in, 0.0, False),
        ("tau past +bound", 2, FC, 0.0, t_out, 0.0, True), ("tau past -bound", 3, FC, 0.0, -t_out, 0.0, True),
        ("tau nan", 2, FC, 0.0, np.nan, 0.0, True), ("tau inf", 2, FC, 0.0, np.inf, 0.0, True),
        ("f/fs below +1e15", 4, FC, nxt(big, 0) * fs, 1.0, 0.0, False), ("f/fs below -1e15", 4, FC, -nxt(big, 0) * fs, 1.0, 0.0, False),
        ("f/fs +1e15", 4, FC, big * fs, 1.0, 0.0, True), ("f/fs -1e15", 4, FC, -big * fs, 1.0, 0.0, True),
        ("f nan", 4, FC, np.nan, 1.0, 0.0, True), ("f +inf", 4, FC, np.inf, 1.0, 0.0, True), ("f -inf", 4, FC, -np.inf, 1.0, 0.0, True),
        ("phi below +1e15", 5, FC, 0.0, 1.0, nxt(big, 0), False), ("phi below -1e15", 5, FC, 0.0, 1.0, -nxt(big, 0), False),
        ("phi +1e15", 5, FC, 0.0, 1.0, big, True), ("phi -1e15", 5, FC, 0.0, 1.0, -big, True),
        ("phi nan", 5, FC, 0.0, 1.0, np.nan, True), ("phi +inf", 5, FC, 0.0, 1.0, np.inf, True),
        ("phi -inf", 5, FC, 0.0, 1.0, -np.inf, True),
    ]
    # the carrier step is f / fs as the kernels divide it: make the records at +-1e15 land there exactly
    out = []
    for name, prn, fc, f, tau, phi, bad in rec:
        if "f/fs" in name:
            want = f / fs
            while f / fs < want if want > 0 else f / fs > want:
                f = nxt(f, np.inf if want > 0 else -np.inf)
            while abs(f / fs) > abs(want):
                f = nxt(f, 0)
            assert f / fs == want, name
        out.append((name, prn, fc, f, tau, phi, bad))
    return out


FS_C = 4.096e6
N_C = 4096


def poison_launch(g, codes, M, N, path):
    """Records: a good channel after every bound record (random PRN, code phase and carrier); a noise signal, integer
    valued for the integer layouts."""
    P, lc = codes.shape
    reach = N + 3
    recs = bound_records(lc, P, reach, FS_C)
    if path.startswith("mc-"):  # the matrix-core kernels' own rule: a code rate of Lc / 32 chips per sample
        recs.append(("ratio * 32 = Lc", 6, lc / 32.0 * FS_C, 0.0, 1.0, 0.0, True))
    rng = np.random.default_rng(23)
    rows = []
    for rec in recs:
        rows.append(rec)
        rows.append(("good", int(rng.integers(0, P)), FC, float(rng.uniform(-5e3, 5e3)), float(rng.uniform(0, lc)),
                     float(rng.uniform(0, 1)), False))
    prm = g.make_params(np.array([r[1] for r in rows]), np.array([r[2] for r in rows]), np.array([r[3] for r in rows]),
                        np.array([r[4] for r in rows]), np.array([r[5] for r in rows]))[None, :]
    rng2 = np.random.default_rng(29)
    re = rng2.standard_normal((M, (N + 7) // 8 * 8)).astype(np.float32)
    im = rng2.standard_normal(re.shape).astype(np.float32)
    layout = PATHS[path].get("layout", 0)
    if layout in (2, 3):
        q = 600.0 if layout == 2 else 20.0
        re, im = np.rint(re * q).clip(-127, 127) if layout == 3 else np.rint(re * q), np.rint(im * q).clip(-127, 127) \
            if layout == 3 else np.rint(im * q)
        re, im = re.astype(np.float32), im.astype(np.float32)
    return rows, prm, re, im


def clean_for_reference(prm, rows):
    """Poisoned records replaced by a tame one, so that the reference can be built over the whole launch."""
    p = prm.copy()
    for k, r in enumerate(rows):
        if r[6]:
            p[0, k] = (0, 0, FC, 0.0, 0.0, 0.0)
    return p


@pytest.mark.parametrize("path", list(PATHS))
def test_poison_predicate_device_records(g, ctx, path):
    """Device records at every bound and one step past it, each next to a good channel: exactly the poisoned channels' L x M
    outputs are NaN (re and im), every other channel matches the reference."""
    codes = oracle.codes("GPSL1", 32)
    ctx.set_codes(codes)
    configure(g, ctx, path)
    N, M, _ = geometry(path, N_C, 4, 1)
    rows, prm, re, im = poison_launch(g, codes, M, N, path)
    got, info = correlate(g, ctx, path, re, im, prm, N, FS_C, SHIFTS_B)
    ref = correlate_reduced(re, im, codes, as_oracle(clean_for_reference(prm, rows)), FS_C, SHIFTS_B, N,
                            blk_stride=re.shape[1])
    for k, r in enumerate(rows):
        nan = np.isnan(got[0, k].real) & np.isnan(got[0, k].imag)
        if r[6]:
            assert nan.all(), (path, r[0], got[0, k], info)
        else:
            assert not np.isnan(got[0, k]).any(), (path, r[0], info)
            check_close(got[:, k:k + 1], ref[:, k:k + 1], what=f"{path} {r[0]} {info}")


@pytest.mark.parametrize("path", ["default-planar", "default-i8", "tiling-1-1-1", "2x2-quads", "scalar-load", "ragged-tail",
                                  "mc-f32", "mc-bf16-f32"])
def test_poison_predicate_host_records(g, ctx, path):
    """The same records as host records: the call returns an error for exactly the records the device paths poison, and
    leaves the sentinel-filled outputs untouched; the valid ones at a bound match the reference (the matrix-core rule
    ratio * 32 = Lc is no error here: such host records run on the vector kernel)."""
    codes = oracle.codes("GPSL1", 32)
    ctx.set_codes(codes)
    configure(g, ctx, path)
    N, M, _ = geometry(path, N_C, 4, 1)
    rows, prm, re, im = poison_launch(g, codes, M, N, path)
    ref = correlate_reduced(re, im, codes, as_oracle(clean_for_reference(prm, rows)), FS_C, SHIFTS_B, N, blk_stride=re.shape[1])
    for k in range(0, len(rows), 2):
        r = rows[k]
        pair = np.ascontiguousarray(prm[:, k:k + 2])
        mc_rule = r[0] == "ratio * 32 = Lc"
        if r[6] and not mc_rule:
            with pytest.raises(g._lib.GatError) as e:
                correlate(g, ctx, path, re, im, pair, N, FS_C, SHIFTS_B, host=True, check_want=False)
            assert e.value.status in (1, 2), (path, r[0], e.value)
        else:
            got, info = correlate(g, ctx, path, re, im, pair, N, FS_C, SHIFTS_B, host=True, check_want=False)
            if mc_rule:
                assert info["matrix_core"] == 0, (path, info)
                continue
            check_close(got, ref[:, k:k + 2], what=f"{path} host {r[0]} {info}")


def test_poison_predicate_host_outputs_untouched_and_resident(g, ctx):
    """A refused host call writes nothing: outputs pre-filled with a sentinel keep it.  The resident correlator refuses the
    same records (and keeps its previous outputs), and serves the valid ones at a bound."""
    import torch
    codes = oracle.codes("GPSL1", 32)
    ctx.set_codes(codes)
    N, M = N_C, 4
    rows, prm, re, im = poison_launch(g, codes, M, N, "default-planar")
    ref = correlate_reduced(re, im, codes, as_oracle(clean_for_reference(prm, rows)), FS_C, SHIFTS_B, N)
    d_re, d_im = torch.from_numpy(re).to(ctx.device), torch.from_numpy(im).to(ctx.device)
    desc = g._lib.SignalDesc(d_re.data_ptr(), d_im.data_ptr(), g.GAT_LAYOUT_PLANAR, M, N, N, N, 0)
    o_re = torch.full((1, 2, 3, M), SENTINEL, device=ctx.device)
    o_im = torch.full((1, 2, 3, M), SENTINEL, device=ctx.device)
    torch.cuda.synchronize()
    with ctx.open_resident(desc, 2, SHIFTS_B, FS_C) as res:
        for k in range(0, len(rows), 2):
            r = rows[k]
            pair = np.ascontiguousarray(prm[0, k:k + 2])
            if r[6]:
                with pytest.raises(g._lib.GatError) as e:
                    ctx.downconvert_and_correlate(desc, pair, 1, 2, SHIFTS_B, FS_C, o_re, o_im)
                assert e.value.status in (1, 2), (r[0], e.value)
                ctx.sync()
                assert (o_re == SENTINEL).all() and (o_im == SENTINEL).all(), r[0]
                res._re[...] = SENTINEL
                res._im[...] = SENTINEL
                with pytest.raises(g._lib.GatError) as e2:
                    res.correlate(pair)
                assert e2.value.status == e.value.status, (r[0], e.value, e2.value)
                assert (res._re == SENTINEL).all() and (res._im == SENTINEL).all(), r[0]
            else:
                a_re, a_im = res.correlate(pair)
                got = (a_re.astype(np.float64) + 1j * a_im.astype(np.float64))[None]
                check_close(got, ref[:, k:k + 2], what=f"resident {r[0]}")


def test_poison_predicate_replica_generators(g, ctx):
    """gat_gen_code_replica refuses the code-side bound records (prn, code rate, code phase past the span bound) and leaves
    its output untouched; gat_gen_code_replica_multi, on device records, writes NaN rows for exactly those channels."""
    import torch
    codes = oracle.codes("GPSL1", 32)
    ctx.set_codes(codes)
    P, lc = codes.shape
    count, first = 4093, -3
    recs = [r for r in bound_records(lc, P, count + abs(first), FS_C) if r[0].split()[0] in ("prn", "code", "tau")]
    one = torch.full((count,), SENTINEL, device=ctx.device)
    prm = g.make_params(np.array([r[1] for r in recs]), np.array([r[2] for r in recs]), 0.0, np.array([r[4] for r in recs]), 0.0)
    rep = torch.full((len(recs), count), SENTINEL, device=ctx.device)
    ctx.gen_code_replica_multi(rep, count, ctx.params_to_device(prm), len(recs), FS_C, first)
    multi = rep.cpu().numpy()
    for k, (name, prn, fc, _, tau, _, bad) in enumerate(recs):
        if bad:
            with pytest.raises(g._lib.GatError):
                ctx.gen_code_replica(one, count, prn, fc, FS_C, tau, first)
            assert (one.cpu().numpy() == SENTINEL).all(), name
            assert np.isnan(multi[k]).all(), name
        else:
            want = oracle.gen_code_replica(codes, prn, fc, FS_C, tau, first, count)
            ctx.gen_code_replica(one, count, prn, fc, FS_C, tau, first)
            assert np.array_equal(one.cpu().numpy(), want), name
            assert np.array_equal(multi[k], want), name
            one.fill_(SENTINEL)
