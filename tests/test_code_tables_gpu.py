"""Every kernel on a caller's code table (GNSSSystem(codes=..., code_frequency=...) -> gat_set_codes: any int8 chips, 1 to
120 000 per row, any number of PRNs) against the FP64 oracle: tables of one chip (a pure carrier) to the 120 000-chip limit,
lengths around the 16-byte rows and the sign-bit dwords, on both sides of the sign-bit threshold of the vector kernel
(code_row_stride > 2048 bytes: 2048 chips and more), +-1 chips, +-1 with zeros, {-1, 0, +1} and the whole int8 range; one
PRN and 64 (the last row included), code phases that put the block across the table's end.  The default planner in every
layout, the vector kernel under each forced tiling and chip-table form, integer chip sums that must be exact, the
matrix-core kernels, the resident correlator, the stand-alone replica and signal generators, the acquisition grid, the
long int8 tables the 2 x 2 tile once refused, the size limit, and rebinding through a replayed tracking-loop graph.
Run with -m gpu."""
import ctypes as C
import zlib

import numpy as np
import pytest

import oracle
from tests.helpers import (acq_power_oracle, check_close, check_power_close, code_table, make_case, oracle_result,
                           standard_codes_after)  # noqa: F401  (standard_codes_after: a fixture)

pytestmark = pytest.mark.gpu

# length, PRNs, chip kind
TABLES = [
    (1, 1, "pm1"), (1, 64, "int8"),                   # a pure carrier (one chip per row)
    (7, 64, "ternary"),                               # a step covers ~150 laps of the table
    (16, 1, "pm1"), (17, 64, "pm1_zeros"), (31, 1, "int8"), (32, 64, "pm1"), (33, 1, "ternary"),  # row / dword padding
    (511, 64, "pm1"), (2046, 1, "pm1_zeros"), (4092, 64, "int8"), (5115, 1, "pm1"),               # other GNSS lengths
    (2032, 64, "pm1"), (2033, 1, "pm1"), (2047, 1, "pm1"), (2048, 64, "pm1"),  # around the sign-bit threshold (2048 chips)
    (20000, 1, "int8"), (30000, 64, "pm1_zeros"), (65536, 1, "pm1"), (120000, 4, "pm1"), (120000, 1, "int8"),
]
TABLE_IDS = [f"Lc{t[0]}-P{t[1]}-{t[2]}" for t in TABLES]
FC = 1.023e6


@pytest.fixture(scope="module")
def g():
    import gpuacceleratedtracking_amd as g
    g.load_library()
    return g


@pytest.fixture()
def ctx(g, standard_codes_after):
    """The default context with the library's default kernel selection, tiling and options restored after the test."""
    c = g.get_context()
    yield c
    c.set_matrix_core(g.GAT_MC_AUTO)
    c.set_vector_tiling(4, 4, 16)
    for name, val in (("dc_bits", 1), ("dc_quads", -1), ("dc_aw2", -1), ("dc_one_wave_min", -1), ("dc_depth", 2)):
        c.set_option(name, val)


def table(t):
    lc, P, kind = t
    return code_table(lc, P, zlib.crc32(repr(t).encode()), kind)


def is_pm1(codes):
    return bool(np.all(np.abs(codes.astype(np.int32)) == 1))


def row_bytes(lc, bits):
    """LDS bytes of one staged chip row: int8 rows (16-byte rows with the wrap chip) or sign-bit rows (gat_set_codes)."""
    return ((lc + 1 + 32 + 31) // 32 + 3 & ~3) * 4 if bits else (lc + 16) & ~15


def edge_taus(lc, B, K, rng, adv):
    """[B, K] code phases: the table's end (Lc - 1e-9), a block that crosses it half way (Lc - adv / 2), zero, random."""
    fixed = [lc - 1e-9, (lc - 0.5 * adv) % lc, 0.0, lc - 0.5]
    t = rng.uniform(0, lc, B * K)
    t[:min(len(fixed), t.size)] = fixed[:t.size]
    return t.reshape(B, K)


def table_case(t, seed, N, M, L, K, B, fs=None, quantize=None):
    codes = table(t)
    lc, P = t[0], t[1]
    rng = np.random.default_rng(seed)
    fs = N / 1e-3 if fs is None else fs
    prns = np.concatenate([[P - 1], rng.integers(0, P, K - 1)]) if K > 1 else np.array([P - 1])
    case = make_case(seed, N=N, M=M, L=L, K=K, B=B, fs=fs, codes=codes, fc=FC, prns=prns,
                     tau=edge_taus(lc, B, K, rng, FC * N / fs))
    if quantize:  # integer samples for the int16 / int8 layouts: the oracle sees the same values
        peak = max(np.abs(case["re"]).max(), np.abs(case["im"]).max(), 1e-30)
        case["re"] = np.rint(case["re"] * (quantize / peak)).astype(np.float32)
        case["im"] = np.rint(case["im"] * (quantize / peak)).astype(np.float32)
    return case


def run(g, ctx, case, layout=0):
    """One call on the case's table through StreamCorrelator; returns (complex [B, K, L, M], launch info)."""
    import torch
    sysobj = g.GPSL1(codes=case["codes"], code_frequency=case["fc"])
    N, M, B, K = case["N"], case["M"], case["B"], case["K"]
    op = g.StreamCorrelator(sysobj, N, M, B, K, case["shifts"], case["fs"], ctx=ctx)
    p = case["prm"]
    op.set_params(g.make_params(p["prn0"], p["code_freq_hz"], p["carrier_freq_hz"], p["code_phase_chips"],
                                p["carrier_phase_cycles"]))
    re, im = torch.from_numpy(case["re"]).to(ctx.device), torch.from_numpy(case["im"]).to(ctx.device)
    if layout == 0:
        op(re, im)
    elif layout == 1:
        op(torch.stack([re, im], dim=-1).contiguous(), None)
    else:
        op(torch.stack([re, im], dim=-1).to(torch.int16 if layout == 2 else torch.int8).contiguous(), None)
    return op.result(), ctx.last_launch_info()


# ---- the default planner, every layout -----------------------------------------------------------------------------------
@pytest.mark.parametrize("t", TABLES, ids=TABLE_IDS)
def test_default_planner_every_layout(g, ctx, t):
    for layout, q in ((0, None), (1, None), (2, 3000.0), (3, 100.0)):
        case = table_case(t, 11 + layout, N=6000, M=4, L=3, K=3, B=2, quantize=q)
        got, info = run(g, ctx, case, layout)
        check_close(got, oracle_result(case), what=f"{t} layout {layout} {info}")


# ---- the vector kernel with its settings forced --------------------------------------------------------------------------
TILINGS = [(1, 1, 1), (4, 1, 1), (1, 4, 1), (4, 4, 16), (2, 2, 4), (4, 2, 1)]
FORCED = ([("tiling", tl) for tl in TILINGS] +
          [("opts", dict(dc_bits=b, dc_quads=q)) for b in (0, 1, 2) for q in (0, -1)] +
          [("opts", dict(dc_aw2=0)), ("opts", dict(dc_aw2=1)), ("opts", dict(dc_aw2=1, dc_quads=0)),
           ("opts", dict(dc_depth=1)), ("opts", dict(dc_depth=2))])


def force(ctx, kind, val):
    ctx.set_vector_tiling(4, 4, 16)
    for name, v in (("dc_bits", 1), ("dc_quads", -1), ("dc_aw2", -1), ("dc_one_wave_min", -1), ("dc_depth", 2)):
        ctx.set_option(name, v)
    if kind == "tiling":
        ctx.set_vector_tiling(*val)
    else:
        for name, v in val.items():
            ctx.set_option(name, v)


@pytest.mark.parametrize("shifts", [(-3, 0, 3), (-2, 0, 2)], ids=["odd-taps", "even-taps"])
@pytest.mark.parametrize("t", TABLES, ids=TABLE_IDS)
def test_vector_kernel_every_forced_setting(g, ctx, t, shifts):
    """Taps at odd distances (the replica's shifted copy) and at even ones (where the 2 x 2 tile fills the replica by quads,
    reading "this chip and the next" -- the wrap chip at index Lc)."""
    ctx.set_matrix_core(g.GAT_MC_VECTOR)
    case = table_case(t, 21, N=6000, M=4, L=3, K=3, B=2)
    case["shifts"] = np.array(shifts, dtype=np.int32)
    ref = oracle_result(case)
    pm1, lc = is_pm1(case["codes"]), t[0]
    lds = {}
    for kind, val in FORCED:
        force(ctx, kind, val)
        got, info = run(g, ctx, case)
        assert info["matrix_core"] == 0, info
        check_close(got, ref, what=f"{t} {kind} {val} {info}")
        if kind == "tiling":
            assert info["channels_per_wg"] <= val[1] and info["blocks_per_wg"] <= val[2], info
        elif "dc_aw2" in val and val["dc_aw2"] == 1:
            # the 2 x 2 tile wherever its two channels' tables fit: everywhere but long int8 rows
            long_int8 = not pm1 and lc >= 16000
            assert info["channels_per_wg"] == (1 if long_int8 else 2) and info["ant_tile"] == 4, (t, info)
        elif "dc_bits" in val:
            lds[val["dc_bits"], val["dc_quads"]] = info["lds_bytes"]
    # which chip-table form ran: sign-bit rows only for +-1 tables -- under dc_bits = 1 only from 2048 chips on (rows of more
    # than 2048 bytes) -- else int8 rows; the two forms differ in LDS size wherever their row sizes differ
    for q in (0, -1):
        for b in (1, 2):
            bits = pm1 and (b == 2 or lc >= 2048)
            if row_bytes(lc, True) != row_bytes(lc, False):
                assert (lds[b, q] != lds[0, q]) == bits, (t, b, q, lds)


def test_one_wave_workgroups_on_short_tables(g, ctx):
    """Short blocks of one- and two-antenna tiles, forced onto one-wave workgroups (dc_one_wave_min = 1), which read int8 rows:
    tables of every kind up to the 2048-byte rows they take."""
    ctx.set_matrix_core(g.GAT_MC_VECTOR)
    ctx.set_option("dc_one_wave_min", 1)
    for t in [x for x in TABLES if x[0] <= 2032]:
        case = table_case(t, 31, N=1000, M=2, L=3, K=2, B=8)
        got, info = run(g, ctx, case)
        assert info["threads"] == 64, (t, info)
        check_close(got, oracle_result(case), what=f"{t} {info}")


# ---- exact chip edges --------------------------------------------------------------------------------------------------
def chip_count(codes, prm, fs, shifts, N, B, K):
    """Integer sums of the chips each (block, channel, tap) window reads -- the all-ones signal at zero carrier: numpy's
    count, int64 [B, K, L]."""
    out = np.zeros((B, K, len(shifts)), dtype=np.int64)
    n = np.arange(N, dtype=np.float64)
    lc = codes.shape[1]
    for b in range(B):
        for k in range(K):
            p = prm[b, k]
            row = codes[p["prn0"]].astype(np.int64)
            for i, s in enumerate(shifts):
                idx = np.floor(p["code_freq_hz"] / fs * (n + s) + p["code_phase_chips"]).astype(np.int64) % lc
                out[b, k, i] = row[idx].sum()
    return out


EXACT_TABLES = [(1, 1, "int8"), (7, 64, "int8"), (17, 64, "int8"), (33, 1, "ternary"), (2032, 64, "pm1"),
                (2048, 64, "pm1"), (5115, 1, "int8"), (30000, 4, "pm1_zeros"), (120000, 4, "pm1"), (120000, 1, "int8")]


@pytest.mark.parametrize("t", EXACT_TABLES, ids=[f"Lc{t[0]}-P{t[1]}-{t[2]}" for t in EXACT_TABLES])
def test_chip_edges_exact(g, ctx, t):
    """All-ones signal, zero Doppler and carrier phase, code rate fs / 16: every accumulator is an integer sum of chips (below
    2^24: exact in float) and must equal numpy's count of the window's chips exactly -- phases at the table's end and on
    chip edges, every tiling and table form.  An off-by-one chip or a wrong wrap chip changes a sum by a whole chip."""
    import torch
    ctx.set_matrix_core(g.GAT_MC_VECTOR)
    codes = table(t)
    lc, P = t[0], t[1]
    N = 1 << 17 if t == (120000, 1, "int8") else 1 << 15
    M, K, B = 4, 2, 2
    fs = 16 * FC
    shifts = np.array([-8, 0, 8], dtype=np.int32)
    # (on a chip edge, and the table's end 1e-9 before one: the replica fill evaluates those samples exactly; 0.3 and 0.02
    # off the edges: the quads of the 2 x 2 tile read "this chip and the next", the wrap chip at index Lc)
    taus = np.array([[lc - 1e-9, (lc - 0.3) % lc], [(lc - 17 / 16) % lc, (3 / 16 + 0.02) % lc]])
    prm = oracle.make_params(np.array([[P - 1, 0], [0, P - 1]]), FC, 0.0, taus, 0.0)
    want = chip_count(codes, prm, fs, shifts, N, B, K)
    assert np.abs(want).max() < 2 ** 24
    re = np.ones((M, B * N), dtype=np.float32)
    im = np.zeros_like(re)
    ref = oracle.correlate_f64(re, im, codes, prm, fs, shifts, N=N)
    assert np.array_equal(ref.real, np.broadcast_to(want[..., None], ref.shape).astype(np.float64))
    sysobj = g.GPSL1(codes=codes, code_frequency=FC)
    op = g.StreamCorrelator(sysobj, N, M, B, K, shifts, fs, ctx=ctx)
    op.set_params(g.make_params(prm["prn0"], prm["code_freq_hz"], prm["carrier_freq_hz"], prm["code_phase_chips"],
                                prm["carrier_phase_cycles"]))
    d_re, d_im = torch.from_numpy(re).to(ctx.device), torch.from_numpy(im).to(ctx.device)
    settings = [("tiling", tl) for tl in TILINGS] + [("opts", dict(dc_bits=b, dc_quads=q)) for b in (0, 2) for q in (0, -1)] + \
               [("opts", dict(dc_aw2=1)), ("opts", dict(dc_aw2=1, dc_quads=0)), ("opts", dict(dc_aw2=1, dc_bits=2)),
                ("opts", dict(dc_aw2=1, dc_bits=0))]
    for kind, val in settings:
        force(ctx, kind, val)
        op(d_re, d_im)
        got = op.result()
        assert np.array_equal(got.real.astype(np.float64), np.broadcast_to(want[..., None], got.shape)) and np.all(got.imag == 0), \
            (t, kind, val, ctx.last_launch_info())


# ---- the matrix-core kernels ---------------------------------------------------------------------------------------------
MFMA_TABLES = [(1, 1, "int8"), (7, 64, "pm1"), (17, 64, "pm1"), (63, 1, "ternary"), (64, 1, "pm1"), (2048, 64, "pm1"), (5115, 1, "pm1_zeros"), (30000, 64, "pm1_zeros"),
               (120000, 4, "pm1"), (120000, 1, "int8")]


@pytest.mark.parametrize("t", MFMA_TABLES, ids=[f"Lc{t[0]}-P{t[1]}-{t[2]}" for t in MFMA_TABLES])
def test_matrix_core_kernels(g, ctx, t):
    """M = 16: GAT_MC_AUTO, GAT_MC_F32 (multiplies by the chip value: any table) and GAT_MC_BF16_SPLIT (sign-bit tables: +-1
    only -- on any other table the call must fall back) against the oracle.  Tables of fewer than 64 chips take the vector
    kernel in every mode: both matrix-core kernels poison a channel that wraps the table more than once per 32 samples
    (ratio * 32 >= Lc), and GAT_MC_F32 once returned NaN for the one-chip table here."""
    case = table_case(t, 41, N=8000, M=16, L=3, K=5, B=1, fs=5e6)
    ref = oracle_result(case)
    pm1 = is_pm1(case["codes"])
    for mode in (g.GAT_MC_AUTO, g.GAT_MC_F32, g.GAT_MC_BF16_SPLIT):
        ctx.set_matrix_core(mode)
        got, info = run(g, ctx, case)
        if not pm1:
            assert info["matrix_core"] != 2, (t, mode, info)
        if t[0] < 64:
            assert info["matrix_core"] == 0, (t, mode, info)
        elif mode == g.GAT_MC_F32:
            assert info["matrix_core"] == 1, (t, info)
        elif mode == g.GAT_MC_BF16_SPLIT and pm1 and t[0] <= 2048:  # (longer sign-bit tables may not fit its LDS tile)
            assert info["matrix_core"] == 2, (t, info)
        check_close(got, ref, what=f"{t} mode {mode} {info}")


# ---- the resident correlator ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", [(7, 64, "ternary"), (30000, 64, "pm1_zeros"), (120000, 1, "int8")], ids=["short", "long-int8-rows", "limit"])
def test_resident_correlator(g, ctx, t):
    """Single-block calls through the resident kernel.  These shapes are within its documented rule (<= 16 channels, <= 8 taps
    one launch wide, aligned whole load groups: test_resident_gpu.py::test_resident_rejects_what_it_cannot_serve), so it
    must open on every table and match the oracle on each of the blocks."""
    import torch
    N, M, K, B = 4096, 4, 2, 3
    case = table_case(t, 51, N=N, M=M, L=3, K=K, B=B)
    ref = oracle_result(case)
    ctx.set_codes(case["codes"])
    re = torch.from_numpy(case["re"]).to(ctx.device)
    im = torch.from_numpy(case["im"]).to(ctx.device)
    desc = g._lib.SignalDesc(re.data_ptr(), im.data_ptr(), g.GAT_LAYOUT_PLANAR, M, N, B * N, N, 0)
    torch.cuda.synchronize()
    with ctx.open_resident(desc, K, case["shifts"], case["fs"]) as res:
        for b in range(B):
            p = case["prm"][b]
            prm = g.make_params(p["prn0"], p["code_freq_hz"], p["carrier_freq_hz"], p["code_phase_chips"], p["carrier_phase_cycles"])
            o_re, o_im = res.correlate(prm, block_offset=b * N)
            got = (np.asarray(o_re, dtype=np.float64) + 1j * np.asarray(o_im, dtype=np.float64)).reshape(1, K, 3, M)
            check_close(got, ref[b:b + 1], what=f"{t} block {b}")


# ---- the stand-alone generators ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", [(1, 1, "pm1"), (7, 64, "int8"), (33, 1, "ternary"), (2047, 64, "pm1_zeros"), (30000, 64, "int8"),
                               (120000, 1, "int8")], ids=lambda t: f"Lc{t[0]}-P{t[1]}-{t[2]}")
def test_gen_code_replica_and_gen_signal(g, ctx, t):
    """gat_gen_code_replica bit for bit against oracle.gen_code_replica (the last row, phases at the table's end, taps in
    front of the block); gat_gen_signal against oracle.gen_signal (float32 chips times the same carrier)."""
    import torch
    codes = table(t)
    lc, P = t[0], t[1]
    ctx.set_codes(codes)
    rng = np.random.default_rng(61)
    count = 20011
    for fs, tau, first in ((2.5e6, lc - 1e-9, -3), (20e6, (lc - 0.5) % lc, -40), (16 * FC, rng.uniform(0, lc), 0)):
        rep = torch.full((count + 8,), 7.0, device=ctx.device)
        ctx.gen_code_replica(rep, count, P - 1, FC, fs, tau, first)
        got = rep.cpu().numpy()
        want = oracle.gen_code_replica(codes, P - 1, FC, fs, tau, first, count)
        assert np.array_equal(got[:count], want), (t, fs, tau)
        assert (got[count:] == 7.0).all()
    N, fs, f, tau, phi = 20000, 5e6, 1234.5, lc - 1e-9, 0.3  # (gat_gen_signal reads the carrier phase in radians)
    prm = g.make_params(P - 1, FC, f, tau, phi, shape=(1, 1))
    re = torch.zeros((1, N), device=ctx.device)
    im = torch.zeros((1, N), device=ctx.device)
    ctx.gen_signal(re, im, g.GAT_LAYOUT_PLANAR, N, 1, N, N, 1, 1, ctx.params_to_device(prm), fs, amplitude=1.0)
    ore, oim = oracle.gen_signal(codes, P - 1, FC, fs, f, tau, phi, N, 1)
    tol = 1e-6 * max(1, int(np.abs(codes.astype(np.int32)).max()))
    assert np.abs(re.cpu().numpy() - ore).max() <= tol and np.abs(im.cpu().numpy() - oim).max() <= tol, t


# ---- the acquisition grid ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", [(17, 64, "pm1"), (511, 64, "ternary"), (5115, 1, "pm1_zeros"), (30000, 4, "int8")],
                         ids=lambda t: f"Lc{t[0]}-P{t[1]}-{t[2]}")
def test_acquisition_grid(g, ctx, t):
    """The search's power grid on a caller's table (a satellite of its last row in noise, two blocks) against the oracle's
    correlator, sampled on the grid's edges, tile seams and the peak."""
    import torch
    codes = table(t)
    lc, P = t[0], t[1]
    fs, N, B, M = 4e6, 6000, 2, 2
    D, J, s, first, f_first, f_step = 9, 300, 3, -5, -2000.0, 500.0
    rng = np.random.default_rng(71)
    r1, i1 = oracle.gen_signal(codes, P - 1, FC, fs, 500.0, rng.uniform(0, lc), 0.7, B * N, 1)
    x = (r1[0] + 1j * i1[0])[None, :] * np.exp(2j * np.pi * rng.uniform(0, 1, (M, 1)))
    x = x + 0.5 * float(np.abs(codes).max()) * (rng.standard_normal(x.shape) + 1j * rng.standard_normal(x.shape))
    re, im = x.real.astype(np.float32), x.imag.astype(np.float32)
    ctx.set_codes(codes)
    cfg = g._lib.AcqConfig()
    cfg.struct_size = C.sizeof(g._lib.AcqConfig)
    cfg.num_doppler_bins, cfg.num_code_bins, cfg.code_step_samples = D, J, s
    cfg.if_hz, cfg.code_freq_hz, cfg.doppler_first_hz, cfg.doppler_step_hz = 0.0, FC, f_first, f_step
    cfg.first_shift, cfg.min_peak_ratio, cfg.code_length = first, 2.0, lc
    from gpuacceleratedtracking_amd.acquisition import _as_desc
    d_re, d_im = torch.from_numpy(re).cuda(), torch.from_numpy(im).cuda()
    desc = _as_desc((d_re, d_im), N, B, N)
    prns = np.array([P - 1, 0], dtype=np.int32)
    power = torch.full((2, D, J), float("nan"), dtype=torch.float32, device="cuda")
    res = np.zeros(2, dtype=g._lib.ACQ_RESULT_DTYPE)
    rc = ctx.lib.gat_acquire(ctx._h, C.byref(desc), B, prns.ctypes.data_as(C.POINTER(C.c_int32)), 2, fs, C.byref(cfg),
                             C.c_void_p(power.data_ptr()), C.c_void_p(res.ctypes.data))
    assert rc == 0, ctx.lib.gat_last_error(ctx._h)
    power = power.cpu().numpy()
    for i, p in enumerate(prns):
        rows = np.array([0, 4, D - 1])
        cols = np.unique([0, 1, 255, 256, J - 1, int(res["code_bin"][i]), *rng.integers(0, J, 8)])
        ref = acq_power_oracle(re, im, codes, int(p), FC, lc, fs, 0.0, f_first, f_step, rows, first, s, cols, N, B, N)
        check_power_close(power[i][np.ix_(rows, cols)], ref, what=f"{t} prn {p}")


# ---- long int8 tables with several channels: the planner's 2 x 2 tile no longer refuses them ---------------------------
@pytest.mark.parametrize("variant", ["one-zero-chip", "pm1-dc_bits0"])
def test_long_int8_table_with_several_channels_launches(g, ctx, variant):
    """Lc = 30 000, 4 PRNs, planar float, M = 4, K = 3, B = 256, N = 20 000, taps {-1, 0, 1}, fs = 20 MHz: the default planner
    chose the two-channel 2 x 2 tile and then could not fit two 30 KB int8 tables in its LDS budget -- GAT_ERR_UNSUPPORTED
    ("no kernel instance for this shape").  It must launch and match the oracle: with a table whose chips are not all +-1,
    and with a +-1 table staged as int8 rows (dc_bits = 0)."""
    codes = code_table(30000, 4, 81, "pm1")
    if variant == "one-zero-chip":
        codes[2, 12345] = 0
    else:
        ctx.set_option("dc_bits", 0)
    N, M, K, B, fs = 20000, 4, 3, 256, 20e6
    case = make_case(82, N=N, M=M, L=3, K=K, B=B, fs=fs, codes=codes, fc=FC)
    case["shifts"] = np.array([-1, 0, 1], dtype=np.int32)
    got, info = run(g, ctx, case)
    assert info["matrix_core"] == 0, info
    check_close(got, oracle_result(case), what=f"{variant} {info}")


# ---- the table-size limit ------------------------------------------------------------------------------------------------
def test_table_size_limit(g, ctx):
    """120 000 chips per row bind and correlate (test_default_planner_every_layout); 120 001 return GAT_ERR_RANGE and leave the
    bound table in place."""
    t = (120000, 4, "pm1")
    case = table_case(t, 91, N=4000, M=1, L=3, K=2, B=1)
    got, _ = run(g, ctx, case)
    check_close(got, oracle_result(case), what="120000 chips")
    big = np.ones((2, 120001), dtype=np.int8)
    rc = ctx.lib.gat_set_codes(ctx._h, big.ctypes.data_as(C.POINTER(C.c_int8)), 120001, 2)
    assert rc == 2, rc  # GAT_ERR_RANGE
    ctx.invalidate_codes()  # (the Python layer's record of the bound table; the library kept its own)
    got, _ = run(g, ctx, case)
    check_close(got, oracle_result(case), what="120000 chips after a refused table")


# ---- rebinding: long, short, long on one context, through a replayed tracking-loop graph -------------------------------
def test_rebinding_long_short_long_through_a_replayed_loop_graph(g):
    """One context binds a long int8 table, then a short one, then the long one again.  After each rebind a correlate call
    and a tracking loop's graph -- recorded, then replayed -- must match the oracle (block 0 of each run, from the
    parameters the run starts with)."""
    import torch
    ctx = g.Context(0, "own")  # (a stream of its own: graphs are recorded on it)
    try:
        long_t, short_t = (30000, 4, "int8"), (7, 4, "ternary")
        N, M, fs, nblk = 4000, 2, 4e6, 4  # even: every run starts from parameter buffer A
        shifts = np.array([-2, 0, 2], dtype=np.int32)
        for step, t in enumerate((long_t, short_t, long_t)):
            case = table_case(t, 100 + step, N=N, M=M, L=3, K=2, B=nblk, fs=fs)
            case["shifts"] = shifts
            got, _ = run(g, ctx, case)
            check_close(got, oracle_result(case), what=f"rebind {step}: correlate")
            system = g.GPSL1(codes=case["codes"], code_frequency=FC)
            p0 = case["prm"][0]
            loop = g.TrackingLoop(system, p0["prn0"] + 1, N, M, fs, shifts, init_carrier_doppler=p0["carrier_freq_hz"],
                                  init_code_phase=p0["code_phase_chips"], ctx=ctx)
            re = torch.from_numpy(case["re"]).to(ctx.device)
            im = torch.from_numpy(case["im"]).to(ctx.device)
            out = (torch.empty((nblk, 2, 3, M), device=ctx.device), torch.empty((nblk, 2, 3, M), device=ctx.device))
            for rep in ("record", "replay", "replay again"):
                start = loop.params()  # synchronises: the parameters block 0 of this run is correlated with
                loop.run(re, im, nblk, graph=True, out=out)
                ctx.sync()
                ref = oracle.correlate_f64(case["re"], case["im"], case["codes"], _as_oracle(start).reshape(1, 2), fs, shifts, N=N)
                got = (out[0][:1].cpu().numpy().astype(np.float64) + 1j * out[1][:1].cpu().numpy())
                check_close(got, ref, what=f"rebind {step}: loop {rep}")
    finally:
        ctx.close()
        g.get_context().set_codes(g.GPSL1().codes)


def _as_oracle(p):
    """Library channel records (gpuacceleratedtracking_amd.make_params) -> the oracle's parameter records."""
    return oracle.make_params(p["prn"], p["code_freq_hz"], p["carrier_freq_hz"], p["code_phase_chips"], p["carrier_phase_cycles"])
