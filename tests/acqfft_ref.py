"""What the tests of the FFT acquisition search (gat_acquire_fft, gat_acquire_fft_host; csrc/gat_acq_fft.h) share: the shapes that
reach every instance, the scenes (satellites in noise, so that every Doppler row has a floor, in the four sample layouts), the
configuration record, the host twin's call and the bins to sample: the grid's ends, the first and last lag of every lag segment
(the seams), the peak and a few random ones.  The FP64 reference is tests/helpers.acq_power_oracle: the contract itself.
DOMAIN, domain_scene and what follows them are the cases of the domain tests (tests/test_acquisition_fft_domain_host.py,
tests/test_acquisition_fft_domain_gpu.py): every transform length, the ends of the lag-segment geometry, the work split, caller
code tables, the ends of the code-phase span, the descriptor and the carrier; BOUNDARIES are the calls on both sides of each refusal."""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional

import numpy as np

import oracle

FC, LC = 1.023e6, 1023
PLANAR, CF32, I16, I8 = 0, 1, 2, 3
PRNS = [3, 17, 30]
F_FIRST, F_STEP = -5000.0, 250.0

# name: layout, M, B, N, block_stride, fs, s, first_shift, J, D, if_hz, acq_fft_log2 (0: the plan's choice)
SHAPES = {
    "one-pass": (PLANAR, 1, 1, 2000, 2000, 2.0e6, 1, 0, 2000, 9, 0.0, 12),            # F = 4096, one segment
    "two-pass-two-segments": (CF32, 1, 1, 5000, 5000, 5.0e6, 1, 0, 5115, 5, 1.0e4, 13),  # F = 8192: Jseg = 3193, G = 2
    "odd-blocks": (PLANAR, 2, 3, 4001, 4100, 4.0e6, 3, -37, 700, 7, -2.5e3, 0),       # the plan takes F = 8192; s = 3
    "int16": (I16, 2, 2, 2000, 2011, 2.0e6, 2, 5, 900, 5, 0.0, 12),                   # F = 4096
    "int8": (I8, 1, 2, 3000, 3000, 3.0e6, 1, -3, 3069, 5, 500.0, 12),                 # F = 4096: Jseg = 1097, G = 3
}
SCALE = {PLANAR: 1.0, CF32: 1.0, I16: 1000.0, I8: 20.0}


def config(g, D, J, s, first_shift=0, f_first=F_FIRST, f_step=F_STEP, if_hz=0.0, lc=LC, fc=FC):
    cfg = g._lib.AcqConfig()
    cfg.struct_size = C.sizeof(g._lib.AcqConfig)
    cfg.num_doppler_bins, cfg.num_code_bins, cfg.code_step_samples = D, J, s
    cfg.if_hz, cfg.code_freq_hz, cfg.doppler_first_hz, cfg.doppler_step_hz = if_hz, fc, f_first, f_step
    cfg.first_shift, cfg.min_peak_ratio, cfg.code_length = first_shift, 2.0, lc
    return cfg


def scene(seed, layout, M, ld, fs, if_hz, prns=PRNS, noise=0.5):
    """The searched satellites (one on a Doppler bin, two between) in noise, as tests/test_acquisition_gpu.py builds them.  Returns
    (host arrays in `layout` [M, ld(, 2)], re, im float32 [M, ld]: the same values planar for the oracle)."""
    rng = np.random.default_rng(seed)
    codes = oracle.codes("GPSL1", 32)
    x = np.zeros(ld, dtype=np.complex128)
    for k, p in enumerate(prns):
        r1, i1 = oracle.gen_signal(codes, p, FC, fs, if_hz + 250.0 * (k - 1) + 100.0 * k, rng.uniform(0, LC), 0.3 * k, ld, 1)
        x += r1[0] + 1j * i1[0]
    x = x[None, :] * np.exp(2j * np.pi * rng.uniform(0, 1, (M, 1))) + noise * (rng.standard_normal((M, ld)) + 1j * rng.standard_normal((M, ld)))
    x = x * SCALE[layout]
    if layout in (I16, I8):
        dt = np.int16 if layout == I16 else np.int8
        lim = np.iinfo(dt).max
        pair = np.ascontiguousarray(np.clip(np.stack([np.rint(x.real), np.rint(x.imag)], axis=-1), -lim, lim).astype(dt))
        return (pair,), pair[..., 0].astype(np.float32), pair[..., 1].astype(np.float32)
    re, im = np.ascontiguousarray(x.real.astype(np.float32)), np.ascontiguousarray(x.imag.astype(np.float32))
    if layout == PLANAR:
        return (re, im), re, im
    return (np.ascontiguousarray(np.stack([re, im], axis=-1)),), re, im


def length(B, N, bstride):
    return (B - 1) * bstride + N + 7


def host_desc(g, arrays, layout, M, N, ld, bstride):
    from gpuacceleratedtracking_amd.frontend import host_desc as hd
    return hd(arrays[0], arrays[1] if layout == PLANAR else None, layout, M, N, ld, bstride)


def plan(g, desc, B, P, fs, cfg, log2=0, num_cus=256, dbatch=0, ubatch=0, own_power=False):
    from gpuacceleratedtracking_amd.acquisition import acquire_fft_plan
    return acquire_fft_plan(desc, B, P, fs, cfg, fft_log2=log2, doppler_batch=dbatch, unit_batch=ubatch, num_cus=num_cus, own_power=own_power)


def twin(g, desc, B, prns, fs, cfg, log2, groups=1, codes=None):
    from gpuacceleratedtracking_amd.acquisition import acquire_fft_host
    return acquire_fft_host(desc, B, oracle.codes("GPSL1", 32) if codes is None else codes, prns, fs, cfg, log2, groups)


def sample_bins(rng, J, s, N, log2, extra=(), n_random=24, max_seams=8):
    """Code bins to compare: the ends, both sides of the seams between lag segments (the last bin at a lag below the seam and the
    first at or above it; with Jseg < s those are neighbours whatever lies between), `extra` (the peak) and random ones.  Of more
    than `max_seams` seams the first, the last and evenly spaced ones between are kept."""
    jseg = (1 << log2) - N + 1
    c = [0, J - 1, *extra, *rng.choice(J, min(J, n_random), replace=False)]
    seams = np.arange(1, s * (J - 1) // jseg + 1, dtype=np.int64) * jseg  # the lags o = k Jseg <= s (J - 1)
    if seams.size > max_seams:
        seams = seams[np.unique(np.rint(np.linspace(0, seams.size - 1, max_seams)).astype(np.int64))]
    for o in seams:
        c += [(int(o) - 1) // s, -(-int(o) // s)]
    return np.unique([j for j in c if 0 <= j < J]).astype(np.int64)


# ---- the whole accepted domain (tests/test_acquisition_fft_domain_host.py, tests/test_acquisition_fft_domain_gpu.py) --------------
class Case(NamedTuple):
    """One call of the domain tests.  The samples lie in rows of `offset` + length(B, N, block_stride) + `pad` elements (the antenna
    stride), the signal view starting `offset` elements in.  table: None (GPS L1) or (Lc, rows, chip kind) for helpers.code_table;
    prns: the rows searched, in the call's order.  D = 0 / -1: the Doppler bin count is the first / last that short_step_doppler_bins finds.
    log2: the forced transform length; want: the (passes, lag segments) the case is there for.  ubatch: acq_fft_unit_batch, -1 for
    the plan's unit-group count.  peak: the bin under the satellites (-1: 2 J / 3); reduce: compare against the reference with the
    exactly reduced carrier (helpers.correlate_reduced); must: bins that are always compared."""
    group: str
    layout: int
    M: int
    B: int
    N: int
    block_stride: int
    pad: int
    offset: int
    fs: float
    fc: float
    table: Optional[tuple]
    prns: tuple
    s: int
    first_shift: int
    J: int
    D: int
    if_hz: float
    f_first: float
    f_step: float
    log2: int
    want: tuple
    ubatch: int = 0
    peak: int = -1
    reduce: bool = False
    must: tuple = ()


def _case(group, layout, M, B, N, J, log2, want, block_stride=None, pad=0, offset=0, fs=2.046e6, fc=FC, table=None, prns=(17,), s=1,
          first_shift=0, D=2, if_hz=0.0, f_first=-250.0, f_step=500.0, **kw):
    return Case(group, layout, M, B, N, N if block_stride is None else block_stride, pad, offset, fs, fc, table, tuple(prns), s,
                first_shift, J, D, if_hz, f_first, f_step, log2, want, **kw)


def _domain():
    from tests.helpers import floormod_hard_taus
    d = {}
    # A. every transform length: N = 0.76 F (odd), one lag past the first segment and a few more, the satellite on the seam
    for L in range(10, 19):
        F = 1 << L
        N = int(0.76 * F) | 1
        jseg = F - N + 1
        M, B = ((2, 1), (1, 2))[L & 1]
        d[f"A-2^{L}"] = _case("A", (L - 10) % 4, M, B, N, jseg + 9, L, (1 if L <= 12 else 2, 2), block_stride=N + 3, first_shift=-5 * (L & 1),
                              peak=jseg)
    # B. the ends of the lag-segment geometry
    d["B-seams-only"] = _case("B", PLANAR, 1, 2, 1023, 33, 10, (1, 17), block_stride=1030)                      # Jseg = 2
    d["B-empty-segments"] = _case("B", CF32, 2, 1, 2047, 5, 11, (1, 63), s=31, first_shift=-40)                   # Jseg = 2 < s
    d["B-one-sample"] = _case("B", PLANAR, 2, 2, 1, 40, 10, (1, 1), block_stride=5, table=(97, 2, "int8"), prns=(1, 0), fc=0.5 * 2.046e6)
    d["B-one-bin"] = _case("B", I16, 1, 2, 700, 1, 10, (1, 1), block_stride=711, first_shift=-7, peak=0)
    d["B-step-3"] = _case("B", I8, 2, 1, 1847, 180, 11, (1, 3), s=3, first_shift=11)                              # Jseg = 202
    # C. the work split: six units, three PRNs; the Doppler bin count comes from the plan
    for L, N in ((13, 5000), (12, 3000)):
        for pick, ub in ((0, 0), (0, -1), (-1, 0), (-1, -1)):
            d[f"C-short-step-2^{L}" + ("-last" if pick else "") + ("-batches" if ub else "")] = _case(
                "C", (CF32, PLANAR)[L & 1], 2, 3, N, 300, L, ((L > 12) + 1, 1), block_stride=N + 9, fs=4.092e6, prns=PRNS, s=2, D=pick, first_shift=-3, ubatch=ub)
    d["C-block-window"] = _case("C", PLANAR, 3, 4, 700, 800, 10, (1, 3), block_stride=733, prns=PRNS, D=15, first_shift=-11, ubatch=1)
    # D. caller code tables: F = 4096, Jseg = 1097, three segments
    tables = [("D-Lc1-int8", (1, 3, "int8"), (2, 0), 0.5), ("D-Lc2-ternary", (2, 6, "ternary"), (5, 0, 5), 0.5),
              ("D-Lc257-int8", (257, 2, "int8"), (1, 0), 0.5), ("D-Lc257-zeros-2.5", (257, 4, "pm1_zeros"), (3, 1), 2.5),
              ("D-Lc4092-ternary", (4092, 3, "ternary"), (2, 0), 0.5), ("D-Lc4092-int8-2.5", (4092, 2, "int8"), (1, 0), 2.5),
              ("D-Lc120000-int8", (120000, 2, "int8"), (1, 0), 0.5), ("D-Lc120000-ternary", (120000, 6, "ternary"), (5, 0, 5), 0.5)]
    for k, (name, table, prns, ratio) in enumerate(tables):
        d[name] = _case("D", k % 4, 1, 2, 3000, 2500, 12, (1, 3), block_stride=3001, fs=4.0e6, fc=ratio * 4.0e6, table=table, prns=prns,
                        first_shift=-5, f_first=-500.0)
    # E. the ends of the code-phase span: fc = fs, the chip phase is the sample index
    for sign in (1, -1):
        d[f"E-shift-{'+' if sign > 0 else '-'}2^29"] = _case("E", PLANAR, 1, 1, 1500, 600, 11, (1, 2), fs=FC, first_shift=sign * (1 << 29), peak=50)
    hi = (1 << 30) - 8192
    for lo_, hi_, seed in ((hi // 2, hi, 31), (-hi, -(hi // 2), 37)):
        for t in floormod_hard_taus(LC, lo_, hi_, seed, count=1):  # the phase t lies under replica sample 100 of segment 0: lags 0 .. 100 read it
            q = np.floor(np.float32(t) * (np.float32(1.0) / np.float32(LC)))
            name = f"E-hard-{'pos' if t > 0 else 'neg'}-{'low' if t - float(q) * LC < 0 else 'high'}"
            d[name] = _case("E", CF32, 1, 1, 1500, 600, 11, (1, 2), fs=FC, first_shift=int(t) - 100, peak=50, must=(99, 100, 101))
    # F. descriptor and carrier
    d["F-ant-stride"] = _case("F", PLANAR, 2, 2, 1500, 600, 11, (1, 2), block_stride=1507, pad=13)
    d["F-overlap"] = _case("F", CF32, 2, 3, 2000, 300, 12, (1, 1), block_stride=1000)
    for layout, nm in ((CF32, "cf32"), (I16, "int16"), (I8, "int8")):
        d[f"F-offset-{nm}"] = _case("F", layout, 2, 2, 1500, 600, 11, (1, 2), block_stride=1507, pad=13, offset=3)
    d["F-negative-step"] = _case("F", PLANAR, 1, 2, 1500, 600, 11, (1, 2), D=5, f_first=1000.0, f_step=-500.0)
    for nm, cyc in (("0.5", 0.5), ("1.25", 1.25), ("-3.75", -3.75)):  # row 0 exactly there, the others 500 Hz a row beyond
        d[f"F-carrier-{nm}fs"] = _case("F", (PLANAR, I16, CF32)[int(abs(cyc)) % 3], 1, 2, 1500, 600, 11, (1, 2), D=3, if_hz=cyc * 2.046e6 - 500.0,
                                       f_first=500.0, f_step=500.0 if cyc > 0 else -500.0, reduce=True)
    return d


DOMAIN = _domain()


def case_codes(case):
    from tests.helpers import code_table
    if case.table is None:
        return oracle.codes("GPSL1", 32)
    lc, rows, kind = case.table
    return code_table(lc, rows, 1000 + lc + rows, kind)


def case_peak(case):
    return case.peak if case.peak >= 0 else 2 * case.J // 3


def domain_scene(case):
    """A satellite of every row searched (of a caller's table: its last row only, as tests/test_code_tables_gpu.py's
    test_acquisition_grid has it), its code edge on bin case_peak(case), near the middle Doppler row, in noise of 0.5 max|chip|.
    Returns a dict: codes (int8 [rows, Lc]), arrays (the host buffers, rows of `row` elements in the case's layout), row, ld, and
    re / im (float32 [M, ld]: the values the signal view holds, planar, for the oracle)."""
    codes = case_codes(case)
    lc = codes.shape[1]
    amax = float(np.abs(codes).max())
    ld = length(case.B, case.N, case.block_stride)
    row = case.offset + ld + case.pad
    rng = np.random.default_rng(4000 + sum(map(ord, case.group)) + case.N + case.J)
    sats = list(dict.fromkeys(case.prns)) if case.table is None else [codes.shape[0] - 1]
    ratio = case.fc / case.fs
    tau0 = float(np.mod(ratio * float(case.first_shift + case.s * case_peak(case)), float(lc)))
    x = np.zeros(ld, dtype=np.complex128)
    for k, p in enumerate(sats):
        f = case.if_hz + case.f_first + case.f_step * (max(case.D, 0) // 2 + 0.2 * k)
        r1, i1 = oracle.gen_signal(codes, p, case.fc, case.fs, f, tau0, 0.3 * k, ld, 1)
        x += r1[0] + 1j * i1[0]
    x = x[None, :] * np.exp(2j * np.pi * rng.uniform(0, 1, (case.M, 1)))
    x = x + 0.5 * amax * (rng.standard_normal(x.shape) + 1j * rng.standard_normal(x.shape))
    x = x * (SCALE[case.layout] / amax)
    buf = np.zeros((case.M, row), dtype=np.complex128) + (99.0 + 77.0j)  # what lies around the view must not be read
    buf[:, case.offset:case.offset + ld] = x
    if case.layout in (I16, I8):
        dt = np.int16 if case.layout == I16 else np.int8
        lim = np.iinfo(dt).max
        pair = np.ascontiguousarray(np.clip(np.stack([np.rint(buf.real), np.rint(buf.imag)], axis=-1), -lim, lim).astype(dt))
        arrays, fr, fi = (pair,), pair[..., 0].astype(np.float32), pair[..., 1].astype(np.float32)
    else:
        fr, fi = np.ascontiguousarray(buf.real.astype(np.float32)), np.ascontiguousarray(buf.imag.astype(np.float32))
        arrays = (fr, fi) if case.layout == PLANAR else (np.ascontiguousarray(np.stack([fr, fi], axis=-1)),)
    view = slice(case.offset, case.offset + ld)
    return dict(codes=codes, arrays=arrays, row=row, ld=ld, re=np.ascontiguousarray(fr[:, view]), im=np.ascontiguousarray(fi[:, view]))


def case_config(g, case, D=None):
    return config(g, case.D if D is None else D, case.J, case.s, case.first_shift, case.f_first, case.f_step, case.if_hz,
                  lc=LC if case.table is None else case.table[0], fc=case.fc)


def case_host_desc(g, case, sc):
    from gpuacceleratedtracking_amd.frontend import host_desc as hd
    a = sc["arrays"]
    return hd(a[0], a[1] if case.layout == PLANAR else None, case.layout, case.M, case.N, sc["row"], case.block_stride, case.offset)


def short_step_doppler_bins(g, case, desc, num_cus):
    """The first (case.D = 0) or last (case.D = -1) D in 1 .. 64 at which the plan deals the call's units to a group count that does
    not divide them (the last step of the call is short), or None.  Six units, three PRNs and 256 compute units: five groups at the
    first, four at the last."""
    for D in (range(1, 65) if case.D == 0 else range(64, 0, -1)):
        pl = plan(g, desc, case.B, len(case.prns), case.fs, case_config(g, case, D), case.log2, num_cus)
        if (case.M * case.B) % pl["unit_groups"] != 0:
            return D
    return None


def case_oracle(case, sc, prn, D, cols):
    """The FP64 contract's power [D, len(cols)] for code-table row `prn`."""
    from tests.helpers import acq_power_oracle, correlate_reduced
    lc = sc["codes"].shape[1]
    rows = np.arange(D)
    if not case.reduce:
        return acq_power_oracle(sc["re"], sc["im"], sc["codes"], prn, case.fc, lc, case.fs, case.if_hz, case.f_first, case.f_step, rows,
                                case.first_shift, case.s, cols, case.N, case.B, case.block_stride)
    # the same records as acq_power_oracle builds, through the reference that reduces the carrier step exactly
    f = case.if_hz + (case.f_first + rows.astype(np.float64) * case.f_step)
    tau = np.fmod(case.fc / case.fs * (np.arange(case.B, dtype=np.int64) * case.block_stride).astype(np.float64), float(lc))
    prm = oracle.make_params(np.full((case.B, D), prn), case.fc, np.broadcast_to(f, (case.B, D)), np.broadcast_to(tau[:, None], (case.B, D)), 0.0)
    shifts = (case.first_shift + case.s * np.asarray(cols, dtype=np.int64)).astype(np.int32)
    R = correlate_reduced(sc["re"], sc["im"], sc["codes"], prm, case.fs, shifts, case.N, case.block_stride)
    return (R.real ** 2 + R.imag ** 2).sum(axis=(0, 3))


def check_case(case, sc, power, D, log2, what):
    """Every Doppler row of `power` [P, D, J] on the sampled bins against the contract, at the project's RTOL.  Returns the worst
    (norm-wise, element-wise) errors."""
    from tests.helpers import check_power_close
    rng = np.random.default_rng(7)
    worst = [0.0, 0.0]
    for pi, p in enumerate(case.prns):
        peak = int(np.unravel_index(np.argmax(power[pi]), power[pi].shape)[1])
        jsel = sample_bins(rng, case.J, case.s, case.N, log2, extra=[peak, case_peak(case), *case.must], n_random=12)
        e = check_power_close(power[pi][:, jsel], case_oracle(case, sc, p, D, jsel), what=f"{what} prn row {p}")
        worst = [max(worst[0], e[0]), max(worst[1], e[1])]
    return worst


# ---- the refusal boundaries: one antenna, one block, one PRN (row 0), one Doppler bin, fs = FC, planar samples ------------------------
# name: what differs between the call just inside and the call just outside, over the defaults below
_F10 = 1024 + 325  # N = 700 forced into F = 1024: F + G Jseg of one segment
BOUNDARIES = {
    # the plan's reach F + |first_shift| + G Jseg (no less than the N + |first_shift| + s J of include/gat.h) against 2^30, at half
    # a chip a sample so that the code-phase span stays far inside
    "reach-2^30": [dict(first_shift=(1 << 30) - 1 - _F10), dict(first_shift=(1 << 30) - _F10)],
    "reach-2^30-negative": [dict(first_shift=-((1 << 30) - 1 - _F10)), dict(first_shift=-((1 << 30) - _F10))],
    # a table of one chip at a chip a sample: the span Lc + reach + 1 against 2^21 Lc
    "span-2^21-Lc": [dict(lc=1, ratio=1.0, first_shift=(1 << 21) - 3 - _F10), dict(lc=1, ratio=1.0, first_shift=(1 << 21) - 2 - _F10)],
    "block-2^18": [dict(N=(1 << 18) - 1, J=1, log2=0, twin_log2=18), dict(N=1 << 18, J=1, log2=0, twin_log2=18)],
    # forced lengths around N = 2048: the smallest power of two above N, and N rounded down to one (N itself)
    "forced-length": [dict(N=2048, log2=12, twin_log2=12), dict(N=2048, log2=11, twin_log2=11)],
}


def boundary_calls(name):
    return [{**dict(N=700, J=5, first_shift=0, ratio=0.5, lc=LC, log2=10, twin_log2=10), **side} for side in BOUNDARIES[name]]


def boundary_codes(side):
    return np.ascontiguousarray(oracle.codes("GPSL1", 1)) if side["lc"] == LC else np.full((1, side["lc"]), -3, dtype=np.int8)
