"""The self-calibration scene of tests/test_subspace_pipeline_gpu.py and its FP64 restatement on the CPU.

Two GPS L1 C/A satellites on M = 4 antennas whose steering phases (cable lengths, geometry) are (0, 0.31, 0.55, 0.83) cycles --
|sum_m e^{j 2 pi phi_m}|^2 = 0.092 of a possible 16, so the plain antenna sum loses the signal --, fs = 4 MHz, N = 4000 (1 ms),
noise of sigma = 8 per component: SNR = N / (2 sigma^2) = 31.25 per block and antenna, 44.9 dB-Hz.  840 blocks with the data bits
of a fixed draw (a half cycle on the carrier phase, edges on block boundaries); 40 blocks settle, 800 are kept: the steering vector
is estimated from the first 400 of them, the two loops' C/N0 is compared over all 800 (over 400 the spread of the moments
estimator's gain was 0.36 dB, three of which are more than 1 dB).

``python -m tests.sub_pipeline`` runs the restatement over 20 noise seeds -- oracle.np_correlate for the accumulators,
array_ref.tracking_update_weighted for the loop, the library's FP64 host twins for the covariance and its eigenvector,
tests/mon_ref.py for the monitor -- and prints the figures quoted in the test's docstring: the steering estimate's miss
1 - |a^H a^|^2 / (M |a^|^2) of the loop on antenna 0, and what the loop on the conventional beam of a^ gains in C/N0 over it."""
import numpy as np

N, M, FS, FC = 4000, 4, 4e6, 1.023e6
T = N / FS
PRNS = np.array([7, 19])
DOP = np.array([-2210.0, 310.0])
TAU0 = np.array([511.9, 100.3])
PHI0 = np.array([0.6, 0.1])
STEER = np.array([0.0, 0.31, 0.55, 0.83])
SIGMA = 8.0
SETTLE, KEPT, ESTIMATE = 40, 800, 400
BITS = np.where(np.random.default_rng(5).integers(0, 2, (2, (SETTLE + KEPT) // 20)) > 0, 1, -1)
BLOCKS = SETTLE + KEPT
SNR = N / (2.0 * SIGMA ** 2)
GAIN_DB = 10.0 * np.log10(M)
# The restatement's figures (``python -m tests.sub_pipeline``, 20 seeds x 2 channels, 800 kept blocks), fixed before the GPU ran:
#   miss of the steering estimate (400 blocks): mean 6.56e-5, largest 1.75e-4, against the bound 4.84e-4
#   gain - 10 log10 M, narrow-to-wide: mean -0.197 dB, std 0.213 dB, smallest -0.657, largest +0.256
#   gain - 10 log10 M, moments:        mean -0.255 dB, std 0.283 dB, smallest -0.855, largest +0.245
# (over 400 kept blocks: -0.221 / 0.249 and -0.283 / 0.357 dB).  Estimator -> (mean, margin = three standard deviations, rounded up).
GAIN_EXPECTED = {"nwpr": (-0.197, 0.64), "m2m4": (-0.255, 0.85)}


def steering_bound(B=ESTIMATE):
    """8 x the first-order miss of a principal eigenvector from B snapshots, (M - 1) / (M B SNR) (1 + 1 / (M SNR))"""
    return 8.0 * (M - 1) / (M * B * SNR) * (1.0 + 1.0 / (M * SNR))


def truth(blocks=BLOCKS):
    """code frequency [K], and per block the code phase, the carrier phase in cycles (with the bits' half cycles) and the bits"""
    fcode = FC * (1 + DOP / 1575.42e6)
    b = np.arange(blocks, dtype=np.float64)[:, None]
    tau = np.mod(TAU0[None, :] + fcode[None, :] * T * b, 1023.0)
    bits = np.stack([np.repeat(x, 20)[:blocks] for x in BITS], axis=1)
    phi = np.mod(PHI0[None, :] + DOP[None, :] * T * b + 0.25 * (1 - bits), 1.0)
    return fcode, tau, phi, bits


def miss(a_hat):
    """1 - |a^H a^|^2 / (M |a^|^2) per channel, a the scene's steering vector"""
    a = np.exp(2j * np.pi * STEER.astype(np.float32).astype(np.float64))
    a_hat = np.asarray(a_hat)
    return 1.0 - np.abs(a_hat @ a.conj()) ** 2 / (M * np.sum(np.abs(a_hat) ** 2, axis=-1))


def cn0_of(acc_re, acc_im, prompt_index, w):
    """(narrow-to-wide [K], moments over one window [K]) of accumulators [B, K, L, M] under the weights w, by tests/mon_ref.py"""
    from tests import mon_ref as ref
    B = acc_re.shape[0]
    r = ref.monitor(acc_re, acc_im, prompt_index, B, np.ones(20, np.int8), first_block=SETTLE, weights=w)
    nwpr = [ref.cn0_nwpr(r["sym_re"][k], r["sym_im"][k], r["sym_wbp"][k], r["channels"][k][2], 20, T) for k in range(len(PRNS))]
    m2m4 = [ref.cn0_m2m4(r["windows"][k][0], T) for k in range(len(PRNS))]
    return np.array(nwpr), np.array(m2m4)


def cpu_reference(seed):
    """One noise seed through the restatement: (miss [K], gain of the narrow-to-wide C/N0 [K], gain of the moments C/N0 [K]) in dB
    over 10 log10 M."""
    import gpuacceleratedtracking_amd as g
    import oracle
    from tests import array_ref
    codes = [oracle.np_code_gpsl1(int(p)) for p in PRNS]
    fcode, tau, phi, _ = truth()
    K = len(PRNS)
    shifts = oracle.sample_shifts(3, FS, FC, 0.5)
    order = np.argsort(shifts, kind="stable")
    prompt = int(np.nonzero(shifts == 0)[0][0])
    cfg = dict(block_seconds=T, pll_bandwidth_hz=18.0, dll_bandwidth_hz=4.0, code_freq_nominal_hz=FC, carrier_center_hz=1575.42e6, if_hz=0.0,
               early_late_spacing_chips=float(shifts[order[-1]] - shifts[order[0]]) * FC / FS, code_length=1023, num_taps=3,
               early_index=int(order[0]), prompt_index=prompt, late_index=int(order[-1]))
    rng = np.random.default_rng(seed)
    steer = np.exp(2j * np.pi * STEER.astype(np.float32).astype(np.float64))
    n = np.arange(N, dtype=np.float64)
    blocks = []
    for b in range(BLOCKS):
        x = np.zeros(N, np.complex128)
        for k in range(K):
            chips = codes[k][np.mod(np.floor(fcode[k] / FS * n + tau[b, k]).astype(np.int64), 1023)]
            x += chips * np.exp(2j * np.pi * (DOP[k] * n / FS + phi[b, k]))
        x = steer[:, None] * x[None, :] + SIGMA * (rng.standard_normal((M, N)) + 1j * rng.standard_normal((M, N)))
        blocks.append((x.real.astype(np.float32), x.imag.astype(np.float32)))

    def loop(w):
        names = ("init_carrier_doppler_hz", "carrier_doppler_hz", "code_doppler_hz", "pll_acc1", "pll_acc2", "dll_acc", "last_pll_error_cycles",
                 "last_dll_error_chips", "prompt_power")
        state = {name: np.zeros(K) for name in names}
        state["init_carrier_doppler_hz"] = DOP + 0.2
        state["carrier_doppler_hz"] = DOP + 0.2
        dop = DOP + 0.2
        cur = oracle.make_params(PRNS - 1, FC + dop * FC / 1575.42e6, dop, TAU0 + 0.02, np.mod(PHI0 + 0.02, 1.0))
        acc = np.zeros((BLOCKS, K, 3, M), np.complex128)
        for b in range(BLOCKS):
            for k in range(K):
                acc[b, k] = oracle.np_correlate(blocks[b][0], blocks[b][1], codes[k], cur["code_freq_hz"][k], FS, cur["carrier_freq_hz"][k],
                                                cur["code_phase_chips"][k], cur["carrier_phase_cycles"][k], shifts)
            cur, state = array_ref.tracking_update_weighted(acc[b], w, cfg, state, cur)
        kept = acc[SETTLE:]
        return np.ascontiguousarray(kept.real.astype(np.float32)), np.ascontiguousarray(kept.imag.astype(np.float32))

    e0 = np.zeros((K, M), np.complex128)
    e0[:, 0] = 1.0
    re0, im0 = loop(e0)
    cov = g.accumulator_covariance_host(re0[:ESTIMATE], im0[:ESTIMATE], tap_index=prompt)
    _, vec, _ = g.hermitian_eig_host(cov, num_vectors=1)
    a_hat = vec[0, :, 0, :]
    a_hat = a_hat * (np.conj(a_hat[:, :1]) / np.abs(a_hat[:, :1]))
    w = a_hat / np.sum(np.abs(a_hat) ** 2, axis=-1, keepdims=True)
    re1, im1 = loop(w)
    n0, m0 = cn0_of(re0, im0, prompt, e0)
    n1, m1 = cn0_of(re1, im1, prompt, w)
    return miss(a_hat), n1 - n0 - GAIN_DB, m1 - m0 - GAIN_DB, n0, m0


if __name__ == "__main__":
    rows = []
    for seed in range(20):
        r = cpu_reference(seed)
        rows.append(np.concatenate(r[:3]))
        print(f"seed {seed:2d}: miss {r[0]}  nwpr gain - 6.02 dB {r[1]}  m2m4 gain - 6.02 dB {r[2]}  e0 loop nwpr {r[3]} m2m4 {r[4]}", flush=True)
    rows = np.array(rows)
    print("bound on the miss", steering_bound(), "mean", rows[:, :2].mean(), "largest", rows[:, :2].max())
    for name, cols in (("nwpr", rows[:, 2:4]), ("m2m4", rows[:, 4:6])):
        print(f"{name}: gain - 10 log10 M over 20 seeds x 2 channels: mean {cols.mean():+.3f} dB, std {cols.std():.3f} dB, "
              f"smallest {cols.min():+.3f}, largest {cols.max():+.3f}")
