"""An independent FP64 restatement of the snapshot fix (coarse-time navigation) in numpy, on the textbook orbit and clock of
tests/fix_ref.py: the sub-millisecond ranges by numpy's modulo, the predicted ranges with the light time iterated to rest, the
whole milliseconds by ``np.rint`` against the highest satellite, the five-unknown step by ``np.linalg.lstsq`` with the coarse-time
column as a central difference of the modelled range in time (no analytic satellite velocity), the dilutions from the pseudo-
inverse.  It shares no text with the library's rule; the tests compare the two within bounds derived from the arithmetic, and the
integers exactly."""
import numpy as np

from tests import fix_ref as ref

C = ref.C_LIGHT
MS = 1e-3
LAMBDA = C * MS
RATE_STEP = 0.25  # s: the central difference's half width; the range's third derivative (1e-4 m/s^3) leaves 1e-6 m/s


def fractions(code_frac, rx_frac):
    """(z [K] = c phi with phi = (rx_frac - code_frac) mod 1 ms, borrow [K])"""
    d = rx_frac - np.asarray(code_frac, dtype=np.float64)
    return C * np.mod(d, MS), (d < 0).astype(np.int64)


def modelled(ephs, t_sv, xyz):
    """(range - c dts [K], unit vectors [K, 3], range [K]) of satellites whose own clocks read t_sv at transmission"""
    pos, dts = ref.satellite(ephs, np.zeros(len(ephs)), np.mod(t_sv, ref.WEEK))
    rng, los = ref.geometry(pos, xyz)
    return rng - C * dts, los, rng


def predicted(ephs, xyz, bias_m, tc, t_read):
    """(p [K], sin el [K]) at a state: the transmit time t_read - tc - tau with tau iterated to rest"""
    tau = np.full(len(ephs), 0.075)
    for _ in range(6):
        m, los, rng = modelled(ephs, t_read - tc - tau, xyz)
        tau = rng / C
    return m + bias_m, los @ (xyz / np.linalg.norm(xyz))


def integers(p, sin_el, z, use):
    """(n [K], q [K]): the whole milliseconds against the used satellite that stands highest"""
    k0 = int(np.flatnonzero(use)[np.argmax(sin_el[use])])
    n0 = np.rint((p[k0] - z[k0]) / LAMBDA)
    q = (p - p[k0]) / LAMBDA + n0 + (z[k0] - z) / LAMBDA
    return np.rint(q).astype(np.int64), q


def transmit_seconds(rx_ms, n, borrow, code_frac, tc):
    return (int(rx_ms) - n - borrow) * MS + code_frac - tc


def solve(ephs, code_frac, rx_ms, n, borrow, z, use, start, weights=None, tol=1e-9, max_iter=30):
    """weighted least squares over the channels ``use``: (state [5] = x, y, z, b, t_c; residuals [K]; the design matrix [n_used, 5])"""
    st = np.array(start, dtype=np.float64)
    rho = n * LAMBDA + z
    w = np.ones(len(z)) if weights is None else np.asarray(weights, dtype=np.float64)
    sq = np.sqrt(w[use])

    def rows(state):
        t = transmit_seconds(rx_ms, n, borrow, code_frac, state[4])
        m, los, _ = modelled(ephs, t, state[:3])
        ahead, _, _ = modelled(ephs, t + RATE_STEP, state[:3])
        behind, _, _ = modelled(ephs, t - RATE_STEP, state[:3])
        rate = (ahead - behind) / (2 * RATE_STEP)
        return rho - (m + state[3]), np.concatenate([-los, np.ones((len(z), 1)), -rate[:, None]], axis=1)

    for _ in range(max_iter):
        v, a = rows(st)
        step = np.linalg.lstsq(a[use] * sq[:, None], v[use] * sq, rcond=None)[0]
        st = st + step
        if np.linalg.norm(step[:3]) < tol:
            break
    v, a = rows(st)
    return st, v, a[use]


def snapshot(ephs, code_frac, rx_ms, rx_frac, prior, weights=None, margin=0.1):
    """One epoch.  Returns a dict: xyz, clock_bias_s, coarse_time_s, n [K], q [K], use [K], margins (the largest |q - n| over the used
    channels of the first resolution), ambiguous, reresolved, tx_ms [K], rx_ms_out, pdop, gdop, tdop."""
    code_frac = np.asarray(code_frac, dtype=np.float64)
    ok = np.isfinite(code_frac) & (code_frac >= 0) & (code_frac < MS) & (ephs["valid"] != 0)
    w = np.ones(len(code_frac)) if weights is None else np.asarray(weights, dtype=np.float64)
    use = ok & np.isfinite(w) & (w > 0)
    frac = np.where(ok, code_frac, 0.0)
    z, borrow = fractions(frac, rx_frac)
    t_read = int(rx_ms) * MS + rx_frac
    prior = np.asarray(prior, dtype=np.float64)
    p, sin_el = predicted(ephs, prior, 0.0, 0.0, t_read)
    n, q = integers(p, sin_el, z, use)
    worst = float(np.abs(q - n)[use].max())
    st, v, a = solve(ephs, frac, rx_ms, n, borrow, z, use, tuple(prior) + (0.0, 0.0), weights)
    p2, sin_el2 = predicted(ephs, st[:3], st[3], st[4], t_read)
    n2, _ = integers(p2, sin_el2, z, use)
    reresolved = bool((n2 != n)[use].any())
    if reresolved:
        n = n2
        st, v, a = solve(ephs, frac, rx_ms, n, borrow, z, use, st, weights)
    cov = np.linalg.pinv(a.T @ a)
    m = int(np.rint(st[4] * 1e3))
    tx_ms = np.where(ok, (int(rx_ms) - n - borrow - m) % 604800000, -1)
    return {"xyz": st[:3], "clock_bias_s": st[3] / C, "coarse_time_s": st[4], "n": np.where(ok, n, 0), "q": q, "use": use, "ok": ok,
            "worst": worst, "ambiguous": worst > 0.5 - margin, "reresolved": reresolved, "tx_ms": tx_ms, "rx_ms_out": (int(rx_ms) - m) % 604800000,
            "resid": np.where(ok, v, 0.0), "pdop": float(np.sqrt(np.trace(cov[:3, :3]))), "gdop": float(np.sqrt(np.trace(cov[:4, :4]))),
            "tdop": float(np.sqrt(cov[4, 4]))}
