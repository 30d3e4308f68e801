"""An independent restatement of the fix integrity rule on top of tests/fix_ref.py, in the textbook form: the full solve and T =
sum w v^2, leave-one-out solves FROM SCRATCH (the Earth's centre, ``np.linalg.lstsq``, travel times iterated to rest in every
iteration -- nothing frozen, nothing taken over from the contaminated state) and greedy exclusion of the channel whose absence
leaves the smallest T.  It shares no text with the library's rule; the tests compare decisions (status bits, the excluded channels)
exactly and numbers within bounds derived from the arithmetic."""
import numpy as np

from tests import fix_ref as ref

NOT_CHECKED, NO_REDUNDANCY, DETECTED, EXCLUDED, UNRESOLVED = 1, 2, 4, 8, 16


def statistic(resid, w, use):
    return float(np.sum(w[use] * resid[use] ** 2))


def leave_one_out(pos, dts, rho, w, use):
    """T_j [K] of the from-scratch solve of use \\ {j} for every used j, -1 elsewhere; the states [K, 4]"""
    k = len(rho)
    t, states = np.full(k, -1.0), np.zeros((k, 4))
    for j in np.flatnonzero(use):
        sub = use.copy()
        sub[j] = False
        st, v, _, _ = ref.solve(pos[sub], dts[sub], rho[sub], w[sub])
        t[j], states[j] = float(np.sum(w[sub] * v ** 2)), st
    return t, states


def raim(ephs, tx_ms, tx_frac, rx_ms, rx_frac, thresholds, weights=None, max_exclude=1, mask_sin=-1.0):
    """One epoch.  Returns a dict: status (the RAIM bits), dof, excluded (list), xyz, used [K], stat0, stat, trial [K] (round 1's
    from-scratch T_j; -1 for a channel that was no candidate), ratio (runner-up T over the winner's in round 1, inf without)."""
    tx_ms = np.asarray(tx_ms)
    k = len(tx_ms)
    w = np.ones(k) if weights is None else np.asarray(weights, dtype=np.float64)
    ok = (tx_ms >= 0) & np.isfinite(tx_frac) & (ephs["valid"] != 0)
    out = {"status": 0, "dof": 0, "excluded": [], "xyz": np.zeros(3), "used": np.zeros(k, bool), "stat0": 0.0, "stat": 0.0, "trial": np.full(k, -1.0),
           "ratio": np.inf}
    if (ok & np.isfinite(w) & (w > 0)).sum() < 4 or not np.isfinite(rx_frac):
        out["status"] = NOT_CHECKED
        return out
    f = ref.fix(ephs, tx_ms, tx_frac, rx_ms, rx_frac, weights, mask_sin)
    use = f["used"].copy()
    rho = ref.pseudorange(rx_ms, rx_frac, np.where(ok, tx_ms, 0), np.where(ok, tx_frac, 0.0))
    pos, dts = f["sat"], f["dts"]
    n = int(use.sum())
    t0 = statistic(f["resid"], w, use)
    out.update(xyz=f["xyz"], used=use.copy(), stat0=t0, stat=t0, dof=n - 4)
    if n == 4:
        out.update(status=NO_REDUNDANCY, dof=0)
        return out
    if not t0 > thresholds[n - 4]:
        return out
    out["status"] = DETECTED | UNRESOLVED
    excluded = []
    for r in range(max_exclude):
        if use.sum() < 6:
            return out
        t, states = leave_one_out(pos, dts, rho, w, use)
        cand = np.flatnonzero(use)
        order = cand[np.argsort(t[cand], kind="stable")]
        if r == 0:
            out["trial"] = t
            out["ratio"] = float(t[order[1]] / t[order[0]])
        j = int(order[0])
        use[j] = False
        excluded.append(j)
        if not t[j] > thresholds[int(use.sum()) - 4]:
            out.update(status=DETECTED | EXCLUDED, excluded=excluded, xyz=states[j, :3], used=use.copy(), stat=float(t[j]))
            return out
    return out
