// gat_raim_plan.h -- the pure part of gat_position_fix_raim (include/gat.h, "fix integrity"): its refusals and the launch geometry as a
// function of the call's arguments alone, and the host twin's loops over the rules of gat_fix.h and gat_raim.h.  No HIP call and no
// HIP header: the device entry point, the host twin and a stand-alone test program (tests/raimplan) compile the same text.
#pragma once

#include "gat_fix_plan.h"
#include "gat_raim.h"

namespace gat {

// a wave's LDS: the fix's terms and sums, then the K frozen channels of a round
constexpr int kRaimWaveDoubles = kFixWaveDoubles + kRaimEntry * kFixWave;
constexpr int kRaimLdsBytes = kFixWaves * kRaimWaveDoubles * (int)sizeof(double);

struct RaimCall {
    FixCall fix;
    const gat_raim_config *raim;
    const void *integrity;
};

// Work units: the fix's (workgroup g, wave w: epoch g * kFixWaves + w; lane k: channel k, and in a round candidate k).
struct RaimPlan {
    FixPlan fix;
    int max_exclude, trial_iter;
    double threshold[kRaimThresholds];
};

// The whole call.  *plan is written only with GAT_OK.
inline Refusal raim_plan(const RaimCall &a, RaimPlan *plan)
{
    const gat_raim_config *rc = a.raim;
    if (!rc || !a.integrity || !plan) return {GAT_ERR_ARG, "null argument"};
    if (rc->struct_size != sizeof(gat_raim_config)) return {GAT_ERR_ARG, "raim.struct_size is not sizeof(gat_raim_config)"};
    if (rc->max_exclude < 0 || rc->max_exclude > GAT_RAIM_MAX_EXCLUDE) return {GAT_ERR_ARG, "max_exclude must be 0 .. 4"};
    if (rc->trial_iter < 1) return {GAT_ERR_ARG, "trial_iter must be positive"};
    if (rc->flags != 0) return {GAT_ERR_ARG, "raim.flags must be 0"};
    for (int d = 1; d < kRaimThresholds; ++d)
        if (!(rc->threshold[d] > 0.0)) return {GAT_ERR_ARG, "a threshold is NaN or not positive"};
    RaimPlan p{};
    const Refusal r = fix_plan(a.fix, &p.fix);
    if (r.code != GAT_OK) return r;
    p.max_exclude = rc->max_exclude, p.trial_iter = rc->trial_iter;
    p.threshold[0] = 0.0;
    for (int d = 1; d < kRaimThresholds; ++d) p.threshold[d] = rc->threshold[d];
    *plan = p;
    return {GAT_OK, nullptr};
}

// the public report: the fix's, with the trial's LDS
inline void raim_report(const RaimPlan &p, gat_fix_plan *out)
{
    fix_report(p.fix, out);
    out->lds_bytes = kRaimLdsBytes;
}

// ---- the host twin ----------------------------------------------------------------------------------------------------------------
// T of the used set at the rows as they stand
inline double raim_host_stat(const FixHostEpoch &h)
{
    double T = 0.0;
    for (int k = 0; k < h.K; ++k)
        if (h.used[k]) T += raim_term(h.wk[k], h.row[k].v);
    return T;
}

// One epoch: the fix, the test and the rounds; a candidate where the kernel has a lane.  trial [K] or null.
inline void raim_host_epoch(const RaimPlan &p, const gat_ephemeris *eph, const int32_t *tx_ms, const double *tx_frac, int32_t rx_ms, double rx_frac,
                            const double *w, gat_fix *fix, gat_fix_integrity *integ, double *sat, double *resid, double *sin_el, uint8_t *used_out,
                            double *trial)
{
    const int K = p.fix.K;
    FixHostEpoch h;
    h.init(p.fix, eph, tx_ms, tx_frac, rx_ms, rx_frac, w);
    h.solve();
    h.write(0, fix, sat, resid, sin_el, used_out); // the full set's outputs: they stand unless a channel is left out
    if (trial)
        for (int k = 0; k < K; ++k) trial[k] = -1.0;
    if (fix_failed(h.status) || (h.status & GAT_FIX_NOT_CONVERGED)) {
        *integ = raim_full_set(GAT_RAIM_NOT_CHECKED, 0, 0.0, 0.0);
        return;
    }
    const double T0 = raim_host_stat(h);
    const int d0 = h.num_used - 4;
    if (d0 == 0) {
        *integ = raim_full_set(GAT_RAIM_NO_REDUNDANCY, 0, T0, 0.0);
        return;
    }
    if (!raim_detected(T0, p.threshold[d0])) {
        *integ = raim_full_set(0, d0, T0, p.threshold[d0]);
        return;
    }
    const gat_fix_integrity full = raim_full_set(GAT_RAIM_DETECTED | GAT_RAIM_UNRESOLVED, d0, T0, p.threshold[d0]);
    *integ = full;
    int ex[GAT_RAIM_MAX_EXCLUDE] = {-1, -1, -1, -1};
    double ent[kRaimEntry * GAT_MAX_FIX_CHANNELS];
    for (int r = 0; r < p.max_exclude; ++r) {
        if (h.num_used < 6) return;
        for (int k = 0; k < K; ++k) raim_entry(h.s[k], h.tau[k], h.wk[k], h.used[k], ent + kRaimEntry * k);
        bool any = false;
        RaimTrial best{};
        int jbest = -1;
        for (int j = 0; j < K; ++j) {
            if (!h.used[j]) continue;
            const RaimTrial t = raim_trial(ent, K, j, h.st, p.trial_iter, p.fix.tol_m);
            if (!t.counts) continue;
            if (r == 0 && trial) trial[j] = t.T;
            if (!any || raim_before(t.T, j, best.T, jbest)) best = t, jbest = j, any = true;
        }
        if (!any) return;
        h.used[jbest] = false;
        h.num_used -= 1;
        for (int i = 0; i < 4; ++i) h.st[i] = best.st[i];
        h.rows(); // the travel times of the state the fault had moved give way to this state's before the pass
        if (!h.pass()) return;
        h.elevations();
        ex[r] = jbest;
        const double T = raim_host_stat(h);
        const double thr = p.threshold[h.num_used - 4];
        if (!raim_detected(T, thr)) {
            *integ = raim_excluded(full, r + 1, ex[0], ex[1], ex[2], ex[3], T, thr);
            h.write(GAT_FIX_EXCLUDED, fix, sat, resid, sin_el, used_out);
            return;
        }
    }
}

// The twin's loops (gat_position_fix_raim_host) for a planned call, every pointer host memory.
inline void raim_host_run(const RaimPlan &p, const gat_ephemeris *eph, const int32_t *tx_ms, const double *tx_frac, const int32_t *rx_ms,
                          const double *rx_frac, const double *w, gat_fix *fixes, gat_fix_integrity *integ, double *sat, double *resid, double *sin_el,
                          uint8_t *used, double *trial)
{
    for (int e = 0; e < p.fix.E; ++e) {
        const size_t o = (size_t)e * (size_t)p.fix.K;
        raim_host_epoch(p, eph, tx_ms + o, tx_frac + o, rx_ms[e], rx_frac[e], w ? w + o : nullptr, fixes + e, integ + e, sat ? sat + 4 * o : nullptr,
                        resid ? resid + o : nullptr, sin_el ? sin_el + o : nullptr, used ? used + o : nullptr, trial ? trial + o : nullptr);
    }
}

} // namespace gat
