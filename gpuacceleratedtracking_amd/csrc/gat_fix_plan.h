// gat_fix_plan.h -- the pure part of gat_position_fix (include/gat.h): its refusals and the launch geometry as a function of the
// call's arguments alone, and the host twin's loops over the rule of gat_fix.h.  No HIP call and no HIP header: the device entry
// point, the host twin and a stand-alone test program (tests/fixplan) compile the same text.
#pragma once

#include "gat_fix.h"
#include "gat_sig_plan.h" // Refusal

namespace gat {

constexpr int kFixWave = 64;                        // a wave an epoch, a lane a channel
constexpr int kFixWaves = 4;                        // epochs a workgroup
constexpr int kFixThreads = kFixWave * kFixWaves;
constexpr int kFixPitch = kFixWave + 1;             // doubles between the rows of a wave's terms in LDS: lane q reads row q
constexpr int kFixWaveDoubles = kFixTerms * kFixPitch + 16; // a wave's LDS: the channels' terms and the sums
constexpr int kFixLdsBytes = kFixWaves * kFixWaveDoubles * (int)sizeof(double);

// The call as the entry points receive it.  The plan reads *cfg and nothing else behind a pointer.
struct FixCall {
    const void *eph, *tx_ms, *tx_frac, *rx_ms, *rx_frac;
    int E, K;
    const gat_fix_config *cfg;
    const void *fixes;
};

// Work units: workgroup g, wave w: epoch e = g * kFixWaves + w < E; lane k < K: channel k.
struct FixPlan {
    int E, K, max_iter;
    double tol_m, mask_sin, init_xyz[3];
    long long groups;
};

GAT_HD inline bool fix_epoch_unit(long long group, int wave, int E, int *e)
{
    const long long u = group * kFixWaves + wave;
    if (u >= E) return false;
    *e = (int)u;
    return true;
}

// The whole call.  *plan is written only with GAT_OK.
inline Refusal fix_plan(const FixCall &a, FixPlan *plan)
{
    const gat_fix_config *cfg = a.cfg;
    if (!a.eph || !a.tx_ms || !a.tx_frac || !a.rx_ms || !a.rx_frac || !cfg || !a.fixes || !plan) return {GAT_ERR_ARG, "null argument"};
    if (cfg->struct_size != sizeof(gat_fix_config)) return {GAT_ERR_ARG, "config.struct_size is not sizeof(gat_fix_config)"};
    if (a.E < 1 || a.K < 1) return {GAT_ERR_ARG, "num_epochs and num_channels must be positive"};
    if (cfg->max_iter < 1) return {GAT_ERR_ARG, "max_iter must be positive"};
    if (!(cfg->tol_m > 0.0)) return {GAT_ERR_ARG, "tol_m must be positive"};
    if (!fix_finite(cfg->mask_sin) || !fix_finite(cfg->init_xyz[0]) || !fix_finite(cfg->init_xyz[1]) || !fix_finite(cfg->init_xyz[2]))
        return {GAT_ERR_ARG, "mask_sin and init_xyz must be finite"};
    if (cfg->flags != 0 || cfg->reserved != 0) return {GAT_ERR_ARG, "flags must be 0"};
    if (a.K > GAT_MAX_FIX_CHANNELS) return {GAT_ERR_RANGE, "more than 64 channels"};
    if (a.E > GAT_MAX_FIX_EPOCHS) return {GAT_ERR_RANGE, "more than 2^24 epochs"};
    FixPlan p{};
    p.E = a.E, p.K = a.K, p.max_iter = cfg->max_iter, p.tol_m = cfg->tol_m, p.mask_sin = cfg->mask_sin;
    for (int i = 0; i < 3; ++i) p.init_xyz[i] = cfg->init_xyz[i];
    p.groups = ((long long)a.E + kFixWaves - 1) / kFixWaves;
    *plan = p;
    return {GAT_OK, nullptr};
}

// the public report
inline void fix_report(const FixPlan &p, gat_fix_plan *out)
{
    out->struct_size = sizeof(gat_fix_plan);
    out->workgroups = (int32_t)p.groups;
    out->waves_per_workgroup = kFixWaves;
    out->threads = kFixThreads;
    out->lds_bytes = kFixLdsBytes;
    out->reserved = 0;
    out->scratch_bytes = 0;
}

// ---- the host twin ----------------------------------------------------------------------------------------------------------------
// One epoch in plain loops over its K channels: what a wave of the kernel does, a channel where the kernel has a lane.  The state
// is a struct so that the integrity twin (gat_raim_plan.h) goes on from where the fix ends.
struct FixHostEpoch {
    int K, max_iter;
    double tol_m, mask_sin;
    FixSat s[GAT_MAX_FIX_CHANNELS];
    FixRow row[GAT_MAX_FIX_CHANNELS];
    double wk[GAT_MAX_FIX_CHANNELS], tau[GAT_MAX_FIX_CHANNELS], sel[GAT_MAX_FIX_CHANNELS];
    bool used[GAT_MAX_FIX_CHANNELS];
    int num_valid, num_used;
    double st[4];
    int status, iterations;
    double last_step;

    void init(const FixPlan &p, const gat_ephemeris *eph, const int32_t *tx_ms, const double *tx_frac, int32_t rx_ms, double rx_frac, const double *w)
    {
        K = p.K, max_iter = p.max_iter, tol_m = p.tol_m, mask_sin = p.mask_sin;
        num_valid = 0, num_used = 0;
        for (int k = 0; k < K; ++k) {
            s[k] = fix_sat(eph[k], tx_ms[k], tx_frac[k], rx_ms, rx_frac);
            wk[k] = w ? w[k] : 1.0;
            used[k] = s[k].ok && fix_weight_ok(wk[k]);
            tau[k] = kFixFirstTravel;
            row[k] = FixRow{0.0, 0.0, 0.0, 0.0, 0.0};
            sel[k] = 0.0;
            num_valid += s[k].ok ? 1 : 0;
            num_used += used[k] ? 1 : 0;
        }
        st[0] = p.init_xyz[0], st[1] = p.init_xyz[1], st[2] = p.init_xyz[2], st[3] = 0.0;
        status = 0, iterations = 0;
        last_step = 0.0;
    }
    // the rows of every counting channel at the state, each with its own travel time
    void rows()
    {
        for (int k = 0; k < K; ++k)
            if (s[k].ok) {
                row[k] = fix_row(s[k], tau[k], st);
                tau[k] = row[k].r / kFixC;
            }
    }
    // one pass over the used set; true: converged
    bool pass()
    {
        if (num_used < 4) {
            status |= GAT_FIX_FEW_SATS;
            return false;
        }
        for (int it = 0; it < max_iter; ++it) {
            rows();
            double sums[kFixTerms] = {};
            for (int k = 0; k < K; ++k) {
                if (!used[k]) continue;
                double t[kFixTerms];
                fix_terms(row[k], wk[k], t);
                for (int q = 0; q < kFixTerms; ++q) sums[q] += t[q];
            }
            double d[4];
            const int rc = fix_step(sums, d);
            if (rc) {
                status |= rc;
                return false;
            }
            for (int i = 0; i < 4; ++i) st[i] += d[i];
            last_step = __builtin_sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
            iterations += 1;
            if (last_step < tol_m) return true;
        }
        status |= GAT_FIX_NOT_CONVERGED;
        return false;
    }
    double elevations()
    {
        rows();
        const double radius = fix_radius(st);
        for (int k = 0; k < K; ++k) sel[k] = s[k].ok ? fix_sin_el(row[k], st, radius) : 0.0;
        return radius;
    }
    // the first pass, the mask and the second pass
    void solve()
    {
        const bool converged = pass();
        if (fix_failed(status)) return;
        const double radius = elevations();
        if (converged && mask_sin > -1.0 && radius >= kFixMaskRadius) {
            int kept = 0;
            for (int k = 0; k < K; ++k) kept += used[k] && sel[k] >= mask_sin ? 1 : 0;
            if (kept != num_used) {
                if (kept >= 4) {
                    for (int k = 0; k < K; ++k) used[k] = used[k] && sel[k] >= mask_sin;
                    num_used = kept;
                    status |= GAT_FIX_MASKED;
                    pass();
                    if (!fix_failed(status)) elevations();
                } else
                    status |= GAT_FIX_MASK_STARVED;
            }
        }
    }
    // the record and the channels' outputs of the state as it stands, `extra` status bits added
    void write(int extra, gat_fix *fix, double *sat, double *resid, double *sin_el, uint8_t *used_out) const
    {
        const bool failed = fix_failed(status);
        double sums[kFixTerms] = {};
        if (!failed)
            for (int k = 0; k < K; ++k) {
                if (!used[k]) continue;
                double t[kFixTerms];
                fix_terms(row[k], 1.0, t);
                t[10] = row[k].v * row[k].v;
                for (int q = 0; q < 11; ++q) sums[q] += t[q];
            }
        *fix = fix_record(status | extra, num_valid, num_used, iterations, st, sums[10], last_step, sums);
        for (int k = 0; k < K; ++k) {
            if (sat) sat[4 * k] = s[k].X, sat[4 * k + 1] = s[k].Y, sat[4 * k + 2] = s[k].Z, sat[4 * k + 3] = s[k].dts;
            if (resid) resid[k] = !failed && s[k].ok ? row[k].v : 0.0;
            if (sin_el) sin_el[k] = !failed ? sel[k] : 0.0;
            if (used_out) used_out[k] = (uint8_t)(!failed && used[k] ? 1 : 0);
        }
    }
};

inline void fix_host_epoch(const FixPlan &p, const gat_ephemeris *eph, const int32_t *tx_ms, const double *tx_frac, int32_t rx_ms, double rx_frac,
                           const double *w, gat_fix *fix, double *sat, double *resid, double *sin_el, uint8_t *used_out)
{
    FixHostEpoch h;
    h.init(p, eph, tx_ms, tx_frac, rx_ms, rx_frac, w);
    h.solve();
    h.write(0, fix, sat, resid, sin_el, used_out);
}

// The twin's loops (gat_position_fix_host) for a planned call, every pointer host memory.
inline void fix_host_run(const FixPlan &p, const gat_ephemeris *eph, const int32_t *tx_ms, const double *tx_frac, const int32_t *rx_ms,
                         const double *rx_frac, const double *w, gat_fix *fixes, double *sat, double *resid, double *sin_el, uint8_t *used)
{
    for (int e = 0; e < p.E; ++e) {
        const size_t o = (size_t)e * (size_t)p.K;
        fix_host_epoch(p, eph, tx_ms + o, tx_frac + o, rx_ms[e], rx_frac[e], w ? w + o : nullptr, fixes + e, sat ? sat + 4 * o : nullptr,
                       resid ? resid + o : nullptr, sin_el ? sin_el + o : nullptr, used ? used + o : nullptr);
    }
}

} // namespace gat
