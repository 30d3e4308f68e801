// gat_snap_plan.h -- the pure part of gat_snapshot_fix (include/gat.h, "snapshot fix"): its refusals and the launch geometry as a
// function of the call's arguments alone, and the host twin's loops over the rule of gat_snap.h.  No HIP call and no HIP header:
// the device entry point, the host twin and a stand-alone test program (tests/snapplan) compile the same text.
#pragma once

#include "gat_fix_plan.h"
#include "gat_snap.h"

namespace gat {

// The fix's geometry (a wave an epoch, a lane a channel, kFixWaves epochs a workgroup) with a wave's LDS for 20 terms.
constexpr int kSnapPitch = kFixWave + 1;                        // doubles between the rows of a wave's terms in LDS
constexpr int kSnapSumsAt = kSnapTerms * kSnapPitch;            // where the wave's sums stand
constexpr int kSnapWaveDoubles = kSnapSumsAt + 32;
constexpr int kSnapLdsBytes = kFixWaves * kSnapWaveDoubles * (int)sizeof(double);

// The call as the entry points receive it.  The plan reads *cfg and nothing else behind a pointer.
struct SnapCall {
    const void *eph, *code_frac, *rx_ms, *rx_frac;
    int E, K;
    const gat_snap_config *cfg;
    const void *fixes;
};

// Work units: the fix's (workgroup g, wave w: epoch g * kFixWaves + w < E; lane k < K: channel k).
struct SnapPlan {
    int E, K, max_iter;
    double tol_m, mask_sin, init_xyz[3], margin;
    long long groups;
};

// The whole call.  *plan is written only with GAT_OK.
inline Refusal snap_plan(const SnapCall &a, SnapPlan *plan)
{
    const gat_snap_config *cfg = a.cfg;
    if (!a.eph || !a.code_frac || !a.rx_ms || !a.rx_frac || !cfg || !a.fixes || !plan) return {GAT_ERR_ARG, "null argument"};
    if (cfg->struct_size != sizeof(gat_snap_config)) return {GAT_ERR_ARG, "config.struct_size is not sizeof(gat_snap_config)"};
    if (a.E < 1 || a.K < 1) return {GAT_ERR_ARG, "num_epochs and num_channels must be positive"};
    if (cfg->max_iter < 1) return {GAT_ERR_ARG, "max_iter must be positive"};
    if (!(cfg->tol_m > 0.0)) return {GAT_ERR_ARG, "tol_m must be positive"};
    if (!fix_finite(cfg->mask_sin) || !fix_finite(cfg->init_xyz[0]) || !fix_finite(cfg->init_xyz[1]) || !fix_finite(cfg->init_xyz[2]))
        return {GAT_ERR_ARG, "mask_sin and init_xyz must be finite"};
    if (!(cfg->ambiguity_margin >= 0.0 && cfg->ambiguity_margin <= 0.5)) return {GAT_ERR_ARG, "ambiguity_margin must lie in [0, 0.5]"};
    if (cfg->flags != 0 || cfg->reserved != 0) return {GAT_ERR_ARG, "flags must be 0"};
    if (a.K > GAT_MAX_FIX_CHANNELS) return {GAT_ERR_RANGE, "more than 64 channels"};
    if (a.E > GAT_MAX_FIX_EPOCHS) return {GAT_ERR_RANGE, "more than 2^24 epochs"};
    SnapPlan p{};
    p.E = a.E, p.K = a.K, p.max_iter = cfg->max_iter, p.tol_m = cfg->tol_m, p.mask_sin = cfg->mask_sin, p.margin = cfg->ambiguity_margin;
    for (int i = 0; i < 3; ++i) p.init_xyz[i] = cfg->init_xyz[i];
    p.groups = ((long long)a.E + kFixWaves - 1) / kFixWaves;
    *plan = p;
    return {GAT_OK, nullptr};
}

// the public report: the fix's geometry, the snapshot fix's LDS
inline void snap_report(const SnapPlan &p, gat_fix_plan *out)
{
    out->struct_size = sizeof(gat_fix_plan);
    out->workgroups = (int32_t)p.groups;
    out->waves_per_workgroup = kFixWaves;
    out->threads = kFixThreads;
    out->lds_bytes = kSnapLdsBytes;
    out->reserved = 0;
    out->scratch_bytes = 0;
}

// ---- the host twin ----------------------------------------------------------------------------------------------------------------
// One epoch in plain loops over its K channels: what a wave of the kernel does, a channel where the kernel has a lane.
struct SnapHostEpoch {
    int K, max_iter;
    double tol_m, mask_sin, margin;
    const gat_ephemeris *eph;
    int32_t rx_ms;
    double R;
    SnapChan c[GAT_MAX_FIX_CHANNELS];
    int num_valid, num_used;
    double st[kSnapUnknowns];
    int status, iterations;
    double last_step;

    void init(const SnapPlan &p, const gat_ephemeris *eph_, const double *code_frac, int32_t rx_ms_, double rx_frac, const double *xyz, const double *w)
    {
        K = p.K, max_iter = p.max_iter, tol_m = p.tol_m, mask_sin = p.mask_sin, margin = p.margin;
        eph = eph_, rx_ms = rx_ms_;
        R = fix_seconds(rx_ms_, rx_frac);
        for (int k = 0; k < K; ++k) c[k] = snap_measure(eph[k], code_frac[k], rx_ms_, rx_frac, w ? w[k] : 1.0);
        st[0] = xyz[0], st[1] = xyz[1], st[2] = xyz[2], st[3] = 0.0, st[4] = 0.0;
        num_valid = 0, num_used = 0, status = 0, iterations = 0;
        last_step = 0.0;
    }
    // steps 2 and 3 at the state; first: the usable and the used set are made.  True: a used channel's whole milliseconds changed.
    bool resolve(bool first)
    {
        const double radius = fix_radius(st);
        double rows[4 * kSnapPitch];
        for (int k = 0; k < K; ++k) {
            if (c[k].ok) snap_predict(c[k], eph[k], R, st, radius);
            if (first) {
                c[k].ok = c[k].ok && snap_predicted(c[k]);
                c[k].used = c[k].ok && fix_weight_ok(c[k].w);
                num_valid += c[k].ok ? 1 : 0;
                num_used += c[k].used ? 1 : 0;
            }
            rows[k] = c[k].used ? 1.0 : 0.0, rows[kSnapPitch + k] = c[k].sel, rows[2 * kSnapPitch + k] = c[k].p, rows[3 * kSnapPitch + k] = c[k].z;
        }
        if (num_used < kSnapMinSats) {
            status |= GAT_SNAP_FEW_SATS;
            return false;
        }
        const SnapRef r = snap_reference(rows, kSnapPitch, K);
        double n[GAT_MAX_FIX_CHANNELS] = {};
        bool good = r.good;
        for (int k = 0; k < K && good; ++k) {
            if (c[k].ok) good = snap_integer(c[k], r, &n[k]);
        }
        if (!good) {
            status |= GAT_SNAP_NONFINITE;
            return false;
        }
        bool changed = false;
        for (int k = 0; k < K; ++k) {
            if (!c[k].ok) continue;
            if (c[k].used && snap_ambiguous(c[k].q, n[k], margin)) status |= GAT_SNAP_AMBIGUOUS;
            changed = changed || (c[k].used && (int)n[k] != c[k].n);
            c[k].n = (int)n[k];
        }
        return changed;
    }
    void rows()
    {
        for (int k = 0; k < K; ++k)
            if (c[k].ok) snap_eval(c[k], eph[k], rx_ms, st);
    }
    // one pass over the used set; true: converged
    bool pass()
    {
        for (int it = 0; it < max_iter; ++it) {
            rows();
            double sums[kSnapTerms] = {};
            for (int k = 0; k < K; ++k) {
                if (!c[k].used) continue;
                double t[kSnapTerms];
                snap_terms(c[k], c[k].w, t);
                for (int q = 0; q < kSnapTerms; ++q) sums[q] += t[q];
            }
            double d[kSnapUnknowns];
            const int rc = snap_step(sums, d);
            if (rc) {
                status |= rc;
                return false;
            }
            for (int i = 0; i < kSnapUnknowns; ++i) st[i] += d[i];
            last_step = __builtin_sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
            iterations += 1;
            if (last_step < tol_m) return true;
        }
        status |= GAT_SNAP_NOT_CONVERGED;
        return false;
    }
    double elevations()
    {
        rows();
        const double radius = fix_radius(st);
        for (int k = 0; k < K; ++k) c[k].sel = c[k].ok ? fix_sin_el(c[k].row, st, radius) : 0.0;
        return radius;
    }
    // the resolution, the first pass, the resolution again, the mask
    void solve()
    {
        resolve(true);
        if (snap_failed(status)) return;
        bool converged = pass();
        if (snap_failed(status)) return;
        if (converged) {
            const bool changed = resolve(false);
            if (snap_failed(status)) return;
            if (changed) {
                status |= GAT_SNAP_RERESOLVED;
                converged = pass();
                if (snap_failed(status)) return;
            }
        }
        const double radius = elevations();
        if (converged && mask_sin > -1.0 && radius >= kFixMaskRadius) {
            int kept = 0;
            for (int k = 0; k < K; ++k) kept += c[k].used && c[k].sel >= mask_sin ? 1 : 0;
            if (kept != num_used) {
                if (kept >= kSnapMinSats) {
                    for (int k = 0; k < K; ++k) c[k].used = c[k].used && c[k].sel >= mask_sin;
                    num_used = kept;
                    status |= GAT_SNAP_MASKED;
                    pass();
                    if (!snap_failed(status)) elevations();
                } else
                    status |= GAT_SNAP_MASK_STARVED;
            }
        }
    }
    void write(gat_snap_fix *fix, int32_t *tx_ms, int32_t *rx_ms_out, int32_t *n_ms, double *resid, double *sin_el, uint8_t *used_out) const
    {
        const bool failed = snap_failed(status);
        double sums[kSnapTerms] = {};
        if (!failed)
            for (int k = 0; k < K; ++k) {
                if (!c[k].used) continue;
                double t[kSnapTerms];
                snap_terms(c[k], 1.0, t);
                t[15] = c[k].row.v * c[k].row.v;
                for (int q = 0; q < 16; ++q) sums[q] += t[q];
            }
        *fix = snap_record(status, num_valid, num_used, iterations, st, sums[15], last_step, sums);
        const int64_t m = snap_shift_ms(st[4]);
        if (rx_ms_out) *rx_ms_out = failed ? -1 : snap_week_ms((int64_t)rx_ms - m);
        for (int k = 0; k < K; ++k) {
            const bool has = !failed && c[k].ok;
            if (tx_ms) tx_ms[k] = has ? snap_tx_ms(rx_ms, c[k], m) : -1;
            if (n_ms) n_ms[k] = has ? c[k].n : 0;
            if (resid) resid[k] = has ? c[k].row.v : 0.0;
            if (sin_el) sin_el[k] = has ? c[k].sel : 0.0;
            if (used_out) used_out[k] = (uint8_t)(!failed && c[k].used ? 1 : 0);
        }
    }
};

// The twin's loops (gat_snapshot_fix_host) for a planned call, every pointer host memory.
inline void snap_host_run(const SnapPlan &p, const gat_ephemeris *eph, const double *code_frac, const int32_t *rx_ms, const double *rx_frac,
                          const double *prior, const double *w, gat_snap_fix *fixes, int32_t *tx_ms, int32_t *rx_ms_out, int32_t *n_ms, double *resid,
                          double *sin_el, uint8_t *used)
{
    for (int e = 0; e < p.E; ++e) {
        const size_t o = (size_t)e * (size_t)p.K;
        SnapHostEpoch h;
        h.init(p, eph, code_frac + o, rx_ms[e], rx_frac[e], prior ? prior + 3 * (size_t)e : p.init_xyz, w ? w + o : nullptr);
        h.solve();
        h.write(fixes + e, tx_ms ? tx_ms + o : nullptr, rx_ms_out ? rx_ms_out + e : nullptr, n_ms ? n_ms + o : nullptr, resid ? resid + o : nullptr,
                sin_el ? sin_el + o : nullptr, used ? used + o : nullptr);
    }
}

} // namespace gat
