// gat_vel_plan.h -- the pure part of gat_velocity_fix (include/gat.h, "velocity fix"): its refusals and the launch geometry as a
// function of the call's arguments alone, and the host twin's loops over the rules of gat_fix.h and gat_vel.h.  No HIP call and no
// HIP header: the device entry point, the host twin and a stand-alone test program (tests/velplan) compile the same text.
#pragma once

#include "gat_fix_plan.h"
#include "gat_vel.h"

namespace gat {

// The call as the entry points receive it.  The plan reads *cfg and nothing else behind a pointer.
struct VelCall {
    const void *eph, *tx_ms, *tx_frac, *doppler, *fixes;
    int E, K;
    const gat_vel_config *cfg;
    const void *velocities;
};

// Work units: the fix's (workgroup g, wave w: epoch g * kFixWaves + w < E; lane k < K: channel k); the wave's LDS is the fix's.
struct VelPlan {
    int E, K;
    double lambda; // c / carrier_hz, m
    long long groups;
};

// The whole call.  *plan is written only with GAT_OK.
inline Refusal vel_plan(const VelCall &a, VelPlan *plan)
{
    const gat_vel_config *cfg = a.cfg;
    if (!a.eph || !a.tx_ms || !a.tx_frac || !a.doppler || !a.fixes || !cfg || !a.velocities || !plan) return {GAT_ERR_ARG, "null argument"};
    if (cfg->struct_size != sizeof(gat_vel_config)) return {GAT_ERR_ARG, "config.struct_size is not sizeof(gat_vel_config)"};
    if (a.E < 1 || a.K < 1) return {GAT_ERR_ARG, "num_epochs and num_channels must be positive"};
    if (cfg->flags != 0) return {GAT_ERR_ARG, "flags must be 0"};
    if (!fix_finite(cfg->carrier_hz) || !(cfg->carrier_hz > 0.0)) return {GAT_ERR_ARG, "carrier_hz must be finite and positive"};
    if (a.K > GAT_MAX_FIX_CHANNELS) return {GAT_ERR_RANGE, "more than 64 channels"};
    if (a.E > GAT_MAX_FIX_EPOCHS) return {GAT_ERR_RANGE, "more than 2^24 epochs"};
    VelPlan p{};
    p.E = a.E, p.K = a.K;
    p.lambda = kFixC / cfg->carrier_hz;
    p.groups = ((long long)a.E + kFixWaves - 1) / kFixWaves;
    *plan = p;
    return {GAT_OK, nullptr};
}

// the public report: the fix's geometry and LDS
inline void vel_report(const VelPlan &p, gat_fix_plan *out)
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
// One epoch in plain loops over its K channels: what a wave of the kernel does, a channel where the kernel has a lane.
// used_in, w, sat_vel, resid: null where not given / not asked for.
inline void vel_host_epoch(const VelPlan &p, const gat_ephemeris *eph, const int32_t *tx_ms, const double *tx_frac, const double *doppler,
                           const gat_fix &fix, const uint8_t *used_in, const double *w, gat_velocity *vel, double *sat_vel, double *resid)
{
    const int K = p.K;
    const double zero[4] = {0.0, 0.0, 0.0, 0.0};
    if (!vel_fix_given(fix)) {
        *vel = vel_record(GAT_VEL_NO_FIX, 0, 0, zero, 0.0, zero);
        for (int k = 0; k < K; ++k) {
            if (sat_vel) sat_vel[4 * k] = 0.0, sat_vel[4 * k + 1] = 0.0, sat_vel[4 * k + 2] = 0.0, sat_vel[4 * k + 3] = 0.0;
            if (resid) resid[k] = 0.0;
        }
        return;
    }
    const double st[4] = {fix.x, fix.y, fix.z, kFixC * fix.clock_bias_s};
    VelSat c[GAT_MAX_FIX_CHANNELS];
    FixRow row[GAT_MAX_FIX_CHANNELS];
    double wk[GAT_MAX_FIX_CHANNELS];
    bool used[GAT_MAX_FIX_CHANNELS];
    int num_valid = 0, num_used = 0;
    for (int k = 0; k < K; ++k) {
        c[k] = vel_sat(eph[k], tx_ms[k], tx_frac[k], doppler[k]);
        wk[k] = w ? w[k] : 1.0;
        used[k] = c[k].s.ok && fix_weight_ok(wk[k]) && (!used_in || used_in[k] != 0);
        row[k] = FixRow{0.0, 0.0, 0.0, 0.0, 0.0};
        num_valid += c[k].s.ok ? 1 : 0;
        num_used += used[k] ? 1 : 0;
    }
    int status = 0;
    double s[4] = {0.0, 0.0, 0.0, 0.0}, sum_v2 = 0.0;
    if (num_used < 4)
        status |= GAT_VEL_FEW_SATS;
    else {
        double sums[kFixTerms] = {};
        for (int k = 0; k < K; ++k) {
            if (c[k].s.ok) row[k] = vel_row(c[k], st, p.lambda);
            if (!used[k]) continue;
            double t[kFixTerms];
            fix_terms(row[k], wk[k], t);
            for (int q = 0; q < kFixTerms; ++q) sums[q] += t[q];
        }
        status |= fix_step(sums, s);
    }
    const bool failed = vel_failed(status);
    double v[GAT_MAX_FIX_CHANNELS];
    for (int k = 0; k < K; ++k) {
        v[k] = !failed && c[k].s.ok ? vel_resid(row[k], s) : 0.0;
        if (used[k]) sum_v2 += v[k] * v[k];
    }
    *vel = vel_record(status, num_valid, num_used, s, sum_v2, st);
    for (int k = 0; k < K; ++k) {
        if (sat_vel) sat_vel[4 * k] = c[k].vx, sat_vel[4 * k + 1] = c[k].vy, sat_vel[4 * k + 2] = c[k].vz, sat_vel[4 * k + 3] = c[k].ddts;
        if (resid) resid[k] = v[k];
    }
}

// The twin's loops (gat_velocity_fix_host) for a planned call, every pointer host memory.
inline void vel_host_run(const VelPlan &p, const gat_ephemeris *eph, const int32_t *tx_ms, const double *tx_frac, const double *doppler,
                         const gat_fix *fixes, const uint8_t *used, const double *w, gat_velocity *vel, double *sat_vel, double *resid)
{
    for (int e = 0; e < p.E; ++e) {
        const size_t o = (size_t)e * (size_t)p.K;
        vel_host_epoch(p, eph, tx_ms + o, tx_frac + o, doppler + o, fixes[e], used ? used + o : nullptr, w ? w + o : nullptr, vel + e,
                       sat_vel ? sat_vel + 4 * o : nullptr, resid ? resid + o : nullptr);
    }
}

} // namespace gat
