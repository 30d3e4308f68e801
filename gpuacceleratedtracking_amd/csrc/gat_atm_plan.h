// gat_atm_plan.h -- the pure part of gat_range_corrections (include/gat.h, "atmosphere"): its refusals and the launch geometry as a
// function of the call's arguments alone, and the host twin's loops over the rules of gat_fix.h, gat_vel.h and gat_atm.h.  No HIP call
// and no HIP header: the device entry point, the host twin and a stand-alone test program (tests/atmplan) compile the same text.
#pragma once

#include "gat_fix_plan.h"
#include "gat_atm.h"

namespace gat {

constexpr int kAtmThreads = 256; // a thread an (epoch, channel)
constexpr uint32_t kAtmFlags = GAT_ATM_IONO | GAT_ATM_TROPO;

// The call as the entry points receive it.  The plan reads *cfg and nothing else behind a pointer.
struct AtmCall {
    const void *eph, *tx_ms, *tx_frac, *rx_ms, *rx_frac, *fixes;
    int E, K;
    const gat_atm_config *cfg;
    const void *tx_frac_out;
};

// Work units: thread t = g * kAtmThreads + lane < E * K is epoch t / K, channel t % K.
struct AtmPlan {
    int E, K;
    AtmParams prm;
    long long cells; // E * K
    long long groups;
};
// the (epoch, channel) of thread `lane` of workgroup `group`; false: none
GAT_HD inline bool atm_unit(long long group, int lane, long long cells, int K, int *e, int *k)
{
    const long long t = group * kAtmThreads + lane;
    if (t >= cells) return false;
    *e = (int)(t / K), *k = (int)(t % K);
    return true;
}

// The whole call.  *plan is written only with GAT_OK.
inline Refusal atm_plan(const AtmCall &a, AtmPlan *plan)
{
    const gat_atm_config *cfg = a.cfg;
    if (!a.eph || !a.tx_ms || !a.tx_frac || !a.rx_ms || !a.rx_frac || !a.fixes || !cfg || !a.tx_frac_out || !plan) return {GAT_ERR_ARG, "null argument"};
    if (cfg->struct_size != sizeof(gat_atm_config)) return {GAT_ERR_ARG, "config.struct_size is not sizeof(gat_atm_config)"};
    if (a.E < 1 || a.K < 1) return {GAT_ERR_ARG, "num_epochs and num_channels must be positive"};
    if (cfg->flags & ~kAtmFlags) return {GAT_ERR_ARG, "flags other than GAT_ATM_IONO and GAT_ATM_TROPO"};
    if (!fix_finite(cfg->carrier_hz) || !(cfg->carrier_hz > 0.0)) return {GAT_ERR_ARG, "carrier_hz must be finite and positive"};
    if (!fix_finite(cfg->floor_sin)) return {GAT_ERR_ARG, "floor_sin must be finite"};
    if (a.K > GAT_MAX_FIX_CHANNELS) return {GAT_ERR_RANGE, "more than 64 channels"};
    if (a.E > GAT_MAX_FIX_EPOCHS) return {GAT_ERR_RANGE, "more than 2^24 epochs"};
    AtmPlan p{};
    p.E = a.E, p.K = a.K;
    p.prm.flags = cfg->flags, p.prm.floor_sin = cfg->floor_sin;
    const double ratio = kAtmL1 / cfg->carrier_hz;
    p.prm.scale = ratio * ratio;
    for (int i = 0; i < 4; ++i) p.prm.alpha[i] = cfg->alpha[i], p.prm.beta[i] = cfg->beta[i];
    p.prm.zd = cfg->zenith_dry_m, p.prm.zw = cfg->zenith_wet_m;
    p.cells = (long long)a.E * a.K;
    p.groups = (p.cells + kAtmThreads - 1) / kAtmThreads;
    *plan = p;
    return {GAT_OK, nullptr};
}

// the public report: no LDS, no scratch
inline void atm_report(const AtmPlan &p, gat_fix_plan *out)
{
    out->struct_size = sizeof(gat_fix_plan);
    out->workgroups = (int32_t)p.groups;
    out->waves_per_workgroup = kAtmThreads / kFixWave;
    out->threads = kAtmThreads;
    out->lds_bytes = 0;
    out->reserved = 0;
    out->scratch_bytes = 0;
}

// One (epoch, channel) from the call's arrays to its outputs: what a thread of the kernel does and what the twin does in its loops.
// zenith, delay, geom, ch_status, ep_status: null where not given / not asked for.
GAT_HD inline void atm_cell(const AtmParams &prm, int K, int e, int k, const gat_ephemeris *eph, const int32_t *tx_ms, const double *tx_frac,
                            const int32_t *rx_ms, const double *rx_frac, const gat_fix *fixes, const double *zenith, double *tx_frac_out,
                            double *delay, double *geom, uint8_t *ch_status, int32_t *ep_status)
{
    const size_t o = (size_t)e * (size_t)K + (size_t)k;
    const AtmEpoch ep = atm_epoch(fixes[e]);
    const double zd = zenith ? zenith[2 * (size_t)e] : prm.zd, zw = zenith ? zenith[2 * (size_t)e + 1] : prm.zw;
    const AtmChannel c = atm_channel(prm, ep, eph[k], tx_ms[o], tx_frac[o], rx_ms[e], rx_frac[e], zd, zw);
    tx_frac_out[o] = c.tx_frac;
    if (delay) delay[2 * o] = c.iono, delay[2 * o + 1] = c.tropo;
    if (geom) geom[3 * o] = c.sin_el, geom[3 * o + 1] = c.cos_a, geom[3 * o + 2] = c.sin_a;
    if (ch_status) ch_status[o] = c.status;
    if (ep_status && k == 0) ep_status[e] = ep.status;
}

// The twin's loops (gat_range_corrections_host) for a planned call, every pointer host memory.
inline void atm_host_run(const AtmPlan &p, const gat_ephemeris *eph, const int32_t *tx_ms, const double *tx_frac, const int32_t *rx_ms,
                         const double *rx_frac, const gat_fix *fixes, const double *zenith, double *tx_frac_out, double *delay, double *geom,
                         uint8_t *ch_status, int32_t *ep_status)
{
    for (int e = 0; e < p.E; ++e)
        for (int k = 0; k < p.K; ++k)
            atm_cell(p.prm, p.K, e, k, eph, tx_ms, tx_frac, rx_ms, rx_frac, fixes, zenith, tx_frac_out, delay, geom, ch_status, ep_status);
}

} // namespace gat
