// gat_smooth_plan.h -- the pure part of gat_smooth_observables (include/gat.h, "carrier smoothing"): its refusals, the work split and
// the scratch layout as a function of the call's arguments alone, and the host twin's loops over the rule of gat_smooth.h.  No HIP
// call and no HIP header: the device entry point, the host twin and a stand-alone test program (tests/smoothplan) compile the same
// text.
//
// The split.  The arrays are [E][K]: kSmChunk consecutive epochs are one contiguous span for all channels (K <= 64).  A workgroup
// of kSmThreads takes one chunk; it is rows x lanes, lanes the power of two that holds K, lane l holds channel l and row r walks the
// chunk's run r: lanes consecutive epochs (rows x lanes = kSmThreads = kSmChunk, so the runs tile the chunk).  The lanes of a row
// read consecutive elements; a thread keeps the epoch it read as the next one's predecessor, so every element is loaded once a pass.
// The output kernel is one thread an (epoch, channel), t = e K + k.
#pragma once

#include <vector>

#include "gat_smooth.h"
#include "gat_sig_plan.h" // Refusal

namespace gat {

constexpr int kSmThreads = 256;
constexpr int kSmChunk = 256; // epochs a chunk
constexpr int kSmWave = 64;
constexpr int kSmChanWaves = 4; // channels (waves) a workgroup of the channel kernel
constexpr long long kSmMaxScratch = 1ll << 30;
constexpr int kSmLdsBytes = kSmThreads * (int)sizeof(SmSeg);
constexpr uint32_t kSmFlags = GAT_SMOOTH_RATE_TEST;

// The call as the entry points receive it.  The plan reads *cfg and nothing else behind a pointer.
struct SmCall {
    SmIn in;
    int E, K;
    const gat_smooth_config *cfg;
    SmOut out;
};

struct SmPlan {
    SmRule rule;
    int E, K;
    int chunks, lanes, rows, run;
    long long cells, chan_groups, out_groups;
    // context scratch: the chunks' totals, then exclusive prefixes [chunks][K]; every thread's run [chunks][kSmThreads]; C and SS
    // [E][K]; the arc start of every measured (epoch, channel), -1 of the others [E][K]
    size_t off_totals, off_runs, off_C, off_SS, off_arc, bytes;
};

// thread t of a chunk's workgroup: the lane (channel) and the row (run of the chunk) it holds
GAT_HD inline void sm_thread(int lanes, int t, int *lane, int *row)
{
    *lane = t & (lanes - 1);
    *row = t / lanes;
}
// run r of chunk c: the epochs [*e0, *e1) (false: none)
GAT_HD inline bool sm_run(int E, int run, int c, int r, int *e0, int *e1)
{
    const long long lo = (long long)c * kSmChunk, hi = lo + kSmChunk < E ? lo + kSmChunk : E;
    const long long a = lo + (long long)r * run, b = a + run < hi ? a + run : hi;
    if (a >= b) return false;
    *e0 = (int)a, *e1 = (int)b;
    return true;
}
// the (epoch, channel) of thread `lane` of workgroup `group` of the output kernel; false: none
GAT_HD inline bool sm_unit(long long group, int lane, long long cells, int K, int *e, int *k)
{
    const long long t = group * kSmThreads + lane;
    if (t >= cells) return false;
    *e = (int)(t / K), *k = (int)(t % K);
    return true;
}

// The whole call.  *plan is written only with GAT_OK.
inline Refusal sm_plan(const SmCall &a, SmPlan *plan)
{
    const gat_smooth_config *cfg = a.cfg;
    const SmIn &in = a.in;
    if (!in.tx_ms || !in.tx_frac || !in.rx_ms || !in.rx_frac || !in.cycles || !in.cfrac || !cfg || !a.out.tx_frac_out || !plan)
        return {GAT_ERR_ARG, "null argument"};
    if (cfg->struct_size != sizeof(gat_smooth_config)) return {GAT_ERR_ARG, "config.struct_size is not sizeof(gat_smooth_config)"};
    if (a.E < 1 || a.K < 1) return {GAT_ERR_ARG, "num_epochs and num_channels must be positive"};
    if (cfg->flags & ~kSmFlags) return {GAT_ERR_ARG, "flags other than GAT_SMOOTH_RATE_TEST"};
    if (cfg->reserved != 0) return {GAT_ERR_ARG, "config.reserved must be 0"};
    const bool rate = (cfg->flags & GAT_SMOOTH_RATE_TEST) != 0;
    if (rate && !in.doppler) return {GAT_ERR_ARG, "the rate test needs doppler_hz"};
    if (!obs_finite(cfg->carrier_hz) || !(cfg->carrier_hz > 0.0)) return {GAT_ERR_ARG, "carrier_hz must be finite and positive"};
    if (!obs_finite(cfg->epoch_seconds) || !(cfg->epoch_seconds > 0.0)) return {GAT_ERR_ARG, "epoch_seconds must be finite and positive"};
    if (!obs_finite(cfg->if_hz)) return {GAT_ERR_ARG, "if_hz must be finite"};
    if (cfg->window < 1 || cfg->window > kSmMaxWindow) return {GAT_ERR_RANGE, "window outside 1 .. 65536"};
    if (!(cfg->cmc_gate_s > 0.0 && cfg->cmc_gate_s <= kSmMaxGate)) return {GAT_ERR_RANGE, "cmc_gate_s outside (0, 2^-18]"};
    if (rate && (!obs_finite(cfg->rate_gate_cycles) || !(cfg->rate_gate_cycles > 0.0))) return {GAT_ERR_RANGE, "rate_gate_cycles must be finite and positive"};
    if (a.K > GAT_MAX_FIX_CHANNELS) return {GAT_ERR_RANGE, "more than 64 channels"};
    if (a.E > GAT_MAX_SMOOTH_EPOCHS) return {GAT_ERR_RANGE, "more than 2^20 epochs"};

    SmPlan p{};
    SmRule &r = p.rule;
    r.flags = cfg->flags, r.W = cfg->window;
    r.carrier_hz = cfg->carrier_hz, r.if_cycles = cfg->if_hz * cfg->epoch_seconds, r.epoch_seconds = cfg->epoch_seconds;
    r.cmc_gate = cfg->cmc_gate_s, r.rate_gate = rate ? cfg->rate_gate_cycles : 0.0;
    p.E = a.E, p.K = a.K;
    p.chunks = (a.E + kSmChunk - 1) / kSmChunk;
    p.lanes = 1;
    while (p.lanes < a.K) p.lanes *= 2;
    p.rows = kSmThreads / p.lanes;
    p.run = kSmChunk / p.rows;
    p.cells = (long long)a.E * a.K;
    p.chan_groups = ((long long)a.K + kSmChanWaves - 1) / kSmChanWaves;
    p.out_groups = (p.cells + kSmThreads - 1) / kSmThreads;
    auto up = [](size_t v) { return (v + 15) & ~(size_t)15; };
    p.off_totals = 0;
    p.off_runs = up(p.off_totals + (size_t)p.chunks * (size_t)a.K * sizeof(SmSeg));
    p.off_C = up(p.off_runs + (size_t)p.chunks * kSmThreads * sizeof(SmSeg));
    p.off_SS = up(p.off_C + (size_t)p.cells * sizeof(uint64_t));
    p.off_arc = up(p.off_SS + (size_t)p.cells * sizeof(uint64_t));
    p.bytes = up(p.off_arc + (size_t)p.cells * sizeof(int32_t));
    if ((long long)p.bytes > kSmMaxScratch) return {GAT_ERR_RANGE, "the call's scratch would exceed 1 GiB"};
    *plan = p;
    return {GAT_OK, nullptr};
}

// the public report
inline void sm_report(const SmPlan &p, gat_smooth_plan *out)
{
    out->struct_size = sizeof(gat_smooth_plan);
    out->chunk_epochs = kSmChunk, out->num_chunks = p.chunks;
    out->lanes = p.lanes, out->rows = p.rows, out->run_epochs = p.run;
    out->threads = kSmThreads, out->lds_bytes = kSmLdsBytes;
    out->chunk_workgroups = p.chunks;
    out->channel_workgroups = (int32_t)p.chan_groups;
    out->output_workgroups = (int32_t)p.out_groups;
    out->reserved = 0;
    out->scratch_bytes = (int64_t)p.bytes;
}

// ---- the host twin --------------------------------------------------------------------------------------------------------------------
// One channel in plain loops: the three scans over all epochs, then the outputs.  C, SS, arc: E entries each.
inline void sm_host_channel(const SmPlan &p, const SmIn &in, const SmOut &out, int k, uint64_t *C, uint64_t *SS, int32_t *arc)
{
    const SmRule &r = p.rule;
    SmSeg all = sm_empty();
    SmEpoch prev{};
    for (int e = 0; e < p.E; ++e) {
        const SmEpoch cur = sm_load(r, in, p.K, e, k);
        int64_t q;
        const int st = sm_step(r, e == 0, prev, cur, &q);
        sm_push(&all, e, q, st);
        C[e] = all.Q, SS[e] = all.S, arc[e] = cur.measured ? all.reset : -1;
        if (out.status) out.status[(size_t)e * (size_t)p.K + (size_t)k] = (uint8_t)st;
        prev = cur;
    }
    if (out.channels) out.channels[k] = gat_smooth_channel{all.cnt[0], all.cnt[1], all.cnt[2], all.cnt[3]};
    for (int e = 0; e < p.E; ++e) {
        const size_t o = (size_t)e * (size_t)p.K + (size_t)k;
        const int a = arc[e];
        const int back = a < 0 ? -1 : e - sm_count(r, e, a);
        sm_emit(r, out, o, e, in.tx_frac[o], a, C[e], SS[e], back >= 0 ? SS[back] : 0, a < 0 ? 0 : C[a]);
    }
}

// The twin's loops (gat_smooth_observables_host) for a planned call, every pointer host memory.
inline void sm_host_run(const SmPlan &p, const SmIn &in, const SmOut &out)
{
    std::vector<uint64_t> C((size_t)p.E), SS((size_t)p.E);
    std::vector<int32_t> arc((size_t)p.E);
    for (int k = 0; k < p.K; ++k) sm_host_channel(p, in, out, k, C.data(), SS.data(), arc.data());
}

} // namespace gat
