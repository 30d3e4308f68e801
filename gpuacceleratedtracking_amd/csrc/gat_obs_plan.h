// gat_obs_plan.h -- the pure part of gat_observables (include/gat.h): its refusals, the work split and the scratch layout as a
// function of the call's arguments alone, and the host twin's loops over the rule of gat_obs.h.  No HIP call and no HIP header: the
// device entry point, the host twin and a stand-alone test program (tests/obsplan) compile the same text.
//
// The split.  The history is [B + 1][K]: kObsChunk consecutive blocks are one contiguous span for all channels.  A workgroup of
// kObsThreads takes one chunk and one group of at most kObsThreads consecutive channels; it is rows x lanes, lanes the power of two
// that holds the group, lane l holds channel l of the group and row r walks the chunk's run r: lanes consecutive blocks (rows x
// lanes = kObsThreads = kObsChunk, so the runs tile the chunk).  The lanes of a row read consecutive records; a thread keeps the
// record it read as the next block's predecessor, so every record is loaded once a pass.
#pragma once

#include <vector>

#include "gat_obs.h"
#include "gat_sig_plan.h" // Refusal

namespace gat {

constexpr int kObsThreads = 256;
constexpr int kObsChunk = 256;       // blocks a chunk
constexpr int kObsWave = 64;
constexpr int kObsChanWaves = 4;     // channels (waves) a workgroup of the channel kernel
constexpr long long kObsMaxScratch = 1ll << 30;

struct ObsSum {
    int64_t w, c;
};
constexpr int kObsLdsBytes = kObsThreads * ((int)sizeof(ObsSum) + (int)sizeof(int32_t));

// The call as the entry points receive it.  The plan reads *cfg and nothing else behind a pointer.
struct ObsCall {
    const void *history, *mon, *nav, *frames;
    int B, K, E;
    const gat_obs_config *cfg;
    ObsOut out;
};

struct ObsPlan {
    ObsRule rule;
    int chunks, group, groups, lanes, rows, run;
    long long chunk_groups, chan_groups;
    // context scratch: the chunks' totals, then exclusive prefixes [chunks][K]; their bad flags [chunks][K]; every thread's run sums
    // [chunks][groups][kObsThreads]; the resolved channels [K]; the anchor
    size_t off_totals, off_bad, off_runs, off_chan, off_anchor, bytes;
};

// thread t of a (chunk, group) workgroup: the lane (channel of the group) and the row (run of the chunk) it holds
GAT_HD inline void obs_thread(int lanes, int t, int *lane, int *row)
{
    *lane = t & (lanes - 1);
    *row = t / lanes;
}
// workgroup wg of the sum and epoch kernels: its chunk and its channel group
GAT_HD inline void obs_workgroup(int groups, long long wg, int *chunk, int *gi)
{
    *chunk = (int)(wg / groups);
    *gi = (int)(wg % groups);
}
// run r of chunk c: the blocks [*i0, *i1) (false: none), for which this thread forms the wraps
GAT_HD inline bool obs_run(int B, int run, int c, int r, long long *i0, long long *i1)
{
    const long long lo = (long long)c * kObsChunk, hi = lo + kObsChunk < B ? lo + kObsChunk : B;
    const long long a = lo + (long long)r * run, b = a + run < hi ? a + run : hi;
    if (a >= b) return false;
    *i0 = a, *i1 = b;
    return true;
}
// the chunk whose span holds the wraps below record i (0 <= i <= B)
GAT_HD inline int obs_chunk_of(int chunks, long long i)
{
    const long long c = i / kObsChunk;
    return c < chunks ? (int)c : chunks - 1;
}
GAT_HD inline int obs_group_channels(int K, int group, int gi)
{
    const int k0 = gi * group;
    return K - k0 < group ? K - k0 : group;
}

// The whole call.  *plan is written only with GAT_OK.
inline Refusal obs_plan(const ObsCall &a, ObsPlan *plan)
{
    const gat_obs_config *cfg = a.cfg;
    if (!a.history || !a.mon || !a.nav || !a.frames || !cfg || !plan) return {GAT_ERR_ARG, "null argument"};
    if (cfg->struct_size != sizeof(gat_obs_config)) return {GAT_ERR_ARG, "config.struct_size is not sizeof(gat_obs_config)"};
    if (cfg->format != GAT_NAV_LNAV && cfg->format != GAT_NAV_CNAV) return {GAT_ERR_ARG, "unknown format"};
    if (cfg->rx_mode != GAT_OBS_RX_GIVEN && cfg->rx_mode != GAT_OBS_RX_FROM_TX) return {GAT_ERR_ARG, "unknown rx_mode"};
    if (a.B < 1 || a.K < 1 || a.E < 1) return {GAT_ERR_ARG, "num_blocks, num_channels and num_epochs must be positive"};
    if (cfg->symbol_blocks < 1 || cfg->max_frames < 1 || cfg->epoch_stride < 1) return {GAT_ERR_ARG, "symbol_blocks, max_frames and epoch_stride must be positive"};
    if (cfg->epoch_first < 0) return {GAT_ERR_ARG, "epoch_first must not be negative"};
    if ((long long)cfg->epoch_first + (long long)(a.E - 1) * cfg->epoch_stride > a.B) return {GAT_ERR_ARG, "an epoch lies beyond the last record"};
    if (!(cfg->edge_margin >= 0.0 && cfg->edge_margin <= 0.5)) return {GAT_ERR_ARG, "edge_margin must lie in [0, 0.5]"};
    if (!(cfg->block_seconds > 0.0) || !obs_finite(cfg->block_seconds) || cfg->block_samples < 1) return {GAT_ERR_ARG, "block_seconds and block_samples must be positive"};
    const ObsOut &o = a.out;
    if (!o.tx_ms && !o.tx_frac && !o.rx_ms && !o.rx_frac && !o.carrier_cycles && !o.carrier_frac && !o.doppler_hz && !o.code_rate_hz && !o.channels)
        return {GAT_ERR_ARG, "every output is null"};
    if (cfg->travel_ms < 0 || cfg->travel_ms > 1000) return {GAT_ERR_RANGE, "travel_ms outside 0 .. 1000"};
    if (cfg->rx_mode == GAT_OBS_RX_GIVEN && (cfg->rx0_ms < 0 || cfg->rx0_ms >= kObsWeekMs || !(cfg->rx0_frac >= 0.0 && cfg->rx0_frac < 1e-3)))
        return {GAT_ERR_RANGE, "rx0 outside a week's milliseconds or [0, 1e-3)"};
    if (a.K > GAT_MAX_MONITOR_CHANNELS) return {GAT_ERR_RANGE, "more than 4096 channels"};
    if (a.B > GAT_MAX_MONITOR_BLOCKS) return {GAT_ERR_RANGE, "more than 2^20 blocks"};
    if (cfg->code_length < 1 || (double)cfg->code_length * 1000.0 != cfg->code_freq_nominal_hz) return {GAT_ERR_RANGE, "the code period must be 1 ms"};
    const double fs = cfg->sampling_freq_hz;
    if (!(fs >= 1.0 && fs <= 0x1p40) || fs != __builtin_rint(fs)) return {GAT_ERR_RANGE, "sampling_freq_hz must be a whole number in 1 .. 2^40"};
    if ((long long)a.B * cfg->block_samples >= (1ll << 62) / 1000) return {GAT_ERR_RANGE, "num_blocks * block_samples * 1000 must stay below 2^62"};
    if (!obs_finite(cfg->if_hz)) return {GAT_ERR_RANGE, "if_hz must be finite"};

    ObsPlan p{};
    ObsRule &r = p.rule;
    r.P = cfg->format == GAT_NAV_CNAV ? 2 : 1;
    r.full_status = cfg->format == GAT_NAV_CNAV ? 0x3 : 0x7ff;
    r.Pd = cfg->symbol_blocks, r.max_frames = cfg->max_frames, r.min_tow_steps = cfg->min_tow_steps;
    r.rx_mode = cfg->rx_mode, r.travel_ms = cfg->travel_ms, r.rx0_ms = cfg->rx0_ms, r.rx0_frac = cfg->rx0_frac;
    r.B = a.B, r.K = a.K, r.E = a.E, r.first = cfg->epoch_first, r.stride = cfg->epoch_stride;
    r.N = cfg->block_samples, r.Fs = (long long)fs, r.fs = fs;
    r.Lc = (double)cfg->code_length, r.fc = cfg->code_freq_nominal_hz, r.T = cfg->block_seconds, r.if_hz = cfg->if_hz;
    r.edge_margin = cfg->edge_margin;
    p.chunks = (a.B + kObsChunk - 1) / kObsChunk;
    p.group = a.K < kObsThreads ? a.K : kObsThreads;
    p.groups = (a.K + p.group - 1) / p.group;
    p.lanes = 1;
    while (p.lanes < p.group) p.lanes *= 2;
    p.rows = kObsThreads / p.lanes;
    p.run = kObsChunk / p.rows;
    p.chunk_groups = (long long)p.chunks * p.groups;
    p.chan_groups = ((long long)a.K + kObsChanWaves - 1) / kObsChanWaves;
    auto up = [](size_t v) { return (v + 15) & ~(size_t)15; };
    const size_t cells = (size_t)p.chunks * (size_t)a.K;
    p.off_totals = 0;
    p.off_bad = up(p.off_totals + cells * sizeof(ObsSum));
    p.off_runs = up(p.off_bad + cells * sizeof(int32_t));
    p.off_chan = up(p.off_runs + (size_t)p.chunk_groups * kObsThreads * sizeof(ObsSum));
    p.off_anchor = up(p.off_chan + (size_t)a.K * sizeof(ObsChan));
    p.bytes = up(p.off_anchor + sizeof(ObsAnchor));
    if ((long long)p.bytes > kObsMaxScratch) return {GAT_ERR_RANGE, "the call's scratch would exceed 1 GiB"};
    *plan = p;
    return {GAT_OK, nullptr};
}

// the public report
inline void obs_report(const ObsPlan &p, gat_obs_plan *out)
{
    out->struct_size = sizeof(gat_obs_plan);
    out->chunk_blocks = kObsChunk, out->num_chunks = p.chunks;
    out->channel_group = p.group, out->num_groups = p.groups;
    out->lanes = p.lanes, out->rows = p.rows, out->run_blocks = p.run;
    out->threads = kObsThreads, out->lds_bytes = kObsLdsBytes;
    out->chunk_workgroups = (int32_t)p.chunk_groups;
    out->channel_workgroups = (int32_t)p.chan_groups;
    out->scratch_bytes = (int64_t)p.bytes;
}

// ---- the host twin --------------------------------------------------------------------------------------------------------------------
// One channel in plain loops: the prefix sums over the whole history, its record, its epochs.  Returns the channel's ObsChan.
inline ObsChan obs_host_channel(const ObsPlan &p, const gat_channel_params *hist, const gat_monitor_channel &mon, const gat_nav_channel &nav,
                                const gat_nav_frame *frames, int k, const ObsOut &out, std::vector<int64_t> &n, std::vector<int64_t> &W)
{
    const ObsRule &o = p.rule;
    const size_t K = (size_t)o.K;
    bool bad = false;
    n[0] = W[0] = 0;
    for (int i = 0; i <= o.B; ++i) {
        const gat_channel_params &r = hist[(size_t)i * K + k];
        int e;
        if (!obs_record_finite(r)) bad = true;
        if (obs_epoch_at(o, i, &e) && !obs_tau_inside(o, r.code_phase_chips)) bad = true;
        if (i < o.B) {
            int64_t w, c;
            obs_wraps(o, r, hist[(size_t)(i + 1) * K + k], &w, &c, &bad);
            n[i + 1] = n[i] + w, W[i + 1] = W[i] + c;
        }
    }
    const ObsSync s = obs_sync(o, mon, nav, frames);
    const bool inside = s.synced && !(s.status & GAT_OBS_FRAME_OUTSIDE);
    const gat_obs_channel ch = obs_channel(o, s, bad, inside ? n[s.g] : 0, inside ? hist[(size_t)s.g * K + k].code_phase_chips : 0.0);
    if (out.channels) out.channels[k] = ch;
    ObsChan c{};
    c.status = ch.status, c.frame0_ms = ch.frame0_ms, c.pstar = ch.edge_period;
    obs_tx(o, c, hist[(size_t)o.first * K + k], n[o.first], &c.tx0_ms, &c.tx0_frac);
    for (int e = 0; e < o.E; ++e) {
        const size_t b = (size_t)o.first + (size_t)e * (size_t)o.stride;
        obs_emit(o, out, c, hist[b * K + k], e, k, n[b], W[b]);
    }
    return c;
}

// the anchor from the resolved channels, in channel order
inline ObsAnchor obs_pick_anchor(const ObsRule &o, const ObsChan *chan)
{
    if (o.rx_mode == GAT_OBS_RX_GIVEN) return ObsAnchor{o.rx0_ms, 0, o.rx0_frac};
    int ref = -1, best = -1;
    for (int k = 0; k < o.K; ++k) {
        if (chan[k].tx0_ms < 0) continue;
        if (ref < 0) ref = best = k;
        else if (obs_later(chan[ref].tx0_ms, chan[k].tx0_ms, chan[k].tx0_frac, chan[best].tx0_ms, chan[best].tx0_frac)) best = k;
    }
    if (best < 0) return ObsAnchor{-1, o.first, 0.0};
    return obs_anchor_from(o, chan[best].tx0_ms, chan[best].tx0_frac);
}

// The twin's loops (gat_observables_host) for a planned call, every pointer host memory.
inline void obs_host_run(const ObsPlan &p, const gat_channel_params *hist, const gat_monitor_channel *mon, const gat_nav_channel *nav,
                         const gat_nav_frame *frames, const ObsOut &out)
{
    const ObsRule &o = p.rule;
    std::vector<int64_t> n((size_t)o.B + 1), W((size_t)o.B + 1);
    std::vector<ObsChan> chan((size_t)o.K);
    for (int k = 0; k < o.K; ++k) chan[k] = obs_host_channel(p, hist, mon[k], nav[k], frames + (size_t)k * (size_t)o.max_frames, k, out, n, W);
    const ObsAnchor an = obs_pick_anchor(o, chan.data());
    for (int e = 0; e < o.E; ++e) {
        int32_t ms;
        double frac;
        obs_rx(o, an, e, &ms, &frac);
        if (out.rx_ms) out.rx_ms[e] = ms;
        if (out.rx_frac) out.rx_frac[e] = frac;
    }
}

} // namespace gat
