// gat_nav_plan.h -- the pure part of gat_nav_decode (include/gat.h): its refusals, the counts, the scratch carve-up and the launch
// geometry with the work units' decoding, as a function of the call's arguments alone, and the host twin's loops over it.  No HIP
// call and no HIP header: the device entry point, the host twin and a stand-alone test program (tests/navplan) compile the same
// text.
#pragma once

#include <vector>

#include "gat_nav.h"
#include "gat_sig_plan.h" // Refusal

namespace gat {

constexpr int kNavThreads = 256;
constexpr int kNavWave = 64;                          // the quantiser, the trellis and the choice give one wave to a unit
constexpr int kNavPickWaves = kNavThreads / kNavWave; // the choice: four channels a workgroup
constexpr size_t kNavMaxScratch = (size_t)1 << 30;

// The call as the entry points receive it.  The plan reads *cfg and nothing else behind a pointer.
struct NavCall {
    const void *sym_re, *mon;
    int K;
    const gat_nav_config *cfg;
    const void *channels, *frames, *decoded, *path_metric;
};

// Work units (unit t = workgroup * threads + thread unless said otherwise):
//   slice    LNAV, 256 threads, t < K cap:        (k, j) = (t / cap, t % cap): the hard bit, 0 from n_k on; t < K: path_metric[t] = 0
//   quantise CNAV, one workgroup of 64 a channel: q[k][0 .. cap), 0 from n_k on
//   trellis  CNAV, one workgroup of 64 a (k, ph): workgroup = k * 2 + ph; survivors, decoded bits, path metric
//   score    256 threads, t < K C:                (k, c) = (t / C, t % C), C = P * 300 * 2, c = (ph * 300 + o) * 2 + p, to scores[t]
//   choice   one wave a channel, u = workgroup * kNavPickWaves + wave < K: the channel record
//   frames   256 threads, t < K max_frames:       (k, f) = (t / max_frames, t % max_frames)
// Scratch, 256-byte aligned, each part only where the call needs it and the caller gave no buffer of its own:
// [q int8 K cap | survivors uint64 K 2 (cap / 2) | decoded uint8 K P bit_cap | scores int32 K C | channel records].
struct NavPlan {
    int format, K, cap, P, bit_cap, max_frames, min_frames, C;
    bool do_sync, do_frames; // sync: scores and the choice
    bool own_decoded, own_chan;
    size_t off_q, off_surv, off_decoded, off_scores, off_chan, bytes;
    long long g_slice, g_quant, g_trellis, g_score, g_pick, g_frame; // workgroups; 0: no launch
};

inline size_t nav_align(size_t v) { return (v + 255) & ~(size_t)255; }
constexpr long long nav_groups(long long units, int per) { return (units + per - 1) / per; }

GAT_HD inline bool nav_slice_unit(long long t, int cap, int K, int *k, int *j)
{
    if (t >= (long long)K * cap) return false;
    *k = (int)(t / cap), *j = (int)(t % cap);
    return true;
}
GAT_HD inline bool nav_score_unit(long long t, int C, int K, int *k, int *c)
{
    if (t >= (long long)K * C) return false;
    *k = (int)(t / C), *c = (int)(t % C);
    return true;
}
GAT_HD inline bool nav_frame_unit(long long t, int max_frames, int K, int *k, int *f)
{
    if (t >= (long long)K * max_frames) return false;
    *k = (int)(t / max_frames), *f = (int)(t % max_frames);
    return true;
}

// The whole call.  *plan is written only with GAT_OK.
inline Refusal nav_plan(const NavCall &a, NavPlan *plan)
{
    const gat_nav_config *cfg = a.cfg;
    if (!a.sym_re || !cfg || !plan) return {GAT_ERR_ARG, "null argument"};
    if (cfg->struct_size != sizeof(gat_nav_config)) return {GAT_ERR_ARG, "config.struct_size is not sizeof(gat_nav_config)"};
    if (a.K < 1) return {GAT_ERR_ARG, "num_channels must be positive"};
    if (cfg->symbol_capacity < 0) return {GAT_ERR_ARG, "symbol_capacity must not be negative"};
    if (cfg->max_frames < 1 || cfg->min_frames < 1) return {GAT_ERR_ARG, "max_frames and min_frames must be positive"};
    if (cfg->format != GAT_NAV_LNAV && cfg->format != GAT_NAV_CNAV) return {GAT_ERR_ARG, "unknown format"};
    if (!a.channels && !a.frames && !a.decoded && !a.path_metric) return {GAT_ERR_ARG, "every output is null"};
    if (a.K > GAT_MAX_MONITOR_CHANNELS) return {GAT_ERR_RANGE, "more than 4096 channels"};
    if (cfg->symbol_capacity > GAT_MAX_MONITOR_BLOCKS) return {GAT_ERR_RANGE, "symbol_capacity above 2^20"};

    NavPlan p{};
    p.format = cfg->format, p.K = a.K, p.cap = cfg->symbol_capacity, p.max_frames = cfg->max_frames, p.min_frames = cfg->min_frames;
    p.P = nav_phases(p.format);
    p.bit_cap = p.cap / p.P;
    p.C = nav_candidates(p.format);
    const bool cnav = p.format == GAT_NAV_CNAV;
    p.do_frames = a.frames != nullptr;
    p.do_sync = a.channels || a.frames;
    p.own_decoded = !a.decoded;
    p.own_chan = p.do_sync && !a.channels;
    p.g_frame = p.do_frames ? nav_groups((long long)p.K * p.max_frames, kNavThreads) : 0;
    if (p.g_frame > 0x7fffffffll) return {GAT_ERR_RANGE, "more than 2^31 - 1 workgroups (fewer frames a channel)"};

    const size_t K = (size_t)p.K;
    p.off_q = 0;
    p.off_surv = p.off_q + (cnav ? nav_align(K * (size_t)p.cap) : 0);
    p.off_decoded = p.off_surv + (cnav ? nav_align(K * 2 * (size_t)p.bit_cap * sizeof(uint64_t)) : 0); // at most 2^12 * 2^20 * 8
    p.off_scores = p.off_decoded + (p.own_decoded ? nav_align(K * (size_t)p.P * (size_t)p.bit_cap) : 0);
    p.off_chan = p.off_scores + (p.do_sync ? nav_align(K * (size_t)p.C * sizeof(int32_t)) : 0);
    p.bytes = p.off_chan + (p.own_chan ? nav_align(K * sizeof(gat_nav_channel)) : 0);
    if (p.bytes > kNavMaxScratch) return {GAT_ERR_RANGE, "the decoder needs more than 1 GiB of scratch (fewer channels or symbols a call)"};

    p.g_slice = !cnav ? nav_groups((long long)p.K * (p.cap > 1 ? p.cap : 1), kNavThreads) : 0; // K units at least: they write path_metric
    p.g_quant = cnav ? p.K : 0;
    p.g_trellis = cnav ? 2ll * p.K : 0;
    p.g_score = p.do_sync ? nav_groups((long long)p.K * p.C, kNavThreads) : 0;
    p.g_pick = p.do_sync ? nav_groups(p.K, kNavPickWaves) : 0;
    *plan = p;
    return {GAT_OK, nullptr};
}

// the public report
inline void nav_report(const NavPlan &p, gat_nav_plan *out)
{
    out->struct_size = sizeof(gat_nav_plan);
    out->num_phases = p.P;
    out->bit_capacity = p.bit_cap;
    out->num_candidates = p.C;
    out->slice_workgroups = (int32_t)p.g_slice;
    out->quantise_workgroups = (int32_t)p.g_quant;
    out->trellis_workgroups = (int32_t)p.g_trellis;
    out->score_workgroups = (int32_t)p.g_score;
    out->pick_workgroups = (int32_t)p.g_pick;
    out->frame_workgroups = (int32_t)p.g_frame;
    out->scratch_bytes = (int64_t)p.bytes;
}

// ---- the host twin ----------------------------------------------------------------------------------------------------------------
// The quantiser of one channel: x[0 .. n) to q[0 .. cap), 0 from n on.
inline void nav_host_quantise(const double *x, int n, int cap, int8_t *q)
{
    double part[kNavWave];
    for (int l = 0; l < kNavWave; ++l) {
        double s = 0.0;
        for (int j = l; j < n; j += kNavWave) s += nav_abs(x[j]);
        part[l] = s;
    }
    double S = 0.0;
    for (int l = 0; l < kNavWave; ++l) S += part[l];
    const double unit = S / (double)n;
    for (int j = 0; j < cap; ++j) q[j] = j < n ? (int8_t)nav_quantise(x[j], unit) : (int8_t)0;
}
// The trellis of one (channel, phase): T steps over q[ph + 2 t], q[ph + 2 t + 1]; bits[0 .. bit_cap), 0 from T on.  Returns the
// largest final metric.
inline int32_t nav_host_trellis(const int8_t *q, int ph, int T, int bit_cap, uint8_t *bits)
{
    std::vector<uint64_t> surv((size_t)T);
    int32_t m[kNavStates] = {}, next[kNavStates];
    for (int t = 0; t < T; ++t) {
        const int q0 = q[ph + 2 * t], q1 = q[ph + 2 * t + 1];
        uint64_t word = 0;
        for (int s = 0; s < kNavStates; ++s) {
            const int bm = nav_branch0(s, q0, q1);
            int dec;
            next[s] = nav_acs(m[nav_pred(s, 0)] + bm, m[nav_pred(s, 1)] - bm, &dec);
            word |= (uint64_t)dec << s;
        }
        surv[(size_t)t] = word;
        for (int s = 0; s < kNavStates; ++s) m[s] = next[s];
    }
    int best = 0;
    for (int s = 1; s < kNavStates; ++s)
        if (m[s] > m[best]) best = s;
    const int32_t metric = m[best];
    for (int t = T - 1; t >= 0; --t) {
        bits[t] = (uint8_t)(best >> 5);
        best = nav_back(best, surv[(size_t)t]);
    }
    for (int t = T; t < bit_cap; ++t) bits[t] = 0;
    return metric;
}

// The twin's loops (gat_nav_decode_host) for a planned call: the units of the kernels in plain loops, every pointer host memory.
inline void nav_host_run(const NavPlan &p, const double *sym_re, const gat_monitor_channel *mon, gat_nav_channel *channels, gat_nav_frame *frames,
                         uint8_t *decoded, int32_t *path_metric)
{
    const size_t row = (size_t)p.P * (size_t)p.bit_cap;
    std::vector<uint8_t> own_dec(p.own_decoded ? row : 0);
    std::vector<int8_t> q(p.format == GAT_NAV_CNAV ? (size_t)p.cap : 0);
    for (int k = 0; k < p.K; ++k) {
        const int n = nav_symbols(mon, k, p.cap);
        const double *x = sym_re + (size_t)k * (size_t)p.cap;
        uint8_t *dec = p.own_decoded ? own_dec.data() : decoded + (size_t)k * row;
        if (p.format == GAT_NAV_CNAV) {
            nav_host_quantise(x, n, p.cap, q.data());
            for (int ph = 0; ph < 2; ++ph) {
                const int32_t metric = nav_host_trellis(q.data(), ph, nav_bits(p.format, n, ph), p.bit_cap, dec + (size_t)ph * p.bit_cap);
                if (path_metric) path_metric[(size_t)k * 2 + ph] = metric;
            }
        } else {
            for (int j = 0; j < p.cap; ++j) dec[j] = (uint8_t)(j < n ? nav_lnav_bit(x[j]) : 0);
            if (path_metric) path_metric[k] = 0;
        }
        if (!p.do_sync) continue;
        NavBest best{};
        for (int c = 0; c < p.C; ++c) {
            int ph, o, pol;
            nav_candidate(c, &ph, &o, &pol);
            const int search = nav_search_bits(p.format, nav_bits(p.format, n, ph));
            const NavBest one = nav_best_one(nav_score(p.format, dec + (size_t)ph * p.bit_cap, search, o, pol), c);
            best = c == 0 ? one : nav_best_merge(best, one);
        }
        gat_nav_channel ch;
        nav_record(p.format, best, n, p.max_frames, p.min_frames, ch);
        const uint8_t *bits = dec + (size_t)ch.symbol_phase * p.bit_cap + (ch.frame_offset < 0 ? 0 : ch.frame_offset);
        gat_nav_frame prev{}, cur{};
        for (int f = 0; f < ch.num_frames; ++f) {
            nav_frame(p.format, bits + (size_t)f * GAT_NAV_FRAME_BITS, ch.inverted, cur);
            if (f > 0 && nav_tow_step(p.format, prev, cur)) ch.tow_steps += 1;
            if (frames) frames[(size_t)k * p.max_frames + f] = cur;
            prev = cur;
        }
        if (frames)
            for (int f = ch.num_frames; f < p.max_frames; ++f) frames[(size_t)k * p.max_frames + f] = gat_nav_frame{};
        if (channels) channels[k] = ch;
    }
}

} // namespace gat
