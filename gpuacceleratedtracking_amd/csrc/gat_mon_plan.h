// gat_mon_plan.h -- the pure part of gat_track_monitor (include/gat.h): its refusals, the counts (windows, symbols of the search,
// symbol capacity), the scratch carve-up and the launch geometry with the work units' decoding, as a function of the call's
// arguments alone.  No HIP call and no HIP header: the device entry point, the host twin and a stand-alone test program
// (tests/monplan) compile the same text.
#pragma once

#include <vector>

#include "gat_mon.h"
#include "gat_sig_plan.h" // Refusal

namespace gat {

constexpr int kMonThreads = 256;
constexpr int kMonWave = 64;                          // the window kernel gives one wave to a window
constexpr int kMonWindowWaves = kMonThreads / kMonWave;
constexpr size_t kMonMaxScratch = (size_t)1 << 30;

// The call as the entry points receive it.  The plan reads *cfg and nothing else behind a pointer.
struct MonCall {
    const void *acc_re, *acc_im;
    long long acc_block_stride;
    int B, K, M;
    const gat_monitor_config *cfg;
    const void *w_re, *w_im;
    const void *prompt_re, *prompt_im, *windows, *energy, *channels, *sym_re, *sym_im, *sym_wbp;
};

// Work units, `threads` = kMonThreads to a workgroup, unit t = workgroup * threads + thread (the window kernel: wave u =
// workgroup * kMonWindowWaves + wave of the workgroup):
//   prompts  t < K B:       (k, b) = (t / B, t % B), written to series[k B + b]
//   windows  u < K NW:      (k, v) = (u / NW, u % NW)
//   terms    t < K J Pd:    (k, j, c) = (t / (J Pd), t / Pd % J, t % Pd), written to terms[t]
//   energies t < K Pd:      (k, c) = (t / Pd, t % Pd), adds terms[(k J + j) Pd + c] in j order
//   choice   t < K
//   symbols  t < K cap:     (k, j) = (t / cap, t % cap)
// Scratch, 256-byte aligned, each part only where the caller gave no buffer of its own (own_*) and the call needs it:
// [prompt re | prompt im | terms | energy | channel records].
struct MonPlan {
    int B, K, M, L, prompt, W, Pd, forced;
    long long first_block, NW, J, cap;
    bool do_windows, do_sync, do_symbols; // sync: terms, energies and the choice
    bool own_pr, own_pi, own_energy, own_chan;
    size_t off_pr, off_pi, off_terms, off_energy, off_chan, bytes;
    long long g_prompt, g_window, g_term, g_energy, g_pick, g_symbol; // workgroups; 0: no launch
};

inline size_t mon_align(size_t v) { return (v + 255) & ~(size_t)255; }
constexpr long long mon_groups(long long units, int per) { return (units + per - 1) / per; }

GAT_HD inline bool mon_prompt_unit(long long t, int B, int K, int *k, int *b)
{
    if (t >= (long long)K * B) return false;
    *k = (int)(t / B), *b = (int)(t % B);
    return true;
}
GAT_HD inline bool mon_window_unit(long long u, long long NW, int K, int *k, long long *v)
{
    if (u >= (long long)K * NW) return false;
    *k = (int)(u / NW), *v = u % NW;
    return true;
}
GAT_HD inline bool mon_term_unit(long long t, long long J, int Pd, int K, int *k, long long *j, int *c)
{
    if (t >= (long long)K * J * Pd) return false;
    *k = (int)(t / (J * Pd)), *j = t / Pd % J, *c = (int)(t % Pd);
    return true;
}
GAT_HD inline bool mon_energy_unit(long long t, int Pd, int K, int *k, int *c)
{
    if (t >= (long long)K * Pd) return false;
    *k = (int)(t / Pd), *c = (int)(t % Pd);
    return true;
}
GAT_HD inline bool mon_symbol_unit(long long t, long long cap, int K, int *k, long long *j)
{
    if (t >= (long long)K * cap) return false;
    *k = (int)(t / cap), *j = t % cap;
    return true;
}

// The whole call.  *plan is written only with GAT_OK.
inline Refusal mon_plan(const MonCall &a, MonPlan *plan)
{
    const gat_monitor_config *cfg = a.cfg;
    if (!a.acc_re || !a.acc_im || !cfg || !plan) return {GAT_ERR_ARG, "null argument"};
    if (cfg->struct_size != sizeof(gat_monitor_config)) return {GAT_ERR_ARG, "config.struct_size is not sizeof(gat_monitor_config)"};
    if (a.B < 1 || a.K < 1 || a.M < 1 || cfg->num_taps < 1) return {GAT_ERR_ARG, "num_blocks, num_channels, num_ants and num_taps must be positive"};
    if (a.M > GAT_MAX_ARRAY_ANTS) return {GAT_ERR_RANGE, "more than 64 antennas"};
    if (a.B > GAT_MAX_MONITOR_BLOCKS) return {GAT_ERR_RANGE, "more than 2^20 blocks a call"};
    if (a.K > GAT_MAX_MONITOR_CHANNELS) return {GAT_ERR_RANGE, "more than 4096 channels"};
    if (cfg->prompt_index < 0 || cfg->prompt_index >= cfg->num_taps) return {GAT_ERR_RANGE, "prompt_index outside the tap list"};
    if (cfg->window_blocks < 1) return {GAT_ERR_ARG, "window_blocks must be positive"};
    if (cfg->symbol_blocks < 1 || cfg->symbol_blocks > GAT_MAX_SYMBOL_BLOCKS) return {GAT_ERR_RANGE, "symbol_blocks outside 1 .. 128"};
    for (int i = 0; i < cfg->symbol_blocks; ++i)
        if (cfg->overlay[i] != 1 && cfg->overlay[i] != -1) return {GAT_ERR_ARG, "an overlay entry is neither +1 nor -1"};
    if (cfg->symbol_offset < -1 || cfg->symbol_offset >= cfg->symbol_blocks) return {GAT_ERR_RANGE, "symbol_offset outside -1 .. symbol_blocks - 1"};
    if (cfg->first_block < 0) return {GAT_ERR_ARG, "first_block must not be negative"};
    if (a.B > 1 && (double)a.acc_block_stride < (double)a.K * (double)cfg->num_taps * (double)a.M)
        return {GAT_ERR_ARG, "acc_block_stride is below one block's accumulators"};
    if ((a.w_re == nullptr) != (a.w_im == nullptr)) return {GAT_ERR_ARG, "one weight pointer without the other"};
    const bool syms = a.sym_re || a.sym_im || a.sym_wbp;
    if (!a.prompt_re && !a.prompt_im && !a.windows && !a.energy && !a.channels && !syms) return {GAT_ERR_ARG, "every output is null"};

    MonPlan p{};
    p.B = a.B, p.K = a.K, p.M = a.M, p.L = cfg->num_taps, p.prompt = cfg->prompt_index, p.W = cfg->window_blocks, p.Pd = cfg->symbol_blocks;
    p.forced = cfg->symbol_offset, p.first_block = cfg->first_block;
    p.NW = ((long long)a.B + p.W - 1) / p.W;
    p.J = ((long long)a.B - p.Pd + 1) / p.Pd; // B - Pd + 1 >= 1 - Pd > -Pd: the quotient of a negative numerator is 0
    if (p.J < 0) p.J = 0;
    p.cap = a.B / p.Pd;
    p.do_windows = a.windows != nullptr;
    p.do_symbols = syms && p.cap > 0;
    p.do_sync = a.energy || a.channels || syms;
    p.own_pr = !a.prompt_re, p.own_pi = !a.prompt_im;
    p.own_energy = p.do_sync && !a.energy, p.own_chan = p.do_sync && !a.channels;

    const size_t series = mon_align((size_t)p.K * (size_t)p.B * sizeof(double)); // at most 2^32 * 8
    const size_t terms = p.do_sync ? mon_align((size_t)p.K * (size_t)p.J * (size_t)p.Pd * sizeof(double)) : 0; // K J Pd <= K B
    if ((double)series * 2.0 + (double)terms > (double)kMonMaxScratch) return {GAT_ERR_RANGE, "the monitor needs more than 1 GiB of scratch (fewer channels or blocks a call)"};
    p.off_pr = 0;
    p.off_pi = p.off_pr + (p.own_pr ? series : 0);
    p.off_terms = p.off_pi + (p.own_pi ? series : 0);
    p.off_energy = p.off_terms + terms;
    p.off_chan = p.off_energy + (p.own_energy ? mon_align((size_t)p.K * (size_t)p.Pd * sizeof(double)) : 0);
    p.bytes = p.off_chan + (p.own_chan ? mon_align((size_t)p.K * sizeof(gat_monitor_channel)) : 0);
    if (p.bytes > kMonMaxScratch) return {GAT_ERR_RANGE, "the monitor needs more than 1 GiB of scratch (fewer channels or blocks a call)"};

    p.g_prompt = mon_groups((long long)p.K * p.B, kMonThreads);
    p.g_window = p.do_windows ? mon_groups((long long)p.K * p.NW, kMonWindowWaves) : 0;
    p.g_term = p.do_sync ? mon_groups((long long)p.K * p.J * p.Pd, kMonThreads) : 0;
    p.g_energy = p.do_sync ? mon_groups((long long)p.K * p.Pd, kMonThreads) : 0;
    p.g_pick = p.do_sync ? mon_groups(p.K, kMonThreads) : 0;
    p.g_symbol = p.do_symbols ? mon_groups((long long)p.K * p.cap, kMonThreads) : 0;
    *plan = p;
    return {GAT_OK, nullptr};
}

// the public report
inline void mon_report(const MonPlan &p, gat_monitor_plan *out)
{
    out->struct_size = sizeof(gat_monitor_plan);
    out->num_windows = (int32_t)p.NW;
    out->search_symbols = (int32_t)p.J;
    out->symbol_capacity = (int32_t)p.cap;
    out->prompt_workgroups = (int32_t)p.g_prompt;
    out->window_workgroups = (int32_t)p.g_window;
    out->term_workgroups = (int32_t)p.g_term;
    out->energy_workgroups = (int32_t)p.g_energy;
    out->pick_workgroups = (int32_t)p.g_pick;
    out->symbol_workgroups = (int32_t)p.g_symbol;
    out->scratch_bytes = (int64_t)p.bytes;
}

// The host twin's loops (gat_track_monitor_host) for a planned call: the units of the kernels in plain loops, every pointer host memory.
inline void mon_host_run(const MonPlan &p, const float *acc_re, const float *acc_im, long long stride, const gat_monitor_config *cfg, const double *w_re,
                         const double *w_im, double *prompt_re, double *prompt_im, gat_monitor_window *windows, double *energy,
                         gat_monitor_channel *channels, double *sym_re, double *sym_im, double *sym_wbp)
{
    const size_t Bz = (size_t)p.B, Kz = (size_t)p.K;
    std::vector<double> own_r(p.own_pr ? Kz * Bz : 0), own_i(p.own_pi ? Kz * Bz : 0), own_e(p.own_energy ? Kz * p.Pd : 0);
    double *pr = p.own_pr ? own_r.data() : prompt_re, *pi = p.own_pi ? own_i.data() : prompt_im, *en = p.own_energy ? own_e.data() : energy;
    for (int k = 0; k < p.K; ++k)
        for (int b = 0; b < p.B; ++b) {
            const size_t o = p.B > 1 ? (size_t)b * (size_t)stride : 0;
            tap_sum(acc_re + o, acc_im + o, k, p.L, p.prompt, p.M, w_re, w_im, pr[k * Bz + b], pi[k * Bz + b]);
        }
    if (p.do_windows)
        for (int k = 0; k < p.K; ++k)
            for (long long v = 0; v < p.NW; ++v) {
                gat_monitor_window w;
                mon_window_begin(w);
                for (long long b = v * p.W; b < (v + 1) * p.W && b < p.B; ++b) mon_window_add(w, pr[k * Bz + b], pi[k * Bz + b]);
                windows[k * (size_t)p.NW + v] = w;
            }
    if (!p.do_sync) return;
    for (int k = 0; k < p.K; ++k) {
        for (int c = 0; c < p.Pd; ++c) {
            double e = 0.0;
            for (long long j = 0; j < p.J; ++j) e += mon_symbol_energy(pr + k * Bz, pi + k * Bz, c, j, p.Pd, cfg->overlay);
            en[k * (size_t)p.Pd + c] = e;
        }
        gat_monitor_channel ch;
        mon_pick(en + k * (size_t)p.Pd, p.Pd, p.B, p.J, p.forced, p.first_block, ch);
        if (channels) channels[k] = ch;
        if (!p.do_symbols) continue;
        for (long long j = 0; j < p.cap; ++j) {
            double sr = 0.0, si = 0.0, wbp = 0.0;
            if (ch.start >= 0 && j < ch.num_symbols) mon_symbol(pr + k * Bz, pi + k * Bz, ch.start + j * p.Pd, p.Pd, cfg->overlay, sr, si, wbp);
            const size_t t = k * (size_t)p.cap + j;
            if (sym_re) sym_re[t] = sr;
            if (sym_im) sym_im[t] = si;
            if (sym_wbp) sym_wbp[t] = wbp;
        }
    }
}

} // namespace gat
