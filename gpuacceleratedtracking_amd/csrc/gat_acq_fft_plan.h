// gat_acq_fft_plan.h -- the pure part of gat_acquire_fft (include/gat.h): its refusals, the transform length, the lag segments,
// the work split, the batches and the scratch carve-up, as a function of the descriptor, the configuration and the device's
// compute-unit count alone.  No HIP call and no HIP header: the device entry point, the host twin and a stand-alone test program
// (tests/acqfftplan) compile the same text.
//
// The search's linear correlation R[l] = sum_{n < N} w[n] c[n + l] comes out of transforms of F > N points for the lags
// 0 <= l <= F - N (the zero padding keeps the circular wrap out of them), so the lag axis Delta = first_shift + o, 0 <= o <= s (J - 1),
// is cut into G segments of Jseg = F - N + 1 lags: segment g transforms the replica from sample first_shift + g Jseg on, and bin j
// (o = s j) lies in segment o / Jseg at lag o mod Jseg -- exactly one (segment, lag) per bin (acq_fft_lag_bin is the inverse).
#pragma once

#include "gat_acq_plan.h" // AcqScratch; the configuration's refusals (gat_acq_check.h)
#include "gat_hd.h"

namespace gat {

constexpr int kAcqFftMinLog2 = 10, kAcqFftMaxLog2 = 18; // F = 1024 .. 262144
constexpr int kAcqFftOnePassLog2 = 12;                  // F <= 4096: one workgroup, one trip through LDS
constexpr int kAcqFftTileLog2 = 12;                     // points of a workgroup's LDS tile (32 KB of float pairs)
constexpr size_t kAcqFftMaxScratch = (size_t)1 << 30;   // what gat_acquire allows itself too
constexpr size_t kAcqFftProductBytes = (size_t)96 << 20; // a Doppler batch's intermediate products: what a 256 MiB last-level cache keeps beside the spectra read with it

constexpr int acq_fft_ilog2(long long v) { return v <= 1 ? 0 : 1 + acq_fft_ilog2(v / 2); }

// bin of lag l of segment g, or -1: the lag lies beyond the segment, between two bins (s > 1) or beyond the grid
GAT_HD inline int acq_fft_lag_bin(long long l, int g, long long Jseg, int s, int J)
{
    if (l < 0 || l >= Jseg) return -1;
    const long long o = l + (long long)g * Jseg;
    if (o % s != 0) return -1;
    const long long j = o / s;
    return j < J ? (int)j : -1;
}

struct AcqFftOptions {
    int log2F;  // 0: the plan's choice
    int dbatch; // Doppler bins at a time, 0: the plan's choice (clamped to D)
    int ubatch; // (block, antenna) units at a time, 0: the plan's choice (rounded up to whole steps of Gu units)
    int groups; // unit groups, 0: by the compute-unit count (the twin takes the device's value)
};

// A transform of F = 2^L points runs its L radix-2 stages in one pass (L <= 12) or in two: the first L1 stages are F / F1
// contiguous transforms of the bit-reversed array, i.e. of the columns n mod F2 of the natural one; the other L2 = L - L1 are F1
// transforms at stride F1.  A workgroup takes a tile of 4096 points either way: `tiles` workgroups a transform and pass.
// Units u = b M + m; unit group k (< Gu) owns the units u = k, k + Gu, ... in order and a slice of its own (Gu > 1), the slices are
// added in group order; a step is Gu consecutive units from a multiple of Gu on, one to a group.  A unit batch is Ub units (whole
// steps) whose W spectra are held at once, with the C spectra of the Bb blocks they can span; a Doppler batch is Db bins.
struct AcqFftPlan : AcqScratch {
    int L, L1, L2, passes, tiles;
    long long F, N, Jseg;
    int G, P, D, J, s, B, M;
    long long units;
    int Db, Ub, Gu, Bb;
    // scratch, 256-byte aligned: [results | power (no caller buffer) | twiddles | C | W | Y (two passes) | slices (Gu > 1) | prns];
    // the four regions the tail reads and the total are AcqScratch's (gat_acq_plan.h)
    size_t off_tw, off_C, off_W, off_Y;
};

inline size_t acq_fft_align(size_t v) { return (v + 255) & ~(size_t)255; }

// the carve-up for given batches; false: beyond the bound
inline bool acq_fft_carve(AcqFftPlan *p, bool own_power)
{
    const double F = (double)p->F, cells = (double)p->P * p->D * p->J;
    const double total = 4096.0 + 80.0 * p->P + cells * 4.0 * (1 + p->Gu) + F * 4.0 + F * 8.0 * ((double)p->P * p->Bb * p->G + (double)p->Ub * p->Db) +
                         (p->passes == 2 ? F * 8.0 * ((double)p->Gu * p->P * p->Db * p->G) : 0.0);
    if (total > (double)kAcqFftMaxScratch * 1.5) return false; // (far beyond: the exact sum below cannot overflow)
    const size_t Fz = (size_t)p->F, cz = (size_t)p->P * (size_t)p->D * (size_t)p->J;
    p->off_res = 256;
    p->off_pow = acq_fft_align(p->off_res + (size_t)p->P * sizeof(gat_acq_result));
    p->off_tw = p->off_pow + (own_power ? acq_fft_align(cz * sizeof(float)) : 0);
    p->off_C = p->off_tw + acq_fft_align(Fz / 2 * 2 * sizeof(float));
    p->off_W = p->off_C + acq_fft_align((size_t)p->P * (size_t)p->Bb * (size_t)p->G * Fz * 2 * sizeof(float));
    p->off_Y = p->off_W + acq_fft_align((size_t)p->Ub * (size_t)p->Db * Fz * 2 * sizeof(float));
    p->off_part = p->off_Y + (p->passes == 2 ? acq_fft_align((size_t)p->Gu * (size_t)p->P * (size_t)p->Db * (size_t)p->G * Fz * 2 * sizeof(float)) : 0);
    p->off_prn = p->off_part + (p->Gu > 1 ? acq_fft_align((size_t)p->Gu * cz * sizeof(float)) : 0);
    p->bytes = p->off_prn + acq_fft_align((size_t)p->P * sizeof(int32_t));
    return p->bytes <= kAcqFftMaxScratch;
}

// blocks that Ub consecutive units of M antennas can span
inline int acq_fft_batch_blocks(int Ub, int M, int B)
{
    const long long n = ((long long)Ub + M - 2) / M + 1;
    return (int)(n < B ? n : B);
}

// The whole call.  cfg->code_length is the table's (0 is refused here: the entry point fills it in).  *plan is written only with GAT_OK.
inline Refusal acq_fft_plan(const gat_signal_desc *sig, int32_t B, int32_t P, double fs, const gat_acq_config *cfg, const AcqFftOptions &opt,
                            int num_cus, bool own_power, AcqFftPlan *plan)
{
    if (!sig || !cfg || !plan) return {GAT_ERR_ARG, "null argument"};
    {
        const Refusal r = acq_check_config(cfg, P, cfg->num_doppler_bins, cfg->num_code_bins, fs);
        if (r.code != GAT_OK) return r;
    }
    if (cfg->code_length < 1) return {GAT_ERR_ARG, "config.code_length must be positive"};
    if (B < 1) return {GAT_ERR_ARG, "num_blocks must be positive"};
    {
        const Refusal r = check_desc(sig, B, 0, signal_refusals({GAT_ERR_ARG, "chan_stride must be 0 (one signal for every PRN)"}));
        if (r.code != GAT_OK) return r;
    }
    if (opt.log2F != 0 && (opt.log2F < kAcqFftMinLog2 || opt.log2F > kAcqFftMaxLog2)) return {GAT_ERR_RANGE, "acq_fft_log2 must be 0 or 10 .. 18"};
    if (opt.dbatch < 0 || opt.ubatch < 0 || opt.groups < 0 || num_cus < 1) return {GAT_ERR_ARG, "negative batch, group or compute-unit count"};
    const long long N = sig->num_samples;
    if (N >= (1ll << kAcqFftMaxLog2)) return {GAT_ERR_RANGE, "a block must be shorter than the largest transform (2^18 samples)"};
    if (opt.log2F != 0 && (1ll << opt.log2F) <= N) return {GAT_ERR_RANGE, "the forced transform length does not exceed the block (acq_fft_log2)"};
    if ((long long)sig->num_ants * B > (1ll << 24)) return {GAT_ERR_RANGE, "more than 2^24 (block, antenna) units"};

    AcqFftPlan p{};
    p.N = N, p.P = P, p.D = cfg->num_doppler_bins, p.J = cfg->num_code_bins, p.s = cfg->code_step_samples, p.B = B, p.M = sig->num_ants;
    p.units = (long long)p.M * B;
    const long long lags = (long long)p.s * (p.J - 1) + 1;
    // the F that minimises G F log2 F (the smaller F on ties), or the forced one
    long long best = -1;
    for (int v = kAcqFftMinLog2; v <= kAcqFftMaxLog2; ++v) {
        const long long F = 1ll << v;
        if (F <= N || (opt.log2F != 0 && v != opt.log2F)) continue;
        const long long Jseg = F - N + 1, G = (lags + Jseg - 1) / Jseg, cost = G * F * v;
        if (best < 0 || cost < best) best = cost, p.L = v, p.F = F, p.Jseg = Jseg, p.G = (int)(G < (1ll << 30) ? G : (1ll << 30));
    }
    const double reach = (double)p.F + (double)(cfg->first_shift < 0 ? -cfg->first_shift : cfg->first_shift) + (double)p.G * (double)p.Jseg;
    if (!(reach < 1073741824.0)) return {GAT_ERR_RANGE, "N + |first_shift| + s * J must stay below 2^30 samples"};
    if (code_span_bad(cfg->code_freq_hz / fs, (double)cfg->code_length, reach, cfg->code_length)) return {GAT_ERR_RANGE, "code phase span too large"};
    p.passes = p.L <= kAcqFftOnePassLog2 ? 1 : 2;
    p.L1 = p.passes == 1 ? p.L : (p.L + 1) / 2;
    p.L2 = p.L - p.L1;
    p.tiles = p.passes == 1 ? 1 : 1 << (p.L - kAcqFftTileLog2);

    // unit groups: two workgroups a compute unit from (PRN, Doppler, segment, tile) alone, else the units are dealt to groups
    const double wgs = (double)P * p.D * p.G * p.tiles;
    long long Gu = opt.groups > 0 ? opt.groups : (long long)((2.0 * num_cus + wgs - 1.0) / wgs);
    if (Gu < 1) Gu = 1;
    if (Gu > p.units) {
        if (opt.groups > 0) return {GAT_ERR_ARG, "more unit groups than (block, antenna) units"};
        Gu = p.units;
    }
    const long long cells = (long long)P * p.D * p.J;
    if (opt.groups == 0) {
        const long long by_slices = (long long)(kAcqFftMaxScratch / 4 / ((size_t)cells * sizeof(float)));
        Gu = Gu < by_slices ? Gu : (by_slices < 1 ? 1 : by_slices);
    }
    for (;;) {
        p.Gu = (int)Gu;
        const long long all = (p.units + Gu - 1) / Gu * Gu; // whole steps
        p.Db = opt.dbatch > 0 && opt.dbatch < p.D ? opt.dbatch : p.D;
        if (opt.dbatch == 0 && p.passes == 2) { // the product's first pass is read back at once: keep a batch of it within the last-level cache
            const double per_bin = (double)Gu * P * p.G * (double)p.F * 8.0;
            const double most = (double)kAcqFftProductBytes / per_bin;
            if (most < (double)p.Db) p.Db = most < 1.0 ? 1 : (int)most;
        }
        long long Ub = opt.ubatch > 0 ? (opt.ubatch + Gu - 1) / Gu * Gu : all;
        if (Ub > all) Ub = all;
        bool fits;
        for (;;) {
            p.Ub = (int)Ub, p.Bb = acq_fft_batch_blocks(p.Ub, p.M, B);
            fits = acq_fft_carve(&p, own_power);
            if (fits) break;
            if (p.Db > 1 && opt.dbatch == 0)
                p.Db = (p.Db + 1) / 2;
            else if (Ub > Gu && opt.ubatch == 0)
                Ub = (Ub / Gu + 1) / 2 * Gu;
            else
                break;
        }
        if (fits) break;
        if (Gu > 1 && opt.groups == 0)
            Gu = (Gu + 1) / 2;
        else
            return {GAT_ERR_RANGE, "the search needs more than 1 GiB of scratch (fewer PRNs, bins or blocks a call)"};
    }
    // workgroups of the largest launch
    if ((double)p.Gu * P * p.Db * p.G * p.tiles >= 1073741824.0 || (double)p.Ub * p.Db * p.tiles >= 1073741824.0)
        return {GAT_ERR_RANGE, "too many transforms in one launch"};
    *plan = p;
    return {GAT_OK, nullptr};
}

// the public report
inline void acq_fft_report(const AcqFftPlan &p, gat_acq_fft_plan *out)
{
    out->struct_size = sizeof(gat_acq_fft_plan);
    out->fft_log2 = p.L;
    out->num_segments = p.G;
    out->segment_lags = (int32_t)p.Jseg;
    out->passes = p.passes;
    out->doppler_batch = p.Db;
    out->unit_batch = p.Ub;
    out->unit_groups = p.Gu;
    out->scratch_bytes = (int64_t)p.bytes;
}

} // namespace gat
