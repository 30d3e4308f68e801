// gat_cond_plan.h -- the pure part of gat_condition_samples and gat_sample_stats (include/gat.h): their refusals, the choice
// between the streaming and the general kernel and the work split, as a function of the call's arguments alone.  No HIP call
// and no HIP header: the device entry points, the host twin and the stand-alone test programs (tests/condplan, tests/estplan)
// compile the same text.
#pragma once

#include "gat_est_plan.h"

namespace gat {

constexpr int kCondThreads = 256;
constexpr int kCondStreamMaxAnts = 8; // the streaming kernel holds every antenna's 16-byte loads of a step up to here

// samples a lane of the streaming kernel owns per step: whole 16-byte loads AND whole 16-byte stores -- 8 where either side is
// int8 pairs (a float input then takes two loads per antenna and plane, ComplexF32 four), else 4
constexpr int cond_group_samples(int fmt_in, int fmt_out)
{
    return fmt_in == GAT_LAYOUT_INTERLEAVED_I8 || fmt_out == GAT_LAYOUT_INTERLEAVED_I8 ? 8 : 4;
}

// Work units are (block, chunk of `chunk` samples), `chunks` to a block, unit u = block * chunks + chunk index; workgroup g of
// `grid` takes units g, g + grid, ...  stream: chunk is a multiple of group * kCondThreads, so only a block's end is ragged.
struct CondPlan {
    bool stream, in_place;
    int group; // samples per lane and step (1: the general kernel)
    long long chunk, chunks, units, grid;
};

// unit u of a plan over blocks of N samples: its block and its samples [n0, n1)
#if defined(__HIPCC__)
__host__ __device__
#endif
inline void cond_unit(long long u, long long chunks, long long chunk, long long N, long long *b, long long *n0, long long *n1)
{
    *b = u / chunks;
    *n0 = (u - *b * chunks) * chunk;
    *n1 = *n0 + chunk < N ? *n0 + chunk : N;
}

// The signal side alone (what gat_sample_stats shares): GAT_OK or the refusal
inline Refusal cond_check_signal(const gat_signal_desc *sig, int32_t B)
{
    if (!sig) return {GAT_ERR_ARG, "null argument"};
    if (B < 1) return {GAT_ERR_ARG, "num_blocks must be positive"};
    return check_desc(sig, B, GAT_MAX_ARRAY_ANTS, signal_refusals({GAT_ERR_UNSUPPORTED, "chan_stride must be 0"}));
}

// The whole call.  workgroups_wanted: about eight a compute unit on the device.  *plan is written only with GAT_OK.
inline Refusal cond_plan(const gat_signal_desc *sig, int32_t B, const void *params, uint32_t flags, const gat_signal_desc *out,
                         long long workgroups_wanted, CondPlan *plan)
{
    // (no antenna limit on the output: its antennas are the signal's, below)
    constexpr DescRefusals kOutput{{GAT_ERR_ARG, "bad layout"}, {GAT_ERR_ARG, "bad output planes"}, {GAT_ERR_ARG, "bad output sizes"},
                                   {GAT_ERR_ARG, "the output's ant_stride must be positive"},
                                   {GAT_ERR_ARG, "the output's block_stride must be positive"}, {GAT_OK, nullptr},
                                   {GAT_ERR_UNSUPPORTED, "chan_stride must be 0 on both sides"}, {GAT_ERR_RANGE, "signal extent too large"}};
    if (!sig || !out || !params || !plan) return {GAT_ERR_ARG, "null argument"};
    if (flags & ~(uint32_t)GAT_COND_BLANK_ALL_ANTS) return {GAT_ERR_ARG, "unknown flags"};
    Refusal r = cond_check_signal(sig, B);
    if (r.code != GAT_OK) return r;
    r = check_desc(out, B, 0, kOutput);
    if (r.code != GAT_OK) return r;
    if (out->num_ants != sig->num_ants) return {GAT_ERR_ARG, "the output's num_ants must be the signal's"};
    if (out->num_samples != sig->num_samples) return {GAT_ERR_ARG, "the output's num_samples must be the signal's"};
    const int M = sig->num_ants;
    // in place: the same elements at the same addresses, so that every lane reads what it is about to overwrite and nothing else
    const bool same = out->layout == sig->layout && out->re == sig->re && out->im == sig->im && (M == 1 || out->ant_stride == sig->ant_stride) &&
                      (B == 1 || out->block_stride == sig->block_stride);
    if (!same && descs_overlap(sig, out, B)) return {GAT_ERR_ARG, "the output overlaps the signal without being identical to it"};

    CondPlan p{};
    p.in_place = same;
    p.stream = M <= kCondStreamMaxAnts && blocks_aligned(sig, B) && blocks_aligned(out, B);
    p.group = p.stream ? cond_group_samples(sig->layout, out->layout) : 1;
    const ChunkSplit s = split_chunks(B, sig->num_samples, (long long)kCondThreads * p.group, workgroups_wanted);
    p.chunk = s.chunk, p.chunks = s.chunks, p.units = s.units, p.grid = s.grid;
    *plan = p;
    return {GAT_OK, nullptr};
}

// ---- the statistics -----------------------------------------------------------------------------------------------------------------
constexpr int kStatsThreads = 256;
constexpr int kStatsTile = 8; // antennas whose sums a lane keeps in registers; more antennas run in tiles (blockIdx.y)
constexpr size_t kStatsScratchCap = (size_t)64 << 20; // bytes of the workgroups' slices of one launch; more estimates go in batches

// vec: M <= 8 and the fast-path rule (16-byte loads); else scalar loads.  A launch's grid is its estimates x their workgroups x
// `tiles` tiles of ant_tile antennas (the last tile the rest); a slice is one record per antenna.
struct StatsPlan {
    bool vec;
    int tiles, ant_tile;
    EstimatePlan est;
};

// The whole gat_sample_stats call (the records may be null: no blanking).  *plan is written only with GAT_OK.
inline Refusal stats_plan(const gat_signal_desc *sig, int32_t B, int32_t bpe, uint32_t flags, const gat_sample_stats_t *stats, int num_cus,
                          StatsPlan *plan)
{
    if (!stats || !plan) return {GAT_ERR_ARG, "null argument"};
    if (bpe < 1) return {GAT_ERR_ARG, "blocks_per_estimate must be positive"};
    if (flags & ~(uint32_t)GAT_COND_BLANK_ALL_ANTS) return {GAT_ERR_ARG, "unknown flags"};
    const Refusal r = cond_check_signal(sig, B);
    if (r.code != GAT_OK) return r;
    const int M = sig->num_ants;
    StatsPlan p{};
    p.vec = M <= kStatsTile && blocks_aligned(sig, B);
    p.tiles = (M + kStatsTile - 1) / kStatsTile;
    p.ant_tile = M < kStatsTile ? M : kStatsTile;
    // the covariance's split: (block, segment) units, G workgroups an estimate
    const long long round_to = (long long)kStatsThreads * (p.vec ? layout_vec_samples(sig->layout) : 1);
    p.est = {B, bpe, sig->num_samples, round_to, 4 * round_to, (long long)num_cus * 8, M * sizeof(gat_sample_stats_t), kStatsScratchCap};
    *plan = p;
    return {GAT_OK, nullptr};
}

} // namespace gat
