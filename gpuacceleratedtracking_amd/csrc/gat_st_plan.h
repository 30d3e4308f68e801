// gat_st_plan.h -- the pure part of gat_spacetime_covariance and gat_spacetime_filter (include/gat.h): their refusals, the
// filter's choice between the tiled and the general kernel, the geometry of both and the work split, as a function of the call's
// arguments alone.  No HIP call and no HIP header: the device entry points, the host twin and the stand-alone test programs
// (tests/stplan; the covariance's split: tests/estplan) compile the same text.
#pragma once

#include "gat_est_plan.h"

namespace gat {

constexpr int kStThreads = 256;
constexpr int kStLaneOutputs = 4;    // outputs a lane of the tiled filter keeps in registers, per beam
constexpr int kStLdsSamples = 4096;  // float pairs of samples a workgroup of the tiled filter stages: 32 KiB
constexpr int kStTiledMaxAnts = 16;  // beyond, the 32 KiB hold less than a round of the workgroup's outputs per antenna
constexpr int kStTiledBeams = 4;     // beams whose sums the tiled filter keeps in registers: one pass over the samples
constexpr int kStGeneralBeams = 8;   // the same for the general kernel (one output per lane)

// ---- the filter ------------------------------------------------------------------------------------------------------------------
// outputs of one tile: what fits the LDS next to the T - 1 sample halo of M rows, in whole rounds of the workgroup where there is one
constexpr int st_tile_outputs(int M, int T)
{
    const int fit = kStLdsSamples / M - (T - 1);
    const int most = kStThreads * kStLaneOutputs;
    return fit >= most ? most : fit >= kStThreads ? fit / kStThreads * kStThreads : fit;
}
// the tile of beams a launch works in: the tiled kernel's 1 or 4, the general kernel's smallest of 1, 2, 4, 8 that holds J (or 8)
constexpr int st_beam_tile(bool tiled, int J) { return tiled ? (J == 1 ? 1 : kStTiledBeams) : J == 1 ? 1 : J == 2 ? 2 : J <= 4 ? 4 : kStGeneralBeams; }

// Work units are (block, chunk of `chunk` outputs), `chunks` to a block: unit u = block * chunks + chunk index (st_unit, gat_st.h); workgroup g of
// `grid` takes units g, g + grid, ...  The tiled kernel walks a unit in tiles of `tile` outputs, whose tile + T - 1 samples of
// every antenna lie in LDS as M rows of `row` float pairs (M * row <= kStLdsSamples).
struct StPlan {
    bool tiled;
    int tile, row, beams; // beams: the beam tile (st_beam_tile)
    long long outputs, chunk, chunks, units, grid;
};

// what both entry points ask of num_taps and the signal
inline Refusal st_check_signal(const gat_signal_desc *sig, int32_t B, int32_t T, Refusal chan_stride)
{
    if (T < 1 || T > GAT_MAX_ST_TAPS) return {GAT_ERR_RANGE, "num_taps outside 1 .. 16"};
    const Refusal r = check_desc(sig, B, GAT_MAX_ARRAY_ANTS, signal_refusals(chan_stride));
    if (r.code != GAT_OK) return r;
    if (sig->num_ants * T > GAT_MAX_ARRAY_ANTS) return {GAT_ERR_RANGE, "num_ants * num_taps above 64"};
    if (sig->num_samples < T) return {GAT_ERR_ARG, "a block is shorter than the tap delay line"};
    return {GAT_OK, nullptr};
}

// The whole filter call.  workgroups_wanted: about eight a compute unit on the device.  *plan is written only with GAT_OK.
inline Refusal st_filter_plan(const gat_signal_desc *sig, int32_t B, const double *w_re, const double *w_im, int32_t T, int32_t J,
                              const gat_signal_desc *out, long long workgroups_wanted, StPlan *plan)
{
    // (a bad size of the output is caught as a difference from num_beams or from the signal: `sizes` is left a negative stride)
    constexpr DescRefusals kOutput{{GAT_ERR_ARG, "bad output layout"}, {GAT_ERR_ARG, "bad output planes"}, {GAT_ERR_ARG, "negative output stride"},
                                   {GAT_ERR_ARG, "the output's ant_stride must be positive"}, {GAT_ERR_ARG, "the output's block_stride must be positive"},
                                   {GAT_ERR_RANGE, "more than 64 beams"}, {GAT_ERR_UNSUPPORTED, "chan_stride must be 0 on both sides"},
                                   {GAT_ERR_RANGE, "signal extent too large"}};
    if (!sig || !out || !w_re || !w_im || !plan) return {GAT_ERR_ARG, "null argument"};
    if (B < 1 || J < 1) return {GAT_ERR_ARG, "num_blocks and num_beams must be positive"};
    Refusal r = st_check_signal(sig, B, T, {GAT_ERR_UNSUPPORTED, "chan_stride must be 0 on both sides"});
    if (r.code != GAT_OK) return r;
    if (J > GAT_MAX_ARRAY_ANTS) return kOutput.ants;
    const long long No = sig->num_samples - T + 1;
    if (out->num_ants != J) return {GAT_ERR_ARG, "the output's num_ants must be num_beams"};
    if (out->num_samples != No) return {GAT_ERR_ARG, "the output's num_samples must be N - num_taps + 1"};
    if (out->layout == GAT_LAYOUT_INTERLEAVED_I16 || out->layout == GAT_LAYOUT_INTERLEAVED_I8)
        return {GAT_ERR_UNSUPPORTED, "the output is float32: planar or interleaved"};
    r = check_desc(out, B, GAT_MAX_ARRAY_ANTS, kOutput);
    if (r.code != GAT_OK) return r;
    if (descs_overlap(sig, out, B)) return {GAT_ERR_ARG, "the output overlaps the signal"};

    StPlan p{};
    const int M = sig->num_ants;
    p.tiled = M <= kStTiledMaxAnts && blocks_aligned(sig, B) && blocks_aligned(out, B);
    p.tile = p.tiled ? st_tile_outputs(M, T) : kStThreads;
    p.row = p.tile + T - 1;
    p.beams = st_beam_tile(p.tiled, J);
    p.outputs = No;
    const ChunkSplit s = split_chunks(B, No, p.tile, workgroups_wanted);
    p.chunk = s.chunk, p.chunks = s.chunks, p.units = s.units, p.grid = s.grid;
    *plan = p;
    return {GAT_OK, nullptr};
}

// ---- the covariance --------------------------------------------------------------------------------------------------------------
constexpr int kStCovThreads = 512; // 4 x 4 tiles of the upper triangle x sample phases, as the spatial covariance's tiled kernel
constexpr int kStCovTile = 4;
constexpr int kStCovPad = 4;       // float pairs in front of the staged samples: what the last tile's elements beyond Q read

// Geometry for M antennas and T taps, Q = M * T: nt x nt tiles of 4 x 4 elements, the upper ones (tiles) spread over the
// workgroup's threads with `phases` snapshot phases each; a step takes `chunk` = phases * per_phase snapshots, whose chunk + T - 1
// samples of every antenna are staged as `cols` columns of M float pairs, antennas in REVERSE order inside a column: element q of
// the snapshot whose newest sample is column c lies at kStCovPad + (c + 1) * M - 1 - q, so a snapshot is one contiguous run.
struct StCovGeom {
    int Q, nt, tiles, phases, per_phase, chunk, cols;
    size_t lds_bytes;
};
inline StCovGeom st_cov_geom(int M, int T)
{
    StCovGeom g{};
    g.Q = M * T;
    g.nt = (g.Q + kStCovTile - 1) / kStCovTile;
    g.tiles = g.nt * (g.nt + 1) / 2;
    g.phases = kStCovThreads / g.tiles;
    const int budget = (32768 / 8 - kStCovPad) / M - (T - 1); // snapshots whose samples 32 KiB hold
    g.per_phase = budget / g.phases < 1 ? 1 : (budget / g.phases > 8 ? 8 : budget / g.phases);
    g.chunk = g.phases * g.per_phase;
    g.cols = g.chunk + T - 1;
    const size_t stage = ((size_t)g.cols * M + kStCovPad) * 8, reduce = (size_t)kStCovThreads * 16 * sizeof(float);
    g.lds_bytes = stage > reduce ? stage : reduce;
    return g;
}

constexpr size_t kStCovScratchCap = (size_t)256 << 20; // bytes of the workgroups' slices of one launch; more estimates go in batches

// The covariance call's refusals alone
inline Refusal st_cov_plan(const gat_signal_desc *sig, int32_t B, int32_t bpe, int32_t T, const float *cov_re, const float *cov_im)
{
    if (!sig || !cov_re || !cov_im) return {GAT_ERR_ARG, "null argument"};
    if (B < 1 || bpe < 1) return {GAT_ERR_ARG, "num_blocks and blocks_per_estimate must be positive"};
    return st_check_signal(sig, B, T, {GAT_ERR_UNSUPPORTED, "chan_stride must be 0 (one signal, one covariance)"});
}

// The split is over a block's snapshots (est.N = N - T + 1); a slice is [2][Q][Q] floats, Q = M * T.
struct StCovPlan {
    int Q;
    EstimatePlan est;
};

// The whole covariance call (num_taps == 1 is forwarded to gat_spatial_covariance after the refusals: its plan is cov_plan's).
// *plan is written only with GAT_OK.
inline Refusal st_cov_plan(const gat_signal_desc *sig, int32_t B, int32_t bpe, int32_t T, const float *cov_re, const float *cov_im, int num_cus,
                           StCovPlan *plan)
{
    if (!plan) return {GAT_ERR_ARG, "null argument"};
    const Refusal r = st_cov_plan(sig, B, bpe, T, cov_re, cov_im);
    if (r.code != GAT_OK) return r;
    const int Q = sig->num_ants * T;
    const long long chunk = st_cov_geom(sig->num_ants, T).chunk;
    *plan = {Q, {B, bpe, sig->num_samples - T + 1, chunk, 8 * chunk, (long long)num_cus * 4, (size_t)2 * Q * Q * sizeof(float), kStCovScratchCap}};
    return {GAT_OK, nullptr};
}

} // namespace gat
