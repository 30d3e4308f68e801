// gat_fir_plan.h -- the pure part of gat_filter_samples (include/gat.h): its refusals, the choice between the tiled and the
// general kernel and the work split, as a function of the two descriptors and the configuration alone.  No HIP call and no HIP
// header: the device entry point, the host twin and a stand-alone test program (tests/firplan) compile the same text.
#pragma once

#include "gat_sig_plan.h"

namespace gat {

constexpr int kFirThreads = 256;
constexpr int kFirLaneOutputs = 4;     // outputs a lane of the tiled kernel keeps in registers (R)
constexpr int kFirLdsSamples = 4096;   // float pairs of samples a workgroup of the tiled kernel stages: 32 KiB, five workgroups a CU
constexpr double kFirMaxStream = 2147483648.0; // samples of an antenna's stream one call may span: theta rounds a value below 2^30

// Work units are (block, antenna, chunk of `chunk` outputs), `chunks` to a (block, antenna) pair: unit u = (block * M + antenna) *
// chunks + chunk index; workgroup g of `grid` takes units g, g + grid, ...  The tiled kernel walks a unit in tiles of `tile`
// outputs, whose tile * D + T - 1 samples lie in LDS in polyphase order, D rows of `row` columns (D * row <= kFirLdsSamples).
struct FirPlan {
    bool tiled;
    int tile, row;
    long long Q, chunk, chunks, units, grid;
};

// unit u: its block, antenna and outputs [q0, q1)
#if defined(__HIPCC__)
__host__ __device__
#endif
inline void fir_unit(long long u, long long chunks, long long chunk, long long Q, int M, long long *b, int *m, long long *q0, long long *q1)
{
    const long long bm = u / chunks;
    *b = bm / M;
    *m = (int)(bm - *b * M);
    *q0 = (u - bm * chunks) * chunk;
    *q1 = *q0 + chunk < Q ? *q0 + chunk : Q;
}

// columns of the taps' reach beyond a tile's outputs: ceil((T - 1) / D)
constexpr int fir_halo_cols(int T, int D) { return (T - 1 + D - 1) / D; }
// outputs of one tile: what fits the LDS next to the halo, in whole rounds of the workgroup where there is one, four at the most
constexpr int fir_tile_outputs(int T, int D)
{
    const int fit = kFirLdsSamples / D - fir_halo_cols(T, D) - 1; // (one column to spare: an odd row length)
    const int most = kFirThreads * kFirLaneOutputs;
    return fit >= most ? most : fit >= kFirThreads ? fit / kFirThreads * kFirThreads : fit;
}

inline bool fir_finite(double v) { return v - v == 0.0; }

// The whole call.  workgroups_wanted: about eight a compute unit on the device.  *plan is written only with GAT_OK.
inline Refusal fir_plan(const gat_signal_desc *sig, int32_t B, const float *taps_re, const float *taps_im, const gat_fir_config *cfg,
                        const gat_signal_desc *out, long long workgroups_wanted, FirPlan *plan)
{
    constexpr DescRefusals kOutput{{GAT_ERR_ARG, "bad output layout"}, {GAT_ERR_ARG, "bad output planes"}, {GAT_ERR_ARG, "bad output sizes"},
                                   {GAT_ERR_ARG, "the output's ant_stride must be positive"},
                                   {GAT_ERR_ARG, "the output's block_stride must be positive"}, {GAT_OK, nullptr},
                                   {GAT_ERR_UNSUPPORTED, "chan_stride must be 0 on both sides"}, {GAT_ERR_RANGE, "signal extent too large"}};
    if (!sig || !out || !taps_re || !taps_im || !cfg || !plan) return {GAT_ERR_ARG, "null argument"};
    if (cfg->struct_size != sizeof(gat_fir_config)) return {GAT_ERR_ARG, "struct_size is not sizeof(gat_fir_config)"};
    if (B < 1) return {GAT_ERR_ARG, "num_blocks must be positive"};
    if (cfg->num_taps < 1 || cfg->num_taps > GAT_MAX_FIR_TAPS) return {GAT_ERR_RANGE, "num_taps outside 1 .. 256"};
    if (cfg->decimation < 1 || cfg->decimation > GAT_MAX_FIR_DECIMATION) return {GAT_ERR_RANGE, "decimation outside 1 .. 64"};
    if (!fir_finite(cfg->nco_step) || !fir_finite(cfg->nco_phase)) return {GAT_ERR_ARG, "the oscillator's step and phase must be finite"};
    Refusal r = check_desc(sig, B, GAT_MAX_ARRAY_ANTS, signal_refusals({GAT_ERR_UNSUPPORTED, "chan_stride must be 0 on both sides"}));
    if (r.code != GAT_OK) return r;
    const int T = cfg->num_taps, D = cfg->decimation, M = sig->num_ants;
    const long long N = sig->num_samples;
    if (N < T) return {GAT_ERR_ARG, "a block is shorter than the filter"};
    if ((double)(B - 1) * (double)sig->block_stride + (double)N > kFirMaxStream) return {GAT_ERR_RANGE, "the call spans more than 2^31 samples of a stream"};
    if (out->layout == GAT_LAYOUT_INTERLEAVED_I16 || out->layout == GAT_LAYOUT_INTERLEAVED_I8)
        return {GAT_ERR_UNSUPPORTED, "the output is float32: planar or interleaved"};
    r = check_desc(out, B, 0, kOutput);
    if (r.code != GAT_OK) return r;
    const long long Q = (N - T) / D + 1;
    if (out->num_ants != M) return {GAT_ERR_ARG, "the output's num_ants must be the signal's"};
    if (out->num_samples != Q) return {GAT_ERR_ARG, "the output's num_samples must be (N - T) / D + 1"};
    if (descs_overlap(sig, out, B)) return {GAT_ERR_ARG, "the output overlaps the signal"};

    FirPlan p{};
    p.tiled = blocks_aligned(sig, B) && blocks_aligned(out, B);
    p.tile = p.tiled ? fir_tile_outputs(T, D) : kFirThreads;
    p.row = p.tile + fir_halo_cols(T, D);
    p.row += p.row % 2 == 0; // an odd row length spreads the staging stores over the banks
    p.Q = Q;
    const ChunkSplit s = split_chunks((long long)B * M, Q, p.tile, workgroups_wanted);
    p.chunk = s.chunk, p.chunks = s.chunks, p.units = s.units, p.grid = s.grid;
    *plan = p;
    return {GAT_OK, nullptr};
}

} // namespace gat
