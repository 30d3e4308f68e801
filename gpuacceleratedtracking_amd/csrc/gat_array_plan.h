// gat_array_plan.h -- the pure part of gat_spatial_covariance (include/gat.h): its refusals, the choice between the streaming and
// the LDS-tiled kernel, the tiled kernel's geometry and the work split, as a function of the call's arguments and the device's
// compute units alone.  No HIP call and no HIP header: the device entry point, the kernels and a stand-alone test program
// (tests/estplan) compile the same text.
#pragma once

#include "gat_est_plan.h"

namespace gat {

constexpr int kCovSmallMaxAnts = 8;  // the streaming kernel keeps the whole upper triangle in registers up to here
constexpr int kCovSmallThreads = 256;
constexpr int kCovTileThreads = 512; // the LDS-tiled kernel: 4 x 4 antenna tiles x sample phases
constexpr int kCovTile = 4;
constexpr int kCovFinishLanes = 64;  // the finishing kernel adds a (estimate, element)'s slices in this many interleaved runs
constexpr size_t kCovScratchCap = (size_t)256 << 20; // bytes of the workgroups' slices of one launch; more estimates go in batches

// Geometry of the LDS-tiled kernel for M antennas: nt x nt tiles of 4 x 4, the upper ones (tiles) spread over the
// workgroup's threads with `phases` sample phases each; a chunk of `chunk` = phases * per_phase samples is staged per step
// in rows of `row` float2 (the antennas padded to whole tiles, plus two: consecutive samples start 16 bytes further round
// the banks).
struct CovTileGeom {
    int nt, tiles, phases, per_phase, chunk, row;
    size_t lds_bytes;
};
inline CovTileGeom cov_tile_geom(int M)
{
    CovTileGeom g{};
    g.nt = (M + kCovTile - 1) / kCovTile;
    g.tiles = g.nt * (g.nt + 1) / 2;
    g.phases = kCovTileThreads / g.tiles;
    g.row = g.nt * kCovTile + 2;
    const int budget = 32768 / (g.row * 8); // samples 32 KB hold
    g.per_phase = budget / g.phases < 1 ? 1 : (budget / g.phases > 8 ? 8 : budget / g.phases);
    g.chunk = g.phases * g.per_phase;
    const size_t stage = (size_t)g.chunk * g.row * 8, reduce = (size_t)kCovTileThreads * 16 * sizeof(float);
    g.lds_bytes = stage > reduce ? stage : reduce;
    return g;
}

// vec: the streaming kernel (M <= 8 and the fast-path rule, 16-byte loads); else the tiled one.  A slice is [2][M][M] floats.
struct CovPlan {
    bool vec;
    EstimatePlan est;
};

// The whole call.  *plan is written only with GAT_OK.
inline Refusal cov_plan(const gat_signal_desc *sig, int32_t B, int32_t bpe, const float *cov_re, const float *cov_im, int num_cus, CovPlan *plan)
{
    if (!sig || !cov_re || !cov_im || !plan) return {GAT_ERR_ARG, "null argument"};
    if (B < 1 || bpe < 1) return {GAT_ERR_ARG, "num_blocks and blocks_per_estimate must be positive"};
    // (the antenna limit ahead of the shared check's strides, as this entry point always answered)
    if (sig->num_ants > GAT_MAX_ARRAY_ANTS) return {GAT_ERR_RANGE, "more than 64 antennas"};
    const Refusal r = check_desc(sig, B, GAT_MAX_ARRAY_ANTS, signal_refusals({GAT_ERR_UNSUPPORTED, "chan_stride must be 0 (one signal, one covariance)"}));
    if (r.code != GAT_OK) return r;
    const int M = sig->num_ants;
    CovPlan p{};
    p.vec = M <= kCovSmallMaxAnts && blocks_aligned(sig, B); // the streaming kernel's rule is the correlator's fast-path rule
    // the smallest piece of a block worth a work unit, and what a segment's length is rounded up to
    const long long round_to = p.vec ? (long long)layout_vec_samples(sig->layout) * kCovSmallThreads : cov_tile_geom(M).chunk;
    p.est = {B, bpe, sig->num_samples, round_to, p.vec ? 4 * round_to : 8 * round_to, (long long)num_cus * (p.vec ? 8 : 4),
             (size_t)2 * M * M * sizeof(float), kCovScratchCap};
    *plan = p;
    return {GAT_OK, nullptr};
}

} // namespace gat
