// gat_array_kernels.h -- what the array kernels (gat_array.hip) and their host side (gat_array_api.cpp) share: the covariance
// kernels' geometry, their arguments and the launchers.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "gat.h"

namespace gat {

constexpr int kCovSmallMaxAnts = 8;  // the streaming kernel keeps the whole upper triangle in registers up to here
constexpr int kCovSmallThreads = 256;
constexpr int kCovTileThreads = 512; // the LDS-tiled kernel: 4 x 4 antenna tiles x sample phases
constexpr int kCovTile = 4;
constexpr int kCovFinishLanes = 64;  // the finishing kernel adds a (estimate, element)'s slices in this many interleaved runs

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

// One covariance call.  Work units are (block, segment of seg_len samples): estimate e owns blocks [e * bpe, min(B, (e+1) * bpe))
// and G workgroups (workgroup e * G + g of the grid); workgroup g of e takes its units g, g + G, ... and writes its sums to slice
// (e * G + g) of `partial` ([2][M][M] floats, upper triangle only).
struct CovArgs {
    const void *re, *im;
    int M, B, bpe, E, G, splits;
    long long N, ant_stride, block_stride, seg_len;
    float *partial;
};

hipError_t launch_cov_small(const CovArgs &a, int fmt, hipStream_t st);  // M <= 8, 16-byte loads
hipError_t launch_cov_tiled(const CovArgs &a, int fmt, hipStream_t st);  // any M <= 64, any alignment
hipError_t launch_cov_finish(const float *partial, int M, int E, int G, float *cov_re, float *cov_im, hipStream_t st);
hipError_t array_weights_allow_lds(); // 64 antennas need more than 64 KB of LDS for the factor's two FP64 planes
// l_re | l_im | ok: scratch of 2 * M * M doubles and one int the factor kernel writes and the solve kernel reads
hipError_t launch_array_weights(const float *cov_re, const float *cov_im, int M, const double *steer_re, const double *steer_im, int K,
                                int mode, double loading, double *scratch, double *w_re, double *w_im, hipStream_t st);
hipError_t launch_beamform(const float *acc_re, const float *acc_im, long long rows, int K, int L, int M, const double *w_re,
                           const double *w_im, float *out_re, float *out_im, hipStream_t st);
hipError_t launch_tracking_update_weighted(const float *acc_re, const float *acc_im, int K, int M, const gat_loop_config &cfg,
                                           gat_loop_state *state, const gat_channel_params *cur, gat_channel_params *next,
                                           const double *w_re, const double *w_im, hipStream_t st);

} // namespace gat
