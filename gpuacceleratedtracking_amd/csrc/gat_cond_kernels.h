// gat_cond_kernels.h -- what the sample conditioner's kernels (gat_cond.hip) and their host side (gat_cond_api.cpp) share:
// the kernels' arguments and the launchers.  The geometry and the work split are gat_cond_plan.h.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "gat.h"
#include "gat_cond_plan.h"

namespace gat {

// One gat_condition_samples call.  Element (n, m, b) is sample n + m * ant_stride + b * block_stride of its side's planes.
struct CondArgs {
    const void *re, *im;
    void *out_re, *out_im;
    int M, blank_all;
    long long N, ant_stride, block_stride, out_ant_stride, out_block_stride, chunk, chunks, units;
    unsigned long long *counts; // [M][2] or null
};
// M <= 8, every block of every antenna on a 16-byte boundary on both sides; a.chunk a multiple of group * kCondThreads
hipError_t launch_cond_stream(const CondArgs &a, int fmt_in, int fmt_out, const gat_cond_params *prm, int grid, hipStream_t st);
// any M <= 64, any alignment
hipError_t launch_cond_general(const CondArgs &a, int fmt_in, int fmt_out, const gat_cond_params *prm, int grid, hipStream_t st);

// One gat_sample_stats launch.  Estimate e owns blocks [e * bpe, min(B, (e + 1) * bpe)) and G workgroups (blockIdx.x = e * G + g);
// workgroup g of e takes its (block, segment of seg_len samples) units g, g + G, ... and writes one record per antenna of its
// tile to partial[(e * G + g) * M + m].
struct StatsArgs {
    const void *re, *im;
    int M, B, bpe, E, G, splits, blank_all;
    int m_first; // the first antenna of this launch's tiles (the launcher's: callers leave it 0)
    long long N, ant_stride, block_stride, seg_len;
    const gat_cond_params *prm; // or null: every threshold is +inf
    gat_sample_stats_t *partial;
};
// vec: M <= 8 and the fast-path rule (16-byte loads); else scalar loads, tiles of 8 antennas
hipError_t launch_stats(const StatsArgs &a, int fmt, bool vec, hipStream_t st);
// adds the G slices of every (estimate, antenna) in a fixed order
hipError_t launch_stats_finish(const gat_sample_stats_t *partial, int M, int E, int G, gat_sample_stats_t *stats, hipStream_t st);
hipError_t launch_agc_update(const gat_sample_stats_t *stats, int M, double target_rms, double blank_factor, int remove_dc, gat_cond_params *prm,
                             hipStream_t st);

} // namespace gat
