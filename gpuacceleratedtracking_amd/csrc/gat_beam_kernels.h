// gat_beam_kernels.h -- what the sample beamformer's kernels (gat_beam.hip) and their host side (gat_beam_api.cpp) share: the
// kernels' geometry, their arguments and the launchers.  The streaming rule and the work split are gat_beam_plan.h.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "gat.h"
#include "gat_beam_plan.h"

namespace gat {

constexpr int kBeamStreamTile = 4;    // beams whose sums the streaming kernel keeps in registers: one pass over the samples
constexpr int kBeamGeneralTile = 8;   // the same for the general kernel (one sample per lane)
// the general kernel's instances: the smallest tile of 1, 2, 4, 8 beams that holds J (or 8)
constexpr int beam_general_tile(int J) { return J == 1 ? 1 : J == 2 ? 2 : J <= 4 ? 4 : kBeamGeneralTile; }

// One call.  Work units are (block, chunk of `chunk` samples), `chunks` to a block, B * chunks < 2^31; workgroup g of the grid takes units g,
// g + gridDim.x, ...  Output element (n, j, b) is float n + j * out_ant_stride + b * out_block_stride of out_re / out_im
// (planar), or that float2 of out_re (out_im == nullptr: interleaved).
struct BeamArgs {
    const void *re, *im;
    float *out_re, *out_im;
    int M, B, J, chunks;
    long long N, ant_stride, block_stride, out_ant_stride, out_block_stride, chunk;
};

// The tile of beams a launch works in: the streaming kernel's 1 or 4, the general kernel's 1, 2, 4 or 8.
constexpr int beam_tile(bool stream, int J) { return stream ? (J == 1 ? 1 : kBeamStreamTile) : beam_general_tile(J); }
// floats2 of the narrowed table: whole tiles
constexpr size_t beam_weight_count(int J, int M, int T) { return (size_t)((J + T - 1) / T * T) * M; }
// the one narrowing of the weights: w32[((j / T) * M + m) * T + j % T] = {(float)w_re[j][m], (float)w_im[j][m]}
hipError_t launch_beam_weights(const double *w_re, const double *w_im, int J, int M, int T, float2 *w32, hipStream_t st);
// M <= 8, every block of every antenna and beam on a 16-byte boundary; a.chunk a multiple of beam_group_samples * kBeamThreads
hipError_t launch_beam_stream(const BeamArgs &a, int fmt, const float2 *w32, int grid, hipStream_t st);
// any M <= 64, any alignment; a.chunk a multiple of kBeamThreads
hipError_t launch_beam_general(const BeamArgs &a, int fmt, const float2 *w32, int grid, hipStream_t st);

} // namespace gat
