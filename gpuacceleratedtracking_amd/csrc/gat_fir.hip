// gat_fir.hip -- the sample filter (include/gat.h, "sample filtering"): a complex FIR with decimation and an oscillator over the raw
// samples.  The arithmetic is gat_fir.h, shared with the host twin; the refusals, the kernel choice and the work split are
// gat_fir_plan.h.  Every output is one lane's sum in tap order, so the bits depend neither on the kernel nor on the work split.
//   * fir_tiled_kernel<FI, FO>, every block of every antenna on a 16-byte boundary on both sides: a workgroup walks its unit
//     (block, antenna, chunk of outputs) in tiles of a.tile outputs.  It stages the (tile - 1) * D + T samples of a tile with
//     16-byte loads (scalar loads for a block's last N mod VS samples: nothing outside the block is read), converts them to
//     float pairs and stores them in LDS in POLYPHASE order -- the sample `rel` places after the tile's first at row rel mod D,
//     column rel / D of D rows of a.row columns.  Lane l owns outputs l, l + 256, ... of the tile (up to kFirLaneOutputs, in
//     registers: that many independent FMA chains); tap t of output j is the sample (T - 1 - t) + j * D, so for every tap the
//     lanes of a wave read consecutive columns of ONE row with ds_read_b64: 32 lanes x 8 bytes are the 64 banks once, for every
//     D.  (Sample-major order would read at a lane stride of 2 D dwords: a 2- to 32-way conflict for every even D.)  The taps
//     are restrict-qualified kernel parameters read at a uniform index: scalar loads (s_load_dwordx4: four taps of a plane).  Stores are one float (planar: two planes) or one float pair per lane,
//     consecutive over the lanes.
//   * fir_general_kernel<FI, FO>, any base and strides: one output per lane, scalar loads from global memory for every tap
//     (neighbouring lanes' samples overlap in the cache), the taps staged once in LDS, a component per store.
#include <hip/hip_runtime.h>

#include "gat_fir.h"
#include "gat_fir_kernels.h"
#include "gat_sample_load.h"

namespace gat {

namespace {

// where the sample `rel` places after a tile's first lies in LDS: row rel mod D, column rel / D
__device__ __forceinline__ unsigned fir_lds_index(unsigned rel, unsigned D, unsigned row)
{
    if (D == 1u) return rel;
    const unsigned col = rel / D;
    return (rel - col * D) * row + col;
}

// The sums of a tile's outputs j = tid + k * 256 < nt, k < NR, from the staged samples, rotated and stored.
template <int FO, int NR>
__device__ __forceinline__ void fir_tile_outputs_run(const FirArgs &a, const float *__restrict__ taps_re, const float *__restrict__ taps_im, const float2 *s_x,
                                                     int tid, int nt, long long qt, long long stream0, size_t obase)
{
    float zr[NR], zi[NR];
    int j[NR];
#pragma unroll
    for (int k = 0; k < NR; ++k) {
        zr[k] = zi[k] = 0.0f;
        const int jk = tid + k * kFirThreads;
        j[k] = jk < nt ? jk : 0; // a lane without an output reads output 0's samples and stores nothing
    }
    // tap t reads the samples e = T - 1 - t places after each output's first: row e mod D, column e / D + j
    int er = (a.T - 1) % a.D, ec = (a.T - 1) / a.D;
#pragma unroll 4
    for (int t = 0; t < a.T; ++t) {
        const float gr = taps_re[t], gi = taps_im[t];
        const float2 *line = s_x + er * a.row + ec;
#pragma unroll
        for (int k = 0; k < NR; ++k) {
            const float2 x = line[j[k]];
            fir_tap(zr[k], zi[k], gr, gi, x.x, x.y);
        }
        if (er == 0)
            er = a.D - 1, --ec;
        else
            --er;
    }
#pragma unroll
    for (int k = 0; k < NR; ++k) {
        const int jk = tid + k * kFirThreads;
        if (jk >= nt) continue;
        const long long q = qt + jk;
        float yr, yi;
        fir_rotate(a.nco, stream0 + q * a.D + (a.T - 1), zr[k], zi[k], yr, yi);
        if constexpr (FO == GAT_LAYOUT_PLANAR) {
            a.out_re[obase + (size_t)q] = yr;
            a.out_im[obase + (size_t)q] = yi;
        } else {
            reinterpret_cast<float2 *>(a.out_re)[obase + (size_t)q] = make_float2(yr, yi); // (the output's blocks are 16-byte aligned)
        }
    }
}

// ---- aligned on both sides: samples staged in LDS in polyphase order -------------------------------------------------------------
template <int FI, int FO>
__global__ void __launch_bounds__(kFirThreads) fir_tiled_kernel(const FirArgs a, const float *__restrict__ taps_re, const float *__restrict__ taps_im)
{
    using Vec = SampleVec<FI, false>;
    constexpr int VS = Vec::VS;
    __shared__ float2 s_x[kFirLdsSamples];
    const int tid = threadIdx.x;
    for (long long u = blockIdx.x; u < a.units; u += gridDim.x) {
        long long b, q0, q1;
        int m;
        fir_unit(u, a.chunks, a.chunk, a.Q, a.M, &b, &m, &q0, &q1);
        const size_t base = (size_t)b * (size_t)a.block_stride + (size_t)m * (size_t)a.ant_stride;
        const size_t obase = (size_t)b * (size_t)a.out_block_stride + (size_t)m * (size_t)a.out_ant_stride;
        for (long long qt = q0; qt < q1; qt += a.tile) {
            const int nt = (int)(q1 - qt < a.tile ? q1 - qt : a.tile);
            // the tile's samples [p0, p1) of the block: p1 <= N by the definition of Q
            const long long p0 = qt * a.D, p1 = p0 + (long long)(nt - 1) * a.D + a.T;
            __syncthreads(); // the last tile's sums have read their samples
            // whole 16-byte vectors inside the block, from the one that holds p0 on
            const long long v_end = (p1 + VS - 1) / VS, v_in = a.N / VS, v1 = v_end < v_in ? v_end : v_in;
            for (long long v = p0 / VS + tid; v < v1; v += kFirThreads) {
                Vec raw;
                raw.load(a.re, a.im, base, v);
#pragma unroll
                for (int s = 0; s < VS; ++s) {
                    const long long p = v * VS + s;
                    if (p < p0 || p >= p1) continue;
                    float xr, xi;
                    raw.sample(s, xr, xi);
                    s_x[fir_lds_index((unsigned)(p - p0), (unsigned)a.D, (unsigned)a.row)] = make_float2(xr, xi);
                }
            }
            // the block's last N mod VS samples, one to a lane
            const long long t0 = v1 * VS > p0 ? v1 * VS : p0;
            for (long long p = t0 + tid; p < p1; p += kFirThreads) {
                float xr, xi;
                load_sample<FI>(a.re, a.im, base + (size_t)p, xr, xi);
                s_x[fir_lds_index((unsigned)(p - p0), (unsigned)a.D, (unsigned)a.row)] = make_float2(xr, xi);
            }
            __syncthreads();
            const long long stream0 = b * a.block_stride;
            switch ((nt + kFirThreads - 1) / kFirThreads) { // (uniform: the rounds of the workgroup this tile has outputs for)
            case 1: fir_tile_outputs_run<FO, 1>(a, taps_re, taps_im, s_x, tid, nt, qt, stream0, obase); break;
            case 2: fir_tile_outputs_run<FO, 2>(a, taps_re, taps_im, s_x, tid, nt, qt, stream0, obase); break;
            case 3: fir_tile_outputs_run<FO, 3>(a, taps_re, taps_im, s_x, tid, nt, qt, stream0, obase); break;
            default: fir_tile_outputs_run<FO, kFirLaneOutputs>(a, taps_re, taps_im, s_x, tid, nt, qt, stream0, obase); break;
            }
        }
    }
}

// ---- any alignment: one output per lane --------------------------------------------------------------------------------------------
template <int FI, int FO>
__global__ void __launch_bounds__(kFirThreads) fir_general_kernel(const FirArgs a)
{
    __shared__ float2 s_g[GAT_MAX_FIR_TAPS]; // every lane reads the same address (a broadcast)
    const int tid = threadIdx.x;
    for (int t = tid; t < a.T; t += kFirThreads) s_g[t] = make_float2(a.taps_re[t], a.taps_im[t]);
    __syncthreads();
    for (long long u = blockIdx.x; u < a.units; u += gridDim.x) {
        long long b, q0, q1;
        int m;
        fir_unit(u, a.chunks, a.chunk, a.Q, a.M, &b, &m, &q0, &q1);
        const size_t base = (size_t)b * (size_t)a.block_stride + (size_t)m * (size_t)a.ant_stride;
        const size_t obase = (size_t)b * (size_t)a.out_block_stride + (size_t)m * (size_t)a.out_ant_stride;
        for (long long q = q0 + tid; q < q1; q += kFirThreads) {
            const long long p = q * a.D + (a.T - 1);
            float zr = 0.0f, zi = 0.0f;
            for (int t = 0; t < a.T; ++t) {
                float xr, xi;
                load_sample<FI>(a.re, a.im, base + (size_t)(p - t), xr, xi);
                const float2 g = s_g[t];
                fir_tap(zr, zi, g.x, g.y, xr, xi);
            }
            float yr, yi;
            fir_rotate(a.nco, b * a.block_stride + p, zr, zi, yr, yi);
            const size_t e = obase + (size_t)q;
            if constexpr (FO == GAT_LAYOUT_PLANAR) {
                a.out_re[e] = yr;
                a.out_im[e] = yi;
            } else {
                a.out_re[2 * e] = yr;
                a.out_re[2 * e + 1] = yi;
            }
        }
    }
}

template <int FI, bool TILED>
void fir_dispatch_out(const FirArgs &a, int fo, int grid, hipStream_t st)
{
    const dim3 g((unsigned)grid), b(kFirThreads);
    if constexpr (TILED) {
        if (fo == GAT_LAYOUT_PLANAR)
            hipLaunchKernelGGL((fir_tiled_kernel<FI, GAT_LAYOUT_PLANAR>), g, b, 0, st, a, a.taps_re, a.taps_im);
        else
            hipLaunchKernelGGL((fir_tiled_kernel<FI, GAT_LAYOUT_INTERLEAVED>), g, b, 0, st, a, a.taps_re, a.taps_im);
    } else {
        if (fo == GAT_LAYOUT_PLANAR)
            hipLaunchKernelGGL((fir_general_kernel<FI, GAT_LAYOUT_PLANAR>), g, b, 0, st, a);
        else
            hipLaunchKernelGGL((fir_general_kernel<FI, GAT_LAYOUT_INTERLEAVED>), g, b, 0, st, a);
    }
}

template <bool TILED>
hipError_t fir_dispatch(const FirArgs &a, int fi, int fo, int grid, hipStream_t st)
{
    if (a.M < 1 || a.M > GAT_MAX_ARRAY_ANTS || a.T < 1 || a.T > GAT_MAX_FIR_TAPS || a.D < 1 || a.D > GAT_MAX_FIR_DECIMATION || grid < 1 ||
        (fo != GAT_LAYOUT_PLANAR && fo != GAT_LAYOUT_INTERLEAVED))
        return hipErrorInvalidValue;
    if (TILED && (a.tile < 1 || a.tile > kFirThreads * kFirLaneOutputs || a.row < a.tile + fir_halo_cols(a.T, a.D) || (long long)a.row * a.D > kFirLdsSamples))
        return hipErrorInvalidValue;
    dispatch_layout(fi, [&](auto FI) { fir_dispatch_out<FI, TILED>(a, fo, grid, st); });
    return hipGetLastError();
}

} // namespace

hipError_t launch_fir_tiled(const FirArgs &a, int fmt_in, int fmt_out, int grid, hipStream_t st) { return fir_dispatch<true>(a, fmt_in, fmt_out, grid, st); }

hipError_t launch_fir_general(const FirArgs &a, int fmt_in, int fmt_out, int grid, hipStream_t st) { return fir_dispatch<false>(a, fmt_in, fmt_out, grid, st); }

} // namespace gat
