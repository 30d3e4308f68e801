// gat_beam.hip -- beams of the raw samples (include/gat.h gat_beamform_samples): y[n, j, b] = sum_m conj(w[j][m]) x[n, m, b].
//
// The weights are narrowed to float32 once (beam_weights_kernel, float2 in the context's scratch); both kernels then
// run the same sum for every output sample: antennas in order 0 .. M - 1, one FMA per real product,
//   yr = fma(wr, xr, yr); yr = fma(wi, xi, yr); yi = fma(wr, xi, yi); yi = fma(-wi, xr, yi)
// in float32, one thread per output sample and no reduction across threads.  So the result depends neither on the kernel nor
// on the work split, and a repeat call gives the same bits.  Integer samples convert exactly.
//
// Why float32 is enough here when gat_beamform sums in FP64: gat_beamform's terms are accumulators -- sums over a whole block,
// 70 dB and more above their own noise, which a null has to cancel to below that noise.  Here the terms are single samples,
// and what the sum must not disturb is the noise of ONE sample.  A complex dot product of length M is two real FMA chains of
// length 2 M on weights rounded once: |y - y64| <= (4 M + 4) 2^-24 sum_m |w_m| |x_m| (twice the first-order bound).  For a
// jammer 60 dB over the noise (|x| = 1000) on M = 64 antennas with sum |w| = 1 that is 260 * 6e-8 * 1000 = 1.5e-2 of the noise
// amplitude, -36 dB: the rounding adds 0.001 dB to the noise floor, uncorrelated from sample to sample.
//
//   * beam_stream_kernel<FMT, M, JT>, M <= 8, every block of every antenna (input) and beam (output) on a 16-byte boundary: a
//     lane takes one 16-byte non-temporal load per antenna and plane (two for ComplexF32 pairs) -- 4 / 4 / 4 / 8 samples by
//     layout --, all of a step's loads issued before its arithmetic, keeps the sums of JT <= 4 beams in registers and writes
//     them with 16-byte stores (one per plane and 4 samples, or one per 2 interleaved samples).  Up to 4 beams the samples
//     cross HBM once; further beams take further passes of 4.  The weights are wave-uniform: scalar loads of constant data
//     for one beam, a broadcast read of LDS for four (see beam_const_weights_here).  A block's last N mod group samples go
//     one to a lane through scalar loads and stores, in the same kernel.
//   * beam_general_kernel<FMT, JT>, any M <= 64, base and strides: scalar loads, one sample per lane (consecutive lanes,
//     consecutive samples); the weights of the current tile of JT <= 8 beams are staged once per workgroup in LDS as float2
//     (every lane reads the same address: a broadcast); up to 8 beams the samples are read once.
// Work units are (block, chunk of the block), dealt to a grid sized from the CU count by a fixed stride; 64-bit indices.
#include <hip/hip_runtime.h>

#include "gat_beam_kernels.h"
#include "gat_sample_load.h"

namespace gat {

namespace {

typedef float f4 __attribute__((ext_vector_type(4)));

// one term of the sum: y += conj(w) x
__device__ __forceinline__ void beam_term(float wr, float wi, float xr, float xi, float &yr, float &yi)
{
    yr = __builtin_fmaf(wr, xr, yr);
    yr = __builtin_fmaf(wi, xi, yr);
    yi = __builtin_fmaf(wr, xi, yi);
    yi = __builtin_fmaf(-wi, xr, yi);
}

// output element e (n + j * out_ant_stride + b * out_block_stride) in either output layout
__device__ __forceinline__ void beam_store_scalar(const BeamArgs &a, size_t e, float yr, float yi)
{
    if (a.out_im) {
        a.out_re[e] = yr;
        a.out_im[e] = yi;
    } else {
        reinterpret_cast<float2 *>(a.out_re)[e] = make_float2(yr, yi);
    }
}

// The streaming kernel's weights are wave-uniform.  One beam (JT = 1): constant data (a kernel before this one wrote the
// table), read with scalar loads into 2 M scalar registers.  Four beams: 2 M JT = 64 values at M = 8 do not fit into the
// scalar registers beside the addressing (the compiler spilled up to 84 of them), so a pass's weights are staged in LDS and
// every lane reads the same address (a broadcast, no bank conflict).  Either way the pointer passes through an empty asm
// inside the step: that hides its origin from the optimiser, which would otherwise hoist all the loads out of the sample
// loop and keep their results live across it.
typedef const __attribute__((address_space(4))) float2 *BeamConstWeights;
__device__ __forceinline__ BeamConstWeights beam_const_weights_here(const float2 *w)
{
    unsigned long long p = reinterpret_cast<unsigned long long>(w);
    asm volatile("" : "+s"(p));
    return (BeamConstWeights)p;
}
__device__ __forceinline__ const float2 *beam_lds_weights_here(const float2 *s_w)
{
    int off = 0;
    asm volatile("" : "+v"(off));
    return s_w + off;
}

// The one narrowing of the weights, into the order the kernels read: tiles of T beams, antenna-major inside a tile --
// w32[((j / T) * M + m) * T + j % T] = w[j][m] --, so that one antenna's T weights are consecutive (one scalar load, or one
// contiguous copy into LDS).  The last tile is filled up with copies of beam J - 1 (computed by the kernels, never stored).
__global__ void __launch_bounds__(kBeamThreads) beam_weights_kernel(const double *__restrict__ w_re, const double *__restrict__ w_im, int J, int M,
                                                                    int T, float2 *__restrict__ w32)
{
    const int i = blockIdx.x * kBeamThreads + threadIdx.x;
    if (i >= (J + T - 1) / T * T * M) return;
    const int t = i % T, m = (i / T) % M, tile = i / (T * M);
    const int j = tile * T + t < J ? tile * T + t : J - 1;
    w32[i] = make_float2((float)w_re[(size_t)j * M + m], (float)w_im[(size_t)j * M + m]);
}

// ---- M <= 8, aligned: the streaming kernel ------------------------------------------------------------------------------------
template <int FMT, int M, int JT>
__global__ void __launch_bounds__(kBeamThreads) beam_stream_kernel(const BeamArgs a, const float2 *__restrict__ w32)
{
    using Vec = SampleVec<FMT, true>;
    constexpr int VS = Vec::VS, G = beam_group_samples(FMT), NV = G / VS;
    __shared__ float2 s_w[JT == 1 ? 1 : M * JT];
    const int tid = threadIdx.x;
    const unsigned units = (unsigned)a.B * (unsigned)a.chunks, chunks = (unsigned)a.chunks; // below 2^31 (gat_beam_api.cpp)

    for (int j0 = 0; j0 < a.J; j0 += JT) {
        const float2 *w_pass = w32 + (size_t)(j0 / JT) * (M * JT); // this pass's weights [M][JT]
        if constexpr (JT > 1) {
            __syncthreads(); // the previous pass's reads are done
            if (tid < M * JT) s_w[tid] = w_pass[tid];
            __syncthreads();
        }
        for (unsigned u = blockIdx.x; u < units; u += gridDim.x) {
            const unsigned b = u / chunks;
            const long long n0 = (long long)(u - b * chunks) * a.chunk;
            const long long n1 = (n0 + a.chunk < a.N) ? n0 + a.chunk : a.N;
            const size_t base = (size_t)b * (size_t)a.block_stride;
            const size_t obase = (size_t)b * (size_t)a.out_block_stride + (size_t)j0 * (size_t)a.out_ant_stride;
            const long long g1 = n1 / G; // whole groups end here (chunk is a multiple of G: only the block's end can be ragged)
            for (long long gi = n0 / G + tid; gi < g1; gi += kBeamThreads) {
                const auto w = [&] { if constexpr (JT == 1) return beam_const_weights_here(w_pass); else return beam_lds_weights_here(s_w); }();
                Vec raw[M][NV];
#pragma unroll
                for (int m = 0; m < M; ++m)
#pragma unroll
                    for (int q = 0; q < NV; ++q) raw[m][q].load(a.re, a.im, base + (size_t)m * (size_t)a.ant_stride, gi * NV + q);
                float yr[JT][G], yi[JT][G];
#pragma unroll
                for (int t = 0; t < JT; ++t)
#pragma unroll
                    for (int s = 0; s < G; ++s) yr[t][s] = yi[t][s] = 0.f;
#pragma unroll
                for (int m = 0; m < M; ++m)
#pragma unroll
                    for (int s = 0; s < G; ++s) {
                        float xr, xi;
                        raw[m][s / VS].sample(s % VS, xr, xi);
#pragma unroll
                        for (int t = 0; t < JT; ++t) beam_term(w[m * JT + t].x, w[m * JT + t].y, xr, xi, yr[t][s], yi[t][s]);
                    }
                size_t e = obase + (size_t)(gi * G);
#pragma unroll
                for (int t = 0; t < JT; ++t, e += (size_t)a.out_ant_stride) {
                    if (j0 + t >= a.J) break;
                    if (a.out_im) {
#pragma unroll
                        for (int q = 0; q < G / 4; ++q) {
                            f4 vr = {yr[t][4 * q], yr[t][4 * q + 1], yr[t][4 * q + 2], yr[t][4 * q + 3]};
                            f4 vi = {yi[t][4 * q], yi[t][4 * q + 1], yi[t][4 * q + 2], yi[t][4 * q + 3]};
                            *reinterpret_cast<f4 *>(a.out_re + e + 4 * q) = vr;
                            *reinterpret_cast<f4 *>(a.out_im + e + 4 * q) = vi;
                        }
                    } else {
#pragma unroll
                        for (int q = 0; q < G / 2; ++q) {
                            f4 v = {yr[t][2 * q], yi[t][2 * q], yr[t][2 * q + 1], yi[t][2 * q + 1]};
                            *reinterpret_cast<f4 *>(a.out_re + 2 * (e + 2 * q)) = v;
                        }
                    }
                }
            }
            if (n1 == a.N && g1 * G + tid < a.N) { // the block's last N mod G samples: one each for the first lanes
                const size_t n = (size_t)(g1 * G + tid);
                const auto w = [&] { if constexpr (JT == 1) return beam_const_weights_here(w_pass); else return beam_lds_weights_here(s_w); }();
                float yr[JT], yi[JT];
#pragma unroll
                for (int t = 0; t < JT; ++t) yr[t] = yi[t] = 0.f;
#pragma unroll
                for (int m = 0; m < M; ++m) {
                    float xr, xi;
                    load_sample<FMT>(a.re, a.im, base + (size_t)m * (size_t)a.ant_stride + n, xr, xi);
#pragma unroll
                    for (int t = 0; t < JT; ++t) beam_term(w[m * JT + t].x, w[m * JT + t].y, xr, xi, yr[t], yi[t]);
                }
                size_t e = obase + n;
#pragma unroll
                for (int t = 0; t < JT; ++t, e += (size_t)a.out_ant_stride)
                    if (j0 + t < a.J) beam_store_scalar(a, e, yr[t], yi[t]);
            }
        }
    }
}

// ---- any M, any alignment: one sample per lane, the beam tile's weights in LDS --------------------------------------------------
template <int FMT, int JT>
__global__ void __launch_bounds__(kBeamThreads) beam_general_kernel(const BeamArgs a, const float2 *__restrict__ w32)
{
    __shared__ float2 s_w[GAT_MAX_ARRAY_ANTS][JT]; // antenna-major: one antenna's JT weights are consecutive
    const int tid = threadIdx.x, M = a.M;
    const unsigned units = (unsigned)a.B * (unsigned)a.chunks, chunks = (unsigned)a.chunks; // below 2^31 (gat_beam_api.cpp)

    for (int j0 = 0; j0 < a.J; j0 += JT) {
        __syncthreads(); // the previous tile's reads are done
        for (int idx = tid; idx < JT * M; idx += kBeamThreads) (&s_w[0][0])[idx] = w32[(size_t)(j0 / JT) * (size_t)(M * JT) + idx];
        __syncthreads();
        for (unsigned u = blockIdx.x; u < units; u += gridDim.x) {
            const unsigned b = u / chunks;
            const long long n0 = (long long)(u - b * chunks) * a.chunk;
            const long long n1 = (n0 + a.chunk < a.N) ? n0 + a.chunk : a.N;
            const size_t base = (size_t)b * (size_t)a.block_stride;
            const size_t obase = (size_t)b * (size_t)a.out_block_stride + (size_t)j0 * (size_t)a.out_ant_stride;
            for (long long n = n0 + tid; n < n1; n += kBeamThreads) {
                float yr[JT], yi[JT];
#pragma unroll
                for (int t = 0; t < JT; ++t) yr[t] = yi[t] = 0.f;
#pragma unroll 4
                for (int m = 0; m < M; ++m) {
                    float xr, xi;
                    load_sample<FMT>(a.re, a.im, base + (size_t)m * (size_t)a.ant_stride + (size_t)n, xr, xi);
#pragma unroll
                    for (int t = 0; t < JT; ++t) {
                        const float2 w = s_w[m][t];
                        beam_term(w.x, w.y, xr, xi, yr[t], yi[t]);
                    }
                }
                size_t e = obase + (size_t)n;
#pragma unroll
                for (int t = 0; t < JT; ++t, e += (size_t)a.out_ant_stride)
                    if (j0 + t < a.J) beam_store_scalar(a, e, yr[t], yi[t]);
            }
        }
    }
}

template <int FMT, int M>
void beam_stream_launch(const BeamArgs &a, const float2 *w32, int grid, hipStream_t st)
{
    if (a.J == 1)
        hipLaunchKernelGGL((beam_stream_kernel<FMT, M, 1>), dim3((unsigned)grid), dim3(kBeamThreads), 0, st, a, w32);
    else
        hipLaunchKernelGGL((beam_stream_kernel<FMT, M, kBeamStreamTile>), dim3((unsigned)grid), dim3(kBeamThreads), 0, st, a, w32);
}

template <int FMT>
void beam_stream_dispatch(const BeamArgs &a, const float2 *w32, int grid, hipStream_t st)
{
    switch (a.M) {
    case 1: beam_stream_launch<FMT, 1>(a, w32, grid, st); break;
    case 2: beam_stream_launch<FMT, 2>(a, w32, grid, st); break;
    case 3: beam_stream_launch<FMT, 3>(a, w32, grid, st); break;
    case 4: beam_stream_launch<FMT, 4>(a, w32, grid, st); break;
    case 5: beam_stream_launch<FMT, 5>(a, w32, grid, st); break;
    case 6: beam_stream_launch<FMT, 6>(a, w32, grid, st); break;
    case 7: beam_stream_launch<FMT, 7>(a, w32, grid, st); break;
    default: beam_stream_launch<FMT, 8>(a, w32, grid, st); break;
    }
}

template <int FMT>
void beam_general_dispatch(const BeamArgs &a, const float2 *w32, int grid, hipStream_t st)
{
    const dim3 g((unsigned)grid), b(kBeamThreads);
    switch (beam_general_tile(a.J)) {
    case 1: hipLaunchKernelGGL((beam_general_kernel<FMT, 1>), g, b, 0, st, a, w32); break;
    case 2: hipLaunchKernelGGL((beam_general_kernel<FMT, 2>), g, b, 0, st, a, w32); break;
    case 4: hipLaunchKernelGGL((beam_general_kernel<FMT, 4>), g, b, 0, st, a, w32); break;
    default: hipLaunchKernelGGL((beam_general_kernel<FMT, kBeamGeneralTile>), g, b, 0, st, a, w32); break;
    }
}

} // namespace

hipError_t launch_beam_weights(const double *w_re, const double *w_im, int J, int M, int T, float2 *w32, hipStream_t st)
{
    const int count = (J + T - 1) / T * T * M;
    hipLaunchKernelGGL(beam_weights_kernel, dim3((unsigned)((count + kBeamThreads - 1) / kBeamThreads)), dim3(kBeamThreads), 0, st, w_re, w_im, J, M, T,
                       w32);
    return hipGetLastError();
}

hipError_t launch_beam_stream(const BeamArgs &a, int fmt, const float2 *w32, int grid, hipStream_t st)
{
    if (a.M < 1 || a.M > kBeamStreamMaxAnts || grid < 1) return hipErrorInvalidValue;
    dispatch_layout(fmt, [&](auto F) { beam_stream_dispatch<F>(a, w32, grid, st); });
    return hipGetLastError();
}

hipError_t launch_beam_general(const BeamArgs &a, int fmt, const float2 *w32, int grid, hipStream_t st)
{
    if (a.M < 1 || a.M > GAT_MAX_ARRAY_ANTS || grid < 1) return hipErrorInvalidValue;
    dispatch_layout(fmt, [&](auto F) { beam_general_dispatch<F>(a, w32, grid, st); });
    return hipGetLastError();
}

} // namespace gat
