// gat_cond.hip -- sample conditioning (include/gat.h): the conditioned stream (blanked, scaled, requantised), the level
// statistics and the AGC's records.  The per-sample arithmetic is gat_cond.h, shared with the host twins.
//
// gat_condition_samples: every output sample is one thread's work on one input sample (and, with GAT_COND_BLANK_ALL_ANTS, on
// the same sample of the other antennas), so the bits depend neither on the kernel nor on the work split.
//   * cond_stream_kernel<FI, FO, M>, M <= 8, every block of every antenna on a 16-byte boundary on both sides: a lane owns a
//     group of G = 4 (8 where either side is int8 pairs) consecutive samples of ALL M antennas -- it needs them all for the
//     common verdict --, takes them with 16-byte non-temporal loads (G / VS per antenna and plane: two for a float input next
//     to an int8 output, four for ComplexF32), all of a step's loads issued before its arithmetic, and writes each antenna's
//     group with whole 16-byte stores.  The records are wave-uniform and live in vector registers, as the antenna strides do (the scalar file is the verdicts').  A block's last N mod G samples
//     go one to a lane through scalar loads and stores, in the same kernel.
//   * cond_general_kernel<FI, FO>, any M <= 64, base and strides: one sample per lane, scalar loads and stores, the records
//     in LDS; with GAT_COND_BLANK_ALL_ANTS a first pass over the antennas gives the verdict.
// Work units are (block, chunk), dealt to the grid by a fixed stride (gat_cond_plan.h); 64-bit sample indices.  Counts are
// integer sums: per-lane counters and one 64-bit atomic per wave and antenna (streaming), wave ballots into LDS (general).
//
// gat_sample_stats: stats_kernel<FI, MT, VEC> keeps the sums of MT <= 8 antennas in registers, in FP64 from the first
// addition on (the kernel is bound by its loads: 4 FP64 operations a sample are free), so a DC offset 100 times the noise over
// 2^21 samples costs nothing; VEC: 16-byte non-temporal loads under the fast-path rule, else scalar loads.  More than 8
// antennas run as tiles of 8 in blockIdx.y and a last tile of M mod 8.  Every workgroup ends with a wave butterfly and its four waves in order and
// writes one record per antenna to its slice of the context's scratch; stats_finish_kernel adds a (estimate, antenna)'s
// slices in 64 interleaved runs and a butterfly.  No float atomics: the same bits on every call.
#include <hip/hip_runtime.h>

#include "gat_cond.h"
#include "gat_cond_kernels.h"
#include "gat_sample_load.h"

namespace gat {

namespace {

constexpr bool cond_is_int(int fmt) { return fmt == GAT_LAYOUT_INTERLEAVED_I16 || fmt == GAT_LAYOUT_INTERLEAVED_I8; }

// One output sample as two 32-bit payloads: a float output's bits, an integer output's codes.  A blanked sample is all zero
// bits in every layout (+0.0, +0.0 or 0, 0).  clips: components of this sample that were clipped.
template <int FO>
__device__ __forceinline__ void cond_sample(float xr, float xi, bool keep, float scale, float dc_re, float dc_im, unsigned &o_re, unsigned &o_im,
                                            unsigned &clips)
{
    o_re = o_im = 0u;
    clips = 0u;
    if (!keep) return;
    const float yr = cond_value(xr, dc_re, scale), yi = cond_value(xi, dc_im, scale);
    if constexpr (!cond_is_int(FO)) {
        o_re = __float_as_uint(yr);
        o_im = __float_as_uint(yi);
    } else {
        constexpr int lim = FO == GAT_LAYOUT_INTERLEAVED_I16 ? 32767 : 127;
        bool c_re, c_im;
        o_re = (unsigned)cond_code(yr, lim, &c_re);
        o_im = (unsigned)cond_code(yi, lim, &c_im);
        clips = (unsigned)c_re + (unsigned)c_im;
    }
}

// bit s of `bits` spread over a word: all ones or zero (one bit-field extract)
__device__ __forceinline__ unsigned cond_spread_bit(unsigned bits, int s) { return (unsigned)(((int)(bits << (31 - s))) >> 31); }

// element e of the output, scalar stores (a component at a time where the base may sit on any sample boundary)
template <int FO>
__device__ __forceinline__ void cond_store_scalar(void *re, void *im, size_t e, unsigned o_re, unsigned o_im)
{
    if constexpr (FO == GAT_LAYOUT_PLANAR) {
        static_cast<unsigned *>(re)[e] = o_re;
        static_cast<unsigned *>(im)[e] = o_im;
    } else if constexpr (FO == GAT_LAYOUT_INTERLEAVED) {
        static_cast<unsigned *>(re)[2 * e] = o_re;
        static_cast<unsigned *>(re)[2 * e + 1] = o_im;
    } else if constexpr (FO == GAT_LAYOUT_INTERLEAVED_I16) {
        static_cast<short *>(re)[2 * e] = (short)(int)o_re;
        static_cast<short *>(re)[2 * e + 1] = (short)(int)o_im;
    } else {
        static_cast<signed char *>(re)[2 * e] = (signed char)(int)o_re;
        static_cast<signed char *>(re)[2 * e + 1] = (signed char)(int)o_im;
    }
}

// G consecutive samples from element e (a multiple of G, on a 16-byte boundary) as whole 16-byte stores
template <int FO, int G>
__device__ __forceinline__ void cond_store_group(void *re, void *im, size_t e, const unsigned (&o_re)[G], const unsigned (&o_im)[G])
{
    if constexpr (FO == GAT_LAYOUT_PLANAR) {
#pragma unroll
        for (int q = 0; q < G / 4; ++q) {
            const u4 vr = {o_re[4 * q], o_re[4 * q + 1], o_re[4 * q + 2], o_re[4 * q + 3]};
            const u4 vi = {o_im[4 * q], o_im[4 * q + 1], o_im[4 * q + 2], o_im[4 * q + 3]};
            *reinterpret_cast<u4 *>(static_cast<unsigned *>(re) + e + 4 * q) = vr;
            *reinterpret_cast<u4 *>(static_cast<unsigned *>(im) + e + 4 * q) = vi;
        }
    } else if constexpr (FO == GAT_LAYOUT_INTERLEAVED) {
#pragma unroll
        for (int q = 0; q < G / 2; ++q) {
            const u4 v = {o_re[2 * q], o_im[2 * q], o_re[2 * q + 1], o_im[2 * q + 1]};
            *reinterpret_cast<u4 *>(static_cast<unsigned *>(re) + 2 * (e + 2 * q)) = v;
        }
    } else if constexpr (FO == GAT_LAYOUT_INTERLEAVED_I16) {
#pragma unroll
        for (int q = 0; q < G / 4; ++q) {
            u4 v;
#pragma unroll
            for (int s = 0; s < 4; ++s) v[s] = (o_re[4 * q + s] & 0xffffu) | (o_im[4 * q + s] << 16);
            *reinterpret_cast<u4 *>(static_cast<unsigned *>(re) + e + 4 * q) = v;
        }
    } else {
        static_assert(FO != GAT_LAYOUT_INTERLEAVED_I8 || G == 8, "an int8 output's 16 bytes are 8 samples");
        u4 v;
#pragma unroll
        for (int w = 0; w < 4; ++w)
            v[w] = (o_re[2 * w] & 0xffu) | ((o_im[2 * w] & 0xffu) << 8) | ((o_re[2 * w + 1] & 0xffu) << 16) | (o_im[2 * w + 1] << 24);
        *reinterpret_cast<u4 *>(static_cast<unsigned short *>(re) + e) = v;
    }
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned v)
{
    unsigned long long t = v;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) t += ((unsigned long long)(unsigned)__shfl_xor((int)(t >> 32), off, 64) << 32) | (unsigned)__shfl_xor((int)t, off, 64);
    return t;
}

// a wave-uniform value the compiler must keep in vector registers from here on
__device__ __forceinline__ size_t cond_in_vgprs(size_t v)
{
    asm volatile("" : "+v"(v));
    return v;
}

// The streaming kernel's records are wave-uniform, but it reads them with vector loads (every lane the same address: one
// broadcast 16-byte load a record) into 4 M vector registers: as scalars they sit next to the verdicts of a group's samples, a
// register pair each, and the scalar file overflows.
template <int M>
__device__ __forceinline__ void cond_load_records(const gat_cond_params *prm, size_t zero_in_vgprs, gat_cond_params (&pr)[M])
{
#pragma unroll
    for (int m = 0; m < M; ++m) pr[m] = prm[zero_in_vgprs + m];
}
// ---- M <= 8, aligned on both sides: the streaming kernel ---------------------------------------------------------------------
template <int FI, int FO, int M>
__global__ void __launch_bounds__(kCondThreads) cond_stream_kernel(const CondArgs a, const gat_cond_params *__restrict__ prm)
{
    using Vec = SampleVec<FI, true>;
    constexpr int VS = Vec::VS, G = cond_group_samples(FI, FO), NV = G / VS;
    static_assert(G % VS == 0 && G % layout_vec_samples(FO) == 0, "whole loads and whole stores");
    const int tid = threadIdx.x;
    // The antenna strides live in vector registers: as scalars, the 2 M (planar: 4 M) block-and-antenna base addresses of the two
    // sides are hoisted out of the sample loop into register pairs, and with the records' 4 M values the scalar file overflows.
    // A 64-bit vector addition per 16-byte load or store costs nothing next to the memory traffic.
    const size_t ant_stride = cond_in_vgprs((size_t)a.ant_stride), out_ant_stride = cond_in_vgprs((size_t)a.out_ant_stride);
    gat_cond_params pr[M];
    cond_load_records<M>(prm, cond_in_vgprs((size_t)0), pr);
    // a lane's counts: below 2^32 unless one workgroup conditions 2^40 samples
    unsigned n_blank[M], n_clip[M];
#pragma unroll
    for (int m = 0; m < M; ++m) n_blank[m] = n_clip[m] = 0u;

    for (long long u = blockIdx.x; u < a.units; u += gridDim.x) {
        long long b, n0, n1;
        cond_unit(u, a.chunks, a.chunk, a.N, &b, &n0, &n1);
        const size_t base = (size_t)b * (size_t)a.block_stride, obase = (size_t)b * (size_t)a.out_block_stride;
        const long long g1 = n1 / G; // whole groups end here (chunk is a multiple of G: only the block's end can be ragged)
        for (long long gi = n0 / G + tid; gi < g1; gi += kCondThreads) {
            Vec raw[M][NV];
#pragma unroll
            for (int m = 0; m < M; ++m)
#pragma unroll
                for (int q = 0; q < NV; ++q) raw[m][q].load(a.re, a.im, base + (size_t)m * ant_stride, gi * NV + q);
            unsigned blank[M], any = 0u; // bit s: sample s of the group is blanked
#pragma unroll
            for (int m = 0; m < M; ++m) {
                unsigned bm = 0u;
#pragma unroll
                for (int s = 0; s < G; ++s) {
                    float xr, xi;
                    raw[m][s / VS].sample(s % VS, xr, xi);
                    bm |= cond_keep(xr, xi, pr[m].threshold) ? 0u : 1u << s;
                }
                blank[m] = bm;
                any |= bm;
                __builtin_amdgcn_sched_barrier(0); // an antenna at a time: interleaved, the comparisons' results crowd the scalar file
            }
#pragma unroll
            for (int m = 0; m < M; ++m) {
                const unsigned bm = a.blank_all ? any : blank[m];
                n_blank[m] += (unsigned)__popc(bm);
                unsigned o_re[G], o_im[G];
#pragma unroll
                for (int s = 0; s < G; ++s) {
                    float xr, xi;
                    unsigned clips;
                    raw[m][s / VS].sample(s % VS, xr, xi);
                    cond_sample<FO>(xr, xi, !((bm >> s) & 1u), pr[m].scale, pr[m].dc_re, pr[m].dc_im, o_re[s], o_im[s], clips);
                    n_clip[m] += clips;
                }
                cond_store_group<FO, G>(a.out_re, a.out_im, obase + (size_t)m * out_ant_stride + (size_t)(gi * G), o_re, o_im);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        if (n1 == a.N && g1 * G + tid < a.N) { // the block's last N mod G samples: one each for the first lanes
            const size_t n = (size_t)(g1 * G + tid);
            float xr[M], xi[M];
#pragma unroll
            for (int m = 0; m < M; ++m) load_sample<FI>(a.re, a.im, base + (size_t)m * ant_stride + n, xr[m], xi[m]);
            bool any = false;
#pragma unroll
            for (int m = 0; m < M; ++m) any |= !cond_keep(xr[m], xi[m], pr[m].threshold);
#pragma unroll
            for (int m = 0; m < M; ++m) {
                const bool blanked = a.blank_all ? any : !cond_keep(xr[m], xi[m], pr[m].threshold);
                unsigned o_re, o_im, clips;
                cond_sample<FO>(xr[m], xi[m], !blanked, pr[m].scale, pr[m].dc_re, pr[m].dc_im, o_re, o_im, clips);
                n_blank[m] += blanked ? 1u : 0u;
                n_clip[m] += clips;
                cond_store_scalar<FO>(a.out_re, a.out_im, obase + (size_t)m * out_ant_stride + n, o_re, o_im);
            }
        }
    }
    if (a.counts) {
#pragma unroll
        for (int m = 0; m < M; ++m) {
            const unsigned long long nb = wave_sum(n_blank[m]), nc = wave_sum(n_clip[m]);
            if ((tid & 63) == 0) {
                if (nb) atomicAdd(a.counts + 2 * m, nb);
                if (nc) atomicAdd(a.counts + 2 * m + 1, nc);
            }
        }
    }
}

// ---- any M, any alignment: one sample per lane ---------------------------------------------------------------------------------
template <int FI, int FO>
__global__ void __launch_bounds__(kCondThreads) cond_general_kernel(const CondArgs a, const gat_cond_params *__restrict__ prm)
{
    __shared__ float4 s_prm[GAT_MAX_ARRAY_ANTS]; // scale, dc_re, dc_im, threshold: every lane reads the same address (a broadcast)
    __shared__ unsigned long long s_cnt[GAT_MAX_ARRAY_ANTS][2];
    const int tid = threadIdx.x, M = a.M;
    for (int m = tid; m < M; m += kCondThreads) {
        const gat_cond_params p = prm[m];
        s_prm[m] = make_float4(p.scale, p.dc_re, p.dc_im, p.threshold);
        s_cnt[m][0] = s_cnt[m][1] = 0ull;
    }
    __syncthreads();
    for (long long u = blockIdx.x; u < a.units; u += gridDim.x) {
        long long b, n0, n1;
        cond_unit(u, a.chunks, a.chunk, a.N, &b, &n0, &n1);
        const size_t base = (size_t)b * (size_t)a.block_stride, obase = (size_t)b * (size_t)a.out_block_stride;
        for (long long n = n0 + tid; n < n1; n += kCondThreads) { // (the lanes still here are the first ones of their wave)
            bool any = false;
            if (a.blank_all)
                for (int m = 0; m < M; ++m) {
                    float xr, xi;
                    load_sample<FI>(a.re, a.im, base + (size_t)m * (size_t)a.ant_stride + (size_t)n, xr, xi);
                    any |= !cond_keep(xr, xi, s_prm[m].w);
                }
            for (int m = 0; m < M; ++m) {
                float xr, xi;
                load_sample<FI>(a.re, a.im, base + (size_t)m * (size_t)a.ant_stride + (size_t)n, xr, xi);
                const float4 p = s_prm[m];
                const bool blanked = any || !cond_keep(xr, xi, p.w);
                unsigned o_re, o_im, clips;
                cond_sample<FO>(xr, xi, !blanked, p.x, p.y, p.z, o_re, o_im, clips);
                cond_store_scalar<FO>(a.out_re, a.out_im, obase + (size_t)m * (size_t)a.out_ant_stride + (size_t)n, o_re, o_im);
                const unsigned long long nb = (unsigned long long)__popcll(__ballot(blanked));
                const unsigned long long nc = (unsigned long long)__popcll(__ballot(clips & 1u)) + 2ull * (unsigned long long)__popcll(__ballot(clips >> 1));
                if ((tid & 63) == 0) {
                    if (nb) atomicAdd(&s_cnt[m][0], nb);
                    if (nc) atomicAdd(&s_cnt[m][1], nc);
                }
            }
        }
    }
    __syncthreads();
    if (a.counts && tid < 2 * M) {
        const unsigned long long v = (&s_cnt[0][0])[tid];
        if (v) atomicAdd(a.counts + tid, v);
    }
}

template <int FI, int FO>
void cond_stream_dispatch(const CondArgs &a, const gat_cond_params *prm, int grid, hipStream_t st)
{
    const dim3 g((unsigned)grid), b(kCondThreads);
    switch (a.M) {
    case 1: hipLaunchKernelGGL((cond_stream_kernel<FI, FO, 1>), g, b, 0, st, a, prm); break;
    case 2: hipLaunchKernelGGL((cond_stream_kernel<FI, FO, 2>), g, b, 0, st, a, prm); break;
    case 3: hipLaunchKernelGGL((cond_stream_kernel<FI, FO, 3>), g, b, 0, st, a, prm); break;
    case 4: hipLaunchKernelGGL((cond_stream_kernel<FI, FO, 4>), g, b, 0, st, a, prm); break;
    case 5: hipLaunchKernelGGL((cond_stream_kernel<FI, FO, 5>), g, b, 0, st, a, prm); break;
    case 6: hipLaunchKernelGGL((cond_stream_kernel<FI, FO, 6>), g, b, 0, st, a, prm); break;
    case 7: hipLaunchKernelGGL((cond_stream_kernel<FI, FO, 7>), g, b, 0, st, a, prm); break;
    default: hipLaunchKernelGGL((cond_stream_kernel<FI, FO, 8>), g, b, 0, st, a, prm); break;
    }
}

// ---- level statistics -------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double wave_sum_f64(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// a lane's sums of the MT antennas of its tile
template <int MT>
struct StatsAcc {
    size_t ant[MT]; // where each antenna's stream starts, in samples
    float th[MT], mx[MT];
    double sr[MT], si[MT], pw[MT];
    unsigned kept[MT], taken; // below 2^32 unless one workgroup reads 2^40 samples; blanked = taken - kept
};

// One sample of the tile's antennas into the sums; out: an antenna outside the tile blanks it.  A blanked sample enters the sums
// as +0.0, by masking its bits with the verdict's bit spread over a word, and the additions are the same for every sample
// (s + 0.0 = s to the bit: no sum here is ever -0.0, and max_abs is never below 0).  Kept as the condition of every update, the
// verdicts of a whole 16-byte group stay live together as register pairs of the scalar file, which overflows with them.
template <int MT>
__device__ __forceinline__ void stats_take(StatsAcc<MT> &c, const float (&xr)[MT], const float (&xi)[MT], bool out, bool blank_all)
{
    unsigned keep = 0u; // bit i: antenna i keeps the sample by its own threshold
#pragma unroll
    for (int i = 0; i < MT; ++i) keep |= cond_keep(xr[i], xi[i], c.th[i]) ? 1u << i : 0u;
    constexpr unsigned all = (1u << MT) - 1u;
    if (blank_all) keep = (out || keep != all) ? 0u : all;
    c.taken += 1u;
#pragma unroll
    for (int i = 0; i < MT; ++i) {
        const unsigned km = cond_spread_bit(keep, i);
        const float fr = __uint_as_float(__float_as_uint(xr[i]) & km), fi = __uint_as_float(__float_as_uint(xi[i]) & km);
        const double dr = (double)fr, di = (double)fi;
        c.sr[i] += dr;
        c.si[i] += di;
        c.pw[i] = fma(dr, dr, c.pw[i]);
        c.pw[i] = fma(di, di, c.pw[i]);
        c.mx[i] = fmaxf(c.mx[i], fmaxf(fabsf(fr), fabsf(fi)));
        c.kept[i] += km & 1u;
    }
}

// sample n of the block at `base` through scalar loads; others: the antennas outside the tile [m0, m0 + MT) are asked too
template <int FI, int MT>
__device__ __forceinline__ void stats_take_scalar(StatsAcc<MT> &c, const StatsArgs &a, size_t base, size_t n, int m0, bool others)
{
    float xr[MT], xi[MT];
#pragma unroll
    for (int i = 0; i < MT; ++i) load_sample<FI>(a.re, a.im, base + c.ant[i] + n, xr[i], xi[i]);
    bool out = false;
    if (others)
        for (int m = 0; m < a.M; ++m) {
            if (m >= m0 && m < m0 + MT) continue;
            float yr, yi;
            load_sample<FI>(a.re, a.im, base + (size_t)m * (size_t)a.ant_stride + n, yr, yi);
            out |= !cond_keep(yr, yi, a.prm ? a.prm[m].threshold : INFINITY);
        }
    stats_take<MT>(c, xr, xi, out, a.blank_all != 0);
}

template <int FI, int MT, bool VEC>
__global__ void __launch_bounds__(kStatsThreads) stats_kernel(const StatsArgs a)
{
    using Vec = SampleVec<FI, true>;
    constexpr int VS = Vec::VS;
    __shared__ gat_sample_stats_t s_red[kStatsThreads / 64][MT];
    const int tid = threadIdx.x, e = blockIdx.x / a.G, g = blockIdx.x % a.G;
    const int m0 = a.m_first + (int)blockIdx.y * kStatsTile; // the tile's first antenna
    const int b0 = e * a.bpe;
    const int nb = (a.B - b0 < a.bpe) ? a.B - b0 : a.bpe;
    const long long units = (long long)nb * a.splits;
    const bool others = !VEC && a.blank_all && a.M > MT; // antennas outside the tile have a say in the verdict

    StatsAcc<MT> c;
#pragma unroll
    for (int i = 0; i < MT; ++i) {
        const int m = m0 + i; // (a tile is whole: the launcher sizes the last one)
        c.ant[i] = cond_in_vgprs((size_t)m * (size_t)a.ant_stride); // (as scalars the MT base addresses crowd the scalar file)
        c.th[i] = a.prm ? a.prm[m].threshold : INFINITY;
        asm volatile("" : "+v"(c.th[i])); // (in a vector register, as the base: the verdicts need the scalar file)
        c.mx[i] = 0.f;
        c.sr[i] = c.si[i] = c.pw[i] = 0.0;
        c.kept[i] = 0u;
    }
    c.taken = 0u;

    for (long long u = g; u < units; u += a.G) {
        const int b = b0 + (int)(u / a.splits);
        const long long n0 = (u % a.splits) * a.seg_len;
        const long long n1 = (n0 + a.seg_len < a.N) ? n0 + a.seg_len : a.N;
        const size_t base = (size_t)b * (size_t)a.block_stride;
        if constexpr (VEC) {
            const long long v1 = n1 / VS; // whole vectors end here (seg_len is a multiple of VS: only the block's end can be ragged)
            for (long long v = n0 / VS + tid; v < v1; v += kStatsThreads) {
                Vec raw[MT];
#pragma unroll
                for (int i = 0; i < MT; ++i) raw[i].load(a.re, a.im, base + c.ant[i], v);
#pragma unroll
                for (int s = 0; s < VS; ++s) {
                    float xr[MT], xi[MT];
#pragma unroll
                    for (int i = 0; i < MT; ++i) raw[i].sample(s, xr[i], xi[i]);
                    stats_take<MT>(c, xr, xi, false, a.blank_all != 0);
                    __builtin_amdgcn_sched_barrier(0); // a sample at a time (the loads are all issued above)
                }
            }
            if (n1 == a.N && v1 * VS + tid < a.N) stats_take_scalar<FI, MT>(c, a, base, (size_t)(v1 * VS + tid), m0, others); // the block's last N mod VS samples
        } else {
            for (long long n = n0 + tid; n < n1; n += kStatsThreads) stats_take_scalar<FI, MT>(c, a, base, (size_t)n, m0, others);
        }
    }

    // wave butterfly (fixed order), then the four waves in order
#pragma unroll
    for (int i = 0; i < MT; ++i) {
        const double sr = wave_sum_f64(c.sr[i]), si = wave_sum_f64(c.si[i]), pw = wave_sum_f64(c.pw[i]);
        float mx = c.mx[i];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
        const unsigned long long nk = wave_sum(c.kept[i]), nbl = wave_sum(c.taken - c.kept[i]);
        if ((tid & 63) == 0) {
            gat_sample_stats_t &r = s_red[tid >> 6][i];
            r.kept = (int64_t)nk, r.blanked = (int64_t)nbl;
            r.sum_re = sr, r.sum_im = si, r.sum_pow = pw;
            r.max_abs = mx, r.pad_ = 0.f;
        }
    }
    __syncthreads();
    if (tid < MT) {
        long long nk = s_red[0][tid].kept, nbl = s_red[0][tid].blanked;
        double vr = s_red[0][tid].sum_re, vi = s_red[0][tid].sum_im, vp = s_red[0][tid].sum_pow;
        float vm = s_red[0][tid].max_abs;
#pragma unroll
        for (int w = 1; w < kStatsThreads / 64; ++w) {
            nk += s_red[w][tid].kept, nbl += s_red[w][tid].blanked;
            vr += s_red[w][tid].sum_re, vi += s_red[w][tid].sum_im, vp += s_red[w][tid].sum_pow;
            vm = fmaxf(vm, s_red[w][tid].max_abs);
        }
        gat_sample_stats_t *o = a.partial + ((size_t)e * a.G + g) * a.M + m0 + tid;
        o->kept = nk, o->blanked = nbl;
        o->sum_re = vr, o->sum_im = vi, o->sum_pow = vp;
        o->max_abs = vm, o->pad_ = 0.f;
    }
}

// one wave per (estimate, antenna): lane r adds slices r, r + 64, ... in that order, then the butterfly
__global__ void __launch_bounds__(64) stats_finish_kernel(const gat_sample_stats_t *__restrict__ partial, int M, int G, gat_sample_stats_t *__restrict__ stats)
{
    const int e = blockIdx.x / M, m = blockIdx.x % M, lane = threadIdx.x;
    double sr = 0.0, si = 0.0, pw = 0.0;
    float mx = 0.f;
    long long kept = 0, blanked = 0;
    for (int g = lane; g < G; g += 64) {
        const gat_sample_stats_t *r = partial + ((size_t)e * G + g) * M + m;
        sr += r->sum_re, si += r->sum_im, pw += r->sum_pow;
        mx = fmaxf(mx, r->max_abs);
        kept += r->kept, blanked += r->blanked;
    }
    sr = wave_sum_f64(sr), si = wave_sum_f64(si), pw = wave_sum_f64(pw);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        mx = fmaxf(mx, __shfl_xor(mx, off, 64));
        kept += __shfl_xor(kept, off, 64);
        blanked += __shfl_xor(blanked, off, 64);
    }
    if (lane == 0) {
        gat_sample_stats_t *o = stats + (size_t)e * M + m;
        o->kept = kept, o->blanked = blanked;
        o->sum_re = sr, o->sum_im = si, o->sum_pow = pw;
        o->max_abs = mx, o->pad_ = 0.f;
    }
}

__global__ void __launch_bounds__(64) agc_update_kernel(const gat_sample_stats_t *__restrict__ stats, int M, double target_rms, double blank_factor,
                                                       int remove_dc, gat_cond_params *__restrict__ prm)
{
    const int m = threadIdx.x;
    if (m < M) prm[m] = agc_record(stats[m], target_rms, blank_factor, remove_dc);
}

template <int FI, bool VEC>
void stats_launch_tiles(const StatsArgs &a, int mt, int tiles, hipStream_t st)
{
    const dim3 g((unsigned)(a.E * a.G), (unsigned)tiles), b(kStatsThreads);
    switch (mt) {
    case 1: hipLaunchKernelGGL((stats_kernel<FI, 1, VEC>), g, b, 0, st, a); break;
    case 2: hipLaunchKernelGGL((stats_kernel<FI, 2, VEC>), g, b, 0, st, a); break;
    case 3: hipLaunchKernelGGL((stats_kernel<FI, 3, VEC>), g, b, 0, st, a); break;
    case 4: hipLaunchKernelGGL((stats_kernel<FI, 4, VEC>), g, b, 0, st, a); break;
    case 5: hipLaunchKernelGGL((stats_kernel<FI, 5, VEC>), g, b, 0, st, a); break;
    case 6: hipLaunchKernelGGL((stats_kernel<FI, 6, VEC>), g, b, 0, st, a); break;
    case 7: hipLaunchKernelGGL((stats_kernel<FI, 7, VEC>), g, b, 0, st, a); break;
    default: hipLaunchKernelGGL((stats_kernel<FI, kStatsTile, VEC>), g, b, 0, st, a); break;
    }
}

// M <= 8: one tile of M.  More: M / 8 whole tiles in blockIdx.y and, in a launch of its own, a last tile of M mod 8, so that no
// slot of a tile loads an antenna twice.
template <int FI, bool VEC>
void stats_dispatch(const StatsArgs &a, hipStream_t st)
{
    if (a.M <= kStatsTile) {
        stats_launch_tiles<FI, VEC>(a, a.M, 1, st);
        return;
    }
    stats_launch_tiles<FI, VEC>(a, kStatsTile, a.M / kStatsTile, st);
    if (a.M % kStatsTile) {
        StatsArgs t = a;
        t.m_first = a.M / kStatsTile * kStatsTile;
        stats_launch_tiles<FI, VEC>(t, a.M % kStatsTile, 1, st);
    }
}

} // namespace

hipError_t launch_cond_stream(const CondArgs &a, int fmt_in, int fmt_out, const gat_cond_params *prm, int grid, hipStream_t st)
{
    if (a.M < 1 || a.M > kCondStreamMaxAnts || grid < 1) return hipErrorInvalidValue;
    dispatch_layout(fmt_in, [&](auto FI) {
        dispatch_layout(fmt_out, [&](auto FO) { cond_stream_dispatch<decltype(FI)::value, FO>(a, prm, grid, st); });
    });
    return hipGetLastError();
}

hipError_t launch_cond_general(const CondArgs &a, int fmt_in, int fmt_out, const gat_cond_params *prm, int grid, hipStream_t st)
{
    if (a.M < 1 || a.M > GAT_MAX_ARRAY_ANTS || grid < 1) return hipErrorInvalidValue;
    const dim3 g((unsigned)grid), b(kCondThreads);
    dispatch_layout(fmt_in, [&](auto FI) {
        dispatch_layout(fmt_out, [&](auto FO) { hipLaunchKernelGGL((cond_general_kernel<decltype(FI)::value, FO>), g, b, 0, st, a, prm); });
    });
    return hipGetLastError();
}

hipError_t launch_stats(const StatsArgs &a, int fmt, bool vec, hipStream_t st)
{
    if (a.M < 1 || a.M > GAT_MAX_ARRAY_ANTS || a.E < 1 || a.G < 1 || (vec && a.M > kStatsTile)) return hipErrorInvalidValue;
    if (vec)
        dispatch_layout(fmt, [&](auto F) { stats_dispatch<F, true>(a, st); });
    else
        dispatch_layout(fmt, [&](auto F) { stats_dispatch<F, false>(a, st); });
    return hipGetLastError();
}

hipError_t launch_stats_finish(const gat_sample_stats_t *partial, int M, int E, int G, gat_sample_stats_t *stats, hipStream_t st)
{
    hipLaunchKernelGGL(stats_finish_kernel, dim3((unsigned)(E * M)), dim3(64), 0, st, partial, M, G, stats);
    return hipGetLastError();
}

hipError_t launch_agc_update(const gat_sample_stats_t *stats, int M, double target_rms, double blank_factor, int remove_dc, gat_cond_params *prm,
                             hipStream_t st)
{
    hipLaunchKernelGGL(agc_update_kernel, dim3(1), dim3(64), 0, st, stats, M, target_rms, blank_factor, remove_dc, prm);
    return hipGetLastError();
}

} // namespace gat
