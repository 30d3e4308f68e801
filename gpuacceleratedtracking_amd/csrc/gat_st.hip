// gat_st.hip -- space-time adaptive processing (include/gat.h): the tapped covariance of the raw samples and the space-time
// filter.  The snapshot of a block at sample n is z[q] = x[n - t, m], q = t * M + m, Q = M * T elements (gat_st.h); the refusals,
// the kernel choice, the geometry and the work split are gat_st_plan.h.
//
// The filter, y[n'] = sum_q conj(w[q]) z_q[n' + T - 1].  Every output is one lane's sum in q order (st_term, gat_st.h), so the
// bits depend neither on the kernel nor on the work split.  The weights are narrowed once by the beamformer's kernel
// (launch_beam_weights with Q for M), in tiles of JT beams.
//   * st_tiled_kernel<FI, FO, JT>, M <= 16, every block of every antenna and beam on a 16-byte boundary: a workgroup walks its
//     unit (block, chunk of outputs) in tiles of a.tile outputs.  It stages the tile + T - 1 samples of all M antennas with
//     16-byte loads (scalar loads for a block's last N mod VS samples: nothing outside the block is read), converted to float
//     pairs, as M rows of a.row columns.  Lane l owns outputs l, l + 256, ... of the tile (up to kStLaneOutputs) for JT <= 4
//     beams: element (t, m) of output j is row m, column j + T - 1 - t, so for every element the lanes of a wave read consecutive
//     columns of one row with ds_read_b64 (32 lanes x 8 bytes: the 64 banks once), and the element's JT weights are one
//     broadcast read of LDS.  Up to 4 beams the samples cross HBM once; further beams take further passes.  Stores are one
//     float a plane or one float pair per lane, consecutive over the lanes.
//   * st_general_kernel<FI, JT>, any base and strides: one output per lane, scalar loads from global memory for every element
//     (neighbouring lanes' and taps' samples overlap in the cache), the weights of JT <= 8 beams staged in LDS, a component per
//     store.
//
// The covariance, R[q][q'] = sum_n z_q[n] conj(z_q'[n]) over the N - T + 1 snapshots of a block: st_cov_kernel<FMT> is
// gat_array.hip's cov_tiled_kernel with Q virtual antennas that are shifted views of M staged rows.  A step stages `chunk`
// snapshots' samples -- chunk + T - 1 columns: the T - 1 sample halo in front, nothing outside the block -- with the antennas
// in reverse order inside a column, which makes a snapshot ONE contiguous run of Q float pairs (element q at a fixed address
// minus q).  The upper triangle's 4 x 4 element tiles are spread over the 512 threads, each tile over as many snapshot phases
// as fit; a thread reads 4 + 4 elements of one snapshot (8-byte LDS reads: a run starts on any float pair) and does 64 FMAs on
// them; two-level sums, an LDS tree over the phases, one slice of the context's scratch per workgroup.  The slices have the
// spatial covariance's form with Q for M, and its cov_finish_kernel ends them: the fixed order, the mirror, the +0 diagonal.
#include <hip/hip_runtime.h>

#include "gat_sample_load.h"
#include "gat_st.h"
#include "gat_st_kernels.h"

namespace gat {

namespace {

// ---- the filter: aligned on both sides, samples and halo staged in LDS -------------------------------------------------------------
// The sums of a tile's outputs j = tid + k * 256 < nt, k < NR, for the JT beams from j0, from the staged samples; stored.
template <int FO, int JT, int NR>
__device__ __forceinline__ void st_tile_run(const StArgs &a, const float2 *s_x, const float2 *s_w, int tid, int nt, long long nt0, size_t obase, int j0)
{
    float yr[JT][NR], yi[JT][NR];
    int j[NR];
#pragma unroll
    for (int k = 0; k < NR; ++k) {
        const int jk = tid + k * kStThreads;
        j[k] = jk < nt ? jk : 0; // a lane without an output reads output 0's samples and stores nothing
#pragma unroll
        for (int t = 0; t < JT; ++t) yr[t][k] = yi[t][k] = 0.0f;
    }
    int q = 0;
    for (int t = 0; t < a.T; ++t) {
        const float2 *line = s_x + (a.T - 1 - t); // element (t, m) of output j: row m, column j + T - 1 - t
        for (int m = 0; m < a.M; ++m, ++q, line += a.row) {
            float2 w[JT];
#pragma unroll
            for (int t2 = 0; t2 < JT; ++t2) w[t2] = s_w[q * JT + t2];
#pragma unroll
            for (int k = 0; k < NR; ++k) {
                const float2 x = line[j[k]];
#pragma unroll
                for (int t2 = 0; t2 < JT; ++t2) st_term(w[t2].x, w[t2].y, x.x, x.y, yr[t2][k], yi[t2][k]);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < NR; ++k) {
        const int jk = tid + k * kStThreads;
        if (jk >= nt) continue;
        size_t e = obase + (size_t)(nt0 + jk);
#pragma unroll
        for (int t = 0; t < JT; ++t, e += (size_t)a.out_ant_stride) {
            if (j0 + t >= a.J) break;
            if constexpr (FO == GAT_LAYOUT_PLANAR) {
                a.out_re[e] = yr[t][k];
                a.out_im[e] = yi[t][k];
            } else {
                reinterpret_cast<float2 *>(a.out_re)[e] = make_float2(yr[t][k], yi[t][k]); // (the output's blocks are 16-byte aligned)
            }
        }
    }
}

template <int FI, int FO, int JT>
__global__ void __launch_bounds__(kStThreads) st_tiled_kernel(const StArgs a, const float2 *__restrict__ w32)
{
    using Vec = SampleVec<FI, false>;
    constexpr int VS = Vec::VS;
    __shared__ __align__(16) float2 s_x[kStLdsSamples];
    __shared__ __align__(16) float2 s_w[GAT_MAX_ARRAY_ANTS * JT];
    const int tid = threadIdx.x, M = a.M, QJ = a.M * a.T * JT;
    for (int j0 = 0; j0 < a.J; j0 += JT) {
        __syncthreads(); // the previous pass's reads are done
        for (int idx = tid; idx < QJ; idx += kStThreads) s_w[idx] = w32[(size_t)(j0 / JT) * (size_t)QJ + idx];
        for (long long u = blockIdx.x; u < a.units; u += gridDim.x) {
            long long b, n0, n1;
            st_unit(u, a.chunks, a.chunk, a.outputs, &b, &n0, &n1);
            const size_t base = (size_t)b * (size_t)a.block_stride;
            const size_t obase = (size_t)b * (size_t)a.out_block_stride + (size_t)j0 * (size_t)a.out_ant_stride;
            for (long long nt0 = n0; nt0 < n1; nt0 += a.tile) {
                const int nt = (int)(n1 - nt0 < a.tile ? n1 - nt0 : a.tile);
                // the tile's samples [p0, p1) of the block: p1 <= N, since nt0 + nt <= N - T + 1
                const long long p0 = nt0, p1 = nt0 + nt + (a.T - 1);
                __syncthreads(); // the last tile's sums have read their samples
                // whole 16-byte vectors inside the block, from the one that holds p0 on
                const long long v0 = p0 / VS, v_end = (p1 + VS - 1) / VS, v_in = a.N / VS, v1 = v_end < v_in ? v_end : v_in;
                const int nv = (int)(v1 - v0);
                for (int idx = tid; idx < M * nv; idx += kStThreads) {
                    const int m = idx / nv;
                    const long long v = v0 + (idx - m * nv);
                    Vec raw;
                    raw.load(a.re, a.im, base + (size_t)m * (size_t)a.ant_stride, v);
#pragma unroll
                    for (int s = 0; s < VS; ++s) {
                        const long long p = v * VS + s;
                        if (p < p0 || p >= p1) continue;
                        float xr, xi;
                        raw.sample(s, xr, xi);
                        s_x[m * a.row + (int)(p - p0)] = make_float2(xr, xi);
                    }
                }
                // the block's last N mod VS samples, one to a lane
                const long long t0 = v1 * VS > p0 ? v1 * VS : p0;
                const int ntail = p1 > t0 ? (int)(p1 - t0) : 0;
                for (int idx = tid; idx < M * ntail; idx += kStThreads) {
                    const int m = idx / ntail;
                    const long long p = t0 + (idx - m * ntail);
                    float xr, xi;
                    load_sample<FI>(a.re, a.im, base + (size_t)m * (size_t)a.ant_stride + (size_t)p, xr, xi);
                    s_x[m * a.row + (int)(p - p0)] = make_float2(xr, xi);
                }
                __syncthreads(); // (the pass's weights too)
                switch ((nt + kStThreads - 1) / kStThreads) { // (uniform: the rounds of the workgroup this tile has outputs for)
                case 1: st_tile_run<FO, JT, 1>(a, s_x, s_w, tid, nt, nt0, obase, j0); break;
                case 2: st_tile_run<FO, JT, 2>(a, s_x, s_w, tid, nt, nt0, obase, j0); break;
                case 3: st_tile_run<FO, JT, 3>(a, s_x, s_w, tid, nt, nt0, obase, j0); break;
                default: st_tile_run<FO, JT, kStLaneOutputs>(a, s_x, s_w, tid, nt, nt0, obase, j0); break;
                }
            }
        }
    }
}

// ---- the filter: any alignment, one output per lane ---------------------------------------------------------------------------------
template <int FI, int JT>
__global__ void __launch_bounds__(kStThreads) st_general_kernel(const StArgs a, const float2 *__restrict__ w32)
{
    __shared__ float2 s_w[GAT_MAX_ARRAY_ANTS][JT]; // element-major: one element's JT weights are consecutive; every lane reads the same address
    const int tid = threadIdx.x, M = a.M, QJ = a.M * a.T * JT;
    for (int j0 = 0; j0 < a.J; j0 += JT) {
        __syncthreads(); // the previous tile's reads are done
        for (int idx = tid; idx < QJ; idx += kStThreads) (&s_w[0][0])[idx] = w32[(size_t)(j0 / JT) * (size_t)QJ + idx];
        __syncthreads();
        for (long long u = blockIdx.x; u < a.units; u += gridDim.x) {
            long long b, n0, n1;
            st_unit(u, a.chunks, a.chunk, a.outputs, &b, &n0, &n1);
            const size_t base = (size_t)b * (size_t)a.block_stride;
            const size_t obase = (size_t)b * (size_t)a.out_block_stride + (size_t)j0 * (size_t)a.out_ant_stride;
            for (long long n = n0 + tid; n < n1; n += kStThreads) {
                float yr[JT], yi[JT];
#pragma unroll
                for (int t = 0; t < JT; ++t) yr[t] = yi[t] = 0.0f;
                int q = 0;
                for (int t = 0; t < a.T; ++t) {
                    const size_t p = base + (size_t)(n + (a.T - 1 - t));
                    for (int m = 0; m < M; ++m, ++q) {
                        float xr, xi;
                        load_sample<FI>(a.re, a.im, p + (size_t)m * (size_t)a.ant_stride, xr, xi);
#pragma unroll
                        for (int t2 = 0; t2 < JT; ++t2) {
                            const float2 w = s_w[q][t2];
                            st_term(w.x, w.y, xr, xi, yr[t2], yi[t2]);
                        }
                    }
                }
                size_t e = obase + (size_t)n;
#pragma unroll
                for (int t = 0; t < JT; ++t, e += (size_t)a.out_ant_stride) {
                    if (j0 + t >= a.J) break;
                    if (a.out_im) {
                        a.out_re[e] = yr[t];
                        a.out_im[e] = yi[t];
                    } else {
                        a.out_re[2 * e] = yr[t];
                        a.out_re[2 * e + 1] = yi[t];
                    }
                }
            }
        }
    }
}

// ---- the covariance: Q virtual antennas over M staged rows ---------------------------------------------------------------------------
__device__ __forceinline__ void st_tile_of(int tile, int nt, int &ti, int &tj)
{
    ti = 0;
    while (tile >= nt - ti) tile -= nt - ti, ++ti;
    tj = ti + tile;
}

// a.N: the snapshots of a block (N - T + 1); snapshot s reads samples s .. s + T - 1
template <int FMT>
__global__ void __launch_bounds__(kStCovThreads, 2) st_cov_kernel(const CovArgs a, const StCovGeom geo, const int T)
{
    extern __shared__ __align__(16) unsigned char st_cov_lds[];
    float2 *s_x = reinterpret_cast<float2 *>(st_cov_lds); // kStCovPad, then [cols][M], the antennas of a column in reverse order
    float *s_f = reinterpret_cast<float *>(st_cov_lds);   // the phases' tree at the end: [threads][16]

    const int tid = threadIdx.x, e = blockIdx.x / a.G, g = blockIdx.x % a.G;
    const int M = a.M, Q = geo.Q, chunk = geo.chunk, cols = geo.cols, tiles = geo.tiles, phases = geo.phases;
    const int tile = tid % tiles, phase = tid / tiles;
    const bool active = phase < phases;
    int ti, tj;
    st_tile_of(tile, geo.nt, ti, tj);
    const int b0 = e * a.bpe;
    const int nb = (a.B - b0 < a.bpe) ? a.B - b0 : a.bpe;
    const long long units = (long long)nb * a.splits;
    const int flush_every = geo.per_phase >= 32 ? 1 : 32 / geo.per_phase; // chunks of one first-level run: ~32 snapshots per thread

    float t_re[16], t_im[16], s_re[16], s_im[16];
#pragma unroll
    for (int p = 0; p < 16; ++p) t_re[p] = t_im[p] = s_re[p] = s_im[p] = 0.f;
    // elements Q .. 4 nt - 1 of the first snapshots reach in front of the samples: zero, once (their sums are never stored)
    if (tid < kStCovPad) s_x[tid] = make_float2(0.f, 0.f);

    for (long long u = g; u < units; u += a.G) {
        const int b = b0 + (int)(u / a.splits);
        const long long s0 = (u % a.splits) * a.seg_len;
        const long long s1 = (s0 + a.seg_len < a.N) ? s0 + a.seg_len : a.N;
        const long long lim = s1 + (T - 1); // one past the last sample of the segment's snapshots: at most the block's length
        const size_t base = (size_t)b * (size_t)a.block_stride;
        int since = 0;
        for (long long c0 = s0; c0 < s1; c0 += chunk) {
            __syncthreads(); // the previous chunk's reads are done
            for (int idx = tid; idx < M * cols; idx += kStCovThreads) {
                const int m = idx / cols, c = idx - m * cols; // column c: sample c0 + c
                float xr = 0.f, xi = 0.f;
                if (c0 + c < lim) load_sample<FMT>(a.re, a.im, base + (size_t)m * (size_t)a.ant_stride + (size_t)(c0 + c), xr, xi);
                s_x[kStCovPad + c * M + (M - 1 - m)] = make_float2(xr, xi);
            }
            __syncthreads();
            if (active) {
                for (int k = 0; k < geo.per_phase; ++k) {
                    const int n = k * phases + phase; // snapshot c0 + n: its newest sample is column n + T - 1
                    if (c0 + n >= s1) break;          // (n grows with k)
                    const float2 *z = s_x + kStCovPad + (n + T) * M - 1; // element q of the snapshot: z[-q]
                    const float2 *pi = z - kStCovTile * ti, *pj = z - kStCovTile * tj;
                    float ir[4], ii[4], jr[4], ji[4];
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float2 vi = pi[-r], vj = pj[-r];
                        ir[r] = vi.x, ii[r] = vi.y, jr[r] = vj.x, ji[r] = vj.y;
                    }
#pragma unroll
                    for (int r = 0; r < 4; ++r)
#pragma unroll
                        for (int c = 0; c < 4; ++c) {
                            s_re[r * 4 + c] = __builtin_fmaf(ir[r], jr[c], s_re[r * 4 + c]);
                            s_re[r * 4 + c] = __builtin_fmaf(ii[r], ji[c], s_re[r * 4 + c]);
                            s_im[r * 4 + c] = __builtin_fmaf(ii[r], jr[c], s_im[r * 4 + c]);
                            s_im[r * 4 + c] = __builtin_fmaf(-ir[r], ji[c], s_im[r * 4 + c]);
                        }
                }
            }
            if (++since == flush_every || c0 + chunk >= s1) {
                since = 0;
#pragma unroll
                for (int p = 0; p < 16; ++p) {
                    t_re[p] += s_re[p], t_im[p] += s_im[p];
                    s_re[p] = s_im[p] = 0.f;
                }
            }
        }
    }

    // the phases of a tile meet in a tree over LDS (fixed shape), the real plane first, then the imaginary one
    float *out = a.partial + ((size_t)e * a.G + g) * (size_t)(2 * Q * Q);
    int top = 1;
    while (top < phases) top <<= 1;
    for (int plane = 0; plane < 2; ++plane) {
        __syncthreads();
        if (active)
#pragma unroll
            for (int p = 0; p < 16; ++p) s_f[(phase * tiles + tile) * 16 + p] = plane ? t_im[p] : t_re[p];
        for (int h = top >> 1; h > 0; h >>= 1) {
            __syncthreads();
            if (active && phase < h && phase + h < phases) {
#pragma unroll
                for (int p = 0; p < 16; ++p) s_f[(phase * tiles + tile) * 16 + p] += s_f[((phase + h) * tiles + tile) * 16 + p];
            }
        }
        __syncthreads();
        for (int idx = tid; idx < tiles * 16; idx += kStCovThreads) {
            int oi, oj;
            st_tile_of(idx / 16, geo.nt, oi, oj);
            const int i = kStCovTile * oi + (idx % 16) / 4, j = kStCovTile * oj + idx % 4;
            if (i < Q && j < Q && j >= i) out[(size_t)plane * Q * Q + (size_t)i * Q + j] = s_f[idx];
        }
    }
}

template <int FI, bool TILED>
void st_dispatch_out(const StArgs &a, const float2 *w32, int grid, hipStream_t st)
{
    const dim3 g((unsigned)grid), b(kStThreads);
    const int jt = st_beam_tile(TILED, a.J);
    if constexpr (TILED) {
        const bool planar = a.out_im != nullptr;
        if (jt == 1) {
            if (planar)
                hipLaunchKernelGGL((st_tiled_kernel<FI, GAT_LAYOUT_PLANAR, 1>), g, b, 0, st, a, w32);
            else
                hipLaunchKernelGGL((st_tiled_kernel<FI, GAT_LAYOUT_INTERLEAVED, 1>), g, b, 0, st, a, w32);
        } else {
            if (planar)
                hipLaunchKernelGGL((st_tiled_kernel<FI, GAT_LAYOUT_PLANAR, kStTiledBeams>), g, b, 0, st, a, w32);
            else
                hipLaunchKernelGGL((st_tiled_kernel<FI, GAT_LAYOUT_INTERLEAVED, kStTiledBeams>), g, b, 0, st, a, w32);
        }
    } else {
        switch (jt) {
        case 1: hipLaunchKernelGGL((st_general_kernel<FI, 1>), g, b, 0, st, a, w32); break;
        case 2: hipLaunchKernelGGL((st_general_kernel<FI, 2>), g, b, 0, st, a, w32); break;
        case 4: hipLaunchKernelGGL((st_general_kernel<FI, 4>), g, b, 0, st, a, w32); break;
        default: hipLaunchKernelGGL((st_general_kernel<FI, kStGeneralBeams>), g, b, 0, st, a, w32); break;
        }
    }
}

template <bool TILED>
hipError_t st_dispatch(const StArgs &a, int fi, const float2 *w32, int grid, hipStream_t st)
{
    if (a.M < 1 || a.T < 1 || a.T > GAT_MAX_ST_TAPS || a.M * a.T > GAT_MAX_ARRAY_ANTS || a.J < 1 || grid < 1 || a.outputs != a.N - a.T + 1 || a.outputs < 1)
        return hipErrorInvalidValue;
    if (TILED && (a.M > kStTiledMaxAnts || a.tile < 1 || a.tile > kStThreads * kStLaneOutputs || a.row < a.tile + a.T - 1 || (long long)a.row * a.M > kStLdsSamples))
        return hipErrorInvalidValue;
    dispatch_layout(fi, [&](auto FI) { st_dispatch_out<FI, TILED>(a, w32, grid, st); });
    return hipGetLastError();
}

} // namespace

hipError_t launch_st_tiled(const StArgs &a, int fmt, const float2 *w32, int grid, hipStream_t st) { return st_dispatch<true>(a, fmt, w32, grid, st); }

hipError_t launch_st_general(const StArgs &a, int fmt, const float2 *w32, int grid, hipStream_t st) { return st_dispatch<false>(a, fmt, w32, grid, st); }

hipError_t launch_st_cov(const CovArgs &a, int T, int fmt, hipStream_t st)
{
    if (a.M < 1 || T < 1 || T > GAT_MAX_ST_TAPS || a.M * T > GAT_MAX_ARRAY_ANTS || a.N < 1 || a.G < 1 || a.E < 1) return hipErrorInvalidValue;
    const StCovGeom geo = st_cov_geom(a.M, T);
    if (geo.lds_bytes > 65536 || a.seg_len % geo.chunk != 0) return hipErrorInvalidValue;
    const dim3 grid((unsigned)(a.G * a.E)), block(kStCovThreads);
    dispatch_layout(fmt, [&](auto F) { hipLaunchKernelGGL(st_cov_kernel<F>, grid, block, geo.lds_bytes, st, a, geo, T); });
    return hipGetLastError();
}

} // namespace gat
