// gat_array.hip -- antenna-array processing (include/gat.h): the spatial covariance of the raw samples, the beamformer
// weights, beamformed accumulators and the weighted loop update.
//
// Spatial covariance, R_e[i][j] = sum_{b in e} sum_n x[n,i,b] conj(x[n,j,b]).  Only the upper triangle (j >= i) is ever
// computed: M (M + 1) / 2 products per sample, the diagonal's real only.  Two kernels produce per-workgroup sums, a third
// finishes them:
//   * cov_small_kernel<FMT, M>, M <= 8, every block of every antenna 16-byte aligned: a read-once stream.  Each lane
//     takes one 16-byte load per antenna (and plane) and step -- 4 / 2 / 4 / 8 samples by layout -- and keeps the whole upper
//     triangle in registers (16 floats at M = 4, 64 at M = 8).  A run of 64 samples per lane is summed into a first
//     register set, which is then added into the lane's second set: two-level sums, because a single running f32 sum over
//     the 8 000 samples a lane sees of a 2^21-sample block drifts towards 1e-5 on the diagonal (all terms positive).  One
//     butterfly over the wave and one pass over the workgroup's four waves end it.  HBM traffic: the samples, once.
//   * cov_tiled_kernel<FMT>, any M <= 64, any alignment: 8 M (M + 1) / 2 flop per 8 M bytes is arithmetic-bound from M = 16
//     on, so a chunk of samples is staged in LDS (scalar loads: any layout, base and stride) as float2 rows, and the upper
//     triangle's 4 x 4 antenna tiles are spread over the workgroup's 512 threads, each tile over as many sample phases
//     as fit (M = 64: 136 tiles x 3 phases, M = 16: 10 x 51).  A thread reads 4 + 4 antennas of one sample with four
//     16-byte LDS reads and does 64 FMAs on them; its 16 complex sums are two-level as above; phases meet in an LDS tree.
//     Rows are padded by two float2 so that consecutive samples start 16 bytes further round the banks.
//   * every workgroup stores its sums to its own slice of the context's scratch; cov_finish_kernel adds a (estimate,
//     element)'s slices in a fixed order -- 64 interleaved runs, then those 64 in order --, writes the upper element, its
//     exact conjugate below the diagonal and +0 as the diagonal's imaginary part.  No atomics: the same bits every call.
// Integer samples are converted exactly and every product goes through an FMA, so sums below 2^24 are exact integers.
//
// Weights: array_factor_kernel builds R' = L L^H once (one thread per row, gat_array.h's element routines, FP64, LDS);
// array_solve_kernel runs one workgroup per channel on that factor.  The arithmetic is the host entry point's, to the bit.
#include <hip/hip_runtime.h>

#include "gat_array.h"
#include "gat_array_kernels.h"
#include "gat_loop.h"
#include "gat_sample_load.h"

namespace gat {

namespace {

// one sample's M (M + 1) / 2 products into the upper-triangle sums (row-major over j >= i; the diagonal's s_im stays unused)
template <int M>
__device__ __forceinline__ void cov_accumulate(const float (&xr)[M], const float (&xi)[M], float (&s_re)[M * (M + 1) / 2],
                                               float (&s_im)[M * (M + 1) / 2])
{
    int idx = 0;
#pragma unroll
    for (int i = 0; i < M; ++i)
#pragma unroll
        for (int j = i; j < M; ++j, ++idx) {
            s_re[idx] = __builtin_fmaf(xr[i], xr[j], s_re[idx]);
            s_re[idx] = __builtin_fmaf(xi[i], xi[j], s_re[idx]);
            if (j > i) {
                s_im[idx] = __builtin_fmaf(xi[i], xr[j], s_im[idx]);
                s_im[idx] = __builtin_fmaf(-xr[i], xi[j], s_im[idx]);
            }
        }
}

template <class Vec, int M, int S>
__device__ __forceinline__ void cov_accumulate_vec(const Vec (&raw)[M], float (&s_re)[M * (M + 1) / 2], float (&s_im)[M * (M + 1) / 2])
{
    if constexpr (S < Vec::VS) {
        float xr[M], xi[M];
#pragma unroll
        for (int m = 0; m < M; ++m) raw[m].sample(std::integral_constant<int, S>{}, xr[m], xi[m]);
        cov_accumulate<M>(xr, xi, s_re, s_im);
        cov_accumulate_vec<Vec, M, S + 1>(raw, s_re, s_im);
    }
}

// ---- M <= 8: the streaming kernel ---------------------------------------------------------------------------------------------
template <int FMT, int M>
__global__ void __launch_bounds__(kCovSmallThreads) cov_small_kernel(const CovArgs a)
{
    using Vec = SampleVec<FMT, true>;
    constexpr int VS = Vec::VS, P = M * (M + 1) / 2, PLANES = FMT == GAT_LAYOUT_PLANAR ? 2 : 1;
    constexpr int kRun = 64 / VS;                                     // vectors of one first-level run: 64 samples per lane
    constexpr int U = (M * PLANES <= 2) ? 4 : (M * PLANES <= 8) ? 2 : 1; // vectors in flight per lane and antenna
    __shared__ float s_red[kCovSmallThreads / 64][2][M * M];

    const int tid = threadIdx.x, e = blockIdx.x / a.G, g = blockIdx.x % a.G;
    const int b0 = e * a.bpe;
    const int nb = (a.B - b0 < a.bpe) ? a.B - b0 : a.bpe;
    const long long units = (long long)nb * a.splits;

    float t_re[P], t_im[P], s_re[P], s_im[P];
#pragma unroll
    for (int p = 0; p < P; ++p) t_re[p] = t_im[p] = 0.f;

    for (long long u = g; u < units; u += a.G) {
        const int b = b0 + (int)(u / a.splits);
        const long long n0 = (u % a.splits) * a.seg_len;
        const long long n1 = (n0 + a.seg_len < a.N) ? n0 + a.seg_len : a.N;
        const size_t base = (size_t)b * (size_t)a.block_stride;
        const long long v1 = n1 / VS; // whole vectors end here (seg_len is a multiple of VS: only the block's end can be ragged)
        long long v = n0 / VS + tid;
        while (v < v1) {
#pragma unroll
            for (int p = 0; p < P; ++p) s_re[p] = s_im[p] = 0.f;
            int k = 0;
            for (; k < kRun && v + (U - 1) * kCovSmallThreads < v1; k += U, v += U * kCovSmallThreads) {
                Vec raw[U][M];
#pragma unroll
                for (int q = 0; q < U; ++q)
#pragma unroll
                    for (int m = 0; m < M; ++m) raw[q][m].load(a.re, a.im, base + (size_t)m * (size_t)a.ant_stride, v + q * kCovSmallThreads);
#pragma unroll
                for (int q = 0; q < U; ++q) cov_accumulate_vec<Vec, M, 0>(raw[q], s_re, s_im);
            }
            for (; k < kRun && v < v1; ++k, v += kCovSmallThreads) {
                Vec raw[M];
#pragma unroll
                for (int m = 0; m < M; ++m) raw[m].load(a.re, a.im, base + (size_t)m * (size_t)a.ant_stride, v);
                cov_accumulate_vec<Vec, M, 0>(raw, s_re, s_im);
            }
#pragma unroll
            for (int p = 0; p < P; ++p) t_re[p] += s_re[p], t_im[p] += s_im[p];
        }
        if (n1 == a.N && v1 * VS + tid < a.N) { // the block's last N mod VS samples: one each for the first lanes
            float xr[M], xi[M];
#pragma unroll
            for (int m = 0; m < M; ++m) load_sample<FMT>(a.re, a.im, base + (size_t)m * (size_t)a.ant_stride + (size_t)(v1 * VS + tid), xr[m], xi[m]);
#pragma unroll
            for (int p = 0; p < P; ++p) s_re[p] = s_im[p] = 0.f;
            cov_accumulate<M>(xr, xi, s_re, s_im);
#pragma unroll
            for (int p = 0; p < P; ++p) t_re[p] += s_re[p], t_im[p] += s_im[p];
        }
    }

    // wave butterfly (fixed order), then the four waves in order
#pragma unroll
    for (int p = 0; p < P; ++p)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            t_re[p] += __shfl_xor(t_re[p], off, 64);
            t_im[p] += __shfl_xor(t_im[p], off, 64);
        }
    if ((tid & 63) == 0) {
        int idx = 0;
#pragma unroll
        for (int i = 0; i < M; ++i)
#pragma unroll
            for (int j = i; j < M; ++j, ++idx) {
                s_red[tid >> 6][0][i * M + j] = t_re[idx];
                s_red[tid >> 6][1][i * M + j] = t_im[idx];
            }
    }
    __syncthreads();
    if (tid < 2 * M * M) {
        const int q = tid % (M * M), plane = tid / (M * M);
        if (q % M >= q / M) {
            float v = s_red[0][plane][q];
#pragma unroll
            for (int w = 1; w < kCovSmallThreads / 64; ++w) v += s_red[w][plane][q];
            a.partial[((size_t)e * a.G + g) * (2 * M * M) + tid] = v;
        }
    }
}

// ---- any M, any alignment: chunks staged in LDS, 4 x 4 tiles of the upper triangle ---------------------------------------------
__device__ __forceinline__ void cov_tile_of(int tile, int nt, int &ti, int &tj)
{
    ti = 0;
    while (tile >= nt - ti) tile -= nt - ti, ++ti;
    tj = ti + tile;
}

template <int FMT>
__global__ void __launch_bounds__(kCovTileThreads, 2) cov_tiled_kernel(const CovArgs a, const CovTileGeom geo)
{
    extern __shared__ __align__(16) unsigned char cov_lds[];
    float2 *s_x = reinterpret_cast<float2 *>(cov_lds); // [chunk][row]
    float *s_f = reinterpret_cast<float *>(cov_lds);   // the phases' tree at the end: [threads][16]

    const int tid = threadIdx.x, e = blockIdx.x / a.G, g = blockIdx.x % a.G;
    const int M = a.M, row = geo.row, chunk = geo.chunk, tiles = geo.tiles, phases = geo.phases;
    const int tile = tid % tiles, phase = tid / tiles;
    const bool active = phase < phases;
    int ti, tj;
    cov_tile_of(tile, geo.nt, ti, tj);
    const int b0 = e * a.bpe;
    const int nb = (a.B - b0 < a.bpe) ? a.B - b0 : a.bpe;
    const long long units = (long long)nb * a.splits;
    const int flush_every = geo.per_phase >= 32 ? 1 : 32 / geo.per_phase; // chunks of one first-level run: ~32 samples per thread

    float t_re[16], t_im[16], s_re[16], s_im[16];
#pragma unroll
    for (int p = 0; p < 16; ++p) t_re[p] = t_im[p] = s_re[p] = s_im[p] = 0.f;
    // the rows' padding (antennas M .. row - 1) is read by the last tiles: zero, once
    for (int idx = tid; idx < chunk * (row - M); idx += kCovTileThreads) s_x[(idx / (row - M)) * row + M + idx % (row - M)] = make_float2(0.f, 0.f);

    for (long long u = g; u < units; u += a.G) {
        const int b = b0 + (int)(u / a.splits);
        const long long n0 = (u % a.splits) * a.seg_len;
        const long long n1 = (n0 + a.seg_len < a.N) ? n0 + a.seg_len : a.N;
        const size_t base = (size_t)b * (size_t)a.block_stride;
        int since = 0;
        for (long long c0 = n0; c0 < n1; c0 += chunk) {
            __syncthreads(); // the previous chunk's reads are done
            for (int idx = tid; idx < M * chunk; idx += kCovTileThreads) {
                const int m = idx / chunk, n = idx - m * chunk;
                float xr = 0.f, xi = 0.f;
                if (c0 + n < n1) load_sample<FMT>(a.re, a.im, base + (size_t)m * (size_t)a.ant_stride + (size_t)(c0 + n), xr, xi);
                s_x[n * row + m] = make_float2(xr, xi);
            }
            __syncthreads();
            if (active) {
                for (int k = 0; k < geo.per_phase; ++k) {
                    const int n = k * phases + phase;
                    const float4 *pi = reinterpret_cast<const float4 *>(s_x + n * row + kCovTile * ti);
                    const float4 *pj = reinterpret_cast<const float4 *>(s_x + n * row + kCovTile * tj);
                    const float4 i01 = pi[0], i23 = pi[1], j01 = pj[0], j23 = pj[1];
                    const float ir[4] = {i01.x, i01.z, i23.x, i23.z}, ii[4] = {i01.y, i01.w, i23.y, i23.w};
                    const float jr[4] = {j01.x, j01.z, j23.x, j23.z}, ji[4] = {j01.y, j01.w, j23.y, j23.w};
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
            if (++since == flush_every || c0 + chunk >= n1) {
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
    float *out = a.partial + ((size_t)e * a.G + g) * (size_t)(2 * M * M);
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
        for (int idx = tid; idx < tiles * 16; idx += kCovTileThreads) {
            int oi, oj;
            cov_tile_of(idx / 16, geo.nt, oi, oj);
            const int i = kCovTile * oi + (idx % 16) / 4, j = kCovTile * oj + idx % 4;
            if (i < M && j < M && j >= i) out[(size_t)plane * M * M + (size_t)i * M + j] = s_f[idx];
        }
    }
}

// ---- the slices' sum, the mirror, the diagonal -----------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) cov_finish_kernel(const float *__restrict__ partial, int M, int G, float *__restrict__ cov_re,
                                                        float *__restrict__ cov_im)
{
    __shared__ float s_v[2][kCovFinishLanes][256 / kCovFinishLanes];
    static_assert(256 % kCovFinishLanes == 0, "whole columns");
    const int cols = 256 / kCovFinishLanes, per_e = (M * M + cols - 1) / cols;
    const int e = blockIdx.x / per_e, tid = threadIdx.x;
    const int col = tid % cols, run = tid / cols;
    const int q = (blockIdx.x % per_e) * cols + col; // element i * M + j
    const int i = q / M, j = q % M;
    const bool live = q < M * M && j >= i;
    float vr = 0.f, vi = 0.f;
    if (live) {
        // run r adds slices r, r + runs, ...: eight loads in flight, added in that order
        const size_t slice = (size_t)(2 * M * M), step = (size_t)kCovFinishLanes * slice;
        const float *p = partial + ((size_t)e * G + run) * slice + q;
        const int im_off = j > i ? M * M : 0; // the diagonal's imaginary sums are never written: read its real ones, drop them below
        int g = run;
        for (; g + 7 * kCovFinishLanes < G; g += 8 * kCovFinishLanes, p += 8 * step) {
            float a[8], b[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) a[u] = p[u * step], b[u] = p[u * step + im_off];
#pragma unroll
            for (int u = 0; u < 8; ++u) vr += a[u], vi += b[u];
        }
        for (; g < G; g += kCovFinishLanes, p += step) vr += p[0], vi += p[im_off];
    }
    s_v[0][run][col] = vr;
    s_v[1][run][col] = vi;
    __syncthreads();
    if (run == 0 && live) {
        vr = s_v[0][0][col], vi = s_v[1][0][col];
        for (int r = 1; r < kCovFinishLanes; ++r) vr += s_v[0][r][col], vi += s_v[1][r][col];
        float *o_re = cov_re + (size_t)e * M * M, *o_im = cov_im + (size_t)e * M * M;
        o_re[i * M + j] = vr;
        if (i == j) {
            o_im[i * M + j] = 0.0f;
        } else {
            o_im[i * M + j] = vi;
            o_re[j * M + i] = vr;
            o_im[j * M + i] = -vi;
        }
    }
}

// ---- weights ---------------------------------------------------------------------------------------------------------------------
// One workgroup, thread i = row i: column by column, the diagonal element first, then every row below it.  scratch: l_re | l_im | ok
__global__ void __launch_bounds__(64) array_factor_kernel(const float *__restrict__ cov_re, const float *__restrict__ cov_im, int M, double loading,
                                                         double *__restrict__ scratch)
{
    extern __shared__ __align__(16) unsigned char fac_lds[];
    double *l_re = reinterpret_cast<double *>(fac_lds), *l_im = l_re + M * M;
    __shared__ int s_ok;
    const int t = threadIdx.x;
    for (int idx = t; idx < M * M; idx += 64) l_re[idx] = l_im[idx] = 0.0;
    if (t == 0) s_ok = 1;
    const double load = array_loading_term(cov_re, M, loading);
    __syncthreads();
    for (int j = 0; j < M; ++j) {
        if (t == j && !array_chol_diag(cov_re, load, l_re, l_im, M, j)) s_ok = 0;
        __syncthreads();
        if (!s_ok) break; // uniform: read after the barrier
        if (t > j && t < M) array_chol_offdiag(cov_re, cov_im, l_re, l_im, M, t, j);
        __syncthreads();
    }
    for (int idx = t; idx < M * M; idx += 64) {
        scratch[idx] = l_re[idx];
        scratch[M * M + idx] = l_im[idx];
    }
    if (t == 0) *reinterpret_cast<int *>(scratch + 2 * M * M) = s_ok;
}

// One workgroup per channel: the factor into LDS by all threads, the two solves by thread 0 (the host's loop, gat_array.h)
__global__ void __launch_bounds__(64) array_solve_kernel(int M, const double *__restrict__ steer_re, const double *__restrict__ steer_im, int mode,
                                                        const double *__restrict__ scratch, double *__restrict__ w_re, double *__restrict__ w_im)
{
    extern __shared__ __align__(16) unsigned char sol_lds[];
    double *l_re = reinterpret_cast<double *>(sol_lds), *l_im = l_re + M * M, *z_re = l_im + M * M, *z_im = z_re + M;
    const int k = blockIdx.x, t = threadIdx.x;
    bool ok = true;
    if (mode != GAT_BF_CONVENTIONAL) {
        for (int idx = t; idx < M * M; idx += 64) {
            l_re[idx] = scratch[idx];
            l_im[idx] = scratch[M * M + idx];
        }
        ok = *reinterpret_cast<const int *>(scratch + 2 * M * M) != 0;
    }
    __syncthreads();
    if (t != 0) return;
    double *o_re = w_re + (size_t)k * M, *o_im = w_im + (size_t)k * M;
    const double *a_re = mode == GAT_BF_POWER_INVERSION ? nullptr : steer_re + (size_t)k * M;
    const double *a_im = mode == GAT_BF_POWER_INVERSION ? nullptr : steer_im + (size_t)k * M;
    if (ok) ok = mode == GAT_BF_CONVENTIONAL ? array_conventional_weights(M, a_re, a_im, o_re, o_im)
                                             : array_solve_weights(l_re, l_im, M, a_re, a_im, z_re, z_im, o_re, o_im);
    if (!ok)
        for (int m = 0; m < M; ++m) o_re[m] = o_im[m] = __builtin_nan("");
}

// ---- the weights at work ---------------------------------------------------------------------------------------------------------
// y[row] = sum_m conj(w[k][m]) acc[row][m], row = (b, k, l); FP64 sum: a null subtracts nearly equal terms
__global__ void __launch_bounds__(256) beamform_kernel(const float *__restrict__ acc_re, const float *__restrict__ acc_im, long long rows, int K,
                                                      int L, int M, const double *__restrict__ w_re, const double *__restrict__ w_im,
                                                      float *__restrict__ out_re, float *__restrict__ out_im)
{
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    const int k = (int)((r / L) % K);
    double yr = 0.0, yi = 0.0;
    for (int m = 0; m < M; ++m) {
        const double ar = (double)acc_re[(size_t)r * M + m], ai = (double)acc_im[(size_t)r * M + m];
        const double wr = w_re[(size_t)k * M + m], wi = w_im[(size_t)k * M + m];
        yr += wr * ar + wi * ai;
        yi += wr * ai - wi * ar;
    }
    out_re[r] = (float)yr;
    out_im[r] = (float)yi;
}

// gat_kernels.hip's tracking_update_kernel with the weights handed to the shared update (gat_loop.h)
__global__ void __launch_bounds__(64) tracking_update_weighted_kernel(const float *__restrict__ acc_re, const float *__restrict__ acc_im, int K, int M,
                                                                     const gat_loop_config cfg, gat_loop_state *__restrict__ state,
                                                                     const gat_channel_params *cur, gat_channel_params *next,
                                                                     const double *__restrict__ w_re, const double *__restrict__ w_im)
{
    const int k = blockIdx.x * 64 + threadIdx.x;
    if (k >= K) return;
    gat_loop_state st = state[k];
    gat_channel_params n;
    loop_update_channel(acc_re, acc_im, k, M, cfg, st, cur[k], n, w_re, w_im);
    next[k] = n;
    state[k] = st;
}

template <int FMT, int M>
void cov_small_launch(const CovArgs &a, hipStream_t st)
{
    hipLaunchKernelGGL((cov_small_kernel<FMT, M>), dim3((unsigned)(a.G * a.E)), dim3(kCovSmallThreads), 0, st, a);
}

template <int FMT>
void cov_small_dispatch(const CovArgs &a, hipStream_t st)
{
    switch (a.M) {
    case 1: cov_small_launch<FMT, 1>(a, st); break;
    case 2: cov_small_launch<FMT, 2>(a, st); break;
    case 3: cov_small_launch<FMT, 3>(a, st); break;
    case 4: cov_small_launch<FMT, 4>(a, st); break;
    case 5: cov_small_launch<FMT, 5>(a, st); break;
    case 6: cov_small_launch<FMT, 6>(a, st); break;
    case 7: cov_small_launch<FMT, 7>(a, st); break;
    default: cov_small_launch<FMT, 8>(a, st); break;
    }
}

} // namespace

hipError_t launch_cov_small(const CovArgs &a, int fmt, hipStream_t st)
{
    if (a.M < 1 || a.M > kCovSmallMaxAnts) return hipErrorInvalidValue;
    dispatch_layout(fmt, [&](auto F) { cov_small_dispatch<F>(a, st); });
    return hipGetLastError();
}

hipError_t launch_cov_tiled(const CovArgs &a, int fmt, hipStream_t st)
{
    const CovTileGeom geo = cov_tile_geom(a.M);
    const dim3 grid((unsigned)(a.G * a.E)), block(kCovTileThreads);
    dispatch_layout(fmt, [&](auto F) { hipLaunchKernelGGL(cov_tiled_kernel<F>, grid, block, geo.lds_bytes, st, a, geo); });
    return hipGetLastError();
}

hipError_t launch_cov_finish(const float *partial, int M, int E, int G, float *cov_re, float *cov_im, hipStream_t st)
{
    const int cols = 256 / kCovFinishLanes;
    hipLaunchKernelGGL(cov_finish_kernel, dim3((unsigned)((M * M + cols - 1) / cols * E)), dim3(256), 0, st, partial, M, G, cov_re, cov_im);
    return hipGetLastError();
}

hipError_t launch_array_weights(const float *cov_re, const float *cov_im, int M, const double *steer_re, const double *steer_im, int K, int mode,
                                double loading, double *scratch, double *w_re, double *w_im, hipStream_t st)
{
    const size_t plane = (size_t)M * M * sizeof(double);
    if (mode != GAT_BF_CONVENTIONAL) {
        hipLaunchKernelGGL(array_factor_kernel, dim3(1), dim3(64), 2 * plane, st, cov_re, cov_im, M, loading, scratch);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    const size_t lds = mode != GAT_BF_CONVENTIONAL ? 2 * plane + 2 * (size_t)M * sizeof(double) : 16;
    hipLaunchKernelGGL(array_solve_kernel, dim3((unsigned)K), dim3(64), lds, st, M, steer_re, steer_im, mode, scratch, w_re, w_im);
    return hipGetLastError();
}

hipError_t array_weights_allow_lds()
{
    // 64 antennas: two planes of 64 x 64 doubles = 64 KB, and the solve's 2 x 64 doubles on top
    const int lds = 2 * GAT_MAX_ARRAY_ANTS * GAT_MAX_ARRAY_ANTS * (int)sizeof(double) + 2 * GAT_MAX_ARRAY_ANTS * (int)sizeof(double);
    hipError_t e = hipFuncSetAttribute((const void *)array_factor_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    const hipError_t e2 = hipFuncSetAttribute((const void *)array_solve_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    return e != hipSuccess ? e : e2;
}

hipError_t launch_beamform(const float *acc_re, const float *acc_im, long long rows, int K, int L, int M, const double *w_re, const double *w_im,
                           float *out_re, float *out_im, hipStream_t st)
{
    hipLaunchKernelGGL(beamform_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, acc_re, acc_im, rows, K, L, M, w_re, w_im, out_re,
                       out_im);
    return hipGetLastError();
}

hipError_t launch_tracking_update_weighted(const float *acc_re, const float *acc_im, int K, int M, const gat_loop_config &cfg, gat_loop_state *state,
                                           const gat_channel_params *cur, gat_channel_params *next, const double *w_re, const double *w_im,
                                           hipStream_t st)
{
    hipLaunchKernelGGL(tracking_update_weighted_kernel, dim3((unsigned)((K + 63) / 64)), dim3(64), 0, st, acc_re, acc_im, K, M, cfg, state, cur, next,
                       w_re, w_im);
    return hipGetLastError();
}

} // namespace gat
