// gat_acq.hip -- the acquisition search (include/gat.h gat_acquire): power over PRN x Doppler x code phase.
//
// What is computed, per PRN p, Doppler bin i, code bin j:
//   P[p,i,j] = sum_b sum_m | sum_{n<N} x[n,m,b] * conj(exp(j2pi n (if + f_i)/fs)) * c_p[floor(fc/fs (n + Delta_j) + tau_b) mod Lc] |^2
// i.e. gat_downconvert_and_correlate's R for the channel {p, fc, if + f_i, tau_b, 0} and the tap Delta_j = first_shift + s j,
// squared after the coherent sum over one antenna's block, summed over antennas and blocks.
//
// The structure the kernel exploits: the wiped signal x conj(carrier_i) does not depend on the PRN or the code bin, and the
// replica does not depend on the Doppler bin -- it is a Toeplitz window, the same chip sequence shifted by s samples per code
// bin.  So one workgroup owns (PRN, 32 Doppler bins, 256 code bins) and walks a block in chunks of kAcqChunk samples:
//   * the chunk's replica window (kAcqChunk + s * 255 chips) goes to LDS once, as float pairs (chip x, chip x + 1): any
//     code bin reads the chips of two consecutive samples with one 8-byte read;
//   * the chunk's wiped samples for the workgroup's 32 Doppler bins go to LDS once (carrier: the correlator's exact
//     evaluation, gat_phase.h sincos_cycles on the double-precision phase);
//   * wave w owns Doppler bins 8w .. 8w+7, lane l the code bins l + 64 r (r < 4): an 8 x 4 register tile of complex sums,
//     two FMAs per (Doppler, code, sample), one 16-byte broadcast read per (Doppler bin, two samples) and one 8-byte read per
//     (code bin, two samples).  The tile sums kAcqChunksPerSum chunks (1024 samples) and is then added to a second tile
//     holding the block's sums: a two-level sum.  A single running sum per lane over a whole 1 ms block at 20 MHz drifts to
//     ~1e-5; adding every 128-sample chunk into the block's sum kept 20 000 samples at ~1e-6 but not 2^21 (a bin of a
//     Doppler row off the peak missed 1e-5).  1024-sample sums balance the two levels' rounding over that range.
// An antenna's coherent sums are finished before they are squared.  Antennas and blocks (the non-coherent units) are split
// over G workgroup groups when the grid alone does not fill the device; every group owns its own slice of a scratch grid
// (plain stores / read-modify-writes of bins only it touches), and a second kernel adds the G slices in a fixed order: no
// atomics, the same bits on every run.  Samples are read with scalar loads (any layout, any alignment, any N: a chunk
// past the block's end reads zeros); the search is bound by arithmetic, not by the signal's bytes.
#include <hip/hip_runtime.h>

#include "gat_acq.h"
#include "gat_acq_kernels.h"
#include "gat_phase.h"
#include "gat_sample_load.h"

namespace gat {

namespace {

constexpr int kAcqChunksPerSum = 8; // chunks the register tile sums before it is added to the block's sum

template <int FMT>
__global__ void __launch_bounds__(kAcqThreads, 2) acq_grid_kernel(const AcqArgs a)
{
    extern __shared__ __align__(16) unsigned char acq_lds[];
    double *s_step = reinterpret_cast<double *>(acq_lds);                                // [kAcqDopTile] cycles per sample
    float4 *s_w = reinterpret_cast<float4 *>(acq_lds + kAcqDopTile * sizeof(double));   // [kAcqDopTile][kAcqChunk / 2]
    float *s_rep = reinterpret_cast<float *>(acq_lds + kAcqDopTile * sizeof(double) +
                                             (size_t)kAcqDopTile * kAcqChunk * 2 * sizeof(float)); // pairs [rep_len][2]

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int j0 = blockIdx.x * kAcqCodeTile, d0 = blockIdx.y * kAcqDopTile;
    const int p = blockIdx.z / a.G, g = blockIdx.z % a.G;
    const int s = a.s;
    const int8_t *code = a.codes + (size_t)a.prns[p] * a.code_row_stride;
    const float inv_lc = 1.0f / (float)a.Lc;
    if (tid < kAcqDopTile) {
        const double f = a.if_hz + (a.f_first + (double)(d0 + tid) * a.f_step); // the channel record's carrier_freq_hz
        s_step[tid] = f / a.fs;
    }
    const int rep_len = kAcqChunk + s * (kAcqCodeTile - 1); // chips of one chunk's window
    const int units = a.M * a.B;

    for (int u = g; u < units; u += a.G) {
        const int m = u % a.M, b = u / a.M;
        const double tau = __builtin_fmod(a.ratio * (double)((long long)b * a.block_stride), (double)a.Lc);
        const size_t base = (size_t)b * a.block_stride + (size_t)m * a.ant_stride;
        float tot_re[kAcqDopPerWave][kAcqCodePerLane], tot_im[kAcqDopPerWave][kAcqCodePerLane];
#pragma unroll
        for (int d = 0; d < kAcqDopPerWave; ++d)
#pragma unroll
            for (int r = 0; r < kAcqCodePerLane; ++r) tot_re[d][r] = tot_im[d][r] = 0.f;

        float acc_re[kAcqDopPerWave][kAcqCodePerLane], acc_im[kAcqDopPerWave][kAcqCodePerLane];
        for (long long n0 = 0; n0 < a.N; n0 += kAcqChunk) {
            const int chunk = (int)(n0 / kAcqChunk); // N < 2^30
            __syncthreads(); // the previous chunk's reads are done (and s_step is written before the first)
            // replica window: entry e <-> x = n0 + first_shift + s j0 + e; pair e = (chip e, chip e + 1)
            const long long x0 = n0 + a.first_shift + (long long)s * j0;
            for (int e = tid; e < rep_len; e += kAcqThreads) {
                const float c = (float)code[chip_index(a.ratio, tau, (int)(x0 + e), a.Lc, inv_lc)];
                s_rep[2 * e] = c;
                if (e > 0) s_rep[2 * e - 1] = c;
            }
            // wiped samples: thread t -> sample n = t % kAcqChunk of the chunk, Doppler bins t / kAcqChunk + 2 k
            {
                const int n = tid & (kAcqChunk - 1), dh = tid / kAcqChunk;
                const long long nn = n0 + n;
                float xr = 0.f, xi = 0.f;
                if (nn < a.N) load_sample<FMT>(a.re, a.im, base + (size_t)nn, xr, xi);
                float *w = reinterpret_cast<float *>(s_w);
#pragma unroll 4
                for (int d = dh; d < kAcqDopTile; d += kAcqThreads / kAcqChunk) {
                    const double th = __builtin_fma((double)nn, s_step[d], 0.0); // the correlator's carrier, phase 0
                    float cr, ci;
                    sincos_cycles(th - __builtin_rint(th), cr, ci);
                    w[(d * kAcqChunk + n) * 2] = __builtin_fmaf(xr, cr, xi * ci); // conjugate wipe-off
                    w[(d * kAcqChunk + n) * 2 + 1] = __builtin_fmaf(xi, cr, -(xr * ci));
                }
            }
            __syncthreads();
            const float4 *wv = s_w + (size_t)wave * kAcqDopPerWave * (kAcqChunk / 2);
            const float2 *rp = reinterpret_cast<const float2 *>(s_rep) + (size_t)s * lane;
            if (chunk % kAcqChunksPerSum == 0) {
#pragma unroll
                for (int d = 0; d < kAcqDopPerWave; ++d)
#pragma unroll
                    for (int r = 0; r < kAcqCodePerLane; ++r) acc_re[d][r] = acc_im[d][r] = 0.f;
            }
#pragma unroll 2
            for (int n = 0; n < kAcqChunk; n += 2) {
                float2 cp[kAcqCodePerLane];
#pragma unroll
                for (int r = 0; r < kAcqCodePerLane; ++r) cp[r] = rp[n + s * 64 * r];
#pragma unroll
                for (int d = 0; d < kAcqDopPerWave; ++d) {
                    const float4 x = wv[d * (kAcqChunk / 2) + n / 2];
#pragma unroll
                    for (int r = 0; r < kAcqCodePerLane; ++r) {
                        acc_re[d][r] = __builtin_fmaf(cp[r].x, x.x, acc_re[d][r]);
                        acc_im[d][r] = __builtin_fmaf(cp[r].x, x.y, acc_im[d][r]);
                        acc_re[d][r] = __builtin_fmaf(cp[r].y, x.z, acc_re[d][r]);
                        acc_im[d][r] = __builtin_fmaf(cp[r].y, x.w, acc_im[d][r]);
                    }
                }
            }
            if (chunk % kAcqChunksPerSum == kAcqChunksPerSum - 1 || n0 + kAcqChunk >= a.N) {
#pragma unroll
                for (int d = 0; d < kAcqDopPerWave; ++d)
#pragma unroll
                    for (int r = 0; r < kAcqCodePerLane; ++r) {
                        tot_re[d][r] += acc_re[d][r];
                        tot_im[d][r] += acc_im[d][r];
                    }
            }
        }
        // |R|^2 of this antenna and block into the group's slice: the first unit stores, the later ones add
        float *out = a.out + (size_t)(g * a.P + p) * a.D * a.J;
#pragma unroll
        for (int d = 0; d < kAcqDopPerWave; ++d) {
            const int i = d0 + wave * kAcqDopPerWave + d;
#pragma unroll
            for (int r = 0; r < kAcqCodePerLane; ++r) {
                const int j = j0 + lane + 64 * r;
                if (i < a.D && j < a.J) {
                    const float v = tot_re[d][r] * tot_re[d][r] + tot_im[d][r] * tot_im[d][r];
                    float *o = out + (size_t)i * a.J + j;
                    *o = (u == g) ? v : *o + v;
                }
            }
        }
    }
}

// power[i] = sum over the G group slices in order
__global__ void __launch_bounds__(256) acq_sum_groups_kernel(const float *__restrict__ part, float *__restrict__ power,
                                                            long long cells, int G)
{
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < cells; i += (long long)gridDim.x * 256) {
        float v = part[i];
        for (int g = 1; g < G; ++g) v += part[(size_t)g * cells + i];
        power[i] = v;
    }
}

// One workgroup per PRN: peak (first on ties), then the noise set's sum (double, per-thread strided order then a fixed
// tree), size and maximum; thread 0 finishes with the shared arithmetic (gat_acq.h).
__global__ void __launch_bounds__(256) acq_stats_kernel(const float *__restrict__ power, int D, int J, gat_acq_config cfg,
                                                        double fs, long long N, const int *__restrict__ prns,
                                                        gat_acq_result *__restrict__ res)
{
    __shared__ float s_v[256];
    __shared__ long long s_i[256];
    __shared__ double s_sum[256];
    __shared__ long long s_cnt[256];
    const int p = blockIdx.x, t = threadIdx.x;
    const float *P = power + (size_t)p * D * J;
    const long long cells = (long long)D * J;
    float best = -1.0f;
    long long bi = 0;
    for (long long c = t; c < cells; c += 256)
        if (P[c] > best) best = P[c], bi = c;
    s_v[t] = best;
    s_i[t] = bi;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (t < h) {
            const float v2 = s_v[t + h];
            const long long i2 = s_i[t + h];
            if (v2 > s_v[t] || (v2 == s_v[t] && i2 < s_i[t])) s_v[t] = v2, s_i[t] = i2;
        }
        __syncthreads();
    }
    const long long pk = s_i[0];
    const int pi = (int)(pk / J), pj = (int)(pk % J);
    const double Lc = (double)cfg.code_length;
    const double ph_pk = acq_code_phase(cfg, fs, (double)pj);
    __syncthreads();
    double sum = 0.0;
    long long cnt = 0;
    float second = -1.0f;
    for (long long c = t; c < cells; c += 256) {
        const int j = (int)(c % J);
        if (acq_in_noise_set(acq_code_phase(cfg, fs, (double)j), ph_pk, Lc)) {
            sum += (double)P[c];
            ++cnt;
            second = P[c] > second ? P[c] : second;
        }
    }
    s_sum[t] = sum;
    s_cnt[t] = cnt;
    s_v[t] = second;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (t < h) {
            s_sum[t] += s_sum[t + h];
            s_cnt[t] += s_cnt[t + h];
            s_v[t] = s_v[t + h] > s_v[t] ? s_v[t + h] : s_v[t];
        }
        __syncthreads();
    }
    if (t == 0) {
        const double nan = __builtin_nan("");
        gat_acq_result r{};
        r.prn = prns[p];
        acq_finish(cfg, fs, N, D, J, pi, pj, (double)P[pk], pi > 0 ? (double)P[pk - J] : nan,
                   pi < D - 1 ? (double)P[pk + J] : nan, pj > 0 ? (double)P[pk - 1] : nan, pj < J - 1 ? (double)P[pk + 1] : nan,
                   s_sum[0], s_cnt[0], (double)s_v[0], r);
        res[p] = r;
    }
}

} // namespace

hipError_t launch_acq_grid(const AcqArgs &a, int fmt, hipStream_t st)
{
    const dim3 grid((unsigned)((a.J + kAcqCodeTile - 1) / kAcqCodeTile), (unsigned)((a.D + kAcqDopTile - 1) / kAcqDopTile),
                    (unsigned)(a.P * a.G));
    const size_t lds = acq_grid_lds_bytes(a.s);
    dispatch_layout(fmt, [&](auto F) { hipLaunchKernelGGL(acq_grid_kernel<F>, grid, dim3(kAcqThreads), lds, st, a); });
    return hipGetLastError();
}

hipError_t acq_grid_allow_lds(int s)
{
    const int lds = (int)acq_grid_lds_bytes(s);
    hipError_t e = hipSuccess;
    for (const void *k : {(const void *)acq_grid_kernel<GAT_LAYOUT_PLANAR>, (const void *)acq_grid_kernel<GAT_LAYOUT_INTERLEAVED>,
                          (const void *)acq_grid_kernel<GAT_LAYOUT_INTERLEAVED_I16>,
                          (const void *)acq_grid_kernel<GAT_LAYOUT_INTERLEAVED_I8>}) {
        const hipError_t e2 = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        if (e2 != hipSuccess) e = e2;
    }
    return e;
}

hipError_t launch_acq_sum_groups(const float *part, float *power, long long cells, int G, hipStream_t st)
{
    long long blocks = (cells + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(acq_sum_groups_kernel, dim3((unsigned)blocks), dim3(256), 0, st, part, power, cells, G);
    return hipGetLastError();
}

hipError_t launch_acq_stats(const float *power, int P, int D, int J, const gat_acq_config &cfg, double fs, long long N,
                            const int *prns, gat_acq_result *res, hipStream_t st)
{
    hipLaunchKernelGGL(acq_stats_kernel, dim3((unsigned)P), dim3(256), 0, st, power, D, J, cfg, fs, N, prns, res);
    return hipGetLastError();
}

} // namespace gat
