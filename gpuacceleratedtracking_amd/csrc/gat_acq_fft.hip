// gat_acq_fft.hip -- the FFT acquisition search (include/gat.h gat_acquire_fft): every code phase of a block from one forward
// transform per (unit, Doppler bin), one per (PRN, block, segment) and one of their product per (PRN, Doppler bin, segment,
// unit).  The arithmetic is gat_acq_fft.h, shared with the host twin; the transform length, the segments, the batches and the
// work split are gat_acq_fft_plan.h.  Every value meets the same operands in the same order whichever lane holds it and however
// the stages are cut into passes, so the bits depend on nothing but the plan's F and group count.
//
// A transform is one of three KINDS, which differ in where a point n of its input comes from and where an output goes:
//   signal:    w[n] = the wiped sample (any layout, scalar loads, zeros from N on)        -> W[unit][Doppler bin][F]
//   replica:   c_g[n] = the chip of sample n + first_shift + g Jseg                       -> C[PRN][block][segment][F]
//   product:   Y[q] = C[q] W[(F - q) mod F]                                               -> the lags the grid keeps, squared, scaled
//                                                                                            and added to the bin by its one owner
// and runs in one of two shapes, a workgroup of 256 lanes holding a tile of 4096 points (32 KB) in LDS either way:
//   * F <= 4096, acq_fft_one_kernel: a workgroup loads its transform's input to the bit-reversed index, runs all L stages and emits.
//   * F > 4096, two passes with the intermediate in memory.  acq_fft_first_kernel: a workgroup takes 4096 / F1 neighbouring COLUMNS
//     n mod F2 of the input (runs of 64 bytes and more), which are that many contiguous chunks of F1 points of the bit-reversed array,
//     runs their first L1 stages and writes each chunk as F1 contiguous points.  acq_fft_second_kernel: a workgroup takes 4096 / F2
//     neighbouring columns p mod F1 of that array (runs of 64 bytes and more again), runs the other L2 stages with the twiddles of
//     the whole transform's stages L1 .. L - 1 and emits -- in place for the signal and the replica, which read and write the same
//     points.  L1 = ceil(L / 2), so 4096 / F1 and 4096 / F2 are 8 .. 64 columns.
// Inside a tile a lane takes four points through two stages between two trips through LDS (one stage first where the count is
// odd); the tile is indexed through spec_skew (gat_spec_plan.h), which spreads the power-of-two strides over the banks.  The
// twiddles are a table of F / 2 built once per call by spec_twiddle: the values computing them in place would give.
//
// The product's owner: a workgroup of the (group k, PRN, Doppler bin, segment, tile) grid emits the bins of its tile's lags for
// unit us + k of this launch; the host enqueues the steps in unit order, so a bin meets its units in order without atomics.  The
// first unit of a group stores, the later ones add; with Gu > 1 each group has a slice of its own and launch_acq_sum_groups
// (gat_acq.hip) adds the slices in group order.
#include <hip/hip_runtime.h>

#include "gat_acq_fft.h"
#include "gat_acq_fft_kernels.h"
#include "gat_sample_load.h"

namespace gat {

namespace {

constexpr int kTile = 1 << kAcqFftTileLog2;
enum { kSignal = 0, kReplica = 1, kProduct = 2 };

// RS stages from local stage j on, over a tile of 2^tlog transforms of 2^nlog points each (transform tr at tile index tr << nlog).
// A local butterfly number kl at local stage j + q is the whole transform's number (kl << cs) | c at stage cs + j + q: cs = 0 and
// c = 0 for a first (or only) pass, cs = L1 and c = the column for a second one.
template <int RS>
__device__ __forceinline__ void fft_pass(float2 *pts, int nlog, int tlog, int j, int cs, int c0, int L, const float2 *__restrict__ tw, int tid)
{
    constexpr int R = 1 << RS;
    const int per = nlog - RS, total = 1 << (per + tlog);
    const unsigned low = (1u << j) - 1u;
    for (int w = tid; w < total; w += kAcqFftThreads) {
        const unsigned tr = (unsigned)w >> per, v = (unsigned)w & ((1u << per) - 1u);
        const unsigned base = (tr << nlog) | ((v >> j) << (j + RS)) | (v & low);
        const unsigned c = cs ? (unsigned)c0 + tr : 0u;
        float xr[R], xi[R];
#pragma unroll
        for (int i = 0; i < R; ++i) {
            const float2 x = pts[spec_skew(base | ((unsigned)i << j))];
            xr[i] = x.x, xi[i] = x.y;
        }
#pragma unroll
        for (int q = 0; q < RS; ++q) {
            const int shift = L - 1 - cs - j - q;
#pragma unroll
            for (int i = 0; i < R; ++i) {
                if (i & (1 << q)) continue;
                const unsigned kl = (((unsigned)i & ((1u << q) - 1u)) << j) | (v & low);
                const float2 t = tw[((kl << cs) | c) << shift];
                spec_butterfly(xr[i], xi[i], xr[i | (1 << q)], xi[i | (1 << q)], t.x, t.y);
            }
        }
#pragma unroll
        for (int i = 0; i < R; ++i) pts[spec_skew(base | ((unsigned)i << j))] = make_float2(xr[i], xi[i]);
    }
}

// all nlog stages of the tile's transforms; the tile is loaded and a barrier passed before, a barrier passed after
__device__ __forceinline__ void fft_tile(float2 *pts, int nlog, int tlog, int cs, int c0, int L, const float2 *__restrict__ tw, int tid)
{
    int j = 0;
    if (nlog & 1) {
        fft_pass<1>(pts, nlog, tlog, 0, cs, c0, L, tw, tid);
        __syncthreads();
        j = 1;
    }
    for (; j < nlog; j += 2) {
        fft_pass<2>(pts, nlog, tlog, j, cs, c0, L, tw, tid);
        __syncthreads();
    }
}

// one transform of a launch: its input, the buffer of its F points (the signal's and the replica's output, the product's
// intermediate) and the product's emission
template <int KIND, int FMT>
struct Transform {
    // signal
    size_t base;
    double step;
    // replica
    const int8_t *code;
    double tau;
    long long x0;
    float inv_lc;
    // product
    const float2 *C, *W;
    float *out;
    bool first;
    int g;
    // all
    float2 *buf;

    __device__ __forceinline__ bool init(const AcqFftArgs &a, int t)
    {
        const size_t F = (size_t)1 << a.L;
        if constexpr (KIND == kSignal) {
            const int il = t % a.dn, ul = t / a.dn;
            const long long u = a.u0 + ul, b = u / a.M, m = u - b * a.M;
            base = (size_t)b * (size_t)a.block_stride + (size_t)m * (size_t)a.ant_stride;
            step = acq_fft_step(a.if_hz, a.f_first, a.f_step, a.i0 + il, a.fs);
            buf = a.W + ((size_t)ul * (size_t)a.Db + (size_t)il) * F;
        } else if constexpr (KIND == kReplica) {
            const int gg = t % a.G, bl = (t / a.G) % a.bn, p = t / (a.G * a.bn);
            code = a.codes + (size_t)a.prns[p] * (size_t)a.code_row_stride;
            tau = acq_fft_tau(a.ratio, a.b0 + bl, a.block_stride, a.Lc);
            x0 = a.first_shift + (long long)gg * a.Jseg;
            inv_lc = 1.0f / (float)a.Lc;
            buf = a.C + (((size_t)p * (size_t)a.Bb + (size_t)bl) * (size_t)a.G + (size_t)gg) * F;
        } else {
            g = t % a.G;
            const int il = (t / a.G) % a.dn, p = (t / (a.G * a.dn)) % a.P, k = t / (a.G * a.dn * a.P);
            const long long u = (long long)a.us + k;
            if (u >= (long long)a.u0 + a.un) return false; // the last step of a batch may be short
            const long long b = u / a.M;
            C = a.C + (((size_t)p * (size_t)a.Bb + (size_t)(b - a.b0)) * (size_t)a.G + (size_t)g) * F;
            W = a.W + ((size_t)(u - a.u0) * (size_t)a.Db + (size_t)il) * F;
            out = a.out + (a.Gu > 1 ? (size_t)k * (size_t)a.cells : 0) + ((size_t)p * (size_t)a.D + (size_t)(a.i0 + il)) * (size_t)a.J;
            first = u < a.Gu;
            buf = a.Y ? a.Y + (size_t)t * F : nullptr;
        }
        return true;
    }

    __device__ __forceinline__ float2 load(const AcqFftArgs &a, unsigned n) const
    {
        if constexpr (KIND == kSignal) {
            float wr = 0.0f, wi = 0.0f;
            if ((long long)n < a.N) {
                float xr, xi;
                load_sample<FMT>(a.re, a.im, base + (size_t)n, xr, xi);
                acq_fft_wipe(xr, xi, (long long)n, step, wr, wi);
            }
            return make_float2(wr, wi);
        } else if constexpr (KIND == kReplica) {
            return make_float2((float)code[acq_fft_chip_index(a.ratio, tau, (int)(x0 + (long long)n), a.Lc, inv_lc)], 0.0f);
        } else {
            const unsigned F = 1u << a.L;
            const float2 c = C[n], w = W[(F - n) & (F - 1u)];
            float2 y;
            acq_fft_product(c.x, c.y, w.x, w.y, y.x, y.y);
            return y;
        }
    }

    // output idx of the transform
    __device__ __forceinline__ void emit(const AcqFftArgs &a, unsigned idx, float2 x) const
    {
        if constexpr (KIND == kProduct) {
            const unsigned F = 1u << a.L;
            const int j = acq_fft_lag_bin((long long)((F - idx) & (F - 1u)), g, a.Jseg, a.s, a.J);
            if (j < 0) return;
            const float v = acq_fft_term(x.x, x.y, a.scale);
            out[j] = first ? v : out[j] + v;
        } else {
            buf[idx] = x;
        }
    }
};

template <int KIND, int FMT>
__global__ void __launch_bounds__(kAcqFftThreads) acq_fft_one_kernel(const AcqFftArgs a)
{
    __shared__ float2 s_pts[kTile];
    const int tid = threadIdx.x, F = 1 << a.L;
    Transform<KIND, FMT> x;
    if (!x.init(a, (int)blockIdx.x)) return;
    for (int n = tid; n < F; n += kAcqFftThreads) s_pts[spec_skew(spec_bitrev((unsigned)n, a.L))] = x.load(a, (unsigned)n);
    __syncthreads();
    fft_tile(s_pts, a.L, 0, 0, 0, a.L, a.tw, tid);
    for (int idx = tid; idx < F; idx += kAcqFftThreads) x.emit(a, (unsigned)idx, s_pts[spec_skew((unsigned)idx)]);
}

template <int KIND, int FMT>
__global__ void __launch_bounds__(kAcqFftThreads) acq_fft_first_kernel(const AcqFftArgs a)
{
    __shared__ float2 s_pts[kTile];
    const int tid = threadIdx.x, tlog = kAcqFftTileLog2 - a.L1;
    const int t = (int)(blockIdx.x / (unsigned)a.tiles), tile = (int)(blockIdx.x % (unsigned)a.tiles);
    const unsigned c0 = (unsigned)tile << tlog;
    Transform<KIND, FMT> x;
    if (!x.init(a, t)) return;
    // point e of the tile: column c0 + (e mod T) of row e / T, i.e. sample (row << L2) | column, to chunk e mod T at the row's reversal
    for (int e = tid; e < kTile; e += kAcqFftThreads) {
        const unsigned tc = (unsigned)e & ((1u << tlog) - 1u), r = (unsigned)e >> tlog;
        s_pts[spec_skew((tc << a.L1) | spec_bitrev(r, a.L1))] = x.load(a, (r << a.L2) | (c0 + tc));
    }
    __syncthreads();
    fft_tile(s_pts, a.L1, tlog, 0, 0, a.L, a.tw, tid);
    for (int e = tid; e < kTile; e += kAcqFftThreads) {
        const unsigned tc = (unsigned)e >> a.L1, i = (unsigned)e & ((1u << a.L1) - 1u);
        x.buf[((size_t)spec_bitrev(c0 + tc, a.L2) << a.L1) | i] = s_pts[spec_skew((unsigned)e)];
    }
}

template <int KIND>
__global__ void __launch_bounds__(kAcqFftThreads) acq_fft_second_kernel(const AcqFftArgs a)
{
    __shared__ float2 s_pts[kTile];
    const int tid = threadIdx.x, tlog = kAcqFftTileLog2 - a.L2;
    const int t = (int)(blockIdx.x / (unsigned)a.tiles), tile = (int)(blockIdx.x % (unsigned)a.tiles);
    const unsigned c0 = (unsigned)tile << tlog;
    Transform<KIND, GAT_LAYOUT_PLANAR> x;
    if (!x.init(a, t)) return;
    for (int e = tid; e < kTile; e += kAcqFftThreads) {
        const unsigned tc = (unsigned)e & ((1u << tlog) - 1u), r = (unsigned)e >> tlog;
        s_pts[spec_skew((tc << a.L2) | r)] = x.buf[((size_t)r << a.L1) | (c0 + tc)];
    }
    __syncthreads();
    fft_tile(s_pts, a.L2, tlog, a.L1, (int)c0, a.L, a.tw, tid);
    for (int e = tid; e < kTile; e += kAcqFftThreads) {
        const unsigned tc = (unsigned)e & ((1u << tlog) - 1u), r = (unsigned)e >> tlog;
        x.emit(a, (r << a.L1) | (c0 + tc), s_pts[spec_skew((tc << a.L2) | r)]);
    }
}

__global__ void __launch_bounds__(kAcqFftThreads) acq_fft_twiddle_kernel(float2 *__restrict__ tw, int F)
{
    const int i = (int)(blockIdx.x * kAcqFftThreads + threadIdx.x);
    if (i >= F / 2) return;
    float wr, wi;
    spec_twiddle(i, F, wr, wi);
    tw[i] = make_float2(wr, wi);
}

// the geometry the kernels index by: refuse anything the plan could not have made
bool args_ok(const AcqFftArgs &a)
{
    if (a.L < kAcqFftMinLog2 || a.L > kAcqFftMaxLog2 || a.L1 + a.L2 != a.L || a.N < 1 || a.N >= (1ll << a.L) || a.Jseg != (1ll << a.L) - a.N + 1) return false;
    if (a.L <= kAcqFftOnePassLog2 ? (a.L2 != 0 || a.tiles != 1) : (a.L1 != (a.L + 1) / 2 || a.tiles != 1 << (a.L - kAcqFftTileLog2) || !a.Y)) return false;
    if (a.G < 1 || a.Db < 1 || a.Gu < 1 || a.Bb < 1 || a.P < 1 || a.D < 1 || a.J < 1 || a.s < 1 || a.M < 1 || a.Lc < 1 || !a.tw || !a.C || !a.W || !a.out) return false;
    if (a.dn < 1 || a.dn > a.Db || a.i0 < 0 || a.i0 + a.dn > a.D || a.un < 1 || a.u0 < 0 || a.u0 + a.un > a.units || a.bn < 1 || a.bn > a.Bb || a.b0 < 0 || a.b0 + a.bn > a.B) return false;
    return a.u0 / a.M >= a.b0 && (a.u0 + a.un - 1) / a.M < a.b0 + a.bn;
}

template <int KIND, int FMT>
hipError_t launch(const AcqFftArgs &a, long long transforms, hipStream_t st)
{
    if (!args_ok(a) || transforms < 1 || transforms * a.tiles >= (1ll << 30)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)(transforms * a.tiles)), block(kAcqFftThreads);
    if (a.L <= kAcqFftOnePassLog2) {
        hipLaunchKernelGGL((acq_fft_one_kernel<KIND, FMT>), grid, block, 0, st, a);
    } else {
        hipLaunchKernelGGL((acq_fft_first_kernel<KIND, FMT>), grid, block, 0, st, a);
        hipLaunchKernelGGL((acq_fft_second_kernel<KIND>), grid, block, 0, st, a);
    }
    return hipGetLastError();
}

} // namespace

hipError_t launch_acq_fft_twiddles(const AcqFftArgs &a, hipStream_t st)
{
    if (a.L < kAcqFftMinLog2 || a.L > kAcqFftMaxLog2 || !a.tw) return hipErrorInvalidValue;
    const int F = 1 << a.L;
    hipLaunchKernelGGL(acq_fft_twiddle_kernel, dim3((unsigned)(F / 2 / kAcqFftThreads)), dim3(kAcqFftThreads), 0, st, a.tw, F);
    return hipGetLastError();
}

hipError_t launch_acq_fft_replica(const AcqFftArgs &a, hipStream_t st)
{
    return launch<kReplica, GAT_LAYOUT_PLANAR>(a, (long long)a.P * a.bn * a.G, st);
}

hipError_t launch_acq_fft_signal(const AcqFftArgs &a, int fmt, hipStream_t st)
{
    const long long transforms = (long long)a.un * a.dn;
    if (fmt < GAT_LAYOUT_PLANAR || fmt > GAT_LAYOUT_INTERLEAVED_I8) return hipErrorInvalidValue;
    return dispatch_layout(fmt, [&](auto F) { return launch<kSignal, F>(a, transforms, st); });
}

hipError_t launch_acq_fft_correlate(const AcqFftArgs &a, hipStream_t st)
{
    if (a.us < a.u0 || a.us >= a.u0 + a.un || a.us % a.Gu != 0) return hipErrorInvalidValue;
    return launch<kProduct, GAT_LAYOUT_PLANAR>(a, (long long)a.Gu * a.P * a.dn * a.G, st);
}

} // namespace gat
