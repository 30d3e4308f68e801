// gat_spec.hip -- the sample spectrum (include/gat.h, "sample spectrum"): the summed periodogram of the raw samples per (block,
// antenna), a radix-2 FFT in LDS and registers.  The arithmetic is gat_spec.h, shared with the host twin; the refusals, the
// geometry and the work split are gat_spec_plan.h.  Every value meets the same operands in the same order whichever lane holds
// it, so the bits depend neither on the instance nor on the work split.
//   spec_kernel<FMT, VEC, R>: a lane keeps R = max(4, F / 256) points in registers, a TEAM of F / R lanes owns one transform and a
//   workgroup's 256 / team teams each walk the segments of a (block, antenna) pair of their own.  Per segment:
//   * staging: a lane owns fixed positions n of the segment (general path: n = t + team c, one scalar load each; aligned path:
//     the samples of 16-byte loads number t + team c), keeps their window values in registers, and stores w[n] x[n] as a float
//     pair at the bit-reversed index of its team's array.  The next segment's loads are issued before this one's stages run.
//   * passes: log2 R stages on the lane's R registers between two trips through LDS (spec_point_index: which points those are;
//     the first pass takes the 1 .. log2 R stages that log2 F leaves over).  A pass reads and writes back the SAME elements, so
//     one barrier a pass separates them; the last pass is not written back: its registers are bins f = i team + t, squared and
//     added to the lane's R accumulators, which are stored once at the unit's end, consecutive over the lanes.
//   * LDS: both arrays are indexed through spec_skew (the XOR of the index's five-bit digits into its low five bits), which
//     spreads every power-of-two stride of the transform over the banks; scripts/spectrum_lds_model.py counts what is left.
//     The F / 2 twiddles are computed once per workgroup (fir_sincos).
#include <hip/hip_runtime.h>

#include "gat_sample_load.h"
#include "gat_spec.h"
#include "gat_spec_kernels.h"

namespace gat {

namespace {

// rs stages from stage j on, on the lane's R registers
template <int R, int RS>
__device__ __forceinline__ void spec_pass(float (&xr)[R], float (&xi)[R], float2 *pts, const float2 *tw, unsigned t, int j, int L, bool write_back)
{
    unsigned v, ii;
#pragma unroll
    for (int i = 0; i < R; ++i) {
        const float2 x = pts[spec_skew(spec_point_index(t, (unsigned)i, R, j, RS, &v, &ii))];
        xr[i] = x.x, xi[i] = x.y;
    }
#pragma unroll
    for (int q = 0; q < RS; ++q) {
        const int shift = L - 1 - j - q;
#pragma unroll
        for (int i = 0; i < R; ++i) {
            if (i & (1 << q)) continue;
            spec_point_index(t, (unsigned)i, R, j, RS, &v, &ii);
            const unsigned k = ((ii & ((1u << q) - 1u)) << j) | (v & ((1u << j) - 1u));
            const float2 w = tw[spec_skew(k << shift)];
            spec_butterfly(xr[i], xi[i], xr[i | (1 << q)], xi[i | (1 << q)], w.x, w.y);
        }
    }
    if (write_back) {
#pragma unroll
        for (int i = 0; i < R; ++i) pts[spec_skew(spec_point_index(t, (unsigned)i, R, j, RS, &v, &ii))] = make_float2(xr[i], xi[i]);
    }
}

template <int FMT, bool VEC, int R>
__global__ void __launch_bounds__(kSpecThreads) spec_kernel(const SpecArgs a, const float *__restrict__ window)
{
    constexpr int r = spec_ilog2(R);
    constexpr int VS = VEC ? layout_vec_samples(FMT) : 1;
    constexpr int NL = (R + VS - 1) / VS; // loads of a lane per segment (a lane beyond the segment's F / VS loads has none)
    __shared__ float2 s_pts[kSpecThreads * R];
    __shared__ float2 s_tw[kSpecThreads * R / 2];
    const int tid = threadIdx.x, F = a.F, L = a.L, lt = L - r, team = 1 << lt;
    const unsigned t = (unsigned)tid & (unsigned)(team - 1), tm = (unsigned)tid >> lt;
    float2 *pts = s_pts + (size_t)tm * (size_t)F;
    const int passes = (L + r - 1) / r, r0 = L - r * (passes - 1);

    for (int i = tid; i < F / 2; i += kSpecThreads) {
        float wr, wi;
        spec_twiddle(i, F, wr, wi);
        s_tw[spec_skew((unsigned)i)] = make_float2(wr, wi);
    }
    // the lane's positions: load c covers n = (t + team c) VS + s; their window values stay in registers
    float win[NL * VS];
    bool has[NL];
#pragma unroll
    for (int c = 0; c < NL; ++c) {
        const int n0 = ((int)t + team * c) * VS;
        has[c] = n0 < F;
#pragma unroll
        for (int s = 0; s < VS; ++s) win[c * VS + s] = has[c] ? window[n0 + s] : 0.0f;
    }

    for (long long rd = blockIdx.x; rd < a.rounds; rd += gridDim.x) {
        const long long u = rd * a.teams + tm;
        const bool active = u < a.units;
        long long b;
        int m;
        spec_unit(active ? u : 0, a.M, &b, &m);
        const size_t base = (size_t)b * (size_t)a.block_stride + (size_t)m * (size_t)a.ant_stride;
        float acc[R];
#pragma unroll
        for (int i = 0; i < R; ++i) acc[i] = 0.0f;

        // raw samples of one segment: the general path's floats, the aligned path's 16-byte vectors
        float rr[VEC ? 1 : R], ri[VEC ? 1 : R];
        SampleVec<FMT, false> rv[VEC ? NL : 1];
        auto fetch = [&](int s) {
            const size_t seg = base + (size_t)s * (size_t)a.H;
#pragma unroll
            for (int c = 0; c < NL; ++c) {
                if (!active || !has[c]) continue;
                if constexpr (VEC)
                    rv[c].load(a.re, a.im, seg, (long long)((int)t + team * c));
                else
                    load_sample<FMT>(a.re, a.im, seg + (size_t)((int)t + team * c), rr[c], ri[c]);
            }
        };
        fetch(0);
        for (int s = 0; s < a.S; ++s) {
            __syncthreads(); // the last segment's final pass has read its points (the first time: nothing to wait for)
#pragma unroll
            for (int c = 0; c < NL; ++c) {
                if (!active || !has[c]) continue;
#pragma unroll
                for (int e = 0; e < VS; ++e) {
                    float sr, si;
                    if constexpr (VEC)
                        rv[c].sample(e, sr, si);
                    else
                        sr = rr[c], si = ri[c];
                    const float w = win[c * VS + e];
                    const unsigned n = (unsigned)(((int)t + team * c) * VS + e);
                    pts[spec_skew(spec_bitrev(n, L))] = make_float2(spec_mul(w, sr), spec_mul(w, si));
                }
            }
            if (s + 1 < a.S) fetch(s + 1);
            __syncthreads();
            float xr[R], xi[R];
            int j = r0;
            // the stages the first pass takes: R > 4 serves one F = 256 R alone; R = 4 serves F = 64 .. 1024 (uniform)
            if constexpr (R > kSpecMinLanePoints)
                spec_pass<R, (8 + r) - r * ((8 + r + r - 1) / r - 1)>(xr, xi, pts, s_tw, t, 0, L, true);
            else if (r0 == 2)
                spec_pass<R, 2>(xr, xi, pts, s_tw, t, 0, L, true);
            else
                spec_pass<R, 1>(xr, xi, pts, s_tw, t, 0, L, true);
            for (int p = 1; p < passes; ++p, j += r) {
                __syncthreads();
                spec_pass<R, r>(xr, xi, pts, s_tw, t, j, L, p + 1 < passes);
            }
#pragma unroll
            for (int i = 0; i < R; ++i) acc[i] = acc[i] + spec_power(xr[i], xi[i]);
        }
        if (active) {
            float *out = a.power + (size_t)u * (size_t)F + t;
#pragma unroll
            for (int i = 0; i < R; ++i) out[(size_t)i * (size_t)team] = acc[i];
        }
    }
}

template <int FMT, bool VEC>
void spec_dispatch_points(const SpecArgs &a, int R, int grid, hipStream_t st)
{
    const dim3 g((unsigned)grid), b(kSpecThreads);
    switch (R) {
    case 4: hipLaunchKernelGGL((spec_kernel<FMT, VEC, 4>), g, b, 0, st, a, a.window); break;
    case 8: hipLaunchKernelGGL((spec_kernel<FMT, VEC, 8>), g, b, 0, st, a, a.window); break;
    default: hipLaunchKernelGGL((spec_kernel<FMT, VEC, 16>), g, b, 0, st, a, a.window); break;
    }
}

template <bool VEC>
void spec_dispatch(const SpecArgs &a, int R, int fmt, int grid, hipStream_t st)
{
    dispatch_layout(fmt, [&](auto F) { spec_dispatch_points<F, VEC>(a, R, grid, st); });
}

} // namespace

hipError_t launch_spectrum(const SpecArgs &a, const SpecPlan &plan, int fmt, hipStream_t st)
{
    // the geometry the kernels index their LDS by: refuse anything the plan could not have made
    if (a.F < GAT_MIN_SPECTRUM_BINS || a.F > GAT_MAX_SPECTRUM_BINS || (1 << a.L) != a.F || plan.R != spec_lane_points(a.F) || plan.team != a.F / plan.R ||
        a.teams != kSpecThreads / plan.team || a.H < 1 || a.H > a.F || a.S < 1 || a.M < 1 || a.units < 1 || a.rounds != (a.units + a.teams - 1) / a.teams ||
        plan.grid < 1 || plan.grid > a.rounds)
        return hipErrorInvalidValue;
    if (plan.aligned)
        spec_dispatch<true>(a, plan.R, fmt, (int)plan.grid, st);
    else
        spec_dispatch<false>(a, plan.R, fmt, (int)plan.grid, st);
    return hipGetLastError();
}

} // namespace gat
