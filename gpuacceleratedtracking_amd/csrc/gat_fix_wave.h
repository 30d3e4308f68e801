// gat_fix_wave.h -- the wave-wide form of the position fix's passes, shared by the kernels that run an epoch in a wave with a
// channel a lane (gat_fix.hip, gat_raim.hip): the wave's hand-over, the sums through its LDS, a lane's channel, a pass over the used
// set and the elevations.  Device code only; the arithmetic is gat_fix.h, the geometry gat_fix_plan.h.
#pragma once

#include "gat_fix_kernels.h"

namespace gat {

// the wave's LDS writes before, its reads after: the lanes of a wave run in step, the compiler must not move the accesses across
__device__ inline void fix_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// sums[q] = t[q] of lane 0 + t[q] of lane 1 + .. + t[q] of lane K - 1, from +0, q < n <= kFixTerms, in every lane
__device__ inline void fix_wave_sums(double *buf, int lane, int K, const double *t, int n, double *sums)
{
    if (lane < K)
        for (int q = 0; q < n; ++q) buf[q * kFixPitch + lane] = t[q];
    fix_wave_sync();
    if (lane < n) {
        double s = 0.0;
        for (int k = 0; k < K; ++k) s += buf[lane * kFixPitch + k];
        buf[kFixTerms * kFixPitch + lane] = s;
    }
    fix_wave_sync();
    for (int q = 0; q < n; ++q) sums[q] = buf[kFixTerms * kFixPitch + q];
    fix_wave_sync();
}

// a lane's channel and the wave's epoch
struct FixLane {
    FixSat s;
    FixRow row;
    double w, tau, sel;
    bool used;
    double st[4], last_step;
    int status, iterations, num_used;
};

__device__ inline void fix_lane_row(FixLane &l)
{
    if (l.s.ok) {
        l.row = fix_row(l.s, l.tau, l.st);
        l.tau = l.row.r / kFixC;
    }
}

// one pass over the used set; true: converged (the same in every lane)
__device__ inline bool fix_wave_pass(FixLane &l, double *buf, int lane, int K, int max_iter, double tol_m)
{
    if (l.num_used < 4) {
        l.status |= GAT_FIX_FEW_SATS;
        return false;
    }
    for (int it = 0; it < max_iter; ++it) {
        fix_lane_row(l);
        double t[kFixTerms], sums[kFixTerms], d[4];
        fix_terms(l.row, l.w, t);
        for (int q = 0; q < kFixTerms; ++q) t[q] = l.used ? t[q] : 0.0;
        fix_wave_sums(buf, lane, K, t, kFixTerms, sums);
        const int rc = fix_step(sums, d);
        if (rc) {
            l.status |= rc;
            return false;
        }
        for (int i = 0; i < 4; ++i) l.st[i] += d[i];
        l.last_step = __builtin_sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
        l.iterations += 1;
        if (l.last_step < tol_m) return true;
    }
    l.status |= GAT_FIX_NOT_CONVERGED;
    return false;
}

__device__ inline double fix_wave_elevations(FixLane &l)
{
    fix_lane_row(l);
    const double radius = fix_radius(l.st);
    l.sel = l.s.ok ? fix_sin_el(l.row, l.st, radius) : 0.0;
    return radius;
}

} // namespace gat
