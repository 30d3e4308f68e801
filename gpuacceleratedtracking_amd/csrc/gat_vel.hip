// gat_vel.hip -- the velocity fix's kernel (include/gat.h gat_velocity_fix) for gfx950.  The arithmetic is gat_vel.h on top of
// gat_fix.h (the host twin runs the same text), the geometry gat_vel_plan.h, the sums through the wave's LDS gat_fix_wave.h.
//
// One wave runs an epoch and lane k holds channel k: the satellite's clock, orbit and their rates (two Kepler solutions, nothing of
// it depends on the receiver), then its row at the fix's state.  Lane k writes its 14 terms to the wave's own LDS (zeros where the
// channel is not used), lane q < 14 adds row q in channel order, and every lane reads the sums back and solves the 4 x 4 system
// itself, so the solution, the status and every branch on them are the same in all 64 lanes.  A second pass of one term gives the
// sum of the squared residuals; every lane forms the record, lane 0 writes it.  The waves of a workgroup share nothing and meet at
// no barrier.  No atomics.
#include "gat_fix_wave.h"
#include "gat_vel_kernels.h"

namespace gat {

namespace {

__global__ __launch_bounds__(kFixThreads) void vel_kernel(VelArgs a)
{
    __shared__ double lds[kFixWaves * kFixWaveDoubles];
    const int wave = threadIdx.x / kFixWave, lane = threadIdx.x % kFixWave;
    int e;
    if (!fix_epoch_unit(blockIdx.x, wave, a.E, &e)) return; // the whole wave: no barrier follows
    double *buf = lds + wave * kFixWaveDoubles;
    const int K = a.K;
    const bool mine = lane < K;
    const size_t o = (size_t)e * (size_t)K + (size_t)(mine ? lane : 0);
    const double zero[4] = {0.0, 0.0, 0.0, 0.0};

    const gat_fix fix = a.fixes[e]; // the same record in every lane
    if (!vel_fix_given(fix)) {      // the whole wave
        if (lane == 0) a.vel[e] = vel_record(GAT_VEL_NO_FIX, 0, 0, zero, 0.0, zero);
        if (!mine) return;
        if (a.sat_vel) {
            double *q = a.sat_vel + 4 * o;
            q[0] = 0.0, q[1] = 0.0, q[2] = 0.0, q[3] = 0.0;
        }
        if (a.resid) a.resid[o] = 0.0;
        return;
    }
    const double st[4] = {fix.x, fix.y, fix.z, kFixC * fix.clock_bias_s};

    VelSat c{FixSat{0.0, 0.0, 0.0, 0.0, 0.0, false}, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (mine) c = vel_sat(a.eph[lane], a.tx_ms[o], a.tx_frac[o], a.doppler[o]);
    const double w = mine && a.w ? a.w[o] : 1.0;
    const bool used = c.s.ok && fix_weight_ok(w) && (!a.used_in || a.used_in[o] != 0);
    const int num_valid = __popcll(__ballot(c.s.ok));
    const int num_used = __popcll(__ballot(used));

    int status = 0;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    FixRow row{0.0, 0.0, 0.0, 0.0, 0.0};
    if (num_used < 4)
        status |= GAT_VEL_FEW_SATS;
    else {
        if (c.s.ok) row = vel_row(c, st, a.lambda);
        double t[kFixTerms], sums[kFixTerms];
        fix_terms(row, w, t);
        for (int q = 0; q < kFixTerms; ++q) t[q] = used ? t[q] : 0.0;
        fix_wave_sums(buf, lane, K, t, kFixTerms, sums);
        status |= fix_step(sums, s);
    }
    const bool failed = vel_failed(status);
    const double v = !failed && c.s.ok ? vel_resid(row, s) : 0.0;
    double sum_v2[1] = {0.0};
    if (!failed) {
        const double t[1] = {used ? v * v : 0.0};
        fix_wave_sums(buf, lane, K, t, 1, sum_v2);
    }
    if (lane == 0) a.vel[e] = vel_record(status, num_valid, num_used, s, sum_v2[0], st);
    if (!mine) return;
    if (a.sat_vel) {
        double *q = a.sat_vel + 4 * o;
        q[0] = c.vx, q[1] = c.vy, q[2] = c.vz, q[3] = c.ddts;
    }
    if (a.resid) a.resid[o] = v;
}

} // namespace

hipError_t launch_vel(const VelArgs &a, long long grid, hipStream_t st)
{
    if (grid < 1 || grid > 0x7fffffffll) return hipErrorInvalidValue;
    hipLaunchKernelGGL(vel_kernel, dim3((unsigned)grid), dim3(kFixThreads), 0, st, a);
    return hipGetLastError();
}

} // namespace gat
