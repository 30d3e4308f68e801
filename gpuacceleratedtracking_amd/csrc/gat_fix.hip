// gat_fix.hip -- the position fix's kernel (include/gat.h gat_position_fix) for gfx950.  The arithmetic is gat_fix.h (the host twin
// runs the same text), the geometry gat_fix_plan.h, the wave-wide passes gat_fix_wave.h (shared with gat_raim.hip).
//
// One wave runs an epoch and lane k holds channel k: the satellite's clock and orbit (two Kepler solutions, nothing of it depends
// on the receiver) once, then per iteration its row at the state.  The 14 sums of the normal equations go through the wave's own
// LDS: lane k writes its terms (zeros where the channel is not used: adding +0 to a sum that began at +0 changes no bit), lane
// q < 14 adds row q in channel order, and every lane reads the 14 sums back and solves the 4 x 4 system itself, so the state, the
// step and every branch on them are the same in all 64 lanes and the wave leaves the iteration together.  The waves of a
// workgroup share nothing and meet at no barrier: an epoch that fails or converges early holds no other up.  No atomics.
#include "gat_fix_wave.h"

namespace gat {

namespace {

__global__ __launch_bounds__(kFixThreads) void fix_kernel(FixArgs a)
{
    __shared__ double lds[kFixWaves * kFixWaveDoubles];
    const int wave = threadIdx.x / kFixWave, lane = threadIdx.x % kFixWave;
    int e;
    if (!fix_epoch_unit(blockIdx.x, wave, a.E, &e)) return; // the whole wave: no barrier follows
    double *buf = lds + wave * kFixWaveDoubles;
    const int K = a.K;
    const bool mine = lane < K;
    const size_t o = (size_t)e * (size_t)K + (size_t)(mine ? lane : 0);

    FixLane l;
    l.s = FixSat{0.0, 0.0, 0.0, 0.0, 0.0, false};
    if (mine) l.s = fix_sat(a.eph[lane], a.tx_ms[o], a.tx_frac[o], a.rx_ms[e], a.rx_frac[e]);
    l.w = mine && a.w ? a.w[o] : 1.0;
    l.used = l.s.ok && fix_weight_ok(l.w);
    l.tau = kFixFirstTravel;
    l.row = FixRow{0.0, 0.0, 0.0, 0.0, 0.0};
    l.sel = 0.0;
    l.st[0] = a.init_xyz[0], l.st[1] = a.init_xyz[1], l.st[2] = a.init_xyz[2], l.st[3] = 0.0;
    l.status = 0, l.iterations = 0, l.last_step = 0.0;
    const int num_valid = __popcll(__ballot(l.s.ok));
    l.num_used = __popcll(__ballot(l.used));

    const bool converged = fix_wave_pass(l, buf, lane, K, a.max_iter, a.tol_m);
    if (!fix_failed(l.status)) {
        const double radius = fix_wave_elevations(l);
        if (converged && a.mask_sin > -1.0 && radius >= kFixMaskRadius) {
            const bool keep = l.used && l.sel >= a.mask_sin;
            const int kept = __popcll(__ballot(keep));
            if (kept != l.num_used) {
                if (kept >= 4) {
                    l.used = keep;
                    l.num_used = kept;
                    l.status |= GAT_FIX_MASKED;
                    fix_wave_pass(l, buf, lane, K, a.max_iter, a.tol_m);
                    if (!fix_failed(l.status)) fix_wave_elevations(l);
                } else
                    l.status |= GAT_FIX_MASK_STARVED;
            }
        }
    }
    const bool failed = fix_failed(l.status);
    double sums[kFixTerms] = {};
    if (!failed) {
        double t[kFixTerms];
        fix_terms(l.row, 1.0, t);
        t[10] = l.row.v * l.row.v;
        for (int q = 0; q < 11; ++q) t[q] = l.used ? t[q] : 0.0;
        fix_wave_sums(buf, lane, K, t, 11, sums);
    }
    if (lane == 0) a.fixes[e] = fix_record(l.status, num_valid, l.num_used, l.iterations, l.st, sums[10], l.last_step, sums);
    if (!mine) return;
    if (a.sat) {
        double *q = a.sat + 4 * o;
        q[0] = l.s.X, q[1] = l.s.Y, q[2] = l.s.Z, q[3] = l.s.dts;
    }
    if (a.resid) a.resid[o] = !failed && l.s.ok ? l.row.v : 0.0;
    if (a.sin_el) a.sin_el[o] = !failed ? l.sel : 0.0;
    if (a.used) a.used[o] = (uint8_t)(!failed && l.used ? 1 : 0);
}

} // namespace

hipError_t launch_fix(const FixArgs &a, long long grid, hipStream_t st)
{
    if (grid < 1 || grid > 0x7fffffffll) return hipErrorInvalidValue;
    hipLaunchKernelGGL(fix_kernel, dim3((unsigned)grid), dim3(kFixThreads), 0, st, a);
    return hipGetLastError();
}

} // namespace gat
