// gat_raim.hip -- the fix integrity's kernel (include/gat.h gat_position_fix_raim) for gfx950.  The arithmetic is gat_fix.h and
// gat_raim.h (the host twin runs the same text), the geometry gat_raim_plan.h, the wave-wide passes gat_fix_wave.h.
//
// One wave runs an epoch and lane k holds channel k.  The first part is the position fix's kernel: the satellites, the first pass,
// the mask, the second pass.  The final sums carry one more term, T, so the test costs no reduction of its own, and an epoch whose
// test passes -- nearly every one -- leaves there: the branch is the same in all 64 lanes, its cost over gat_position_fix one term
// and the integrity record.  A detected epoch writes the full set's outputs first (they stand unless a channel is left out) and
// runs its rounds lane-per-candidate: after one hand-over every lane has written its channel, frozen where the last row put it, to
// the wave's LDS as six doubles; lane j then solves U \ {j} by itself, reading every channel's entry at the same address in all
// lanes (a broadcast) and forming the 14 sums in registers in channel order, with no reduction through LDS and no hand-over inside
// the trial: lanes that converge early idle until the last one is done.  The choice is a butterfly of shuffles over (T_j, j), a
// total order, the winner's state is broadcast and the final pass is wave-wide again.  The waves of a workgroup share nothing and
// meet at no barrier.  No atomics, no scratch.
#include "gat_fix_wave.h"
#include "gat_raim_kernels.h"

namespace gat {

namespace {

// the 11 sums of the record and T (sums[11]) of the used set at the rows as they stand, in every lane
__device__ inline void raim_wave_record_sums(const FixLane &l, double *buf, int lane, int K, double *sums)
{
    double t[kFixTerms];
    fix_terms(l.row, 1.0, t);
    t[10] = l.row.v * l.row.v;
    t[11] = raim_term(l.w, l.row.v);
    for (int q = 0; q < 12; ++q) t[q] = l.used ? t[q] : 0.0;
    fix_wave_sums(buf, lane, K, t, 12, sums);
}

// the record and the lane's channel of the state as it stands, `extra` status bits added
__device__ inline void raim_wave_write(const RaimArgs &a, int e, size_t o, int lane, bool mine, const FixLane &l, int extra, int num_valid,
                                       const double *sums)
{
    const bool failed = fix_failed(l.status);
    if (lane == 0) a.fix.fixes[e] = fix_record(l.status | extra, num_valid, l.num_used, l.iterations, l.st, sums[10], l.last_step, sums);
    if (!mine) return;
    if (a.fix.sat) {
        double *q = a.fix.sat + 4 * o;
        q[0] = l.s.X, q[1] = l.s.Y, q[2] = l.s.Z, q[3] = l.s.dts;
    }
    if (a.fix.resid) a.fix.resid[o] = !failed && l.s.ok ? l.row.v : 0.0;
    if (a.fix.sin_el) a.fix.sin_el[o] = !failed ? l.sel : 0.0;
    if (a.fix.used) a.fix.used[o] = (uint8_t)(!failed && l.used ? 1 : 0);
}

__global__ __launch_bounds__(kFixThreads) void raim_kernel(RaimArgs a)
{
    __shared__ double lds[kFixWaves * kRaimWaveDoubles];
    const int wave = threadIdx.x / kFixWave, lane = threadIdx.x % kFixWave;
    int e;
    if (!fix_epoch_unit(blockIdx.x, wave, a.fix.E, &e)) return; // the whole wave: no barrier follows
    double *buf = lds + wave * kRaimWaveDoubles;
    double *ent = buf + kFixWaveDoubles;
    const int K = a.fix.K;
    const bool mine = lane < K;
    const size_t o = (size_t)e * (size_t)K + (size_t)(mine ? lane : 0);

    FixLane l;
    l.s = FixSat{0.0, 0.0, 0.0, 0.0, 0.0, false};
    if (mine) l.s = fix_sat(a.fix.eph[lane], a.fix.tx_ms[o], a.fix.tx_frac[o], a.fix.rx_ms[e], a.fix.rx_frac[e]);
    l.w = mine && a.fix.w ? a.fix.w[o] : 1.0;
    l.used = l.s.ok && fix_weight_ok(l.w);
    l.tau = kFixFirstTravel;
    l.row = FixRow{0.0, 0.0, 0.0, 0.0, 0.0};
    l.sel = 0.0;
    l.st[0] = a.fix.init_xyz[0], l.st[1] = a.fix.init_xyz[1], l.st[2] = a.fix.init_xyz[2], l.st[3] = 0.0;
    l.status = 0, l.iterations = 0, l.last_step = 0.0;
    const int num_valid = __popcll(__ballot(l.s.ok));
    l.num_used = __popcll(__ballot(l.used));

    const bool converged = fix_wave_pass(l, buf, lane, K, a.fix.max_iter, a.fix.tol_m);
    if (!fix_failed(l.status)) {
        const double radius = fix_wave_elevations(l);
        if (converged && a.fix.mask_sin > -1.0 && radius >= kFixMaskRadius) {
            const bool keep = l.used && l.sel >= a.fix.mask_sin;
            const int kept = __popcll(__ballot(keep));
            if (kept != l.num_used) {
                if (kept >= 4) {
                    l.used = keep;
                    l.num_used = kept;
                    l.status |= GAT_FIX_MASKED;
                    fix_wave_pass(l, buf, lane, K, a.fix.max_iter, a.fix.tol_m);
                    if (!fix_failed(l.status)) fix_wave_elevations(l);
                } else
                    l.status |= GAT_FIX_MASK_STARVED;
            }
        }
    }
    // the full set's outputs: they stand unless a channel is left out
    double sums[kFixTerms] = {};
    if (!fix_failed(l.status)) raim_wave_record_sums(l, buf, lane, K, sums);
    raim_wave_write(a, e, o, lane, mine, l, 0, num_valid, sums);

    gat_fix_integrity g;
    double tj = -1.0; // the lane's T_j of the first round
    const int d0 = l.num_used - 4;
    if (fix_failed(l.status) || (l.status & GAT_FIX_NOT_CONVERGED))
        g = raim_full_set(GAT_RAIM_NOT_CHECKED, 0, 0.0, 0.0);
    else if (d0 == 0)
        g = raim_full_set(GAT_RAIM_NO_REDUNDANCY, 0, sums[11], 0.0);
    else if (!raim_detected(sums[11], a.threshold[d0]))
        g = raim_full_set(0, d0, sums[11], a.threshold[d0]); // nearly every epoch ends here
    else {
        g = raim_full_set(GAT_RAIM_DETECTED | GAT_RAIM_UNRESOLVED, d0, sums[11], a.threshold[d0]);
        const gat_fix_integrity full = g;
        int ex0 = -1, ex1 = -1, ex2 = -1, ex3 = -1;
        for (int r = 0; r < a.max_exclude; ++r) {
            if (l.num_used < 6) break;
            // the hand-over: every channel frozen where its last row put it
            if (mine) raim_entry(l.s, l.tau, l.w, l.used, ent + kRaimEntry * lane);
            fix_wave_sync();
            RaimTrial t;
            t.st[0] = t.st[1] = t.st[2] = t.st[3] = 0.0, t.T = 0.0, t.counts = false;
            if (l.used) t = raim_trial(ent, K, lane, l.st, a.trial_iter, a.fix.tol_m);
            fix_wave_sync(); // the next round's entries wait for every lane's reads
            if (r == 0) tj = t.counts ? t.T : -1.0;
            // the counting candidate with the smallest (T_j, j)
            double bt = t.counts ? t.T : 0.0;
            int bj = t.counts ? lane : kFixWave;
            for (int m = 1; m < kFixWave; m <<= 1) {
                const double ot = __shfl_xor(bt, m, kFixWave);
                const int oj = __shfl_xor(bj, m, kFixWave);
                const bool take = oj < kFixWave && (bj >= kFixWave || raim_before(ot, oj, bt, bj));
                bt = take ? ot : bt;
                bj = take ? oj : bj;
            }
            if (bj >= kFixWave) break; // no trial counts
            for (int i = 0; i < 4; ++i) l.st[i] = __shfl(t.st[i], bj, kFixWave);
            l.used = l.used && lane != bj;
            l.num_used -= 1;
            fix_lane_row(l); // the travel times of the state the fault had moved give way to this state's before the pass
            if (!fix_wave_pass(l, buf, lane, K, a.fix.max_iter, a.fix.tol_m)) break;
            fix_wave_elevations(l);
            raim_wave_record_sums(l, buf, lane, K, sums);
            ex0 = r == 0 ? bj : ex0, ex1 = r == 1 ? bj : ex1, ex2 = r == 2 ? bj : ex2, ex3 = r == 3 ? bj : ex3;
            const double thr = a.threshold[l.num_used - 4];
            if (!raim_detected(sums[11], thr)) {
                g = raim_excluded(full, r + 1, ex0, ex1, ex2, ex3, sums[11], thr);
                raim_wave_write(a, e, o, lane, mine, l, GAT_FIX_EXCLUDED, num_valid, sums);
                break;
            }
        }
    }
    if (lane == 0) a.integrity[e] = g;
    if (mine && a.trial) a.trial[o] = tj;
}

} // namespace

hipError_t launch_raim(const RaimArgs &a, long long grid, hipStream_t st)
{
    if (grid < 1 || grid > 0x7fffffffll) return hipErrorInvalidValue;
    hipLaunchKernelGGL(raim_kernel, dim3((unsigned)grid), dim3(kFixThreads), 0, st, a);
    return hipGetLastError();
}

} // namespace gat
