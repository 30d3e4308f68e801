// gat_snap.hip -- the snapshot fix's kernel (include/gat.h gat_snapshot_fix) for gfx950.  The arithmetic is gat_snap.h on top of
// gat_fix.h and gat_vel.h (the host twin runs the same text), the geometry gat_snap_plan.h.
//
// One wave runs an epoch and lane k holds channel k.  Unlike the position fix the satellite depends on an unknown, the coarse-time
// error, so every iteration evaluates the lane's clock, orbit and their rates again (two Kepler solutions) before its row.  The
// reference channel of the resolution is found by every lane over four rows of the wave's own LDS (used, sin el, predicted range,
// fraction); the 20 sums of the normal equations go through the same LDS: lane k writes its terms (zeros where the channel is not
// used), lane q < 20 adds row q in channel order, and every lane reads the sums back and solves the 5 x 5 system itself, so the
// state, the step and every branch on them are the same in all 64 lanes and the wave leaves each loop together.  The waves of a
// workgroup share nothing and meet at no barrier.  No atomics.
//
// The wave's functions are inlined by force: called from several places they are otherwise kept as functions, the lane's state then
// lives in 444 bytes of scratch memory behind a pointer and the kernel takes 248 VGPRs; inlined it takes 181 and no scratch.
#include "gat_fix_wave.h"
#include "gat_snap_kernels.h"

namespace gat {

namespace {

// sums[q] = t[q] of lane 0 + .. + t[q] of lane K - 1, from +0, q < n <= kSnapTerms, in every lane
__device__ __forceinline__ void snap_wave_sums(double *buf, int lane, int K, const double *t, int n, double *sums)
{
    if (lane < K)
        for (int q = 0; q < n; ++q) buf[q * kSnapPitch + lane] = t[q];
    fix_wave_sync();
    if (lane < n) {
        double s = 0.0;
        for (int k = 0; k < K; ++k) s += buf[lane * kSnapPitch + k];
        buf[kSnapSumsAt + lane] = s;
    }
    fix_wave_sync();
    for (int q = 0; q < n; ++q) sums[q] = buf[kSnapSumsAt + q];
    fix_wave_sync();
}

// a lane's channel and the wave's epoch
struct SnapLane {
    SnapChan c;
    const gat_ephemeris *g; // the lane's record in global memory: read where it is used, not held in 50 registers
    int32_t rx_ms;
    double R;
    double st[kSnapUnknowns], last_step;
    int status, iterations, num_valid, num_used;
};

// steps 2 and 3 at the state; true: a used channel's whole milliseconds changed (the same in every lane)
__device__ __forceinline__ bool snap_wave_resolve(SnapLane &l, double *buf, int lane, int K, bool first, double margin)
{
    const double radius = fix_radius(l.st);
    if (l.c.ok) snap_predict(l.c, *l.g, l.R, l.st, radius);
    if (first) {
        l.c.ok = l.c.ok && snap_predicted(l.c);
        l.c.used = l.c.ok && fix_weight_ok(l.c.w);
        l.num_valid = __popcll(__ballot(l.c.ok));
        l.num_used = __popcll(__ballot(l.c.used));
    }
    if (l.num_used < kSnapMinSats) {
        l.status |= GAT_SNAP_FEW_SATS;
        return false;
    }
    if (lane < K) {
        buf[lane] = l.c.used ? 1.0 : 0.0;
        buf[kSnapPitch + lane] = l.c.sel;
        buf[2 * kSnapPitch + lane] = l.c.p;
        buf[3 * kSnapPitch + lane] = l.c.z;
    }
    fix_wave_sync();
    const SnapRef r = snap_reference(buf, kSnapPitch, K);
    fix_wave_sync();
    double n = 0.0;
    bool good = r.good;
    if (good && l.c.ok) good = snap_integer(l.c, r, &n);
    if (__ballot(!good)) {
        l.status |= GAT_SNAP_NONFINITE;
        return false;
    }
    if (__ballot(l.c.used && snap_ambiguous(l.c.q, n, margin))) l.status |= GAT_SNAP_AMBIGUOUS;
    const bool changed = __ballot(l.c.used && (int)n != l.c.n) != 0;
    if (l.c.ok) l.c.n = (int)n;
    return changed;
}

__device__ __forceinline__ void snap_lane_row(SnapLane &l)
{
    if (l.c.ok) snap_eval(l.c, *l.g, l.rx_ms, l.st);
}

// one pass over the used set; true: converged (the same in every lane)
__device__ __forceinline__ bool snap_wave_pass(SnapLane &l, double *buf, int lane, int K, int max_iter, double tol_m)
{
    for (int it = 0; it < max_iter; ++it) {
        snap_lane_row(l);
        double t[kSnapTerms], sums[kSnapTerms], d[kSnapUnknowns];
        snap_terms(l.c, l.c.w, t);
        for (int q = 0; q < kSnapTerms; ++q) t[q] = l.c.used ? t[q] : 0.0;
        snap_wave_sums(buf, lane, K, t, kSnapTerms, sums);
        const int rc = snap_step(sums, d);
        if (rc) {
            l.status |= rc;
            return false;
        }
        for (int i = 0; i < kSnapUnknowns; ++i) l.st[i] += d[i];
        l.last_step = __builtin_sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
        l.iterations += 1;
        if (l.last_step < tol_m) return true;
    }
    l.status |= GAT_SNAP_NOT_CONVERGED;
    return false;
}

__device__ __forceinline__ double snap_wave_elevations(SnapLane &l)
{
    snap_lane_row(l);
    const double radius = fix_radius(l.st);
    l.c.sel = l.c.ok ? fix_sin_el(l.c.row, l.st, radius) : 0.0;
    return radius;
}

__global__ __launch_bounds__(kFixThreads) void snap_kernel(SnapArgs a)
{
    __shared__ double lds[kFixWaves * kSnapWaveDoubles];
    const int wave = threadIdx.x / kFixWave, lane = threadIdx.x % kFixWave;
    int e;
    if (!fix_epoch_unit(blockIdx.x, wave, a.E, &e)) return; // the whole wave: no barrier follows
    double *buf = lds + wave * kSnapWaveDoubles;
    const int K = a.K;
    const bool mine = lane < K;
    const size_t o = (size_t)e * (size_t)K + (size_t)(mine ? lane : 0);

    SnapLane l;
    l.g = a.eph + (mine ? lane : 0);
    l.rx_ms = a.rx_ms[e];
    const double rx_frac = a.rx_frac[e];
    l.R = fix_seconds(l.rx_ms, rx_frac);
    l.c = snap_measure(*l.g, a.code_frac[o], l.rx_ms, rx_frac, a.w ? a.w[o] : 1.0);
    l.c.ok = l.c.ok && mine;
    const double *xyz = a.prior ? a.prior + 3 * (size_t)e : a.init_xyz;
    l.st[0] = xyz[0], l.st[1] = xyz[1], l.st[2] = xyz[2], l.st[3] = 0.0, l.st[4] = 0.0;
    l.status = 0, l.iterations = 0, l.num_valid = 0, l.num_used = 0, l.last_step = 0.0;

    // the resolution, the first pass, the resolution again, the mask: SnapHostEpoch::solve
    [&] {
        snap_wave_resolve(l, buf, lane, K, true, a.margin);
        if (snap_failed(l.status)) return;
        bool converged = snap_wave_pass(l, buf, lane, K, a.max_iter, a.tol_m);
        if (snap_failed(l.status)) return;
        if (converged) {
            const bool changed = snap_wave_resolve(l, buf, lane, K, false, a.margin);
            if (snap_failed(l.status)) return;
            if (changed) {
                l.status |= GAT_SNAP_RERESOLVED;
                converged = snap_wave_pass(l, buf, lane, K, a.max_iter, a.tol_m);
                if (snap_failed(l.status)) return;
            }
        }
        const double radius = snap_wave_elevations(l);
        if (converged && a.mask_sin > -1.0 && radius >= kFixMaskRadius) {
            const bool keep = l.c.used && l.c.sel >= a.mask_sin;
            const int kept = __popcll(__ballot(keep));
            if (kept != l.num_used) {
                if (kept >= kSnapMinSats) {
                    l.c.used = keep;
                    l.num_used = kept;
                    l.status |= GAT_SNAP_MASKED;
                    snap_wave_pass(l, buf, lane, K, a.max_iter, a.tol_m);
                    if (!snap_failed(l.status)) snap_wave_elevations(l);
                } else
                    l.status |= GAT_SNAP_MASK_STARVED;
            }
        }
    }();

    const bool failed = snap_failed(l.status);
    double sums[kSnapTerms] = {};
    if (!failed) {
        double t[kSnapTerms];
        snap_terms(l.c, 1.0, t);
        t[15] = l.c.row.v * l.c.row.v;
        for (int q = 0; q < 16; ++q) t[q] = l.c.used ? t[q] : 0.0;
        snap_wave_sums(buf, lane, K, t, 16, sums);
    }
    const int64_t m = snap_shift_ms(l.st[4]);
    if (lane == 0) {
        a.fixes[e] = snap_record(l.status, l.num_valid, l.num_used, l.iterations, l.st, sums[15], l.last_step, sums);
        if (a.rx_ms_out) a.rx_ms_out[e] = failed ? -1 : snap_week_ms((int64_t)l.rx_ms - m);
    }
    if (!mine) return;
    const bool has = !failed && l.c.ok;
    if (a.tx_ms) a.tx_ms[o] = has ? snap_tx_ms(l.rx_ms, l.c, m) : -1;
    if (a.n_ms) a.n_ms[o] = has ? l.c.n : 0;
    if (a.resid) a.resid[o] = has ? l.c.row.v : 0.0;
    if (a.sin_el) a.sin_el[o] = has ? l.c.sel : 0.0;
    if (a.used) a.used[o] = (uint8_t)(!failed && l.c.used ? 1 : 0);
}

} // namespace

hipError_t launch_snap(const SnapArgs &a, long long grid, hipStream_t st)
{
    if (grid < 1 || grid > 0x7fffffffll) return hipErrorInvalidValue;
    hipLaunchKernelGGL(snap_kernel, dim3((unsigned)grid), dim3(kFixThreads), 0, st, a);
    return hipGetLastError();
}

} // namespace gat
