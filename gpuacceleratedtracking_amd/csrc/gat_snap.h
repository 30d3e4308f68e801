// gat_snap.h -- the snapshot fix's rule (include/gat.h, "snapshot fix") on top of the position fix's (gat_fix.h) and the velocity
// fix's (gat_vel.h): a channel's sub-millisecond range, its satellite at a time that depends on the coarse-time unknown, the
// predicted range the whole milliseconds are resolved against, the reference channel, the row of five unknowns, the 5 x 5 Cholesky
// solve, the dilutions and the record, written once for the device kernel (gat_snap.hip) and for the host twin (gat_snap_plan.h).
// As gat_fix.h: FP64, no contraction, every expression evaluated as written, no libm transcendental, so both builds give the same
// bits.
#pragma once

#include "gat_fix.h"
#include "gat_vel.h"

namespace gat {

constexpr double kSnapMs = 1e-3;                 // s: the code period
constexpr double kSnapLambda = kFixC * 1e-3;     // m: the code period as a range
constexpr int kSnapUnknowns = 5;                 // x, y, z, b, t_c
constexpr int kSnapTerms = 20;                   // the distinct sums of the weighted normal equations: 15 of N, 5 of the right side
constexpr int kSnapMinSats = 5;
constexpr double kSnapMaxMs = 1.0e6;             // a range of more whole milliseconds than this is no range: GAT_SNAP_NONFINITE
constexpr int64_t kSnapWeekMs = 604800000;

// the three failures are the fix's bits, the mask's two as well
static_assert(GAT_SNAP_FEW_SATS == GAT_FIX_FEW_SATS && GAT_SNAP_SINGULAR == GAT_FIX_SINGULAR && GAT_SNAP_NONFINITE == GAT_FIX_NONFINITE &&
                  GAT_SNAP_NOT_CONVERGED == GAT_FIX_NOT_CONVERGED && GAT_SNAP_MASK_STARVED == GAT_FIX_MASK_STARVED && GAT_SNAP_MASKED == GAT_FIX_MASKED,
              "status bits");

// ---- a channel -----------------------------------------------------------------------------------------------------------------------
// frac: the caller's fraction; z = c phi, beta the borrow; n the whole milliseconds; ok: usable; used: in the equations; s, v?, ddts:
// the satellite at the last time it was evaluated (s.ok: finite); row, g: its row and the t_c column at the last state; p, q, sel:
// the predicted range, the unrounded whole milliseconds and sin el of the last resolution.
struct SnapChan {
    double frac, z, w;
    int beta, n;
    bool ok, used;
    FixSat s;
    double vx, vy, vz, ddts;
    FixRow row;
    double g, tau, sel, p, q;
};

GAT_HD inline bool snap_frac_given(double f) { return fix_finite(f) && f >= 0.0 && f < kSnapMs; }

// step 1: the fraction of the range.  ok: a given fraction of a usable ephemeris at a given reception
GAT_HD inline SnapChan snap_measure(const gat_ephemeris &g, double code_frac, int32_t rx_ms, double rx_frac, double w)
{
    SnapChan c{};
    c.s = FixSat{0.0, 0.0, 0.0, 0.0, 0.0, false};
    c.row = FixRow{0.0, 0.0, 0.0, 0.0, 0.0};
    c.w = w;
    c.tau = kFixFirstTravel;
    c.ok = fix_eph_usable(g) && snap_frac_given(code_frac) && fix_time_given(rx_ms, rx_frac);
    if (!c.ok) return c;
    c.frac = code_frac;
    double phi = rx_frac - code_frac;
    if (phi < 0.0) {
        phi += kSnapMs;
        c.beta = 1;
    }
    c.z = kFixC * phi;
    return c;
}

// the satellite at its own time t_sv: the clock and the orbit as vel_sat evaluates them
GAT_HD inline void snap_sat(SnapChan &c, const gat_ephemeris &g, double t_sv)
{
    double dts, ddts, X, Y, Z, Vx, Vy, Vz;
    vel_clock(g, t_sv, &dts, &ddts);
    vel_orbit(g, t_sv - dts, &X, &Y, &Z, &Vx, &Vy, &Vz);
    c.s.X = X, c.s.Y = Y, c.s.Z = Z, c.s.dts = dts;
    c.vx = Vx, c.vy = Vy, c.vz = Vz, c.ddts = ddts;
    c.s.ok = fix_finite(X) && fix_finite(Y) && fix_finite(Z) && fix_finite(Vx) && fix_finite(Vy) && fix_finite(Vz) && fix_finite(dts) && fix_finite(ddts);
}
// its row at the state st = (x, y, z, b, t_c) with the travel time of its last range, and the t_c column -(los . v_sat - c ddts),
// the velocity turned with the position
GAT_HD inline void snap_row(SnapChan &c, const double *st)
{
    c.row = fix_row(c.s, c.tau, st);
    double cs, sn;
    fix_sincos(kFixOmegaE * c.tau, &cs, &sn);
    const double vrx = cs * c.vx + sn * c.vy;
    const double vry = cs * c.vy - sn * c.vx;
    c.g = -(c.row.lx * vrx + c.row.ly * vry + c.row.lz * c.vz - kFixC * c.ddts);
    c.tau = c.row.r / kFixC;
}

// step 2: the predicted range at the state: the transmit time R - t_c - tau with tau = 0.075 s, then r / c, kVelRows evaluations
GAT_HD inline void snap_predict(SnapChan &c, const gat_ephemeris &g, double R, const double *st, double radius)
{
    c.tau = kFixFirstTravel;
    c.s.rho = 0.0;
    for (int i = 0; i < kVelRows; ++i) {
        snap_sat(c, g, R - st[4] - c.tau);
        snap_row(c, st);
    }
    c.p = c.row.r + st[3] - kFixC * c.s.dts;
    c.sel = fix_sin_el(c.row, st, radius);
}
GAT_HD inline bool snap_predicted(const SnapChan &c) { return c.s.ok && fix_finite(c.p) && fix_finite(c.sel); }

// step 3: the reference channel from the wave's four rows (used as 0 / 1, sin el, p, z; `pitch` doubles apart): the used channel
// with the largest sin el, the lowest on a tie -- within kFixMaskRadius of the centre every sin el is 0: the lowest used channel
struct SnapRef {
    int k0;
    double p0, z0, n0;
    bool good;
};
GAT_HD inline SnapRef snap_reference(const double *rows, int pitch, int K)
{
    SnapRef r{-1, 0.0, 0.0, 0.0, false};
    double best = 0.0;
    for (int k = 0; k < K; ++k)
        if (rows[k] != 0.0 && (r.k0 < 0 || rows[pitch + k] > best)) r.k0 = k, best = rows[pitch + k];
    if (r.k0 < 0) return r;
    r.p0 = rows[2 * pitch + r.k0], r.z0 = rows[3 * pitch + r.k0];
    const double q0 = (r.p0 - r.z0) / kSnapLambda;
    if (!(q0 >= -kSnapMaxMs && q0 <= kSnapMaxMs)) return r;
    r.n0 = __builtin_rint(q0);
    r.good = true;
    return r;
}
// a channel's whole milliseconds against the reference; false: no range
GAT_HD inline bool snap_integer(SnapChan &c, const SnapRef &r, double *n)
{
    c.q = (c.p - r.p0 + r.n0 * kSnapLambda + r.z0 - c.z) / kSnapLambda;
    if (!(c.q >= -kSnapMaxMs && c.q <= kSnapMaxMs)) return false;
    *n = __builtin_rint(c.q);
    return true;
}
GAT_HD inline bool snap_ambiguous(double q, double n, double margin)
{
    const double d = q - n;
    return (d < 0.0 ? -d : d) > 0.5 - margin;
}

// step 4: the satellite's own time at the coarse-time unknown, and the channel at the state
GAT_HD inline double snap_time(int32_t rx_ms, const SnapChan &c, double tc)
{
    return (double)((int64_t)rx_ms - (int64_t)c.n - (int64_t)c.beta) * kSnapMs + c.frac - tc;
}
GAT_HD inline void snap_eval(SnapChan &c, const gat_ephemeris &g, int32_t rx_ms, const double *st)
{
    snap_sat(c, g, snap_time(rx_ms, c, st[4]));
    c.s.rho = (double)c.n * kSnapLambda + c.z;
    snap_row(c, st);
}
// the channel's 20 terms, row a = (-los, 1, g): N[i][j] for i <= j row by row, then a_i v
GAT_HD inline void snap_terms(const SnapChan &c, double w, double *t)
{
    const double a[kSnapUnknowns] = {-c.row.lx, -c.row.ly, -c.row.lz, 1.0, c.g};
    int n = 0;
    for (int i = 0; i < kSnapUnknowns; ++i)
        for (int j = i; j < kSnapUnknowns; ++j) t[n++] = w * a[i] * a[j];
    for (int i = 0; i < kSnapUnknowns; ++i) t[n++] = w * a[i] * c.row.v;
}

// ---- the 5 x 5 solve: fix_chol's rule on 15 sums ------------------------------------------------------------------------------------------
GAT_HD inline bool snap_chol(const double *s, double L[kSnapUnknowns][kSnapUnknowns])
{
    double N[kSnapUnknowns][kSnapUnknowns];
    int n = 0;
    for (int i = 0; i < kSnapUnknowns; ++i)
        for (int j = i; j < kSnapUnknowns; ++j) N[i][j] = s[n], N[j][i] = s[n], ++n;
    for (int j = 0; j < kSnapUnknowns; ++j) {
        double d = N[j][j];
        for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k];
        if (!(d > N[j][j] * kFixPivot && d <= 1.79769313486231570815e308)) return false;
        L[j][j] = __builtin_sqrt(d);
        for (int i = j + 1; i < kSnapUnknowns; ++i) {
            double v = N[i][j];
            for (int k = 0; k < j; ++k) v -= L[i][k] * L[j][k];
            L[i][j] = v / L[j][j];
        }
    }
    return true;
}
GAT_HD inline void snap_chol_solve(const double L[kSnapUnknowns][kSnapUnknowns], const double *b, double *x)
{
    double y[kSnapUnknowns];
    for (int i = 0; i < kSnapUnknowns; ++i) {
        double v = b[i];
        for (int k = 0; k < i; ++k) v -= L[i][k] * y[k];
        y[i] = v / L[i][i];
    }
    for (int i = kSnapUnknowns - 1; i >= 0; --i) {
        double v = y[i];
        for (int k = i + 1; k < kSnapUnknowns; ++k) v -= L[k][i] * x[k];
        x[i] = v / L[i][i];
    }
}
// The step of one iteration from the 20 sums.  0: d is the step; else the status bit of the failure, as fix_step.
GAT_HD inline int snap_step(const double *s, double *d)
{
    double L[kSnapUnknowns][kSnapUnknowns];
    for (int q = 0; q < kSnapTerms; ++q)
        if (!fix_finite(s[q])) return GAT_SNAP_NONFINITE;
    if (!snap_chol(s, L)) return GAT_SNAP_SINGULAR;
    snap_chol_solve(L, s + 15, d);
    for (int i = 0; i < kSnapUnknowns; ++i)
        if (!fix_finite(d[i])) return GAT_SNAP_NONFINITE;
    return 0;
}
// gdop (x, y, z, b), pdop and tdop (t_c, s / m) from the 15 unweighted sums; 0 where the Cholesky fails
GAT_HD inline void snap_dop(const double *s, double *gdop, double *pdop, double *tdop)
{
    double L[kSnapUnknowns][kSnapUnknowns], q[kSnapUnknowns];
    *gdop = 0.0, *pdop = 0.0, *tdop = 0.0;
    if (!snap_chol(s, L)) return;
    for (int i = 0; i < kSnapUnknowns; ++i) {
        double e[kSnapUnknowns], x[kSnapUnknowns];
        for (int j = 0; j < kSnapUnknowns; ++j) e[j] = i == j ? 1.0 : 0.0;
        snap_chol_solve(L, e, x);
        q[i] = x[i];
    }
    const double p = q[0] + q[1] + q[2];
    *pdop = __builtin_sqrt(p);
    *gdop = __builtin_sqrt(p + q[3]);
    *tdop = __builtin_sqrt(q[4]);
}

// ---- an epoch's record and the times it hands on ---------------------------------------------------------------------------------------
GAT_HD inline bool snap_failed(int status) { return (status & (GAT_SNAP_FEW_SATS | GAT_SNAP_SINGULAR | GAT_SNAP_NONFINITE)) != 0; }
GAT_HD inline gat_snap_fix snap_record(int status, int num_valid, int num_used, int iterations, const double *st, double sum_v2, double last_step,
                                       const double *ata)
{
    gat_snap_fix f{};
    f.status = status, f.num_valid = num_valid, f.num_used = num_used, f.iterations = iterations;
    if (snap_failed(status)) return f;
    f.x = st[0], f.y = st[1], f.z = st[2];
    f.clock_bias_s = st[3] / kFixC;
    f.coarse_time_s = st[4];
    f.rms_residual_m = __builtin_sqrt(sum_v2 / (double)num_used);
    f.last_step_m = last_step;
    snap_dop(ata, &f.gdop, &f.pdop, &f.tdop);
    return f;
}
// m = rint(1000 t_c), 0 where that is no number of milliseconds
GAT_HD inline int64_t snap_shift_ms(double tc)
{
    const double m = __builtin_rint(tc * 1000.0);
    return m >= -1.0e12 && m <= 1.0e12 ? (int64_t)m : 0;
}
GAT_HD inline int32_t snap_week_ms(int64_t v)
{
    const int64_t r = v % kSnapWeekMs;
    return (int32_t)(r < 0 ? r + kSnapWeekMs : r);
}
GAT_HD inline int32_t snap_tx_ms(int32_t rx_ms, const SnapChan &c, int64_t m) { return snap_week_ms((int64_t)rx_ms - c.n - c.beta - m); }

} // namespace gat
