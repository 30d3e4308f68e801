// gat_fix.h -- the position fix's rule (include/gat.h, "position fix"): the sine and cosine, the satellite's clock and orbit from an
// LNAV ephemeris, the observable, a satellite's row at a receiver state, the 4 x 4 Cholesky solve and the dilution of precision,
// written once for the device kernel (gat_fix.hip) and for the host twin (gat_fix_plan.h), as gat_nav.h is for the decoder.  FP64
// throughout, compiled without contraction in both builds, every expression evaluated as written and no libm transcendental: only
// + - * /, sqrt, floor / rint and explicit __builtin_fma, so both builds give the same bits.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "gat.h"
#include "gat_hd.h"

namespace gat {

constexpr double kFixMu = 3.986005e14;           // m^3 / s^2
constexpr double kFixOmegaE = 7.2921151467e-5;   // rad / s
constexpr double kFixC = 299792458.0;            // m / s
constexpr double kFixF = -4.442807633e-10;       // s / m^(1/2)
constexpr double kFixHalfWeek = 302400.0;        // s
constexpr int32_t kFixHalfWeekMs = 302400000;
constexpr double kFixFirstTravel = 0.075;        // s: the travel time before a range is known
constexpr double kFixMaskRadius = 1.0e6;         // m: the mask needs a receiver this far from the Earth's centre
constexpr int kFixKepler = 8;                    // Newton steps, no data-dependent exit
constexpr double kFixPivot = 0x1p-40;            // a pivot this small beside its diagonal element is rounding noise: singular
constexpr int kFixTerms = 14;                    // the distinct sums of the weighted normal equations: 10 of N, 4 of the right side

GAT_HD inline bool fix_finite(double x)
{
    uint64_t u;
    __builtin_memcpy(&u, &x, sizeof u);
    return ((u >> 52) & 0x7ff) != 0x7ff;
}

// ---- sine and cosine ------------------------------------------------------------------------------------------------------------------
// Cody-Waite by pi/2 in three parts (33 + 33 + 53 bits: q P1 and q P2 are exact for |q| < 2^20), then the Taylor polynomials of
// degree 17 and 18 on [-pi/4, pi/4] in Horner form with explicit fused multiply-adds.  |error| <= 1e-15 on |x| <= 72.
// Beyond the reduction's range (|x| well above 2^20) the results are no sine and cosine -- of any magnitude, or not finite --, but
// every operation is defined for every x, NaN and the infinities included, so both builds still give the same bits.
GAT_HD inline void fix_sincos(double x, double *c, double *s)
{
    const double q = __builtin_rint(x * 0.6366197723675814);
    double r = __builtin_fma(q, -1.5707963267341256, x);
    r = __builtin_fma(q, -6.077100506303966e-11, r);
    r = __builtin_fma(q, -2.0222662487959506e-21, r);
    const double r2 = r * r;
    double sp = __builtin_fma(r2, 2.8114572543455206e-15, -7.647163731819816e-13);
    sp = __builtin_fma(r2, sp, 1.6059043836821613e-10);
    sp = __builtin_fma(r2, sp, -2.505210838544172e-08);
    sp = __builtin_fma(r2, sp, 2.7557319223985893e-06);
    sp = __builtin_fma(r2, sp, -1.984126984126984e-04);
    sp = __builtin_fma(r2, sp, 8.333333333333333e-03);
    sp = __builtin_fma(r2, sp, -1.6666666666666666e-01);
    sp = __builtin_fma(r2 * r, sp, r);
    double cp = __builtin_fma(r2, -1.5619206968586225e-16, 4.779477332387385e-14);
    cp = __builtin_fma(r2, cp, -1.1470745597729725e-11);
    cp = __builtin_fma(r2, cp, 2.08767569878681e-09);
    cp = __builtin_fma(r2, cp, -2.755731922398589e-07);
    cp = __builtin_fma(r2, cp, 2.48015873015873e-05);
    cp = __builtin_fma(r2, cp, -1.3888888888888889e-03);
    cp = __builtin_fma(r2, cp, 4.1666666666666664e-02);
    cp = __builtin_fma(r2, cp, -0.5);
    cp = __builtin_fma(r2, cp, 1.0);
    // q mod 4 in doubles: q / 4, its floor, the product and the difference are exact for every finite q, so the conversion sees 0 .. 3
    // whatever |q| is (a conversion of q itself is undefined from 2^63 on and differs between the builds); not finite: quadrant 0
    const double qm = q - 4.0 * __builtin_floor(q * 0.25);
    const int qi = qm < 4.0 ? (int)qm : 0;
    const double cs = (qi & 1) ? sp : cp;
    const double sn = (qi & 1) ? cp : sp;
    *c = (qi == 1 || qi == 2) ? -cs : cs;
    *s = (qi >= 2) ? -sn : sn;
}

// ---- time ------------------------------------------------------------------------------------------------------------------------------
GAT_HD inline double fix_wrap(double d) { return d >= kFixHalfWeek ? d - 2.0 * kFixHalfWeek : (d < -kFixHalfWeek ? d + 2.0 * kFixHalfWeek : d); }
GAT_HD inline int32_t fix_wrap_ms(int64_t d)
{
    return (int32_t)(d >= kFixHalfWeekMs ? d - 2 * (int64_t)kFixHalfWeekMs : (d < -(int64_t)kFixHalfWeekMs ? d + 2 * (int64_t)kFixHalfWeekMs : d));
}
// a time of the week as the rule holds it: whole milliseconds and a fraction in seconds
GAT_HD inline bool fix_time_given(int32_t ms, double frac) { return ms >= 0 && fix_finite(frac); }
GAT_HD inline double fix_seconds(int32_t ms, double frac) { return (double)ms * 1e-3 + frac; }
GAT_HD inline double fix_pseudorange(int32_t rx_ms, double rx_frac, int32_t tx_ms, double tx_frac)
{
    return kFixC * (1e-3 * (double)fix_wrap_ms((int64_t)rx_ms - (int64_t)tx_ms) + (rx_frac - tx_frac));
}

// ---- the satellite ---------------------------------------------------------------------------------------------------------------------
GAT_HD inline bool fix_eph_usable(const gat_ephemeris &g) { return g.valid != 0 && g.e < 0.5 && g.e >= 0.0 && g.sqrt_a > 0.0; }

// E - e sin E = M by kFixKepler Newton steps from E = M; the sine and cosine of the last iterate's E
GAT_HD inline double fix_kepler(double M, double e, double *cE, double *sE)
{
    double E = M;
    for (int i = 0; i < kFixKepler; ++i) {
        double c, s;
        fix_sincos(E, &c, &s);
        E = E - (E - e * s - M) / (1.0 - e * c);
    }
    fix_sincos(E, cE, sE);
    return E;
}
GAT_HD inline double fix_mean_motion(const gat_ephemeris &g)
{
    const double A = g.sqrt_a * g.sqrt_a;
    return __builtin_sqrt(kFixMu / (A * A * A)) + g.delta_n;
}
// Delta t_sv at the satellite's own time t_sv
GAT_HD inline double fix_clock(const gat_ephemeris &g, double t_sv)
{
    const double dt = fix_wrap(t_sv - g.toc);
    const double tk = fix_wrap(t_sv - g.toe);
    double cE, sE;
    fix_kepler(g.m0 + fix_mean_motion(g) * tk, g.e, &cE, &sE);
    return g.af0 + g.af1 * dt + g.af2 * dt * dt + kFixF * g.e * g.sqrt_a * sE - g.tgd;
}
// the ECEF position at GPS time t, in the frame of that instant
GAT_HD inline void fix_orbit(const gat_ephemeris &g, double t, double *X, double *Y, double *Z)
{
    const double A = g.sqrt_a * g.sqrt_a;
    const double tk = fix_wrap(t - g.toe);
    double cE, sE;
    fix_kepler(g.m0 + fix_mean_motion(g) * tk, g.e, &cE, &sE);
    const double den = 1.0 - g.e * cE;
    const double cnu = (cE - g.e) / den;
    const double snu = __builtin_sqrt(1.0 - g.e * g.e) * sE / den;
    double cw, sw;
    fix_sincos(g.omega, &cw, &sw);
    const double sphi = snu * cw + cnu * sw;
    const double cphi = cnu * cw - snu * sw;
    const double s2 = 2.0 * sphi * cphi;
    const double c2 = cphi * cphi - sphi * sphi;
    const double du = g.cus * s2 + g.cuc * c2;
    const double dr = g.crs * s2 + g.crc * c2;
    const double di = g.cis * s2 + g.cic * c2;
    double cdu, sdu;
    fix_sincos(du, &cdu, &sdu);
    const double su = sphi * cdu + cphi * sdu;
    const double cu = cphi * cdu - sphi * sdu;
    const double r = A * den + dr;
    const double inc = g.i0 + di + g.idot * tk;
    const double Om = g.omega0 + (g.omega_dot - kFixOmegaE) * tk - kFixOmegaE * g.toe;
    double ci, si, cO, sO;
    fix_sincos(inc, &ci, &si);
    fix_sincos(Om, &cO, &sO);
    const double xp = r * cu, yp = r * su;
    *X = xp * cO - yp * ci * sO;
    *Y = xp * sO + yp * ci * cO;
    *Z = yp * si;
}

// One (epoch, channel): what does not depend on the receiver's position.  ok: a measurement of a usable ephemeris with a finite state.
struct FixSat {
    double X, Y, Z, dts, rho;
    bool ok;
};
GAT_HD inline FixSat fix_sat(const gat_ephemeris &g, int32_t tx_ms, double tx_frac, int32_t rx_ms, double rx_frac)
{
    FixSat s{0.0, 0.0, 0.0, 0.0, 0.0, false};
    if (!fix_eph_usable(g) || !fix_time_given(tx_ms, tx_frac) || !fix_time_given(rx_ms, rx_frac)) return s;
    const double t_sv = fix_seconds(tx_ms, tx_frac);
    const double dts = fix_clock(g, t_sv);
    double X, Y, Z;
    fix_orbit(g, t_sv - dts, &X, &Y, &Z);
    const double rho = fix_pseudorange(rx_ms, rx_frac, tx_ms, tx_frac);
    if (!(fix_finite(X) && fix_finite(Y) && fix_finite(Z) && fix_finite(dts) && fix_finite(rho))) return s;
    s.X = X, s.Y = Y, s.Z = Z, s.dts = dts, s.rho = rho, s.ok = true;
    return s;
}
GAT_HD inline bool fix_weight_ok(double w) { return fix_finite(w) && w > 0.0; }

// ---- a satellite's row at the receiver state (x, y, z, b) --------------------------------------------------------------------------------
// The satellite is turned about z by the Earth's rotation over the travel time tau; los points from the receiver to it.
struct FixRow {
    double lx, ly, lz, r, v;
};
GAT_HD inline FixRow fix_row(const FixSat &s, double tau, const double *st)
{
    double c, sn;
    fix_sincos(kFixOmegaE * tau, &c, &sn);
    const double xr = c * s.X + sn * s.Y;
    const double yr = c * s.Y - sn * s.X;
    const double dx = xr - st[0], dy = yr - st[1], dz = s.Z - st[2];
    FixRow o;
    o.r = __builtin_sqrt(dx * dx + dy * dy + dz * dz);
    o.lx = dx / o.r, o.ly = dy / o.r, o.lz = dz / o.r;
    o.v = s.rho - (o.r + st[3] - kFixC * s.dts);
    return o;
}
// the satellite's 14 terms of the weighted normal equations, row a = (-los, 1): N[i][j] for i <= j row by row, then a_i v
GAT_HD inline void fix_terms(const FixRow &o, double w, double *t)
{
    const double a[4] = {-o.lx, -o.ly, -o.lz, 1.0};
    int n = 0;
    for (int i = 0; i < 4; ++i)
        for (int j = i; j < 4; ++j) t[n++] = w * a[i] * a[j];
    for (int i = 0; i < 4; ++i) t[n++] = w * a[i] * o.v;
}
// sin of the elevation over a spherical Earth; 0 where the receiver is nearer the centre than kFixMaskRadius
GAT_HD inline double fix_sin_el(const FixRow &o, const double *st, double radius)
{
    if (!(radius >= kFixMaskRadius)) return 0.0;
    return (st[0] / radius) * o.lx + (st[1] / radius) * o.ly + (st[2] / radius) * o.lz;
}
GAT_HD inline double fix_radius(const double *st) { return __builtin_sqrt(st[0] * st[0] + st[1] * st[1] + st[2] * st[2]); }

// ---- the 4 x 4 solve ---------------------------------------------------------------------------------------------------------------------
// N = L L^T from the ten sums s[0 .. 10) (upper triangle row by row), column by column.  False: a pivot is not above kFixPivot times
// its diagonal element -- in exact arithmetic not positive: what is left of a singular system is rounding noise of either sign -- or
// not finite.
GAT_HD inline bool fix_chol(const double *s, double L[4][4])
{
    const double N[4][4] = {{s[0], s[1], s[2], s[3]}, {s[1], s[4], s[5], s[6]}, {s[2], s[5], s[7], s[8]}, {s[3], s[6], s[8], s[9]}};
    for (int j = 0; j < 4; ++j) {
        double d = N[j][j];
        for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k];
        if (!(d > N[j][j] * kFixPivot && d <= 1.79769313486231570815e308)) return false;
        L[j][j] = __builtin_sqrt(d);
        for (int i = j + 1; i < 4; ++i) {
            double v = N[i][j];
            for (int k = 0; k < j; ++k) v -= L[i][k] * L[j][k];
            L[i][j] = v / L[j][j];
        }
    }
    return true;
}
// L L^T x = b
GAT_HD inline void fix_chol_solve(const double L[4][4], const double *b, double *x)
{
    double y[4];
    for (int i = 0; i < 4; ++i) {
        double v = b[i];
        for (int k = 0; k < i; ++k) v -= L[i][k] * y[k];
        y[i] = v / L[i][i];
    }
    for (int i = 3; i >= 0; --i) {
        double v = y[i];
        for (int k = i + 1; k < 4; ++k) v -= L[k][i] * x[k];
        x[i] = v / L[i][i];
    }
}
// The step of one iteration from the 14 sums.  0: d is the step; else the status bit of the failure: a sum that is not finite (a
// receiver state at a satellite or out of the numbers' range) is GAT_FIX_NONFINITE, not a singular system.
GAT_HD inline int fix_step(const double *s, double *d)
{
    double L[4][4];
    for (int q = 0; q < kFixTerms; ++q)
        if (!fix_finite(s[q])) return GAT_FIX_NONFINITE;
    if (!fix_chol(s, L)) return GAT_FIX_SINGULAR;
    fix_chol_solve(L, s + 10, d);
    return fix_finite(d[0]) && fix_finite(d[1]) && fix_finite(d[2]) && fix_finite(d[3]) ? 0 : GAT_FIX_NONFINITE;
}
// gdop and pdop from the ten unweighted sums: the diagonal of (A^T A)^-1 through the same Cholesky; 0 where it fails
GAT_HD inline void fix_dop(const double *s, double *gdop, double *pdop)
{
    double L[4][4], q[4];
    *gdop = 0.0, *pdop = 0.0;
    if (!fix_chol(s, L)) return;
    for (int i = 0; i < 4; ++i) {
        const double e[4] = {i == 0 ? 1.0 : 0.0, i == 1 ? 1.0 : 0.0, i == 2 ? 1.0 : 0.0, i == 3 ? 1.0 : 0.0};
        double x[4];
        fix_chol_solve(L, e, x);
        q[i] = x[i];
    }
    const double p = q[0] + q[1] + q[2];
    *pdop = __builtin_sqrt(p);
    *gdop = __builtin_sqrt(p + q[3]);
}

// ---- an epoch's record -------------------------------------------------------------------------------------------------------------------
GAT_HD inline bool fix_failed(int status) { return (status & (GAT_FIX_FEW_SATS | GAT_FIX_SINGULAR | GAT_FIX_NONFINITE)) != 0; }
GAT_HD inline gat_fix fix_record(int status, int num_valid, int num_used, int iterations, const double *st, double sum_v2, double last_step,
                                 const double *ata)
{
    gat_fix f{};
    f.status = status, f.num_valid = num_valid, f.num_used = num_used, f.iterations = iterations;
    if (fix_failed(status)) return f;
    f.x = st[0], f.y = st[1], f.z = st[2];
    f.clock_bias_s = st[3] / kFixC;
    f.rms_residual_m = __builtin_sqrt(sum_v2 / (double)num_used);
    f.last_step_m = last_step;
    fix_dop(ata, &f.gdop, &f.pdop);
    return f;
}

} // namespace gat
