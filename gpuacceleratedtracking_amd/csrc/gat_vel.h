// gat_vel.h -- the velocity fix's rule (include/gat.h, "velocity fix") on top of the position fix's (gat_fix.h): the satellite's
// velocity and clock rate beside its position and clock, a channel's Doppler row at the fix's state, the residual, the geodetic
// frame of the fix and the record, written once for the device kernel (gat_vel.hip) and for the host twin (gat_vel_plan.h).  As
// gat_fix.h: FP64, no contraction, every expression evaluated as written, no libm transcendental, so both builds give the same bits.
#pragma once

#include "gat_fix.h"

namespace gat {

constexpr double kVelA = 6378137.0;          // m: WGS-84 semi-major axis
constexpr double kVelE2 = 6.69437999014e-3;  // WGS-84 first eccentricity squared
constexpr int kVelFrameSteps = 8;            // fixed-point steps of the latitude, no data-dependent exit
constexpr int kVelRows = 3;                  // evaluations of fix_row: tau = 0.075, then r / c twice

// the three failures are the fix's bits, so that fix_step's answer is the status
static_assert(GAT_VEL_SINGULAR == GAT_FIX_SINGULAR && GAT_VEL_NONFINITE == GAT_FIX_NONFINITE && GAT_VEL_FEW_SATS == GAT_FIX_FEW_SATS, "status bits");

// ---- the satellite ---------------------------------------------------------------------------------------------------------------------
// Delta t_sv and its rate at the satellite's own time t_sv: fix_clock's expressions, and from the same E the rate
GAT_HD inline void vel_clock(const gat_ephemeris &g, double t_sv, double *dts, double *ddts)
{
    const double dt = fix_wrap(t_sv - g.toc);
    const double tk = fix_wrap(t_sv - g.toe);
    const double n = fix_mean_motion(g);
    double cE, sE;
    fix_kepler(g.m0 + n * tk, g.e, &cE, &sE);
    *dts = g.af0 + g.af1 * dt + g.af2 * dt * dt + kFixF * g.e * g.sqrt_a * sE - g.tgd;
    const double Edot = n / (1.0 - g.e * cE);
    *ddts = g.af1 + 2.0 * g.af2 * dt + kFixF * g.e * g.sqrt_a * cE * Edot;
}
// the ECEF position and velocity at GPS time t, in the frame of that instant: X, Y, Z by fix_orbit's expressions in fix_orbit's order
GAT_HD inline void vel_orbit(const gat_ephemeris &g, double t, double *X, double *Y, double *Z, double *Vx, double *Vy, double *Vz)
{
    const double A = g.sqrt_a * g.sqrt_a;
    const double tk = fix_wrap(t - g.toe);
    const double n = fix_mean_motion(g);
    double cE, sE;
    fix_kepler(g.m0 + n * tk, g.e, &cE, &sE);
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
    // the rates
    const double Edot = n / den;
    const double nudot = Edot * __builtin_sqrt(1.0 - g.e * g.e) / den;
    const double udot = nudot + 2.0 * nudot * (g.cus * c2 - g.cuc * s2);
    const double rdot = A * g.e * sE * Edot + 2.0 * nudot * (g.crs * c2 - g.crc * s2);
    const double incdot = g.idot + 2.0 * nudot * (g.cis * c2 - g.cic * s2);
    const double Omdot = g.omega_dot - kFixOmegaE;
    const double xpd = rdot * cu - r * udot * su;
    const double ypd = rdot * su + r * udot * cu;
    *Vx = xpd * cO - ypd * ci * sO + yp * si * sO * incdot - (xp * sO + yp * ci * cO) * Omdot;
    *Vy = xpd * sO + ypd * ci * cO - yp * si * cO * incdot + (xp * cO - yp * ci * sO) * Omdot;
    *Vz = ypd * si + yp * ci * incdot;
}

// One (epoch, channel): what does not depend on the receiver.  s is the position fix's satellite (rho is not measured here: 0).
// s.ok: a Doppler of a usable ephemeris at a given transmit time with a finite state.
struct VelSat {
    FixSat s;
    double vx, vy, vz, ddts, doppler;
};
GAT_HD inline VelSat vel_sat(const gat_ephemeris &g, int32_t tx_ms, double tx_frac, double doppler_hz)
{
    VelSat o{FixSat{0.0, 0.0, 0.0, 0.0, 0.0, false}, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (!fix_eph_usable(g) || !fix_time_given(tx_ms, tx_frac) || !fix_finite(doppler_hz)) return o;
    const double t_sv = fix_seconds(tx_ms, tx_frac);
    double dts, ddts, X, Y, Z, Vx, Vy, Vz;
    vel_clock(g, t_sv, &dts, &ddts);
    vel_orbit(g, t_sv - dts, &X, &Y, &Z, &Vx, &Vy, &Vz);
    if (!(fix_finite(X) && fix_finite(Y) && fix_finite(Z) && fix_finite(Vx) && fix_finite(Vy) && fix_finite(Vz) && fix_finite(dts) && fix_finite(ddts)))
        return o;
    o.s.X = X, o.s.Y = Y, o.s.Z = Z, o.s.dts = dts, o.s.ok = true;
    o.vx = Vx, o.vy = Vy, o.vz = Vz, o.ddts = ddts, o.doppler = doppler_hz;
    return o;
}

// ---- a channel's row at the fix's state st = (x, y, z, c clock_bias_s) --------------------------------------------------------------------
// The light-time equation differentiated: the row a = (-k los, 1) and the right side y, in fix_terms' form (lx, ly, lz hold k los,
// v holds y; r is the range).  lambda = c / carrier_hz.
GAT_HD inline FixRow vel_row(const VelSat &c, const double *st, double lambda)
{
    double tau = kFixFirstTravel;
    FixRow o = fix_row(c.s, tau, st);
    for (int i = 1; i < kVelRows; ++i) {
        tau = o.r / kFixC;
        o = fix_row(c.s, tau, st);
    }
    // the satellite's position and velocity turned by the last evaluation's angle
    double cs, sn;
    fix_sincos(kFixOmegaE * tau, &cs, &sn);
    const double xr = cs * c.s.X + sn * c.s.Y;
    const double yr = cs * c.s.Y - sn * c.s.X;
    const double vrx = cs * c.vx + sn * c.vy;
    const double vry = cs * c.vy - sn * c.vx;
    const double q = o.lx * (vrx - kFixOmegaE * yr) + o.ly * (vry + kFixOmegaE * xr) + o.lz * c.vz;
    const double k = 1.0 / (1.0 + q / kFixC);
    const double lv = o.lx * vrx + o.ly * vry + o.lz * c.vz;
    FixRow a;
    a.lx = k * o.lx, a.ly = k * o.ly, a.lz = k * o.lz, a.r = o.r;
    a.v = -lambda * c.doppler - k * lv + kFixC * c.ddts;
    return a;
}
// v = y - a . s at the solution s = (vx, vy, vz, d)
GAT_HD inline double vel_resid(const FixRow &a, const double *s) { return a.v - (-a.lx * s[0] - a.ly * s[1] - a.lz * s[2] + s[3]); }

// ---- the local frame -----------------------------------------------------------------------------------------------------------------------
struct VelFrame {
    double sin_lat, cos_lat, sin_lon, cos_lon, height;
};
// the geodetic latitude by kVelFrameSteps fixed-point steps from the geocentric one; needs radius = fix_radius(st) >= kFixMaskRadius
GAT_HD inline VelFrame vel_frame(const double *st, double radius)
{
    const double x = st[0], y = st[1], z = st[2];
    const double p = __builtin_sqrt(x * x + y * y);
    double s = z / radius, c = p / radius;
    for (int i = 0; i < kVelFrameSteps; ++i) {
        const double N = kVelA / __builtin_sqrt(1.0 - kVelE2 * s * s);
        const double zp = z + kVelE2 * N * s;
        const double q = __builtin_sqrt(zp * zp + p * p);
        s = zp / q;
        c = p / q;
    }
    VelFrame f;
    f.sin_lat = s, f.cos_lat = c;
    f.height = p * c + z * s - kVelA * __builtin_sqrt(1.0 - kVelE2 * s * s);
    f.cos_lon = p > 0.0 ? x / p : 1.0;
    f.sin_lon = p > 0.0 ? y / p : 0.0;
    return f;
}

// ---- an epoch's record -----------------------------------------------------------------------------------------------------------------------
GAT_HD inline bool vel_failed(int status) { return (status & (GAT_VEL_NO_FIX | GAT_VEL_FEW_SATS | GAT_VEL_SINGULAR | GAT_VEL_NONFINITE)) != 0; }
// the fix gives a state to form the rows at
GAT_HD inline bool vel_fix_given(const gat_fix &f)
{
    return !fix_failed(f.status) && fix_finite(f.x) && fix_finite(f.y) && fix_finite(f.z) && fix_finite(f.clock_bias_s);
}
// s: the solution (vx, vy, vz, c drift); st: the fix's state
GAT_HD inline gat_velocity vel_record(int status, int num_valid, int num_used, const double *s, double sum_v2, const double *st)
{
    gat_velocity o{};
    o.status = status;
    if (status & GAT_VEL_NO_FIX) return o;
    o.num_valid = num_valid, o.num_used = num_used;
    if (vel_failed(status)) return o;
    o.vx = s[0], o.vy = s[1], o.vz = s[2];
    o.clock_drift = s[3] / kFixC;
    o.rms_residual_mps = __builtin_sqrt(sum_v2 / (double)num_used);
    const double radius = fix_radius(st);
    if (!(radius >= kFixMaskRadius)) {
        o.status |= GAT_VEL_NO_GEODETIC;
        return o;
    }
    const VelFrame f = vel_frame(st, radius);
    o.sin_lat = f.sin_lat, o.cos_lat = f.cos_lat, o.sin_lon = f.sin_lon, o.cos_lon = f.cos_lon, o.height_m = f.height;
    o.ve = -f.sin_lon * s[0] + f.cos_lon * s[1];
    o.vn = -f.sin_lat * f.cos_lon * s[0] - f.sin_lat * f.sin_lon * s[1] + f.cos_lat * s[2];
    o.vu = f.cos_lat * f.cos_lon * s[0] + f.cos_lat * f.sin_lon * s[1] + f.sin_lat * s[2];
    return o;
}

} // namespace gat
