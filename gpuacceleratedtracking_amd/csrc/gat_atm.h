// gat_atm.h -- the range corrections' rule (include/gat.h, "atmosphere") on top of the position fix's (gat_fix.h) and the velocity
// fix's frame (gat_vel.h): the arctangent, a channel's local line of sight at the fix's state, the Klobuchar delay of the IS-GPS-200
// single-frequency user, Chao's mapping of the caller's zenith delays and the corrected transmit-time fraction, written once for the
// device kernel (gat_atm.hip) and for the host twin (gat_atm_plan.h).  As gat_fix.h: FP64, no contraction, every expression evaluated
// as written, no libm transcendental, so both builds give the same bits.
#pragma once

#include "gat_fix.h"
#include "gat_vel.h"

namespace gat {

constexpr double kAtmPi = 3.1415926535898; // semicircles, as the interface specification has it
constexpr double kAtmL1 = 1575.42e6;       // Hz: the model's frequency
constexpr double kAtmDay = 86400.0;        // s
constexpr int32_t kAtmDayMs = 86400000;

// ---- the arctangent ----------------------------------------------------------------------------------------------------------------------
// atan(k / 16), k = 0 .. 16, rounded from 200-bit values
GAT_HD inline double atm_atan_knot(int k)
{
    constexpr double A[17] = {0x0.0p+0,
                              0x1.ff55bb72cfdeap-5,
                              0x1.fd5ba9aac2f6ep-4,
                              0x1.7b97b4bce5b02p-3,
                              0x1.f5b75f92c80ddp-3,
                              0x1.362773707ebccp-2,
                              0x1.6f61941e4def1p-2,
                              0x1.a64eec3cc23fdp-2,
                              0x1.dac670561bb4fp-2,
                              0x1.0657e94db30d0p-1,
                              0x1.1e00babdefeb4p-1,
                              0x1.345f01cce37bbp-1,
                              0x1.4978fa3269ee1p-1,
                              0x1.5d58987169b18p-1,
                              0x1.700a7c5784634p-1,
                              0x1.819d0b7158a4dp-1,
                              0x1.921fb54442d18p-1};
    return A[k];
}
constexpr double kAtmPiHi = 0x1.921fb54442d18p+1, kAtmPiLo = 0x1.1a62633145c07p-53;         // pi in two parts
constexpr double kAtmHalfPiHi = 0x1.921fb54442d18p+0, kAtmHalfPiLo = 0x1.1a62633145c07p-54; // pi / 2
GAT_HD inline bool atm_sign(double x)
{
    uint64_t u;
    __builtin_memcpy(&u, &x, sizeof u);
    return (u >> 63) != 0;
}
// The angle of (x, y) in (-pi, pi].  The octant by exact operations (absolute values, a swap); t = min / max in [0, 1] is split at
// the nearest c = k / 16: atan t = atan c + atan s, s = (t - c) / (1 + t c), |s| <= 1 / 32, and atan s is its odd Taylor polynomial to
// degree 11 (the first term left out, s^13 / 13, is below 2^-68).  |error| <= 1e-15 rad.  x = y = 0: +0.  A quotient that is no
// number (inf / inf, a NaN argument) takes knot 0 and gives NaN; no step depends on the data but by selection.
GAT_HD inline double atm_atan2(double y, double x)
{
    const double ax = __builtin_fabs(x), ay = __builtin_fabs(y);
    const bool swap = ay > ax;
    const double num = swap ? ax : ay, den = swap ? ay : ax;
    const bool origin = ax == 0.0 && ay == 0.0;
    const double t = origin ? 0.0 : num / den;
    const int k = t <= 1.0 ? (int)__builtin_rint(t * 16.0) : 0;
    const double c = (double)k * 0.0625;
    const double s = (t - c) / (1.0 + t * c);
    const double s2 = s * s;
    double p = __builtin_fma(s2, -9.090909090909091e-02, 1.1111111111111111e-01);
    p = __builtin_fma(s2, p, -1.4285714285714285e-01);
    p = __builtin_fma(s2, p, 2.0e-01);
    p = __builtin_fma(s2, p, -3.333333333333333e-01);
    double a = atm_atan_knot(k) + __builtin_fma(s2 * s, p, s);
    a = swap ? (kAtmHalfPiHi - a) + kAtmHalfPiLo : a;
    a = x < 0.0 ? (kAtmPiHi - a) + kAtmPiLo : a;
    if (origin) return 0.0;
    return atm_sign(y) ? -a : a;
}

// ---- an epoch: the fix's state and its geodetic frame -----------------------------------------------------------------------------------
struct AtmEpoch {
    int status;   // GAT_ATM_NO_FIX, GAT_ATM_NO_GEODETIC or 0
    double st[4]; // x, y, z, c clock_bias_s
    double bias;  // clock_bias_s
    VelFrame f;
    double phi_u, lambda_u; // semicircles
};
GAT_HD inline AtmEpoch atm_epoch(const gat_fix &fix)
{
    AtmEpoch o{};
    if (!vel_fix_given(fix)) {
        o.status = GAT_ATM_NO_FIX;
        return o;
    }
    o.st[0] = fix.x, o.st[1] = fix.y, o.st[2] = fix.z, o.st[3] = kFixC * fix.clock_bias_s;
    o.bias = fix.clock_bias_s;
    const double radius = fix_radius(o.st);
    if (!(radius >= kFixMaskRadius)) {
        o.status = GAT_ATM_NO_GEODETIC;
        return o;
    }
    o.f = vel_frame(o.st, radius);
    o.phi_u = atm_atan2(o.f.sin_lat, o.f.cos_lat) / kAtmPi;
    o.lambda_u = atm_atan2(o.f.sin_lon, o.f.cos_lon) / kAtmPi;
    return o;
}

// ---- the two delays -------------------------------------------------------------------------------------------------------------------------
// What the plan takes from the config: read by every (epoch, channel)
struct AtmParams {
    uint32_t flags;
    double floor_sin;
    double scale; // (1575.42e6 / carrier_hz)^2
    double alpha[4], beta[4];
    double zd, zw; // the config's zenith delays
};
// Klobuchar (IS-GPS-200 figure 20-4) in metres at the carrier.  u, h: the line of sight's up and horizontal parts; ca, sa: cos A,
// sin A; t_gps: the GPS time of day of the reception.  NaN where AMP or PER is not finite before it is raised.
GAT_HD inline double atm_iono(const AtmParams &p, const AtmEpoch &ep, double u, double h, double ca, double sa, double t_gps)
{
    const double E = atm_atan2(u, h) / kAtmPi;
    const double psi = 0.0137 / (E + 0.11) - 0.022;
    double phi_i = ep.phi_u + psi * ca;
    phi_i = phi_i > 0.416 ? 0.416 : (phi_i < -0.416 ? -0.416 : phi_i);
    double ci, si, cm, sm;
    fix_sincos(kAtmPi * phi_i, &ci, &si);
    const double lambda_i = ep.lambda_u + psi * sa / ci;
    fix_sincos(kAtmPi * (lambda_i - 1.617), &cm, &sm);
    const double phi_m = phi_i + 0.064 * cm;
    double t = 43200.0 * lambda_i + t_gps;
    t = t >= kAtmDay ? t - kAtmDay : t;
    t = t < 0.0 ? t + kAtmDay : t;
    const double F = 1.0 + 16.0 * (0.53 - E) * (0.53 - E) * (0.53 - E);
    double per = p.beta[0] + phi_m * (p.beta[1] + phi_m * (p.beta[2] + phi_m * p.beta[3]));
    double amp = p.alpha[0] + phi_m * (p.alpha[1] + phi_m * (p.alpha[2] + phi_m * p.alpha[3]));
    if (!fix_finite(per) || !fix_finite(amp)) return (per - per) + (amp - amp); // NaN
    per = per < 72000.0 ? 72000.0 : per;
    amp = amp < 0.0 ? 0.0 : amp;
    const double xx = 2.0 * kAtmPi * (t - 50400.0) / per;
    const double T = __builtin_fabs(xx) < 1.57 ? F * (5e-9 + amp * (1.0 - xx * xx / 2.0 + xx * xx * xx * xx / 24.0)) : F * 5e-9;
    return kFixC * T * p.scale;
}
// Chao's mapping of the zenith delays zd (hydrostatic) and zw (wet) at sin el = s in [-1, 1]
GAT_HD inline double atm_tropo(double s, double zd, double zw)
{
    const double tn = s / __builtin_sqrt(1.0 - s * s);
    const double md = 1.0 / (s + 0.00143 / (tn + 0.0445));
    const double mw = 1.0 / (s + 0.00035 / (tn + 0.017));
    return zd * md + zw * mw;
}

// ---- one (epoch, channel) -------------------------------------------------------------------------------------------------------------------
struct AtmChannel {
    double tx_frac, iono, tropo, sin_el, cos_a, sin_a;
    uint8_t status;
};
// zd, zw: the epoch's zenith delays (the caller's array's, or the config's)
GAT_HD inline AtmChannel atm_channel(const AtmParams &p, const AtmEpoch &ep, const gat_ephemeris &g, int32_t tx_ms, double tx_frac, int32_t rx_ms,
                                     double rx_frac, double zd, double zw)
{
    AtmChannel o{tx_frac, 0.0, 0.0, 0.0, 0.0, 0.0, 0};
    if (ep.status != 0) return o;
    const FixSat c = fix_sat(g, tx_ms, tx_frac, rx_ms, rx_frac);
    if (!c.ok) return o;
    double tau = kFixFirstTravel;
    FixRow r = fix_row(c, tau, ep.st);
    for (int i = 1; i < kVelRows; ++i) {
        tau = r.r / kFixC;
        r = fix_row(c, tau, ep.st);
    }
    const VelFrame &f = ep.f;
    const double e = -f.sin_lon * r.lx + f.cos_lon * r.ly;
    const double n = -f.sin_lat * f.cos_lon * r.lx - f.sin_lat * f.sin_lon * r.ly + f.cos_lat * r.lz;
    const double u = f.cos_lat * f.cos_lon * r.lx + f.cos_lat * f.sin_lon * r.ly + f.sin_lat * r.lz;
    if (!(fix_finite(e) && fix_finite(n) && fix_finite(u))) {
        o.status = GAT_ATM_CH_NONFINITE;
        return o;
    }
    const double s = u > 1.0 ? 1.0 : (u < -1.0 ? -1.0 : u);
    const double h = __builtin_sqrt(e * e + n * n);
    const double ca = h > 0.0 ? n / h : 1.0;
    const double sa = h > 0.0 ? e / h : 0.0;
    o.sin_el = s, o.cos_a = ca, o.sin_a = sa;
    if (!(s >= p.floor_sin)) {
        o.status = GAT_ATM_CH_LOW;
        return o;
    }
    double iono = 0.0, tropo = 0.0;
    if (p.flags & GAT_ATM_IONO) {
        const double t_gps = (double)(rx_ms % kAtmDayMs) * 1e-3 + rx_frac - ep.bias;
        iono = atm_iono(p, ep, u, h, ca, sa, t_gps);
    }
    if (p.flags & GAT_ATM_TROPO) tropo = atm_tropo(s, zd, zw);
    const double d = iono + tropo;
    const double out = d == 0.0 ? tx_frac : tx_frac + d / kFixC;
    if (!(fix_finite(iono) && fix_finite(tropo) && fix_finite(d) && fix_finite(out))) {
        o.status = GAT_ATM_CH_NONFINITE;
        return o;
    }
    o.iono = iono, o.tropo = tropo, o.tx_frac = out;
    o.status = GAT_ATM_CH_CORRECTED;
    return o;
}

} // namespace gat
