// gat_raim.h -- the fix integrity's rule (include/gat.h, "fix integrity"): the test statistic's term, a channel frozen for a round of
// trials, the leave-one-out trial and the integrity record, written once for the device kernel (gat_raim.hip) and for the host twin
// (gat_raim_plan.h) on top of the position fix's rule (gat_fix.h) and under its terms: FP64, no contraction, every expression
// evaluated as written, every sum in channel order from +0, so both builds give the same bits.
#pragma once

#include "gat_fix.h"

namespace gat {

constexpr int kRaimEntry = 6;                                 // doubles of a frozen channel: xr, yr, z, g, w, used
constexpr int kRaimThresholds = GAT_MAX_FIX_CHANNELS - 3;     // by d = n - 4 = 0 .. 60

// a channel's term of T at a row's residual
GAT_HD inline double raim_term(double w, double v) { return w * (v * v); }

// T of the used set against the caller's threshold: NaN never detects
GAT_HD inline bool raim_detected(double T, double threshold) { return T > threshold; }

// A channel as a round's trials see it: the satellite turned by the Earth's rotation over tau (the travel time its last row left),
// its range term rho + c dts, its weight and whether it is in the used set.
GAT_HD inline void raim_entry(const FixSat &s, double tau, double w, bool used, double *q)
{
    double c, sn;
    fix_sincos(kFixOmegaE * tau, &c, &sn);
    q[0] = c * s.X + sn * s.Y;
    q[1] = c * s.Y - sn * s.X;
    q[2] = s.Z;
    q[3] = s.rho + kFixC * s.dts;
    q[4] = w;
    q[5] = used ? 1.0 : 0.0;
}
// the frozen channel's row at the state: no sine, no cosine
GAT_HD inline FixRow raim_row(const double *q, const double *st)
{
    const double dx = q[0] - st[0], dy = q[1] - st[1], dz = q[2] - st[2];
    FixRow o;
    o.r = __builtin_sqrt(dx * dx + dy * dy + dz * dz);
    o.lx = dx / o.r, o.ly = dy / o.r, o.lz = dz / o.r;
    o.v = q[3] - (o.r + st[3]);
    return o;
}

// The trial of candidate j over the K entries at ent (the wave's LDS, the same address in every lane; the twin's array) from the
// state `start`: the used channels but j, at most trial_iter iterations.  counts: converged, every step good, T finite.
struct RaimTrial {
    double st[4], T;
    bool counts;
};
GAT_HD inline RaimTrial raim_trial(const double *ent, int K, int j, const double *start, int trial_iter, double tol_m)
{
    RaimTrial t;
    t.st[0] = start[0], t.st[1] = start[1], t.st[2] = start[2], t.st[3] = start[3];
    t.T = 0.0, t.counts = false;
    bool converged = false;
    for (int it = 0; it < trial_iter && !converged; ++it) {
        double sums[kFixTerms] = {};
            for (int k = 0; k < K; ++k) {
            const double *q = ent + kRaimEntry * k;
            if (q[5] == 0.0) continue; // the same in every lane
            double tm[kFixTerms];
            fix_terms(raim_row(q, t.st), q[4], tm);
            for (int n = 0; n < kFixTerms; ++n) sums[n] += k == j ? 0.0 : tm[n];
        }
        double d[4];
        if (fix_step(sums, d)) return t;
        for (int i = 0; i < 4; ++i) t.st[i] += d[i];
        converged = __builtin_sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]) < tol_m;
    }
    if (!converged) return t;
    double T = 0.0;
    for (int k = 0; k < K; ++k) {
        const double *q = ent + kRaimEntry * k;
        if (q[5] == 0.0) continue;
        const double term = raim_term(q[4], raim_row(q, t.st).v);
        T += k == j ? 0.0 : term;
    }
    if (!fix_finite(T)) return t;
    t.T = T, t.counts = true;
    return t;
}
// the order the choice is made in: the smaller T, then the lower channel
GAT_HD inline bool raim_before(double Ta, int ja, double Tb, int jb) { return Ta < Tb || (Ta == Tb && ja < jb); }

// ---- an epoch's integrity record ------------------------------------------------------------------------------------------------
GAT_HD inline gat_fix_integrity raim_blank()
{
    gat_fix_integrity g{};
    g.excluded[0] = g.excluded[1] = g.excluded[2] = g.excluded[3] = -1;
    return g;
}
// the record of an epoch whose fix stands as the full set gave it: the test's result, no exclusion
GAT_HD inline gat_fix_integrity raim_full_set(int status, int dof, double T, double threshold)
{
    gat_fix_integrity g = raim_blank();
    g.status = status, g.dof = dof;
    g.stat0 = g.stat = T;
    g.threshold0 = g.threshold = threshold;
    return g;
}
// the record of an epoch with `count` channels left out (ex[0 .. count), -1 after), the final set passing with T under threshold
GAT_HD inline gat_fix_integrity raim_excluded(const gat_fix_integrity &full, int count, int e0, int e1, int e2, int e3, double T, double threshold)
{
    gat_fix_integrity g = full;
    g.status = GAT_RAIM_DETECTED | GAT_RAIM_EXCLUDED;
    g.num_excluded = count;
    g.excluded[0] = e0, g.excluded[1] = e1, g.excluded[2] = e2, g.excluded[3] = e3;
    g.stat = T, g.threshold = threshold;
    return g;
}

} // namespace gat
