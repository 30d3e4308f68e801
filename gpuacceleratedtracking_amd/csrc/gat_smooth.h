// gat_smooth.h -- the carrier smoothing's rule (include/gat.h, "carrier smoothing"): whether an (epoch, channel) is measured, the
// increment of code minus carrier between two neighbouring epochs and the reasons that begin an arc, the segment that the three
// scans are made of, and the outputs of one (epoch, channel) from the scans' values, written once for the kernels (gat_smooth.hip)
// and for the host twin (gat_smooth_plan.h), as gat_obs.h is for the observables.  Everything that accumulates is an integer (the
// increments are rounded to u = 2^-48 s before they are summed); the floating-point results are single expressions, compiled
// without contraction in both builds, so both give the same bits in any order of summation.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "gat.h"
#include "gat_hd.h"
#include "gat_obs.h" // obs_finite, the week's milliseconds

namespace gat {

constexpr double kSmUnit = 0x1p-48;    // u, s: c u = 1.07 um
constexpr double kSmMaxGate = 0x1p-18; // s: |q| <= 2^30
constexpr int kSmMaxWindow = 65536;
constexpr int64_t kSmMaxDms = 1000;

// what the rule reads of a call's configuration
struct SmRule {
    uint32_t flags;
    int W;
    double carrier_hz, if_cycles /* if_hz * epoch_seconds */, epoch_seconds, cmc_gate, rate_gate;
};

// the call's arrays: tx_ms, tx_frac, cycles, cfrac, doppler, valid [E][K]; rx_ms, rx_frac [E]; doppler and valid may be null
struct SmIn {
    const int32_t *tx_ms;
    const double *tx_frac;
    const int32_t *rx_ms;
    const double *rx_frac;
    const int64_t *cycles;
    const double *cfrac, *doppler;
    const uint8_t *valid;
};
struct SmOut {
    double *tx_frac_out;
    int32_t *count;
    double *cmc_s;
    uint8_t *status;
    gat_smooth_channel *channels;
};

// one (epoch, channel) as the rule reads it; doppler is 0 where the rate test is off
struct SmEpoch {
    int64_t cycles;
    double tx_frac, rx_frac, cfrac, doppler;
    int32_t tx_ms, rx_ms;
    bool measured;
};
GAT_HD inline SmEpoch sm_load(const SmRule &r, const SmIn &in, int K, int e, int k)
{
    const size_t o = (size_t)e * (size_t)K + (size_t)k;
    const bool rate = (r.flags & GAT_SMOOTH_RATE_TEST) != 0;
    SmEpoch s;
    s.tx_ms = in.tx_ms[o], s.rx_ms = in.rx_ms[e];
    s.tx_frac = in.tx_frac[o], s.rx_frac = in.rx_frac[e];
    s.cycles = in.cycles[o], s.cfrac = in.cfrac[o];
    s.doppler = rate ? in.doppler[o] : 0.0;
    s.measured = s.tx_ms >= 0 && s.rx_ms >= 0 && obs_finite(s.tx_frac) && obs_finite(s.rx_frac) && obs_finite(s.cfrac) &&
                 obs_finite(s.doppler) && (!in.valid || in.valid[o] != 0);
    return s;
}

// a difference of milliseconds, wrapped once into [-302400000, 302400000)
GAT_HD inline int64_t sm_wrap_once(int64_t d)
{
    if (d >= kObsHalfWeekMs) return d - kObsWeekMs;
    if (d < -kObsHalfWeekMs) return d + kObsWeekMs;
    return d;
}

// Epoch c behind epoch p (first: there is none): the status bits of c and its increment q in units of u, 0 at an arc start and
// where c is not measured.  |delta| <= cmc_gate <= 2^-18 s wherever q is formed, so |delta / u| <= 2^30 and the cast is defined.
GAT_HD inline int sm_step(const SmRule &r, bool first, const SmEpoch &p, const SmEpoch &c, int64_t *q)
{
    *q = 0;
    if (!c.measured) return 0;
    if (first || !p.measured) return GAT_SMOOTH_MEASURED | GAT_SMOOTH_GAP;
    const int64_t dms = sm_wrap_once((int64_t)c.rx_ms - (int64_t)p.rx_ms) - sm_wrap_once((int64_t)c.tx_ms - (int64_t)p.tx_ms);
    const double dphi = (double)(int64_t)((uint64_t)c.cycles - (uint64_t)p.cycles) + (c.cfrac - p.cfrac);
    const double dphin = dphi - r.if_cycles;
    const double delta = (double)dms * 1e-3 + ((c.rx_frac - p.rx_frac) - (c.tx_frac - p.tx_frac)) + dphin / r.carrier_hz;
    int st = GAT_SMOOTH_MEASURED;
    if (dms > kSmMaxDms || dms < -kSmMaxDms || !(__builtin_fabs(delta) <= r.cmc_gate)) st |= GAT_SMOOTH_CMC;
    if ((r.flags & GAT_SMOOTH_RATE_TEST) && !(__builtin_fabs(dphin - 0.5 * (c.doppler + p.doppler) * r.epoch_seconds) <= r.rate_gate))
        st |= GAT_SMOOTH_RATE;
    if (st == GAT_SMOOTH_MEASURED) *q = (int64_t)__builtin_rint(delta / kSmUnit);
    return st;
}
GAT_HD inline bool sm_arc_start(int status) { return (status & (GAT_SMOOTH_GAP | GAT_SMOOTH_CMC | GAT_SMOOTH_RATE)) != 0; }

// A run of consecutive epochs of one channel: len epochs, Q the sum of their q, S the sum of their local C (the running sum of q
// from the run's first epoch), both modulo 2^64; reset the last arc start among them (the epoch's index in the call, -1: none); the
// channel record's four counts.
struct SmSeg {
    uint64_t Q, S;
    int32_t len, reset;
    int32_t cnt[4];
};
GAT_HD inline SmSeg sm_empty()
{
    SmSeg s{};
    s.reset = -1;
    return s;
}
// epoch e (q and status of sm_step) appended to a run
GAT_HD inline void sm_push(SmSeg *s, int e, int64_t q, int status)
{
    s->Q += (uint64_t)q;
    s->S += s->Q;
    s->len += 1;
    if (sm_arc_start(status)) s->reset = e, s->cnt[1] += 1;
    if (status & GAT_SMOOTH_MEASURED) s->cnt[0] += 1;
    if (status & GAT_SMOOTH_CMC) s->cnt[2] += 1;
    if (status & GAT_SMOOTH_RATE) s->cnt[3] += 1;
}
// run a followed by run b: associative, not commutative
GAT_HD inline SmSeg sm_combine(const SmSeg &a, const SmSeg &b)
{
    SmSeg s;
    s.Q = a.Q + b.Q;
    s.S = a.S + b.S + (uint64_t)(int64_t)b.len * a.Q;
    s.len = a.len + b.len;
    s.reset = a.reset > b.reset ? a.reset : b.reset;
    for (int i = 0; i < 4; ++i) s.cnt[i] = a.cnt[i] + b.cnt[i];
    return s;
}

// n of a measured epoch e whose arc began at a
GAT_HD inline int sm_count(const SmRule &r, int e, int a)
{
    const int len = e - a + 1;
    return len < r.W ? len : r.W;
}
// The outputs of one (epoch, channel) but its status.  a < 0: not measured.  C_e, SS_e the scans at e, SS_back = SS_{e - n} (0 for
// e - n = -1), C_a = C at the arc's start.  The true S = sum over the window of (C_j - C_e) has n <= 65536 terms, the j-th at most
// (n - j) 2^30 in size: |S| <= 2^30 n (n - 1) / 2 < 2^61 < 2^62, and |C_e - C_a| <= 2^30 E <= 2^50; so the differences modulo 2^64,
// read as int64, are the true values whatever the global sums wrapped to.
GAT_HD inline void sm_emit(const SmRule &r, const SmOut &out, size_t o, int e, double tx_frac, int a, uint64_t C_e, uint64_t SS_e, uint64_t SS_back,
                           uint64_t C_a)
{
    if (a < 0) {
        out.tx_frac_out[o] = tx_frac;
        if (out.count) out.count[o] = 0;
        if (out.cmc_s) out.cmc_s[o] = 0.0;
        return;
    }
    const int n = sm_count(r, e, a);
    const int64_t S = (int64_t)(SS_e - SS_back - (uint64_t)(int64_t)n * C_e);
    const double m = ((double)S * kSmUnit) / (double)n;
    out.tx_frac_out[o] = tx_frac - m;
    if (out.count) out.count[o] = n;
    if (out.cmc_s) out.cmc_s[o] = (double)(int64_t)(C_e - C_a) * kSmUnit;
}

} // namespace gat
