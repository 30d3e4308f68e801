// gat_obs.h -- the observables' rule (include/gat.h, "observables"): the wraps of a block read off two neighbouring records, the
// frame block and TOW of a channel from the monitor's and the decoder's records, the bit edge, a transmission time, the anchor's
// order and a reception time, written once for the kernels (gat_obs.hip) and for the host twin (gat_obs_plan.h), as gat_fix.h is for
// the fix.  Everything that accumulates is an integer; the floating-point results are single quotients, compiled without
// contraction in both builds, so both give the same bits.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "gat.h"
#include "gat_hd.h"

namespace gat {

constexpr int64_t kObsWeekMs = 604800000;
constexpr int64_t kObsHalfWeekMs = 302400000;
constexpr int64_t kObsTowCounts = 100800;   // 6 s steps in a week
constexpr double kObsWrapTol = 1e-6;        // a quotient further than this from its integer: a bad record
constexpr double kObsWrapMax = 2147483648.0; // ... or beyond this
constexpr int kObsNoMeasurement = GAT_OBS_BAD_RECORD | GAT_OBS_NO_BIT_SYNC | GAT_OBS_NO_FRAME_SYNC | GAT_OBS_FRAME_OUTSIDE | GAT_OBS_NO_TOW;

GAT_HD inline bool obs_finite(double x)
{
    uint64_t u;
    __builtin_memcpy(&u, &x, sizeof u);
    return ((u >> 52) & 0x7ff) != 0x7ff;
}
// the largest double below 1e-3
GAT_HD inline double obs_below_ms()
{
    double x = 1e-3;
    uint64_t u;
    __builtin_memcpy(&u, &x, sizeof u);
    u -= 1;
    __builtin_memcpy(&x, &u, sizeof u);
    return x;
}
GAT_HD inline int64_t obs_mod(int64_t v, int64_t m)
{
    const int64_t r = v % m;
    return r < 0 ? r + m : r;
}

// what the rule reads of a call's configuration
struct ObsRule {
    int P, Pd, max_frames, min_tow_steps, rx_mode, travel_ms, rx0_ms;
    int B, K, E, first, stride;
    long long N, Fs;
    double Lc, fc, T, fs, if_hz, edge_margin, rx0_frac;
    int full_status; // every status bit of the format's frames
};

GAT_HD inline bool obs_record_finite(const gat_channel_params &r)
{
    return obs_finite(r.code_freq_hz) && obs_finite(r.carrier_freq_hz) && obs_finite(r.code_phase_chips) && obs_finite(r.carrier_phase_cycles);
}
// x within kObsWrapTol of an integer below kObsWrapMax: that integer; else 0 and *bad
GAT_HD inline int64_t obs_whole(double x, bool *bad)
{
    if (!obs_finite(x) || !(x < kObsWrapMax) || !(x > -kObsWrapMax)) {
        *bad = true;
        return 0;
    }
    const double r = __builtin_rint(x);
    const double d = x - r;
    if (!(d <= kObsWrapTol && d >= -kObsWrapTol)) {
        *bad = true;
        return 0;
    }
    return (int64_t)r;
}
// block i from record a = history[i] and b = history[i + 1]: the whole code periods and carrier cycles
GAT_HD inline void obs_wraps(const ObsRule &o, const gat_channel_params &a, const gat_channel_params &b, int64_t *w, int64_t *c, bool *bad)
{
    const double q = ((a.code_phase_chips + a.code_freq_hz * o.T) - b.code_phase_chips) / o.Lc;
    const double d = (a.carrier_phase_cycles + a.carrier_freq_hz * o.T) - b.carrier_phase_cycles;
    *w = obs_whole(q, bad);
    *c = obs_whole(d, bad);
}
GAT_HD inline bool obs_tau_inside(const ObsRule &o, double tau) { return tau >= 0.0 && tau < o.Lc; }
// history index i is epoch *e
GAT_HD inline bool obs_epoch_at(const ObsRule &o, long long i, int *e)
{
    if (i < o.first) return false;
    const long long d = i - o.first;
    if (d % o.stride != 0 || d / o.stride >= o.E) return false;
    *e = (int)(d / o.stride);
    return true;
}

// a channel's record before the edge: the status bits of the syncs and the TOW, g (-1 without one inside the history), f*, frame0_ms
struct ObsSync {
    int status;
    long long g;
    int fstar, frame0_ms;
    bool synced;
};
GAT_HD inline ObsSync obs_sync(const ObsRule &o, const gat_monitor_channel &m, const gat_nav_channel &n, const gat_nav_frame *frames)
{
    ObsSync s{0, -1, 0, 0, false};
    if (m.start < 0) s.status |= GAT_OBS_NO_BIT_SYNC;
    if (n.frame_offset < 0) s.status |= GAT_OBS_NO_FRAME_SYNC;
    if (s.status == 0) {
        s.synced = true;
        s.g = (long long)m.start + ((long long)n.symbol_phase + (long long)o.P * n.frame_offset) * o.Pd;
        if (s.g > o.B || s.g < 0) s.status |= GAT_OBS_FRAME_OUTSIDE;
    }
    int fstar = -1;
    const int nf = n.num_frames < o.max_frames ? n.num_frames : o.max_frames;
    for (int f = 0; f < nf; ++f)
        if (frames[f].status == o.full_status) {
            fstar = f;
            break;
        }
    if (fstar < 0 || n.tow_steps < o.min_tow_steps)
        s.status |= GAT_OBS_NO_TOW;
    else {
        s.fstar = fstar;
        s.frame0_ms = (int)(6000 * obs_mod((int64_t)frames[fstar].tow - 1 - fstar, kObsTowCounts));
    }
    return s;
}

// what the epoch kernel needs of a resolved channel (context scratch, [K])
struct ObsChan {
    int32_t status;
    int32_t frame0_ms;
    int64_t pstar;
    int32_t tx0_ms; // the transmission of epoch 0 (-1: none)
    int32_t pad;
    double tx0_frac;
};

// the channel's record from its syncs, the bad flag of its wraps and epochs, n_g and tau_g (read only with g inside)
GAT_HD inline gat_obs_channel obs_channel(const ObsRule &o, const ObsSync &s, bool bad, int64_t n_g, double tau_g)
{
    gat_obs_channel c{};
    const bool inside = s.synced && !(s.status & GAT_OBS_FRAME_OUTSIDE);
    if (inside && !obs_tau_inside(o, tau_g)) bad = true;
    c.status = s.status | (bad ? GAT_OBS_BAD_RECORD : 0);
    if (s.synced) c.frame_block = (int32_t)s.g;
    if (!(s.status & GAT_OBS_NO_TOW)) c.tow_frame = s.fstar, c.frame0_ms = s.frame0_ms;
    if (inside && !bad) {
        const double x = tau_g / o.Lc;
        c.edge_fraction = x;
        c.edge_period = n_g + (int64_t)__builtin_rint(x);
        const double d = x - 0.5;
        if (d < o.edge_margin && -d < o.edge_margin) c.status |= GAT_OBS_EDGE_AMBIGUOUS;
    }
    return c;
}
GAT_HD inline bool obs_measured(int status) { return (status & kObsNoMeasurement) == 0; }
GAT_HD inline int32_t obs_tx_ms(int32_t frame0_ms, int64_t n_b, int64_t pstar) { return (int32_t)obs_mod((int64_t)frame0_ms + (n_b - pstar), kObsWeekMs); }
GAT_HD inline double obs_tx_frac(const ObsRule &o, double tau)
{
    const double f = tau / o.fc;
    return f >= 1e-3 ? obs_below_ms() : f;
}

// ---- reception ------------------------------------------------------------------------------------------------------------------------
struct ObsAnchor {
    int32_t ms; // -1: none
    int32_t a;
    double frac;
};
// the anchor's order: is (ms, frac) of a later channel later than the best so far, both against the first measured channel's ms?
GAT_HD inline int64_t obs_wrap_ms(int64_t d)
{
    d = obs_mod(d, kObsWeekMs);
    return d >= kObsHalfWeekMs ? d - kObsWeekMs : d;
}
GAT_HD inline bool obs_later(int32_t ref_ms, int32_t ms, double frac, int32_t best_ms, double best_frac)
{
    const int64_t d = obs_wrap_ms((int64_t)ms - ref_ms), b = obs_wrap_ms((int64_t)best_ms - ref_ms);
    return d > b || (d == b && frac > best_frac);
}
GAT_HD inline ObsAnchor obs_anchor_from(const ObsRule &o, int32_t ms, double frac)
{
    return ObsAnchor{(int32_t)obs_mod((int64_t)ms + o.travel_ms, kObsWeekMs), o.first, frac};
}
GAT_HD inline void obs_rx(const ObsRule &o, const ObsAnchor &an, int e, int32_t *rx_ms, double *rx_frac)
{
    if (an.ms < 0) {
        *rx_ms = -1, *rx_frac = 0.0;
        return;
    }
    const long long b = (long long)o.first + (long long)e * o.stride;
    const long long S = (b - an.a) * o.N;
    const long long num = S * 1000;
    long long ms_add = num / o.Fs;
    const long long rem = num % o.Fs;
    double frac = an.frac + (double)rem / (o.fs * 1000.0);
    if (frac >= 1e-3) {
        frac = frac - 1e-3;
        ms_add += 1;
    }
    *rx_ms = (int32_t)obs_mod((int64_t)an.ms + ms_add, kObsWeekMs);
    *rx_frac = frac;
}

// ---- the outputs of one (epoch, channel) ----------------------------------------------------------------------------------------------
struct ObsOut {
    int32_t *tx_ms;
    double *tx_frac;
    int32_t *rx_ms;
    double *rx_frac;
    int64_t *carrier_cycles;
    double *carrier_frac, *doppler_hz, *code_rate_hz;
    gat_obs_channel *channels;
};
GAT_HD inline void obs_tx(const ObsRule &o, const ObsChan &c, const gat_channel_params &r, int64_t n_b, int32_t *ms, double *frac)
{
    const bool m = obs_measured(c.status);
    *ms = m ? obs_tx_ms(c.frame0_ms, n_b, c.pstar) : -1;
    *frac = m ? obs_tx_frac(o, r.code_phase_chips) : 0.0;
}
GAT_HD inline void obs_emit(const ObsRule &o, const ObsOut &out, const ObsChan &c, const gat_channel_params &r, int e, int k, int64_t n_b, int64_t W_b)
{
    const size_t at = (size_t)e * (size_t)o.K + (size_t)k;
    const bool bad = (c.status & GAT_OBS_BAD_RECORD) != 0;
    int32_t ms;
    double frac;
    obs_tx(o, c, r, n_b, &ms, &frac);
    if (out.tx_ms) out.tx_ms[at] = ms;
    if (out.tx_frac) out.tx_frac[at] = frac;
    if (out.carrier_cycles) out.carrier_cycles[at] = bad ? 0 : W_b;
    if (out.carrier_frac) out.carrier_frac[at] = bad ? 0.0 : r.carrier_phase_cycles;
    if (out.doppler_hz) out.doppler_hz[at] = bad ? 0.0 : r.carrier_freq_hz - o.if_hz;
    if (out.code_rate_hz) out.code_rate_hz[at] = bad ? 0.0 : r.code_freq_hz;
}

} // namespace gat
