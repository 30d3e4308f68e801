// Stand-alone check of the fix integrity's pure plan (csrc/gat_raim_plan.h) and of the host twin's loops over it (raim_host_run, the
// rules of csrc/gat_fix.h and csrc/gat_raim.h).  Every documented refusal must return its code with nothing planned; random plans
// must keep the fix's geometry and every lane's frozen channel inside the wave's LDS, behind the fix's terms and sums.  The twin then
// runs on heap buffers of exactly the extents the call describes -- every subset of the optional outputs, with and without weights,
// clean epochs, epochs with a channel a code period off, epochs cut to five and to four measurements and epochs without any -- so
// that AddressSanitizer sees any access outside them, and must leave out the channel that was moved and find the receiver.  Last, a
// round is walked the way the kernel runs it -- 64 lanes in step, lane j holding candidate j, every lane reading the same entry, the
// lanes that are done idling, the choice by a butterfly of exchanges over (T_j, j) -- and must give the twin's T_j and choice to the
// bit; and the twin runs through orbits that are usable by the letter and garbage by their numbers, where the sine's quadrant must
// be taken without an out-of-range conversion.  Built with -fsanitize=address,undefined,float-cast-overflow by
// tests/test_raim_plan_host.py.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "gat_raim_plan.h"

using namespace gat;

namespace {

int failures = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            if (++failures <= 20) {                       \
                std::printf("FAIL %s:%d: ", #cond, __LINE__); \
                std::printf(__VA_ARGS__);                 \
                std::printf("\n");                        \
            }                                             \
        }                                                 \
    } while (0)

const void *const kGiven = reinterpret_cast<const void *>(uintptr_t(0x9000));
const double kInf = std::numeric_limits<double>::infinity();
const double kNaN = std::numeric_limits<double>::quiet_NaN();

gat_fix_config fix_cfg(int max_iter = 10, double tol = 1e-4, double mask = -1.0)
{
    gat_fix_config c{};
    c.struct_size = sizeof(gat_fix_config);
    c.max_iter = max_iter, c.tol_m = tol, c.mask_sin = mask;
    return c;
}
// thresholds that grow with d: 100 m^2 a degree of freedom (errors of a millimetre pass, a code period does not)
gat_raim_config raim_cfg(int max_exclude = 1, int trial_iter = 8)
{
    gat_raim_config c{};
    c.struct_size = sizeof(gat_raim_config);
    c.max_exclude = max_exclude, c.trial_iter = trial_iter;
    for (int d = 0; d < kRaimThresholds; ++d) c.threshold[d] = 100.0 * d;
    c.threshold[0] = kNaN; // not read
    return c;
}
RaimCall call(int E, int K, const gat_fix_config *cfg, const gat_raim_config *raim)
{
    return RaimCall{FixCall{kGiven, kGiven, kGiven, kGiven, kGiven, E, K, cfg, kGiven}, raim, kGiven};
}

void expect_refusal(const RaimCall &a, int code, const char *what)
{
    static RaimPlan p, q;
    std::memset(&p, 0x5a, sizeof p);
    std::memset(&q, 0x5a, sizeof q);
    const Refusal r = raim_plan(a, &p);
    CHECK(r.code == code, "%s: got %d, want %d", what, r.code, code);
    CHECK(std::memcmp(&p, &q, sizeof p) == 0, "%s: the plan was written", what);
}

void refusals()
{
    const gat_fix_config good = fix_cfg();
    const gat_raim_config rgood = raim_cfg();
    RaimCall a = call(3, 6, &good, &rgood);
    const void **ptrs[] = {&a.fix.eph, &a.fix.tx_ms, &a.fix.tx_frac, &a.fix.rx_ms, &a.fix.rx_frac, &a.fix.fixes, &a.integrity};
    for (const void **p : ptrs) {
        *p = nullptr;
        expect_refusal(a, GAT_ERR_ARG, "null pointer");
        *p = kGiven;
    }
    expect_refusal(call(3, 6, nullptr, &rgood), GAT_ERR_ARG, "null config");
    expect_refusal(call(3, 6, &good, nullptr), GAT_ERR_ARG, "null raim config");
    gat_raim_config r = rgood;
    r.struct_size += 8;
    expect_refusal(call(3, 6, &good, &r), GAT_ERR_ARG, "raim struct_size");
    r = rgood, r.max_exclude = -1;
    expect_refusal(call(3, 6, &good, &r), GAT_ERR_ARG, "max_exclude = -1");
    r = rgood, r.max_exclude = GAT_RAIM_MAX_EXCLUDE + 1;
    expect_refusal(call(3, 6, &good, &r), GAT_ERR_ARG, "max_exclude = 5");
    r = rgood, r.trial_iter = 0;
    expect_refusal(call(3, 6, &good, &r), GAT_ERR_ARG, "trial_iter = 0");
    r = rgood, r.flags = 2;
    expect_refusal(call(3, 6, &good, &r), GAT_ERR_ARG, "raim flags");
    const double bad[] = {kNaN, 0.0, -1.0, -kInf};
    for (int d = 1; d < kRaimThresholds; d += 7)
        for (double v : bad) {
            r = rgood, r.threshold[d] = v;
            expect_refusal(call(3, 6, &good, &r), GAT_ERR_ARG, "threshold");
        }
    gat_fix_config c = good;
    c.struct_size -= 4;
    expect_refusal(call(3, 6, &c, &rgood), GAT_ERR_ARG, "struct_size");
    expect_refusal(call(0, 6, &good, &rgood), GAT_ERR_ARG, "E = 0");
    expect_refusal(call(3, 0, &good, &rgood), GAT_ERR_ARG, "K = 0");
    c = good, c.max_iter = 0;
    expect_refusal(call(3, 6, &c, &rgood), GAT_ERR_ARG, "max_iter = 0");
    c = good, c.tol_m = kNaN;
    expect_refusal(call(3, 6, &c, &rgood), GAT_ERR_ARG, "tol_m NaN");
    c = good, c.mask_sin = kNaN;
    expect_refusal(call(3, 6, &c, &rgood), GAT_ERR_ARG, "mask_sin NaN");
    c = good, c.flags = 1;
    expect_refusal(call(3, 6, &c, &rgood), GAT_ERR_ARG, "flags");
    expect_refusal(call(3, GAT_MAX_FIX_CHANNELS + 1, &good, &rgood), GAT_ERR_RANGE, "K = 65");
    expect_refusal(call(GAT_MAX_FIX_EPOCHS + 1, 6, &good, &rgood), GAT_ERR_RANGE, "E = 2^24 + 1");
    // +inf is a threshold, entry 0 is not read
    r = rgood, r.threshold[1] = kInf, r.threshold[0] = -5.0;
    static RaimPlan p;
    CHECK(raim_plan(call(3, 6, &good, &r), &p).code == GAT_OK && p.threshold[1] == kInf && p.threshold[0] == 0.0, "+inf refused");
}

int plans(std::mt19937_64 &rng, int count)
{
    const gat_fix_config cfg = fix_cfg();
    static RaimPlan p;
    for (int n = 0; n < count; ++n) {
        const int E = n < 40 ? n + 1 : 1 + (int)(rng() % GAT_MAX_FIX_EPOCHS);
        const int K = 1 + (int)(rng() % GAT_MAX_FIX_CHANNELS);
        const gat_raim_config rc = raim_cfg((int)(rng() % 5), 1 + (int)(rng() % 12));
        CHECK(raim_plan(call(E, K, &cfg, &rc), &p).code == GAT_OK, "E %d K %d refused", E, K);
        FixPlan f{};
        CHECK(fix_plan(call(E, K, &cfg, &rc).fix, &f).code == GAT_OK && f.groups == p.fix.groups && p.fix.E == E && p.fix.K == K, "the fix's geometry");
        CHECK(p.max_exclude == rc.max_exclude && p.trial_iter == rc.trial_iter && p.threshold[60] == 6000.0, "the configuration");
        gat_fix_plan rep{};
        raim_report(p, &rep);
        CHECK(rep.workgroups == p.fix.groups && rep.threads == kFixThreads && rep.waves_per_workgroup == kFixWaves && rep.scratch_bytes == 0, "report");
        CHECK(rep.lds_bytes == kFixWaves * kRaimWaveDoubles * 8 && rep.lds_bytes <= 160 * 1024, "LDS");
        for (int lane = 0; lane < K; ++lane) { // a lane's frozen channel lies behind the fix's part of the wave's LDS and inside the wave's
            const int first = kFixWaveDoubles + kRaimEntry * lane, last = first + kRaimEntry - 1;
            CHECK(first >= kFixTerms * kFixPitch + kFixTerms && last < kRaimWaveDoubles, "entry of lane %d", lane);
        }
    }
    return count;
}

// a plausible constellation: near-circular orbits in six planes
std::vector<gat_ephemeris> constellation(std::mt19937_64 &rng, int K)
{
    std::uniform_real_distribution<double> u(-1.0, 1.0);
    std::vector<gat_ephemeris> ephs((size_t)K);
    for (int k = 0; k < K; ++k) {
        gat_ephemeris g{};
        g.wn = 77, g.iodc = 300 + k, g.iode = (300 + k) & 0xff, g.ura = 2;
        g.toe = 208800.0, g.toc = 208784.0;
        g.af0 = 2e-4 * u(rng), g.af1 = 3e-12 * u(rng), g.tgd = 8e-9 * u(rng);
        g.sqrt_a = 5153.6 + 0.3 * u(rng), g.e = 0.0105 + 0.0095 * u(rng);
        g.m0 = 3.1 * u(rng), g.delta_n = 4.5e-9 + 1e-9 * u(rng);
        g.omega0 = -3.0 + (k % 6) * 1.0471975512, g.i0 = 0.96 + 0.02 * u(rng), g.omega = 3.0 * u(rng);
        g.omega_dot = -8.2e-9 + 5e-10 * u(rng), g.idot = 4e-10 * u(rng);
        g.cuc = 4e-6 * u(rng), g.cus = 6e-6 * u(rng), g.crc = 250.0 + 90.0 * u(rng), g.crs = 100.0 * u(rng), g.cic = 2e-7 * u(rng), g.cis = 2e-7 * u(rng);
        g.valid = 1;
        ephs[(size_t)k] = g;
    }
    return ephs;
}

// the transmit time a receiver at xyz whose clock reads (rx_ms, rx_frac), `bias` seconds fast, measures; false: below the horizon
bool measure(const gat_ephemeris &g, const double *xyz, int32_t rx_ms, double rx_frac, double bias, int32_t *tx_ms, double *tx_frac)
{
    const double t_rx = fix_seconds(rx_ms, rx_frac) - bias;
    double tau = 0.075, d[3] = {0, 0, 0};
    for (int it = 0; it < 8; ++it) {
        double X, Y, Z, c, s;
        fix_orbit(g, t_rx - tau, &X, &Y, &Z);
        fix_sincos(kFixOmegaE * tau, &c, &s);
        d[0] = c * X + s * Y - xyz[0], d[1] = c * Y - s * X - xyz[1], d[2] = Z - xyz[2];
        tau = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]) / kFixC;
    }
    if (d[0] * xyz[0] + d[1] * xyz[1] + d[2] * xyz[2] <= 0.0) return false;
    double dts = 0.0;
    for (int it = 0; it < 4; ++it) dts = fix_clock(g, t_rx - tau + dts);
    const double off = rx_frac - bias - tau + dts;
    double m = std::floor(off * 1e3), f = off - m * 1e-3;
    if (f >= 1e-3) m += 1, f -= 1e-3;
    if (f < 0) m -= 1, f += 1e-3;
    *tx_ms = (int32_t)(((int64_t)rx_ms + (int64_t)m + 604800000) % 604800000);
    *tx_frac = f;
    return true;
}

template <class T>
struct Heap { // a buffer of exactly n elements, null when not asked for
    std::vector<T> v;
    bool on;
    Heap(size_t n, bool on_) : v(on_ ? n : 0), on(on_) {}
    T *ptr() { return on ? v.data() : nullptr; }
};

// What the kernel does in a round, lane by lane in step: the trial of every candidate of the epoch's used set from its state, then
// the butterfly.  T[j] < 0: lane j has no counting trial.  Returns the chosen channel, 64 for none.
int wave_round(const FixHostEpoch &h, int trial_iter, double tol_m, double *T)
{
    const int K = h.K, W = kFixWave;
    std::vector<double> lds((size_t)kRaimEntry * W, kNaN); // the wave's entries; lanes >= K write nothing
    for (int lane = 0; lane < K; ++lane) raim_entry(h.s[lane], h.tau[lane], h.wk[lane], h.used[lane], &lds[(size_t)kRaimEntry * lane]);
    double st[kFixWave][4];
    bool running[kFixWave], counts[kFixWave];
    for (int lane = 0; lane < W; ++lane) {
        running[lane] = lane < K && h.used[lane];
        counts[lane] = false;
        T[lane] = -1.0;
        for (int i = 0; i < 4; ++i) st[lane][i] = h.st[i];
    }
    for (int it = 0; it < trial_iter; ++it) // every lane that still runs takes the iteration; the others idle
        for (int lane = 0; lane < W; ++lane) {
            if (!running[lane]) continue;
            double sums[kFixTerms] = {};
            for (int k = 0; k < K; ++k) { // the same entry in every lane
                const double *q = &lds[(size_t)kRaimEntry * k];
                if (q[5] == 0.0 || k == lane) continue;
                double t[kFixTerms];
                fix_terms(raim_row(q, st[lane]), q[4], t);
                for (int n = 0; n < kFixTerms; ++n) sums[n] += t[n];
            }
            double d[4];
            if (fix_step(sums, d)) {
                running[lane] = false;
                continue;
            }
            for (int i = 0; i < 4; ++i) st[lane][i] += d[i];
            if (std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]) < tol_m) running[lane] = false, counts[lane] = true;
        }
    double bt[kFixWave];
    int bj[kFixWave];
    for (int lane = 0; lane < W; ++lane) {
        if (counts[lane]) {
            double sum = 0.0;
            for (int k = 0; k < K; ++k) {
                const double *q = &lds[(size_t)kRaimEntry * k];
                if (q[5] == 0.0 || k == lane) continue;
                sum += raim_term(q[4], raim_row(q, st[lane]).v);
            }
            counts[lane] = fix_finite(sum);
            if (counts[lane]) T[lane] = sum;
        }
        bt[lane] = counts[lane] ? T[lane] : 0.0;
        bj[lane] = counts[lane] ? lane : W;
    }
    for (int m = 1; m < W; m <<= 1) { // every lane exchanges with lane ^ m
        double nt[kFixWave];
        int nj[kFixWave];
        for (int lane = 0; lane < W; ++lane) {
            const double ot = bt[lane ^ m];
            const int oj = bj[lane ^ m];
            const bool take = oj < W && (bj[lane] >= W || raim_before(ot, oj, bt[lane], bj[lane]));
            nt[lane] = take ? ot : bt[lane], nj[lane] = take ? oj : bj[lane];
        }
        std::memcpy(bt, nt, sizeof bt), std::memcpy(bj, nj, sizeof bj);
    }
    for (int lane = 1; lane < W; ++lane) CHECK(bj[lane] == bj[0], "the lanes disagree on the choice");
    return bj[0];
}

int twins(std::mt19937_64 &rng, int count, int *rounds)
{
    std::uniform_real_distribution<double> u(-1.0, 1.0);
    int calls = 0;
    for (int n = 0; n < count; ++n) {
        const int K = n % 4 == 0 ? GAT_MAX_FIX_CHANNELS : 14 + (int)(rng() % 30);
        const int E = 6;
        const std::vector<gat_ephemeris> ephs = constellation(rng, K);
        std::vector<int32_t> tx_ms((size_t)E * K), rx_ms((size_t)E);
        std::vector<double> tx_frac((size_t)E * K), rx_frac((size_t)E), truth((size_t)E * 4);
        std::vector<int> seen((size_t)E, 0), moved((size_t)E, -1);
        // epoch 0 clean, 1 a channel a period off, 2 no measurement, 3 cut to five with one off, 4 cut to four, 5 a channel a period off
        for (int e = 0; e < E; ++e) {
            const double lat = 1.4 * u(rng), lon = 3.1 * u(rng), r = 6371e3 + 1000.0 * u(rng);
            double *x = &truth[(size_t)e * 4];
            x[0] = r * std::cos(lat) * std::cos(lon), x[1] = r * std::cos(lat) * std::sin(lon), x[2] = r * std::sin(lat), x[3] = 2e-4 * u(rng);
            rx_ms[(size_t)e] = 208800000 + (int32_t)(3000000.0 * u(rng)), rx_frac[(size_t)e] = 5e-4 * (1.0 + u(rng)) * 0.999;
            const int keep = e == 3 ? 5 : (e == 4 ? 4 : K);
            for (int k = 0; k < K; ++k) {
                const size_t o = (size_t)e * K + k;
                const bool ok = e != 2 && seen[(size_t)e] < keep && measure(ephs[(size_t)k], x, rx_ms[(size_t)e], rx_frac[(size_t)e], x[3], &tx_ms[o], &tx_frac[o]);
                if (!ok) tx_ms[o] = -1, tx_frac[o] = 0.0;
                seen[(size_t)e] += ok ? 1 : 0;
                if (ok && (e == 1 || e == 3 || e == 5) && (moved[(size_t)e] < 0 || rng() % 3 == 0)) moved[(size_t)e] = k;
            }
            if (moved[(size_t)e] >= 0) tx_ms[(size_t)e * K + moved[(size_t)e]] += (e == 5 ? -1 : 1);
        }
        const gat_fix_config cfg = fix_cfg(12, 1e-6, n % 3 == 0 ? 0.05 : -1.0);
        const gat_raim_config rc = raim_cfg(1 + n % 2, 8);
        for (unsigned outs = 0; outs < 32; ++outs)
            for (int wt = 0; wt < 2; ++wt) {
                Heap<double> sat((size_t)E * K * 4, outs & 1), resid((size_t)E * K, outs & 2), sel((size_t)E * K, outs & 4), w((size_t)E * K, wt),
                    trial((size_t)E * K, outs & 16);
                Heap<uint8_t> used((size_t)E * K, outs & 8);
                for (double &v : w.v) v = 1.0 + 0.5 * u(rng);
                std::vector<gat_fix> fixes((size_t)E);
                std::vector<gat_fix_integrity> integ((size_t)E);
                static RaimPlan p;
                const Refusal r = raim_plan(RaimCall{FixCall{ephs.data(), tx_ms.data(), tx_frac.data(), rx_ms.data(), rx_frac.data(), E, K, &cfg, fixes.data()},
                                                     &rc, integ.data()},
                                            &p);
                CHECK(r.code == GAT_OK, "twin call refused");
                raim_host_run(p, ephs.data(), tx_ms.data(), tx_frac.data(), rx_ms.data(), rx_frac.data(), w.ptr(), fixes.data(), integ.data(), sat.ptr(),
                              resid.ptr(), sel.ptr(), used.ptr(), trial.ptr());
                ++calls;
                for (int e = 0; e < E; ++e) {
                    const gat_fix &f = fixes[(size_t)e];
                    const gat_fix_integrity &g = integ[(size_t)e];
                    const double *x = &truth[(size_t)e * 4];
                    const double err = std::sqrt((f.x - x[0]) * (f.x - x[0]) + (f.y - x[1]) * (f.y - x[1]) + (f.z - x[2]) * (f.z - x[2]));
                    const bool repaired = (e == 1 || e == 5) && seen[(size_t)e] >= 7;
                    if (e == 2) {
                        CHECK(g.status == GAT_RAIM_NOT_CHECKED && f.status == GAT_FIX_FEW_SATS && g.num_excluded == 0, "epoch 2: %d %d", g.status, f.status);
                    } else if (e == 4 && seen[4] == 4) {
                        CHECK(g.status == GAT_RAIM_NO_REDUNDANCY && g.dof == 0 && f.num_used == 4, "epoch 4: status %d", g.status);
                    } else if (e == 3 && seen[3] == 5 && f.num_used == 5) { // the mask at the moved state may take one of the five
                        CHECK(g.status == (GAT_RAIM_DETECTED | GAT_RAIM_UNRESOLVED) && g.dof == 1 && g.num_excluded == 0 && err > 1e3, "epoch 3: status %d", g.status);
                    } else if (e == 0 && seen[0] >= 6) {
                        CHECK(g.status == 0 && g.stat == g.stat0 && g.stat < 1e-3 && err < 1e-3, "epoch 0: status %d T %g", g.status, g.stat);
                    } else if (repaired) {
                        CHECK(g.status == (GAT_RAIM_DETECTED | GAT_RAIM_EXCLUDED) && g.num_excluded == 1 && g.excluded[0] == moved[(size_t)e] && g.excluded[1] == -1,
                              "epoch %d: status %d, %d left out (%d moved)", e, g.status, g.excluded[0], moved[(size_t)e]);
                        CHECK((f.status & GAT_FIX_EXCLUDED) && err < 1e-3 && g.stat < 1e-3 && g.stat0 > 1e9, "epoch %d: %g m off, T %g -> %g", e, err, g.stat0, g.stat);
                        if (used.on) CHECK(used.v[(size_t)e * K + moved[(size_t)e]] == 0, "epoch %d: the channel left out is used", e);
                    }
                    if (!(f.status & GAT_FIX_EXCLUDED)) CHECK(g.num_excluded == 0 && g.excluded[0] == -1 && g.stat == g.stat0, "epoch %d: record", e);
                    // the round as the kernel walks it, against the twin's first-round trials and its choice
                    if (trial.on && outs == 31 && (g.status & GAT_RAIM_DETECTED)) {
                        FixHostEpoch h;
                        const size_t o = (size_t)e * K;
                        h.init(p.fix, ephs.data(), &tx_ms[o], &tx_frac[o], rx_ms[(size_t)e], rx_frac[(size_t)e], wt ? &w.v[o] : nullptr);
                        h.solve();
                        if (h.num_used < 6) continue;
                        double T[kFixWave];
                        const int pick = wave_round(h, p.trial_iter, p.fix.tol_m, T);
                        ++*rounds;
                        for (int k = 0; k < K; ++k) CHECK(std::memcmp(&T[k], &trial.v[o + k], sizeof(double)) == 0, "epoch %d: T_%d %a, the twin %a", e, k, T[k], trial.v[o + k]);
                        if (g.num_excluded) CHECK(pick == g.excluded[0], "epoch %d: the wave chooses %d, the twin %d", e, pick, g.excluded[0]);
                    }
                }
            }
    }
    return calls;
}

// Orbits that are usable by the letter and garbage by their numbers (gat.h, "sincos"): sqrt_a of 2^-19, 0.004 and 0.0086 put the mean
// anomaly at 1e28, 1e18 and 1e17 rad, where the quadrant's q passes 2^63 and 2^53, and a transmit time of 1e19 s.  The twin must run
// through them with every operation defined -- the sanitizers' business, float-cast-overflow among them -- and write finite numbers.
void garbage_orbits(std::mt19937_64 &rng)
{
    const int K = 10, E = 2;
    std::vector<gat_ephemeris> ephs = constellation(rng, K);
    std::vector<int32_t> tx_ms((size_t)E * K), rx_ms((size_t)E);
    std::vector<double> tx_frac((size_t)E * K), rx_frac((size_t)E);
    for (int e = 0; e < E; ++e) {
        const double x[3] = {6371e3 * std::cos(0.8 + e), 6371e3 * std::sin(0.8 + e), 0.0};
        rx_ms[(size_t)e] = 208800000 + 1000 * e, rx_frac[(size_t)e] = 2e-4;
        for (int k = 0; k < K; ++k) {
            const size_t o = (size_t)e * K + k;
            if (!measure(ephs[(size_t)k], x, rx_ms[(size_t)e], rx_frac[(size_t)e], 1e-4, &tx_ms[o], &tx_frac[o])) tx_ms[o] = rx_ms[(size_t)e] - 70, tx_frac[o] = 5e-4;
        }
    }
    ephs[0].sqrt_a = 0x1p-19, ephs[1].sqrt_a = 0.004, ephs[2].sqrt_a = 0.0086;
    tx_frac[3] = 1e19;
    const gat_fix_config cfg = fix_cfg(12, 1e-6, -1.0);
    gat_raim_config rc = raim_cfg(4, 8);
    for (int d = 1; d < kRaimThresholds; ++d) rc.threshold[d] = 1e-300; // every checked epoch is detected and runs its rounds
    std::vector<double> sat((size_t)E * K * 4), resid((size_t)E * K), sel((size_t)E * K), trial((size_t)E * K);
    std::vector<uint8_t> used((size_t)E * K);
    std::vector<gat_fix> fixes((size_t)E);
    std::vector<gat_fix_integrity> integ((size_t)E);
    static RaimPlan p;
    const Refusal r = raim_plan(RaimCall{FixCall{ephs.data(), tx_ms.data(), tx_frac.data(), rx_ms.data(), rx_frac.data(), E, K, &cfg, fixes.data()}, &rc, integ.data()},
                                &p);
    CHECK(r.code == GAT_OK, "garbage orbits: refused");
    raim_host_run(p, ephs.data(), tx_ms.data(), tx_frac.data(), rx_ms.data(), rx_frac.data(), nullptr, fixes.data(), integ.data(), sat.data(), resid.data(),
                  sel.data(), used.data(), trial.data());
    for (int e = 0; e < E; ++e) CHECK(fixes[(size_t)e].num_valid >= K - 1, "garbage orbits: epoch %d counts %d channels", e, fixes[(size_t)e].num_valid);
    for (double v : sat) CHECK(std::isfinite(v), "garbage orbits: a state that is not finite was written");
    CHECK(sat[4] != 0.0 && sat[8] != 0.0 && sat[12] != 0.0, "garbage orbits: sqrt_a = 0.004 and 0.0086 and t_sv = 1e19 s count");
}

} // namespace

int main()
{
    std::mt19937_64 rng(20261021);
    refusals();
    const int planned = plans(rng, 3000);
    int rounds = 0;
    const int calls = twins(rng, 6, &rounds);
    garbage_orbits(rng);
    std::printf("planned %d calls, ran the twin %d times, walked %d rounds, %d failures\n", planned, calls, rounds, failures);
    return failures || rounds < 12 ? 1 : 0;
}
