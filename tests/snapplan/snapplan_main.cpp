// Stand-alone check of the snapshot fix's pure plan (csrc/gat_snap_plan.h) and of the host twin's loops over it (snap_host_run, the
// rules of csrc/gat_fix.h, csrc/gat_vel.h and csrc/gat_snap.h).  Every documented refusal must return its code with nothing planned;
// random plans must cover every (epoch, channel) exactly once.  The twin then runs on heap buffers of exactly the extents the call
// describes -- every subset of the optional outputs, with and without prior_xyz and weights -- so that AddressSanitizer sees any
// access outside them, and must find the receivers and the whole milliseconds.  An epoch is walked the way the kernel runs it -- 64
// lanes in step, the reference channel from four rows of the wave's buffer, every lane's terms through the buffer, lane q adding row
// q in channel order, a lane solving from the sums -- and must give the twin's record and outputs to the bit.  Last, hostile
// entries: NaN, the infinities and values outside [0, 1e-3) in code_frac, in the weights, in the prior and in the ephemeris, a prior
// at the Earth's centre and one on a satellite; everything must stay defined (the sanitizers' business, float-cast-overflow among
// them) and no epoch may touch another.  Built with -fsanitize=address,undefined,float-cast-overflow by
// tests/test_snapshot_plan_host.py.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "gat_snap_plan.h"

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

gat_snap_config snap_cfg(double tol = 1e-6, int max_iter = 12)
{
    gat_snap_config c{};
    c.struct_size = sizeof(gat_snap_config);
    c.max_iter = max_iter, c.tol_m = tol, c.mask_sin = -1.0, c.ambiguity_margin = 0.1;
    return c;
}
SnapCall call(int E, int K, const gat_snap_config *cfg) { return SnapCall{kGiven, kGiven, kGiven, kGiven, E, K, cfg, kGiven}; }

void expect_refusal(const SnapCall &a, int code, const char *what)
{
    SnapPlan p, q;
    std::memset(&p, 0x5a, sizeof p);
    std::memset(&q, 0x5a, sizeof q);
    const Refusal r = snap_plan(a, &p);
    CHECK(r.code == code, "%s: got %d, want %d", what, r.code, code);
    CHECK(std::memcmp(&p, &q, sizeof p) == 0, "%s: the plan was written", what);
}

void refusals()
{
    const gat_snap_config good = snap_cfg();
    SnapCall a = call(3, 6, &good);
    const void **ptrs[] = {&a.eph, &a.code_frac, &a.rx_ms, &a.rx_frac, &a.fixes};
    for (const void **p : ptrs) {
        *p = nullptr;
        expect_refusal(a, GAT_ERR_ARG, "null pointer");
        *p = kGiven;
    }
    expect_refusal(call(3, 6, nullptr), GAT_ERR_ARG, "null config");
    gat_snap_config c = good;
    c.struct_size += 8;
    expect_refusal(call(3, 6, &c), GAT_ERR_ARG, "struct_size");
    c = good, c.flags = 1;
    expect_refusal(call(3, 6, &c), GAT_ERR_ARG, "flags");
    c = good, c.reserved = 1;
    expect_refusal(call(3, 6, &c), GAT_ERR_ARG, "reserved");
    c = good, c.max_iter = 0;
    expect_refusal(call(3, 6, &c), GAT_ERR_ARG, "max_iter");
    const double bad_tol[] = {kNaN, 0.0, -0.0, -1.0, -kInf};
    for (double v : bad_tol) {
        c = good, c.tol_m = v;
        expect_refusal(call(3, 6, &c), GAT_ERR_ARG, "tol_m");
    }
    const double not_finite[] = {kNaN, kInf, -kInf};
    for (double v : not_finite) {
        c = good, c.mask_sin = v;
        expect_refusal(call(3, 6, &c), GAT_ERR_ARG, "mask_sin");
        for (int i = 0; i < 3; ++i) {
            c = good, c.init_xyz[i] = v;
            expect_refusal(call(3, 6, &c), GAT_ERR_ARG, "init_xyz");
        }
    }
    const double bad_margin[] = {kNaN, kInf, -kInf, -1e-300, std::nextafter(0.5, 1.0)};
    for (double v : bad_margin) {
        c = good, c.ambiguity_margin = v;
        expect_refusal(call(3, 6, &c), GAT_ERR_ARG, "ambiguity_margin");
    }
    expect_refusal(call(0, 6, &good), GAT_ERR_ARG, "E = 0");
    expect_refusal(call(3, 0, &good), GAT_ERR_ARG, "K = 0");
    expect_refusal(call(-1, 6, &good), GAT_ERR_ARG, "E = -1");
    expect_refusal(call(3, GAT_MAX_FIX_CHANNELS + 1, &good), GAT_ERR_RANGE, "K = 65");
    expect_refusal(call(GAT_MAX_FIX_EPOCHS + 1, 6, &good), GAT_ERR_RANGE, "E = 2^24 + 1");
    CHECK(snap_plan(call(3, 6, &good), nullptr).code == GAT_ERR_ARG, "null plan");
    SnapPlan p{};
    for (double v : {0.0, -0.0, 0.5}) {
        c = good, c.ambiguity_margin = v;
        CHECK(snap_plan(call(3, 6, &c), &p).code == GAT_OK && p.margin == v, "margin %g refused", v);
    }
}

int plans(std::mt19937_64 &rng, int count)
{
    const gat_snap_config cfg = snap_cfg();
    for (int n = 0; n < count; ++n) {
        const bool small = n < 40 || n % 8 == 0;
        const int E = n < 40 ? n + 1 : (small ? 1 + (int)(rng() % 3000) : 1 + (int)(rng() % GAT_MAX_FIX_EPOCHS));
        const int K = 1 + (int)(rng() % GAT_MAX_FIX_CHANNELS);
        SnapPlan p{};
        CHECK(snap_plan(call(E, K, &cfg), &p).code == GAT_OK, "E %d K %d refused", E, K);
        CHECK(p.E == E && p.K == K && p.groups == ((long long)E + kFixWaves - 1) / kFixWaves && p.margin == 0.1 && p.max_iter == 12, "geometry");
        gat_fix_plan rep{};
        snap_report(p, &rep);
        CHECK(rep.workgroups == p.groups && rep.threads == kFixThreads && rep.waves_per_workgroup == kFixWaves && rep.scratch_bytes == 0 &&
                  rep.lds_bytes == kSnapLdsBytes && rep.lds_bytes <= 160 * 1024 && kSnapWaveDoubles >= kSnapSumsAt + kSnapTerms &&
                  kSnapSumsAt >= 4 * kSnapPitch,
              "report");
        if (small) {
            std::vector<uint8_t> hit((size_t)E * K, 0);
            for (long long g = 0; g < p.groups; ++g)
                for (int w = 0; w < kFixWaves; ++w) {
                    int e;
                    if (!fix_epoch_unit(g, w, E, &e)) continue;
                    for (int lane = 0; lane < kFixWave; ++lane)
                        if (lane < K) hit[(size_t)e * K + lane] += 1;
                }
            for (uint8_t h : hit) CHECK(h == 1, "E %d K %d: a cell is covered %d times", E, K, h);
        } else {
            int e = -1;
            CHECK(fix_epoch_unit(p.groups - 1, (E - 1) % kFixWaves, E, &e) && e == E - 1, "the last epoch");
            CHECK(!fix_epoch_unit(p.groups, 0, E, &e), "a unit past the last");
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
        g.af0 = 2e-4 * u(rng), g.af1 = 3e-12 * u(rng), g.af2 = 1e-17 * u(rng), g.tgd = 8e-9 * u(rng);
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

// the transmit time by the satellite's own clock of what a receiver at xyz receives at the GPS time t_rx; *sin_el of the satellite
double transmit_time(const gat_ephemeris &g, const double *xyz, double t_rx, double *sin_el)
{
    double tau = 0.075, d[3] = {0, 0, 0};
    for (int it = 0; it < 8; ++it) {
        double X, Y, Z, c, s;
        fix_orbit(g, t_rx - tau, &X, &Y, &Z);
        fix_sincos(kFixOmegaE * tau, &c, &s);
        d[0] = c * X + s * Y - xyz[0], d[1] = c * Y - s * X - xyz[1], d[2] = Z - xyz[2];
        tau = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]) / kFixC;
    }
    *sin_el = (d[0] * xyz[0] + d[1] * xyz[1] + d[2] * xyz[2]) / (kFixC * tau * fix_radius(xyz));
    double dts = 0.0;
    for (int it = 0; it < 4; ++it) dts = fix_clock(g, t_rx - tau + dts);
    return t_rx - tau + dts;
}

template <class T>
struct Heap { // a buffer of exactly n elements, null when not asked for
    std::vector<T> v;
    bool on;
    Heap(size_t n, bool on_, T fill = T()) : v(on_ ? n : 0, fill), on(on_) {}
    T *ptr() { return on ? v.data() : nullptr; }
};

struct Scene {
    int E, K;
    std::vector<gat_ephemeris> ephs;
    std::vector<double> code_frac, rx_frac, prior, truth, weights; // truth [E][3]
    std::vector<int32_t> rx_ms, tx_ms;                              // tx_ms: the whole milliseconds a decoded time of week would give
    std::vector<int> seen;
};

// receivers on the ground whose clocks are up to 20 s and a fraction of a millisecond off, priors up to 30 km from them
Scene scene(std::mt19937_64 &rng, int E, int K)
{
    std::uniform_real_distribution<double> u(-1.0, 1.0);
    Scene s;
    s.E = E, s.K = K, s.ephs = constellation(rng, K);
    s.code_frac.assign((size_t)E * K, kNaN), s.tx_ms.assign((size_t)E * K, -1), s.weights.assign((size_t)E * K, 1.0);
    s.rx_frac.assign((size_t)E, 0.0), s.rx_ms.assign((size_t)E, 0), s.prior.assign((size_t)E * 3, 0.0), s.truth.assign((size_t)E * 3, 0.0);
    s.seen.assign((size_t)E, 0);
    for (int e = 0; e < E; ++e) {
        const double lat = 1.4 * u(rng), lon = 3.1 * u(rng), r = 6371e3 + 1000.0 * u(rng);
        double *x = &s.truth[(size_t)e * 3];
        x[0] = r * std::cos(lat) * std::cos(lon), x[1] = r * std::cos(lat) * std::sin(lon), x[2] = r * std::sin(lat);
        double dir[3] = {u(rng), u(rng), u(rng)};
        const double len = std::sqrt(dir[0] * dir[0] + dir[1] * dir[1] + dir[2] * dir[2]) + 1e-9, far = 30.0e3 * std::fabs(u(rng));
        for (int i = 0; i < 3; ++i) s.prior[(size_t)e * 3 + i] = x[i] + dir[i] / len * far;
        const int32_t ms = 208800000 + (int32_t)(3.0e6 * u(rng));
        const double frac = 0.0005 + 0.00049 * u(rng), bias = 3e-4 * u(rng); // the clock reads (ms, frac) and is `bias` ahead
        const double t_rx = (double)ms * 1e-3 + frac - bias;
        const int32_t off = (int32_t)(20000.0 * u(rng));
        s.rx_ms[(size_t)e] = ms + off, s.rx_frac[(size_t)e] = frac;
        for (int k = 0; k < K; ++k) {
            const size_t o = (size_t)e * K + k;
            double sel;
            const double t_sv = transmit_time(s.ephs[(size_t)k], x, t_rx, &sel);
            s.weights[o] = 1.0 + 0.5 * u(rng);
            if (!(sel > 0.09)) continue;
            const double m = std::floor(t_sv * 1e3);
            double f = t_sv - m * 1e-3;
            if (f < 0) f = 0;
            if (f >= 1e-3) f = std::nextafter(1e-3, 0.0);
            s.code_frac[o] = f, s.tx_ms[o] = (int32_t)m, s.seen[(size_t)e] += 1;
        }
    }
    return s;
}

struct Outputs {
    Heap<gat_snap_fix> fixes;
    Heap<int32_t> tx_ms, rx_ms_out, n_ms;
    Heap<double> resid, sin_el;
    Heap<uint8_t> used;
    Outputs(int E, int K, unsigned mask)
        : fixes((size_t)E, true), tx_ms((size_t)E * K, mask & 1, 77), rx_ms_out((size_t)E, mask & 2, 77), n_ms((size_t)E * K, mask & 4, 77),
          resid((size_t)E * K, mask & 8, kNaN), sin_el((size_t)E * K, mask & 16, kNaN), used((size_t)E * K, mask & 32, 77)
    {
    }
};

void run(const SnapPlan &p, const Scene &s, bool prior, bool weights, Outputs &o)
{
    // the inputs too on buffers of their exact extents
    std::vector<gat_ephemeris> eph(s.ephs);
    std::vector<double> frac(s.code_frac), rf(s.rx_frac), pr(s.prior), w(s.weights);
    std::vector<int32_t> ms(s.rx_ms);
    snap_host_run(p, eph.data(), frac.data(), ms.data(), rf.data(), prior ? pr.data() : nullptr, weights ? w.data() : nullptr, o.fixes.ptr(), o.tx_ms.ptr(),
                  o.rx_ms_out.ptr(), o.n_ms.ptr(), o.resid.ptr(), o.sin_el.ptr(), o.used.ptr());
}

void twin(std::mt19937_64 &rng)
{
    const int E = 6, K = 32;
    const Scene s = scene(rng, E, K);
    gat_snap_config cfg = snap_cfg();
    SnapPlan p{};
    CHECK(snap_plan(call(E, K, &cfg), &p).code == GAT_OK, "plan");
    Outputs all(E, K, 63);
    run(p, s, true, false, all);
    for (int e = 0; e < E; ++e) {
        const gat_snap_fix &f = all.fixes.v[(size_t)e];
        const double *x = &s.truth[(size_t)e * 3];
        const double err = std::sqrt((f.x - x[0]) * (f.x - x[0]) + (f.y - x[1]) * (f.y - x[1]) + (f.z - x[2]) * (f.z - x[2]));
        CHECK(s.seen[(size_t)e] >= 6, "epoch %d sees %d", e, s.seen[(size_t)e]);
        // the scene's own rounding: a transmit time held in seconds of the week, three operations at half an ulp of 2.1e5 s = 1.5e-11 s
        // each, is 1.3e-2 m of range, times a dilution of up to 4
        CHECK(f.status == 0 && f.num_used == s.seen[(size_t)e] && err < 0.05, "epoch %d: status %d, used %d of %d, %g m off", e, f.status, f.num_used,
              s.seen[(size_t)e], err);
        for (int k = 0; k < K; ++k) CHECK(all.tx_ms.v[(size_t)e * K + k] == s.tx_ms[(size_t)e * K + k], "epoch %d channel %d: tx_ms", e, k);
    }
    // every subset of the optional outputs, with and without the prior (then init_xyz: the first epoch's) and the weights
    for (int i = 0; i < 3; ++i) cfg.init_xyz[i] = s.prior[(size_t)i];
    CHECK(snap_plan(call(E, K, &cfg), &p).code == GAT_OK, "plan");
    for (int pw = 0; pw < 4; ++pw) {
        Outputs full(E, K, 63);
        run(p, s, pw & 1, pw & 2, full);
        for (unsigned mask = 0; mask < 64; ++mask) {
            Outputs o(E, K, mask);
            run(p, s, pw & 1, pw & 2, o);
            CHECK(std::memcmp(o.fixes.v.data(), full.fixes.v.data(), sizeof(gat_snap_fix) * E) == 0, "subset %u: the records differ", mask);
            CHECK(!o.tx_ms.on || o.tx_ms.v == full.tx_ms.v, "subset %u: tx_ms", mask);
            CHECK(!o.rx_ms_out.on || o.rx_ms_out.v == full.rx_ms_out.v, "subset %u: rx_ms_out", mask);
            CHECK(!o.n_ms.on || o.n_ms.v == full.n_ms.v, "subset %u: n_ms", mask);
            CHECK(!o.resid.on || std::memcmp(o.resid.v.data(), full.resid.v.data(), sizeof(double) * E * K) == 0, "subset %u: resid", mask);
            CHECK(!o.sin_el.on || std::memcmp(o.sin_el.v.data(), full.sin_el.v.data(), sizeof(double) * E * K) == 0, "subset %u: sin_el", mask);
            CHECK(!o.used.on || o.used.v == full.used.v, "subset %u: used", mask);
        }
        if (pw & 1) CHECK(full.fixes.v[0].status == 0, "prior and weights %d", pw);
    }
}

// What the kernel does with an epoch, lane by lane in step.  The wave's buffer has the kernel's layout; lanes >= K write nothing.
struct Wave {
    const SnapPlan &p;
    const gat_ephemeris *eph;
    int32_t rx_ms;
    double R;
    std::vector<double> buf;
    std::vector<SnapChan> c;
    double st[kSnapUnknowns], last_step;
    int status, iterations, num_valid, num_used;

    Wave(const SnapPlan &p_, const gat_ephemeris *eph_, const double *frac, int32_t rx_ms_, double rx_frac, const double *xyz, const double *w)
        : p(p_), eph(eph_), rx_ms(rx_ms_), R(fix_seconds(rx_ms_, rx_frac)), buf((size_t)kSnapWaveDoubles, kNaN), c((size_t)kFixWave)
    {
        for (int lane = 0; lane < kFixWave; ++lane) {
            const int k = lane < p.K ? lane : 0;
            c[(size_t)lane] = snap_measure(eph[k], frac[k], rx_ms, rx_frac, w ? w[k] : 1.0);
            c[(size_t)lane].ok = c[(size_t)lane].ok && lane < p.K;
        }
        st[0] = xyz[0], st[1] = xyz[1], st[2] = xyz[2], st[3] = 0.0, st[4] = 0.0;
        status = 0, iterations = 0, num_valid = 0, num_used = 0, last_step = 0.0;
    }
    const gat_ephemeris &g(int lane) const { return eph[lane < p.K ? lane : 0]; }
    void sums(const std::vector<double> &t, int n, double *out) // t [lane][kSnapTerms]
    {
        for (int lane = 0; lane < p.K; ++lane)
            for (int q = 0; q < n; ++q) buf[(size_t)(q * kSnapPitch + lane)] = t[(size_t)lane * kSnapTerms + q];
        for (int lane = 0; lane < n; ++lane) {
            double s = 0.0;
            for (int k = 0; k < p.K; ++k) s += buf[(size_t)(lane * kSnapPitch + k)];
            buf[(size_t)(kSnapSumsAt + lane)] = s;
        }
        for (int q = 0; q < n; ++q) out[q] = buf[(size_t)(kSnapSumsAt + q)];
    }
    bool resolve(bool first)
    {
        const double radius = fix_radius(st);
        for (int lane = 0; lane < kFixWave; ++lane) {
            SnapChan &l = c[(size_t)lane];
            if (l.ok) snap_predict(l, g(lane), R, st, radius);
            if (first) {
                l.ok = l.ok && snap_predicted(l);
                l.used = l.ok && fix_weight_ok(l.w);
                num_valid += l.ok, num_used += l.used;
            }
        }
        if (num_used < kSnapMinSats) {
            status |= GAT_SNAP_FEW_SATS;
            return false;
        }
        for (int lane = 0; lane < p.K; ++lane) {
            const SnapChan &l = c[(size_t)lane];
            buf[(size_t)lane] = l.used ? 1.0 : 0.0, buf[(size_t)(kSnapPitch + lane)] = l.sel, buf[(size_t)(2 * kSnapPitch + lane)] = l.p;
            buf[(size_t)(3 * kSnapPitch + lane)] = l.z;
        }
        const SnapRef r = snap_reference(buf.data(), kSnapPitch, p.K);
        double n[kFixWave] = {};
        bool bad = false, changed = false;
        for (int lane = 0; lane < kFixWave; ++lane) {
            bool good = r.good;
            if (good && c[(size_t)lane].ok) good = snap_integer(c[(size_t)lane], r, &n[lane]);
            bad = bad || !good;
        }
        if (bad) {
            status |= GAT_SNAP_NONFINITE;
            return false;
        }
        for (int lane = 0; lane < kFixWave; ++lane) {
            SnapChan &l = c[(size_t)lane];
            if (l.used && snap_ambiguous(l.q, n[lane], p.margin)) status |= GAT_SNAP_AMBIGUOUS;
            changed = changed || (l.used && (int)n[lane] != l.n);
            if (l.ok) l.n = (int)n[lane];
        }
        return changed;
    }
    void rows()
    {
        for (int lane = 0; lane < kFixWave; ++lane)
            if (c[(size_t)lane].ok) snap_eval(c[(size_t)lane], g(lane), rx_ms, st);
    }
    bool pass()
    {
        for (int it = 0; it < p.max_iter; ++it) {
            rows();
            std::vector<double> t((size_t)kFixWave * kSnapTerms, 0.0);
            for (int lane = 0; lane < kFixWave; ++lane) {
                snap_terms(c[(size_t)lane], c[(size_t)lane].w, &t[(size_t)lane * kSnapTerms]);
                for (int q = 0; q < kSnapTerms; ++q) t[(size_t)lane * kSnapTerms + q] = c[(size_t)lane].used ? t[(size_t)lane * kSnapTerms + q] : 0.0;
            }
            double s[kSnapTerms], d[kSnapUnknowns];
            sums(t, kSnapTerms, s);
            const int rc = snap_step(s, d);
            if (rc) {
                status |= rc;
                return false;
            }
            for (int i = 0; i < kSnapUnknowns; ++i) st[i] += d[i];
            last_step = __builtin_sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
            iterations += 1;
            if (last_step < p.tol_m) return true;
        }
        status |= GAT_SNAP_NOT_CONVERGED;
        return false;
    }
    double elevations()
    {
        rows();
        const double radius = fix_radius(st);
        for (int lane = 0; lane < kFixWave; ++lane) c[(size_t)lane].sel = c[(size_t)lane].ok ? fix_sin_el(c[(size_t)lane].row, st, radius) : 0.0;
        return radius;
    }
    void solve()
    {
        resolve(true);
        if (snap_failed(status)) return;
        bool converged = pass();
        if (snap_failed(status)) return;
        if (converged) {
            const bool changed = resolve(false);
            if (snap_failed(status)) return;
            if (changed) {
                status |= GAT_SNAP_RERESOLVED;
                converged = pass();
                if (snap_failed(status)) return;
            }
        }
        const double radius = elevations();
        if (converged && p.mask_sin > -1.0 && radius >= kFixMaskRadius) {
            int kept = 0;
            for (int lane = 0; lane < kFixWave; ++lane) kept += c[(size_t)lane].used && c[(size_t)lane].sel >= p.mask_sin;
            if (kept != num_used) {
                if (kept >= kSnapMinSats) {
                    for (int lane = 0; lane < kFixWave; ++lane) c[(size_t)lane].used = c[(size_t)lane].used && c[(size_t)lane].sel >= p.mask_sin;
                    num_used = kept;
                    status |= GAT_SNAP_MASKED;
                    pass();
                    if (!snap_failed(status)) elevations();
                } else
                    status |= GAT_SNAP_MASK_STARVED;
            }
        }
    }
    gat_snap_fix record(int32_t *tx_ms, int32_t *rx_ms_out, int32_t *n_ms, double *resid, double *sin_el, uint8_t *used)
    {
        const bool failed = snap_failed(status);
        double s[kSnapTerms] = {};
        if (!failed) {
            std::vector<double> t((size_t)kFixWave * kSnapTerms, 0.0);
            for (int lane = 0; lane < kFixWave; ++lane) {
                double *tl = &t[(size_t)lane * kSnapTerms];
                snap_terms(c[(size_t)lane], 1.0, tl);
                tl[15] = c[(size_t)lane].row.v * c[(size_t)lane].row.v;
                for (int q = 0; q < 16; ++q) tl[q] = c[(size_t)lane].used ? tl[q] : 0.0;
            }
            sums(t, 16, s);
        }
        const int64_t m = snap_shift_ms(st[4]);
        *rx_ms_out = failed ? -1 : snap_week_ms((int64_t)rx_ms - m);
        for (int lane = 0; lane < p.K; ++lane) {
            const SnapChan &l = c[(size_t)lane];
            const bool has = !failed && l.ok;
            tx_ms[lane] = has ? snap_tx_ms(rx_ms, l, m) : -1, n_ms[lane] = has ? l.n : 0;
            resid[lane] = has ? l.row.v : 0.0, sin_el[lane] = has ? l.sel : 0.0, used[lane] = (uint8_t)(!failed && l.used ? 1 : 0);
        }
        return snap_record(status, num_valid, num_used, iterations, st, s[15], last_step, s);
    }
};

bool same_bits(const double *a, const double *b, size_t n) { return std::memcmp(a, b, n * sizeof(double)) == 0; }

// the twin and the wave walk on one call; returns the twin's records.  `hostile` scenes need not fix, only agree.
std::vector<gat_snap_fix> compare(const Scene &s, const gat_snap_config &cfg, bool prior, bool weights, const char *what)
{
    const int E = s.E, K = s.K;
    SnapPlan p{};
    CHECK(snap_plan(call(E, K, &cfg), &p).code == GAT_OK, "%s: plan", what);
    Outputs o(E, K, 63);
    run(p, s, prior, weights, o);
    for (int e = 0; e < E; ++e) {
        const size_t at = (size_t)e * K;
        Wave wv(p, s.ephs.data(), &s.code_frac[at], s.rx_ms[(size_t)e], s.rx_frac[(size_t)e], prior ? &s.prior[(size_t)e * 3] : p.init_xyz,
                weights ? &s.weights[at] : nullptr);
        wv.solve();
        std::vector<int32_t> tx((size_t)K), nm((size_t)K);
        std::vector<double> rs((size_t)K), se((size_t)K);
        std::vector<uint8_t> us((size_t)K);
        int32_t rxo = 0;
        const gat_snap_fix f = wv.record(tx.data(), &rxo, nm.data(), rs.data(), se.data(), us.data());
        CHECK(std::memcmp(&f, &o.fixes.v[(size_t)e], sizeof f) == 0, "%s: epoch %d: the wave's record differs (status %d / %d)", what, e, f.status,
              o.fixes.v[(size_t)e].status);
        CHECK(rxo == o.rx_ms_out.v[(size_t)e] && std::memcmp(tx.data(), &o.tx_ms.v[at], K * sizeof(int32_t)) == 0 &&
                  std::memcmp(nm.data(), &o.n_ms.v[at], K * sizeof(int32_t)) == 0 && std::memcmp(us.data(), &o.used.v[at], (size_t)K) == 0,
              "%s: epoch %d: the wave's integers differ", what, e);
        CHECK(same_bits(rs.data(), &o.resid.v[at], (size_t)K) && same_bits(se.data(), &o.sin_el.v[at], (size_t)K), "%s: epoch %d: the wave's reals differ", what, e);
    }
    return o.fixes.v;
}

void walk(std::mt19937_64 &rng)
{
    for (int K : {1, 4, 5, 6, 24, 63, 64}) {
        Scene s = scene(rng, 3, K);
        gat_snap_config cfg = snap_cfg();
        compare(s, cfg, true, false, "walk");
        cfg.mask_sin = 0.3;
        const std::vector<gat_snap_fix> f = compare(s, cfg, true, true, "walk, mask and weights");
        if (K >= 24) CHECK(!snap_failed(f[0].status) && !(f[0].status & GAT_SNAP_NOT_CONVERGED), "K %d: status %d", K, f[0].status);
        if (K < 5) CHECK(f[0].status == GAT_SNAP_FEW_SATS && f[0].x == 0.0, "K %d: status %d", K, f[0].status);
    }
}

void hostile(std::mt19937_64 &rng)
{
    const int E = 8, K = 16;
    const Scene calm = scene(rng, E, K);
    gat_snap_config cfg = snap_cfg(1e-4, 10);
    const std::vector<gat_snap_fix> want = compare(calm, cfg, true, true, "calm");
    Scene s = calm;
    const size_t e1 = 1 * (size_t)K, e3 = 3 * (size_t)K, e5 = 5 * (size_t)K;
    const double fracs[] = {kNaN, kInf, -kInf, 1e-3, -5e-324, 1e300, -0.0};
    for (size_t i = 0; i < sizeof fracs / sizeof *fracs; ++i) s.code_frac[e1 + i] = fracs[i];
    const double ws[] = {kNaN, kInf, -kInf, 0.0, -0.0, -1.0, 5e-324, 1e300};
    for (size_t i = 0; i < sizeof ws / sizeof *ws; ++i) s.weights[e3 + i] = ws[i];
    s.prior[5 * 3] = 0.0, s.prior[5 * 3 + 1] = 0.0, s.prior[5 * 3 + 2] = 0.0; // the Earth's centre
    (void)e5;
    s.prior[6 * 3] = kNaN;
    s.rx_frac[7] = kInf;
    const std::vector<gat_snap_fix> got = compare(s, cfg, true, true, "hostile entries");
    for (int e : {0, 2, 4}) CHECK(std::memcmp(&got[(size_t)e], &want[(size_t)e], sizeof(gat_snap_fix)) == 0, "epoch %d was touched", e);
    CHECK(got[6].status == GAT_SNAP_FEW_SATS && got[7].status == GAT_SNAP_FEW_SATS, "NaN prior %d, infinite reception %d", got[6].status, got[7].status);
    // hostile ephemerides and priors: a prior on a satellite, absurd orbits; the rx clock at the ends of its type
    Scene t = calm;
    t.ephs[0].sqrt_a = 5e-324, t.ephs[1].sqrt_a = 0.004, t.ephs[2].sqrt_a = 1e200, t.ephs[3].e = 0.4999, t.ephs[4].af0 = kNaN, t.ephs[5].m0 = kInf;
    t.ephs[6].toe = -kInf, t.ephs[7].crc = 1e308, t.ephs[8].valid = 0, t.ephs[9].e = -0.0;
    {
        double X, Y, Z;
        fix_orbit(calm.ephs[10], 208800.0, &X, &Y, &Z);
        t.prior[0] = X, t.prior[1] = Y, t.prior[2] = Z;
    }
    t.prior[3] = 1e300, t.prior[6] = -1e154, t.prior[7] = 1e154;
    t.rx_ms[3] = std::numeric_limits<int32_t>::max(), t.rx_ms[4] = 0, t.rx_ms[5] = -1, t.rx_frac[6] = 1e300, t.rx_frac[2] = -1e-3;
    compare(t, cfg, true, false, "hostile ephemerides");
    cfg.mask_sin = 0.2, cfg.ambiguity_margin = 0.5, cfg.max_iter = 2;
    compare(t, cfg, true, true, "hostile ephemerides, mask");
    // a prior 200 km off: flagged, or seen in the residuals
    Scene f = calm;
    for (int e = 0; e < E; ++e) f.prior[(size_t)e * 3] = f.truth[(size_t)e * 3] + 200.0e3;
    cfg = snap_cfg();
    const std::vector<gat_snap_fix> far = compare(f, cfg, true, false, "far prior");
    for (int e = 0; e < E; ++e) {
        const double *x = &f.truth[(size_t)e * 3];
        const double err = std::sqrt((far[(size_t)e].x - x[0]) * (far[(size_t)e].x - x[0]) + (far[(size_t)e].y - x[1]) * (far[(size_t)e].y - x[1]) +
                                     (far[(size_t)e].z - x[2]) * (far[(size_t)e].z - x[2]));
        // beyond the rule's condition an error of a whole code period clears the margin: with more than five channels the residual shows it
        CHECK(err < 1.0 || (far[(size_t)e].status & (GAT_SNAP_AMBIGUOUS | GAT_SNAP_RERESOLVED | GAT_SNAP_NOT_CONVERGED | 7)) != 0 ||
                  (far[(size_t)e].num_used > kSnapMinSats && far[(size_t)e].rms_residual_m > 1.0),
              "epoch %d is %g m off with status %d and an rms of %g m", e, err, far[(size_t)e].status, far[(size_t)e].rms_residual_m);
    }
}

} // namespace

int main()
{
    std::mt19937_64 rng(20261021);
    refusals();
    const int n = plans(rng, 3000);
    twin(rng);
    walk(rng);
    hostile(rng);
    std::printf("planned %d calls, the twin on exact buffers, the wave walk and the hostile entries: %d failures\n", n, failures);
    return failures ? 1 : 0;
}
