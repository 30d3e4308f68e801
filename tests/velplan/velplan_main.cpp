// Stand-alone check of the velocity fix's pure plan (csrc/gat_vel_plan.h) and of the host twin's loops over it (vel_host_run, the rules
// of csrc/gat_fix.h and csrc/gat_vel.h).  Every documented refusal must return its code with nothing planned; random plans must cover
// every (epoch, channel) exactly once.  The twin then runs on heap buffers of exactly the extents the call describes -- every subset
// of the optional outputs and of `used` and `weights`, receivers that move -- so that AddressSanitizer sees any access outside them,
// and must find the velocity.  vel_orbit's position and vel_clock's correction must have fix_orbit's and fix_clock's bits over random
// and hostile ephemerides.  An epoch is walked the way the kernel runs it -- 64 lanes in step, every lane's terms through the wave's
// buffer, lane q adding row q in channel order, every lane solving from the sums -- and must give the twin's record to the bit.
// Last, hostile entries: NaN and the infinities in doppler_hz, in the weights, in every real field of the ephemeris and in the fix's
// state, sqrt_a of 5e-324, 0.004 and 1e200, a fix at the Earth's centre and one exactly on a satellite; everything must stay defined
// (the sanitizers' business, float-cast-overflow among them) and no epoch may touch another.  Built with
// -fsanitize=address,undefined,float-cast-overflow by tests/test_velocity_plan_host.py.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "gat_vel_plan.h"

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

gat_vel_config vel_cfg(double carrier = 1575.42e6)
{
    gat_vel_config c{};
    c.struct_size = sizeof(gat_vel_config);
    c.carrier_hz = carrier;
    return c;
}
VelCall call(int E, int K, const gat_vel_config *cfg) { return VelCall{kGiven, kGiven, kGiven, kGiven, kGiven, E, K, cfg, kGiven}; }

void expect_refusal(const VelCall &a, int code, const char *what)
{
    VelPlan p, q;
    std::memset(&p, 0x5a, sizeof p);
    std::memset(&q, 0x5a, sizeof q);
    const Refusal r = vel_plan(a, &p);
    CHECK(r.code == code, "%s: got %d, want %d", what, r.code, code);
    CHECK(std::memcmp(&p, &q, sizeof p) == 0, "%s: the plan was written", what);
}

void refusals()
{
    const gat_vel_config good = vel_cfg();
    VelCall a = call(3, 6, &good);
    const void **ptrs[] = {&a.eph, &a.tx_ms, &a.tx_frac, &a.doppler, &a.fixes, &a.velocities};
    for (const void **p : ptrs) {
        *p = nullptr;
        expect_refusal(a, GAT_ERR_ARG, "null pointer");
        *p = kGiven;
    }
    expect_refusal(call(3, 6, nullptr), GAT_ERR_ARG, "null config");
    gat_vel_config c = good;
    c.struct_size += 8;
    expect_refusal(call(3, 6, &c), GAT_ERR_ARG, "struct_size");
    c = good, c.flags = 1;
    expect_refusal(call(3, 6, &c), GAT_ERR_ARG, "flags");
    const double bad[] = {kNaN, kInf, -kInf, 0.0, -0.0, -1575.42e6};
    for (double v : bad) {
        c = good, c.carrier_hz = v;
        expect_refusal(call(3, 6, &c), GAT_ERR_ARG, "carrier_hz");
    }
    expect_refusal(call(0, 6, &good), GAT_ERR_ARG, "E = 0");
    expect_refusal(call(3, 0, &good), GAT_ERR_ARG, "K = 0");
    expect_refusal(call(-1, 6, &good), GAT_ERR_ARG, "E = -1");
    expect_refusal(call(3, GAT_MAX_FIX_CHANNELS + 1, &good), GAT_ERR_RANGE, "K = 65");
    expect_refusal(call(GAT_MAX_FIX_EPOCHS + 1, 6, &good), GAT_ERR_RANGE, "E = 2^24 + 1");
    VelPlan p{};
    CHECK(vel_plan(call(3, 6, &good), nullptr).code == GAT_ERR_ARG, "null plan");
    c = good, c.carrier_hz = 5e-324; // positive and finite: a wavelength of infinity is the caller's
    CHECK(vel_plan(call(3, 6, &c), &p).code == GAT_OK && p.lambda == kInf, "a subnormal carrier refused");
}

int plans(std::mt19937_64 &rng, int count)
{
    const gat_vel_config cfg = vel_cfg();
    for (int n = 0; n < count; ++n) {
        const bool small = n < 40 || n % 8 == 0;
        const int E = n < 40 ? n + 1 : (small ? 1 + (int)(rng() % 3000) : 1 + (int)(rng() % GAT_MAX_FIX_EPOCHS));
        const int K = 1 + (int)(rng() % GAT_MAX_FIX_CHANNELS);
        VelPlan p{};
        CHECK(vel_plan(call(E, K, &cfg), &p).code == GAT_OK, "E %d K %d refused", E, K);
        CHECK(p.E == E && p.K == K && p.groups == ((long long)E + kFixWaves - 1) / kFixWaves && p.lambda == kFixC / 1575.42e6, "geometry");
        gat_fix_plan rep{};
        vel_report(p, &rep);
        CHECK(rep.workgroups == p.groups && rep.threads == kFixThreads && rep.waves_per_workgroup == kFixWaves && rep.scratch_bytes == 0 &&
                  rep.lds_bytes == kFixLdsBytes && rep.lds_bytes <= 160 * 1024,
              "report");
        // the grid's first, last and (where small) every unit: each (epoch, channel) once
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

// the range [m] a receiver at xyz sees at the GPS time t_rx, and the time of transmission by the satellite's own clock
double light_time(const gat_ephemeris &g, const double *xyz, double t_rx, double *t_sv, bool *above)
{
    double tau = 0.075, d[3] = {0, 0, 0};
    for (int it = 0; it < 8; ++it) {
        double X, Y, Z, c, s;
        fix_orbit(g, t_rx - tau, &X, &Y, &Z);
        fix_sincos(kFixOmegaE * tau, &c, &s);
        d[0] = c * X + s * Y - xyz[0], d[1] = c * Y - s * X - xyz[1], d[2] = Z - xyz[2];
        tau = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]) / kFixC;
    }
    *above = d[0] * xyz[0] + d[1] * xyz[1] + d[2] * xyz[2] > 0.0;
    double dts = 0.0;
    for (int it = 0; it < 4; ++it) dts = fix_clock(g, t_rx - tau + dts);
    *t_sv = t_rx - tau + dts;
    return kFixC * tau;
}

// What a receiver at xyz moving at v with clock drift `drift` measures at the GPS time t_rx: the transmit time (ms, frac) and the
// Doppler from the ranges a tenth of a second before and after (good to 1e-6 m/s: the difference's truncation); false: not seen.
bool measure(const gat_ephemeris &g, const double *xyz, const double *v, double drift, double t_rx, double lambda, int32_t *tx_ms, double *tx_frac,
             double *doppler)
{
    bool above, dummy;
    double t_sv, t_unused;
    light_time(g, xyz, t_rx, &t_sv, &above);
    if (!above) return false;
    const double h = 0.1;
    const double xa[3] = {xyz[0] + h * v[0], xyz[1] + h * v[1], xyz[2] + h * v[2]}, xb[3] = {xyz[0] - h * v[0], xyz[1] - h * v[1], xyz[2] - h * v[2]};
    const double rate = (light_time(g, xa, t_rx + h, &t_unused, &dummy) - light_time(g, xb, t_rx - h, &t_unused, &dummy)) / (2 * h);
    double dts, ddts;
    vel_clock(g, t_sv, &dts, &ddts);
    *doppler = -(rate + kFixC * drift - kFixC * ddts) / lambda;
    const double m = std::floor(t_sv * 1e3);
    double f = t_sv - m * 1e-3;
    if (f < 0) f = 0;
    if (f >= 1e-3) f = std::nextafter(1e-3, 0.0);
    *tx_ms = (int32_t)m, *tx_frac = f;
    return true;
}

template <class T>
struct Heap { // a buffer of exactly n elements, null when not asked for
    std::vector<T> v;
    bool on;
    Heap(size_t n, bool on_) : v(on_ ? n : 0), on(on_) {}
    T *ptr() { return on ? v.data() : nullptr; }
};

struct Scene {
    int E, K;
    std::vector<gat_ephemeris> ephs;
    std::vector<int32_t> tx_ms;
    std::vector<double> tx_frac, doppler, truth; // truth [E][7]: x, y, z, vx, vy, vz, drift
    std::vector<gat_fix> fixes;
    std::vector<int> seen;
};

Scene scene(std::mt19937_64 &rng, int E, int K, double lambda)
{
    std::uniform_real_distribution<double> u(-1.0, 1.0);
    Scene s;
    s.E = E, s.K = K, s.ephs = constellation(rng, K);
    s.tx_ms.assign((size_t)E * K, -1), s.tx_frac.assign((size_t)E * K, 0.0), s.doppler.assign((size_t)E * K, 0.0);
    s.truth.assign((size_t)E * 7, 0.0), s.fixes.assign((size_t)E, gat_fix{}), s.seen.assign((size_t)E, 0);
    for (int e = 0; e < E; ++e) {
        const double lat = 1.4 * u(rng), lon = 3.1 * u(rng), r = 6371e3 + 1000.0 * u(rng);
        double *x = &s.truth[(size_t)e * 7];
        x[0] = r * std::cos(lat) * std::cos(lon), x[1] = r * std::cos(lat) * std::sin(lon), x[2] = r * std::sin(lat);
        for (int i = 0; i < 3; ++i) x[3 + i] = e == 0 ? 0.0 : 150.0 * u(rng);
        x[6] = (e % 3 - 1) * 2e-7;
        const double t_rx = 208800.0 + 3000.0 * u(rng);
        for (int k = 0; k < K; ++k) {
            const size_t o = (size_t)e * K + k;
            if (measure(s.ephs[(size_t)k], x, x + 3, x[6], t_rx, lambda, &s.tx_ms[o], &s.tx_frac[o], &s.doppler[o])) s.seen[(size_t)e] += 1;
        }
        gat_fix &f = s.fixes[(size_t)e];
        f.x = x[0], f.y = x[1], f.z = x[2], f.clock_bias_s = 1e-4 * u(rng), f.num_used = s.seen[(size_t)e];
    }
    return s;
}

// What the kernel does with an epoch, lane by lane in step.  The wave's buffer has the kernel's layout; lanes >= K write nothing.
gat_velocity wave_epoch(const VelPlan &p, const gat_ephemeris *eph, const int32_t *tx_ms, const double *tx_frac, const double *doppler, const gat_fix &fix,
                        const uint8_t *used_in, const double *w, double *resid)
{
    const int K = p.K, W = kFixWave;
    const double zero[4] = {0.0, 0.0, 0.0, 0.0};
    if (!vel_fix_given(fix)) return vel_record(GAT_VEL_NO_FIX, 0, 0, zero, 0.0, zero);
    const double st[4] = {fix.x, fix.y, fix.z, kFixC * fix.clock_bias_s};
    std::vector<double> buf((size_t)kFixWaveDoubles, kNaN);
    std::vector<VelSat> c((size_t)W, VelSat{FixSat{0.0, 0.0, 0.0, 0.0, 0.0, false}, 0.0, 0.0, 0.0, 0.0, 0.0});
    std::vector<FixRow> row((size_t)W, FixRow{0.0, 0.0, 0.0, 0.0, 0.0});
    double wl[kFixWave], v[kFixWave];
    bool used[kFixWave];
    int num_valid = 0, num_used = 0;
    for (int lane = 0; lane < W; ++lane) {
        const bool mine = lane < K;
        if (mine) c[(size_t)lane] = vel_sat(eph[lane], tx_ms[lane], tx_frac[lane], doppler[lane]);
        wl[lane] = mine && w ? w[lane] : 1.0;
        used[lane] = c[(size_t)lane].s.ok && fix_weight_ok(wl[lane]) && (!used_in || used_in[mine ? lane : 0] != 0);
        num_valid += c[(size_t)lane].s.ok, num_used += used[lane];
    }
    int status[kFixWave];
    double s[kFixWave][4] = {};
    auto wave_sums = [&](const double (*t)[kFixTerms], int n, double *sums) { // fix_wave_sums, a lane at a time
        for (int lane = 0; lane < K; ++lane)
            for (int q = 0; q < n; ++q) buf[(size_t)(q * kFixPitch + lane)] = t[lane][q];
        for (int lane = 0; lane < n; ++lane) {
            double a = 0.0;
            for (int k = 0; k < K; ++k) a += buf[(size_t)(lane * kFixPitch + k)];
            buf[(size_t)(kFixTerms * kFixPitch + lane)] = a;
        }
        for (int q = 0; q < n; ++q) sums[q] = buf[(size_t)(kFixTerms * kFixPitch + q)];
    };
    static double t[kFixWave][kFixTerms];
    double sums[kFixTerms];
    if (num_used < 4) {
        for (int lane = 0; lane < W; ++lane) status[lane] = GAT_VEL_FEW_SATS;
    } else {
        for (int lane = 0; lane < W; ++lane) {
            if (c[(size_t)lane].s.ok) row[(size_t)lane] = vel_row(c[(size_t)lane], st, p.lambda);
            fix_terms(row[(size_t)lane], wl[lane], t[lane]);
            for (int q = 0; q < kFixTerms; ++q) t[lane][q] = used[lane] ? t[lane][q] : 0.0;
        }
        wave_sums(t, kFixTerms, sums);
        for (int lane = 0; lane < W; ++lane) status[lane] = fix_step(sums, s[lane]);
    }
    for (int lane = 1; lane < W; ++lane) CHECK(status[lane] == status[0] && std::memcmp(s[lane], s[0], sizeof s[0]) == 0, "the lanes disagree");
    const bool failed = vel_failed(status[0]);
    for (int lane = 0; lane < W; ++lane) {
        v[lane] = !failed && c[(size_t)lane].s.ok ? vel_resid(row[(size_t)lane], s[lane]) : 0.0;
        t[lane][0] = used[lane] ? v[lane] * v[lane] : 0.0;
    }
    double sum_v2[1] = {0.0};
    if (!failed) wave_sums(t, 1, sum_v2);
    for (int k = 0; k < K; ++k) resid[k] = v[k];
    return vel_record(status[0], num_valid, num_used, s[0], sum_v2[0], st);
}

int twins(std::mt19937_64 &rng, int count, int *walked)
{
    std::uniform_real_distribution<double> u(-1.0, 1.0);
    const gat_vel_config cfg = vel_cfg();
    int calls = 0;
    for (int n = 0; n < count; ++n) {
        const int K = n % 3 == 0 ? GAT_MAX_FIX_CHANNELS : 10 + (int)(rng() % 30);
        const int E = 6;
        Scene s = scene(rng, E, K, kFixC / cfg.carrier_hz);
        s.fixes[2].status = GAT_FIX_SINGULAR;                        // a failed fix
        s.fixes[4].status = GAT_FIX_NOT_CONVERGED | GAT_FIX_MASKED;  // used as it stands
        for (unsigned outs = 0; outs < 16; ++outs) {
            Heap<double> sat((size_t)E * K * 4, outs & 1), resid((size_t)E * K, outs & 2), w((size_t)E * K, outs & 4);
            Heap<uint8_t> used((size_t)E * K, outs & 8);
            for (double &v : w.v) v = 1.0 + 0.5 * u(rng);
            for (uint8_t &v : used.v) v = 1;
            int left = -1; // epoch 1 leaves a seen channel out, by `used` or by its weight
            for (int k = 0; k < K && left < 0; ++k)
                if (s.tx_ms[(size_t)K + k] >= 0) left = k;
            if (used.on && left >= 0) used.v[(size_t)K + left] = 0;
            if (w.on && !used.on && left >= 0) w.v[(size_t)K + left] = 0.0;
            std::vector<gat_velocity> vel((size_t)E);
            VelPlan p{};
            const Refusal r = vel_plan(VelCall{s.ephs.data(), s.tx_ms.data(), s.tx_frac.data(), s.doppler.data(), s.fixes.data(), E, K, &cfg, vel.data()}, &p);
            CHECK(r.code == GAT_OK, "twin call refused");
            vel_host_run(p, s.ephs.data(), s.tx_ms.data(), s.tx_frac.data(), s.doppler.data(), s.fixes.data(), used.ptr(), w.ptr(), vel.data(), sat.ptr(),
                         resid.ptr());
            ++calls;
            for (int e = 0; e < E; ++e) {
                const gat_velocity &f = vel[(size_t)e];
                const double *x = &s.truth[(size_t)e * 7];
                if (e == 2) {
                    gat_velocity want{};
                    want.status = GAT_VEL_NO_FIX;
                    CHECK(std::memcmp(&f, &want, sizeof f) == 0, "epoch 2: a failed fix gives a record");
                    continue;
                }
                const int seen = s.seen[(size_t)e];
                const int want_used = seen - (e == 1 && left >= 0 && (used.on || w.on) ? 1 : 0);
                CHECK(f.num_valid == seen && f.num_used == want_used, "epoch %d: %d valid %d used, seen %d", e, f.num_valid, f.num_used, seen);
                if (want_used < 6) continue;
                const double err = std::sqrt((f.vx - x[3]) * (f.vx - x[3]) + (f.vy - x[4]) * (f.vy - x[4]) + (f.vz - x[5]) * (f.vz - x[5]));
                CHECK(f.status == 0 && err < 1e-4 && std::fabs(f.clock_drift - x[6]) < 1e-12 && f.rms_residual_mps < 1e-4,
                      "epoch %d: status %d, %g m/s off, drift %g off, rms %g", e, f.status, err, f.clock_drift - x[6], f.rms_residual_mps);
                CHECK(std::fabs(f.ve * f.ve + f.vn * f.vn + f.vu * f.vu - (f.vx * f.vx + f.vy * f.vy + f.vz * f.vz)) < 1e-9 * (1.0 + err + x[3] * x[3] + x[4] * x[4] + x[5] * x[5]),
                      "epoch %d: the frame is no rotation", e);
                CHECK(std::fabs(f.height_m) < 30e3 && std::fabs(f.sin_lat * f.sin_lat + f.cos_lat * f.cos_lat - 1.0) < 1e-15, "epoch %d: the frame", e);
                // the epoch as the kernel walks it
                if (outs == 15 || outs == 3) {
                    const size_t o = (size_t)e * K;
                    std::vector<double> rw((size_t)K);
                    const gat_velocity g = wave_epoch(p, s.ephs.data(), &s.tx_ms[o], &s.tx_frac[o], &s.doppler[o], s.fixes[(size_t)e],
                                                      used.on ? &used.v[o] : nullptr, w.on ? &w.v[o] : nullptr, rw.data());
                    ++*walked;
                    CHECK(std::memcmp(&g, &f, sizeof f) == 0, "epoch %d: the wave's record is not the twin's", e);
                    CHECK(std::memcmp(rw.data(), &resid.v[o], sizeof(double) * (size_t)K) == 0, "epoch %d: the wave's residuals are not the twin's", e);
                }
            }
        }
    }
    return calls;
}

// every real field of an ephemeris
double *real_field(gat_ephemeris &g, int i)
{
    double *f[] = {&g.toc, &g.toe, &g.af0, &g.af1, &g.af2, &g.tgd, &g.sqrt_a, &g.e, &g.m0, &g.delta_n, &g.omega0, &g.i0, &g.omega, &g.omega_dot,
                   &g.idot, &g.cuc, &g.cus, &g.crc, &g.crs, &g.cic, &g.cis};
    return i < (int)(sizeof f / sizeof f[0]) ? f[i] : nullptr;
}

// vel_orbit's position and vel_clock's correction against fix_orbit and fix_clock, bit for bit
int same_bits(std::mt19937_64 &rng, int count)
{
    std::uniform_real_distribution<double> u(-1.0, 1.0);
    int n = 0;
    auto one = [&](const gat_ephemeris &g, double t) {
        double a[3], b[3], v[3], da, db, rate;
        fix_orbit(g, t, &a[0], &a[1], &a[2]);
        vel_orbit(g, t, &b[0], &b[1], &b[2], &v[0], &v[1], &v[2]);
        da = fix_clock(g, t);
        vel_clock(g, t, &db, &rate);
        CHECK(std::memcmp(a, b, sizeof a) == 0 && std::memcmp(&da, &db, sizeof da) == 0, "the state's bits differ at t = %g, sqrt_a = %g, e = %g", t, g.sqrt_a, g.e);
        ++n;
    };
    for (int i = 0; i < count; ++i) {
        std::vector<gat_ephemeris> ephs = constellation(rng, 1);
        gat_ephemeris &g = ephs[0];
        if (i % 2) g.sqrt_a = 3000.0 + 2000.0 * (1.0 + u(rng)), g.e = 0.25 * (1.0 + u(rng)) * 0.999, g.toe = 302400.0 * (1.0 + u(rng));
        one(g, 302400.0 * (1.0 + u(rng)));
    }
    const double hostile[] = {kNaN, kInf, -kInf, 5e-324, 0.004, 1e200, -0.0, 1e300};
    for (int f = 0; f < 21; ++f)
        for (double h : hostile) {
            std::vector<gat_ephemeris> ephs = constellation(rng, 1);
            *real_field(ephs[0], f) = h;
            one(ephs[0], 208800.0 + 100.0 * u(rng));
            one(ephs[0], h);
        }
    return n;
}

// Hostile entries on designated channels of hostile epochs among clean ones: all defined, the clean epochs untouched.
int hostile_entries(std::mt19937_64 &rng)
{
    const gat_vel_config cfg = vel_cfg();
    const int K = 24, E = 9;
    const Scene calm = scene(rng, E, K, kFixC / cfg.carrier_hz);
    auto run = [&](Scene &s, const uint8_t *used, const double *w, std::vector<gat_velocity> &vel, std::vector<double> &sat, std::vector<double> &resid) {
        vel.assign((size_t)E, gat_velocity{}), sat.assign((size_t)E * K * 4, -7.0), resid.assign((size_t)E * K, -7.0);
        VelPlan p{};
        const Refusal r = vel_plan(VelCall{s.ephs.data(), s.tx_ms.data(), s.tx_frac.data(), s.doppler.data(), s.fixes.data(), E, K, &cfg, vel.data()}, &p);
        CHECK(r.code == GAT_OK, "hostile call refused");
        vel_host_run(p, s.ephs.data(), s.tx_ms.data(), s.tx_frac.data(), s.doppler.data(), s.fixes.data(), used, w, vel.data(), sat.data(), resid.data());
    };
    Scene base = calm;
    std::vector<gat_velocity> vel0, vel;
    std::vector<double> sat0, resid0, sat, resid;
    run(base, nullptr, nullptr, vel0, sat0, resid0);
    const int hostile_epochs[3] = {1, 6, 8};
    auto compare_clean = [&](const char *what) {
        for (int e = 0; e < E; ++e) {
            if (e == 1 || e == 6 || e == 8) continue;
            CHECK(std::memcmp(&vel[(size_t)e], &vel0[(size_t)e], sizeof(gat_velocity)) == 0 &&
                      std::memcmp(&resid[(size_t)e * K], &resid0[(size_t)e * K], sizeof(double) * K) == 0 &&
                      std::memcmp(&sat[(size_t)e * K * 4], &sat0[(size_t)e * K * 4], sizeof(double) * K * 4) == 0,
                  "%s: clean epoch %d changed", what, e);
        }
    };
    int entries = 0;
    const double bad[] = {kNaN, kInf, -kInf};
    // the first seen channel of each hostile epoch is the designated one
    int chan[3];
    for (int i = 0; i < 3; ++i) {
        chan[i] = 0;
        while (calm.tx_ms[(size_t)hostile_epochs[i] * K + chan[i]] < 0) ++chan[i];
    }
    // doppler_hz and the weights
    for (double b : bad) {
        Scene s = calm;
        std::vector<double> w((size_t)E * K, 1.0);
        for (int i = 0; i < 3; ++i) s.doppler[(size_t)hostile_epochs[i] * K + chan[i]] = b;
        run(s, nullptr, nullptr, vel, sat, resid);
        compare_clean("doppler");
        for (int i = 0; i < 3; ++i) {
            const int e = hostile_epochs[i];
            CHECK(vel[(size_t)e].num_valid == vel0[(size_t)e].num_valid - 1 && resid[(size_t)e * K + chan[i]] == 0.0 && sat[((size_t)e * K + chan[i]) * 4] == 0.0,
                  "a Doppler that is not finite counts");
        }
        s = calm;
        for (int i = 0; i < 3; ++i) w[(size_t)hostile_epochs[i] * K + chan[i]] = b;
        run(s, nullptr, w.data(), vel, sat, resid);
        compare_clean("weights");
        for (int i = 0; i < 3; ++i) {
            const int e = hostile_epochs[i];
            CHECK(vel[(size_t)e].num_valid == vel0[(size_t)e].num_valid && vel[(size_t)e].num_used == vel0[(size_t)e].num_used - 1, "a weight that is not finite is used");
        }
        entries += 2;
    }
    // every real field of the ephemeris of channel chan[0]: the channel is every epoch's, so only that channel may change
    const double vals[] = {kNaN, kInf, -kInf};
    for (int f = 0; f < 21; ++f)
        for (double b : vals) {
            Scene s = calm;
            *real_field(s.ephs[(size_t)chan[0]], f) = b;
            run(s, nullptr, nullptr, vel, sat, resid);
            for (int e = 0; e < E; ++e)
                if (calm.tx_ms[(size_t)e * K + chan[0]] >= 0)
                    CHECK(vel[(size_t)e].num_valid == vel0[(size_t)e].num_valid - 1 && resid[(size_t)e * K + chan[0]] == 0.0, "field %d = %g counts in epoch %d", f, b, e);
            ++entries;
        }
    const double roots[] = {5e-324, 0.004, 1e200};
    for (double b : roots) {
        Scene s = calm;
        s.ephs[(size_t)chan[0]].sqrt_a = b;
        run(s, nullptr, nullptr, vel, sat, resid);
        for (int e = 0; e < E; ++e) CHECK(vel[(size_t)e].num_valid >= vel0[(size_t)e].num_valid - 1, "sqrt_a = %g: epoch %d", b, e);
        for (double v : sat) CHECK(std::isfinite(v), "sqrt_a = %g: a state that is not finite was written", b);
        ++entries;
    }
    // the fix's state
    for (double b : bad)
        for (int field = 0; field < 4; ++field) {
            Scene s = calm;
            for (int i = 0; i < 3; ++i) {
                gat_fix &f = s.fixes[(size_t)hostile_epochs[i]];
                double *q[] = {&f.x, &f.y, &f.z, &f.clock_bias_s};
                *q[field] = b;
            }
            run(s, nullptr, nullptr, vel, sat, resid);
            compare_clean("fix state");
            for (int i = 0; i < 3; ++i) {
                gat_velocity want{};
                want.status = GAT_VEL_NO_FIX;
                CHECK(std::memcmp(&vel[(size_t)hostile_epochs[i]], &want, sizeof want) == 0, "a fix that is not finite gives a record");
            }
            ++entries;
        }
    {   // the Earth's centre, and exactly on a satellite: from the second evaluation on the travel time is next to nothing and the
        // satellite is not turned, so the last range is zero or a rounding of the coordinates -- defined either way
        Scene s = calm;
        s.fixes[1].x = 0.0, s.fixes[1].y = 0.0, s.fixes[1].z = 0.0;
        const size_t o = (size_t)6 * K + chan[1];
        const VelSat c = vel_sat(s.ephs[(size_t)chan[1]], s.tx_ms[o], s.tx_frac[o], s.doppler[o]);
        s.fixes[6].x = c.s.X, s.fixes[6].y = c.s.Y, s.fixes[6].z = c.s.Z;
        run(s, nullptr, nullptr, vel, sat, resid);
        compare_clean("centre and satellite");
        CHECK(vel[1].status == GAT_VEL_NO_GEODETIC && vel[1].vx != 0.0 && vel[1].ve == 0.0 && vel[1].sin_lat == 0.0 && vel[1].height_m == 0.0, "the centre: status %d", vel[1].status);
        CHECK(c.s.ok && vel[6].num_valid == vel0[6].num_valid && (vel[6].status & ~(GAT_VEL_NONFINITE | GAT_VEL_SINGULAR)) == 0, "on a satellite: status %d", vel[6].status);
        std::printf("a fix on a satellite: status %d\n", vel[6].status);
        entries += 2;
    }
    return entries;
}

} // namespace

int main()
{
    std::mt19937_64 rng(20261021);
    refusals();
    const int planned = plans(rng, 3000);
    int walked = 0;
    const int calls = twins(rng, 6, &walked);
    const int states = same_bits(rng, 4000);
    const int entries = hostile_entries(rng);
    std::printf("planned %d calls, ran the twin %d times, walked %d epochs, compared %d states, %d hostile entries, %d failures\n", planned, calls, walked,
                states, entries, failures);
    return failures || walked < 20 ? 1 : 0;
}
