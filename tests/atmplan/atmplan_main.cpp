// Stand-alone check of the range corrections' pure plan (csrc/gat_atm_plan.h) and of the host twin's loops over it (atm_host_run, the
// rules of csrc/gat_fix.h, csrc/gat_vel.h and csrc/gat_atm.h).  Every documented refusal must return its code with nothing planned;
// random plans must put every (epoch, channel) into exactly one thread.  The twin then runs on heap buffers of exactly the extents the
// call describes -- every subset of the optional outputs, with and without the zenith array -- so that AddressSanitizer sees any access
// outside them, and its delays must be those of a plain libm statement of the model.  Last, hostile entries: NaN, the infinities and
// the zeros in every Klobuchar coefficient, in the zenith delays and in the fix's state, every real field of the ephemeris, a fix at
// the Earth's centre, on the axis and exactly on a satellite, floors of -1 and 1; everything must stay defined (the sanitizers'
// business, float-cast-overflow among them) and no epoch may touch another.  Built with
// -fsanitize=address,undefined,float-cast-overflow by tests/test_atmosphere_plan_host.py.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "gat_atm_page18.h"
#include "gat_atm_plan.h"

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

gat_atm_config atm_cfg(uint32_t flags = GAT_ATM_IONO | GAT_ATM_TROPO, double floor_sin = 0.0)
{
    gat_atm_config c{};
    c.struct_size = sizeof(gat_atm_config);
    c.flags = flags, c.carrier_hz = 1575.42e6, c.floor_sin = floor_sin;
    const double a[4] = {12 * 0x1p-30, 2 * 0x1p-27, -1 * 0x1p-24, -1 * 0x1p-24}, b[4] = {44 * 2048.0, 8 * 16384.0, -65536.0, -6 * 65536.0};
    for (int i = 0; i < 4; ++i) c.alpha[i] = a[i], c.beta[i] = b[i];
    c.zenith_dry_m = 2.3, c.zenith_wet_m = 0.1;
    return c;
}
AtmCall call(int E, int K, const gat_atm_config *cfg) { return AtmCall{kGiven, kGiven, kGiven, kGiven, kGiven, kGiven, E, K, cfg, kGiven}; }

void expect_refusal(const AtmCall &a, int code, const char *what)
{
    AtmPlan p, q;
    std::memset(&p, 0x5a, sizeof p);
    std::memset(&q, 0x5a, sizeof q);
    const Refusal r = atm_plan(a, &p);
    CHECK(r.code == code, "%s: got %d, want %d", what, r.code, code);
    CHECK(std::memcmp(&p, &q, sizeof p) == 0, "%s: the plan was written", what);
}

void refusals()
{
    const gat_atm_config good = atm_cfg();
    AtmCall a = call(3, 6, &good);
    const void **ptrs[] = {&a.eph, &a.tx_ms, &a.tx_frac, &a.rx_ms, &a.rx_frac, &a.fixes, &a.tx_frac_out};
    for (const void **p : ptrs) {
        *p = nullptr;
        expect_refusal(a, GAT_ERR_ARG, "null pointer");
        *p = kGiven;
    }
    expect_refusal(call(3, 6, nullptr), GAT_ERR_ARG, "null config");
    gat_atm_config c = good;
    c.struct_size += 8;
    expect_refusal(call(3, 6, &c), GAT_ERR_ARG, "struct_size");
    for (uint32_t f : {4u, 7u, 0x80000000u}) {
        c = good, c.flags = f;
        expect_refusal(call(3, 6, &c), GAT_ERR_ARG, "flags");
    }
    const double bad[] = {kNaN, kInf, -kInf, 0.0, -0.0, -1575.42e6};
    for (double v : bad) {
        c = good, c.carrier_hz = v;
        expect_refusal(call(3, 6, &c), GAT_ERR_ARG, "carrier_hz");
    }
    for (double v : {kNaN, kInf, -kInf}) {
        c = good, c.floor_sin = v;
        expect_refusal(call(3, 6, &c), GAT_ERR_ARG, "floor_sin");
    }
    expect_refusal(call(0, 6, &good), GAT_ERR_ARG, "E = 0");
    expect_refusal(call(3, 0, &good), GAT_ERR_ARG, "K = 0");
    expect_refusal(call(-1, 6, &good), GAT_ERR_ARG, "E = -1");
    expect_refusal(call(3, GAT_MAX_FIX_CHANNELS + 1, &good), GAT_ERR_RANGE, "K = 65");
    expect_refusal(call(GAT_MAX_FIX_EPOCHS + 1, 6, &good), GAT_ERR_RANGE, "E = 2^24 + 1");
    CHECK(atm_plan(call(3, 6, &good), nullptr).code == GAT_ERR_ARG, "null plan");
    AtmPlan p{};
    for (uint32_t f : {0u, 1u, 2u, 3u}) {
        c = good, c.flags = f, c.floor_sin = -1.0;
        CHECK(atm_plan(call(3, 6, &c), &p).code == GAT_OK && p.prm.flags == f && p.prm.scale == 1.0, "flags %u refused", f);
    }
}

int plans(std::mt19937_64 &rng, int count)
{
    const gat_atm_config cfg = atm_cfg();
    for (int n = 0; n < count; ++n) {
        const bool small = n < 40 || n % 8 == 0;
        const int E = n < 40 ? n + 1 : (small ? 1 + (int)(rng() % 3000) : 1 + (int)(rng() % GAT_MAX_FIX_EPOCHS));
        const int K = 1 + (int)(rng() % GAT_MAX_FIX_CHANNELS);
        AtmPlan p{};
        CHECK(atm_plan(call(E, K, &cfg), &p).code == GAT_OK, "E %d K %d refused", E, K);
        CHECK(p.E == E && p.K == K && p.cells == (long long)E * K && p.groups == (p.cells + kAtmThreads - 1) / kAtmThreads && p.groups <= 0x7fffffffll, "geometry");
        gat_fix_plan rep{};
        atm_report(p, &rep);
        CHECK(rep.workgroups == p.groups && rep.threads == kAtmThreads && rep.waves_per_workgroup == 4 && rep.scratch_bytes == 0 && rep.lds_bytes == 0, "report");
        int e = -1, k = -1;
        if (small) { // every thread of the grid: each (epoch, channel) once
            std::vector<uint8_t> hit((size_t)E * K, 0);
            for (long long g = 0; g < p.groups; ++g)
                for (int lane = 0; lane < kAtmThreads; ++lane)
                    if (atm_unit(g, lane, p.cells, K, &e, &k)) {
                        CHECK(e >= 0 && e < E && k >= 0 && k < K, "a thread outside the call");
                        if (e >= 0 && e < E && k >= 0 && k < K) hit[(size_t)e * K + k] += 1;
                    }
            for (uint8_t h : hit) CHECK(h == 1, "E %d K %d: a cell is covered %d times", E, K, h);
        } else {
            const int last = (int)((p.cells - 1) % kAtmThreads);
            CHECK(atm_unit(p.groups - 1, last, p.cells, K, &e, &k) && e == E - 1 && k == K - 1, "the last cell");
            CHECK(!atm_unit(p.groups - 1, last + 1, p.cells, K, &e, &k) || last + 1 == kAtmThreads, "a thread past the last");
            CHECK(!atm_unit(p.groups, 0, p.cells, K, &e, &k), "a workgroup past the last");
            CHECK(atm_unit(0, 0, p.cells, K, &e, &k) && e == 0 && k == 0, "the first cell");
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

// the time of transmission by the satellite's own clock that a receiver at xyz sees at the GPS time t_rx; false: below the horizon
bool measure(const gat_ephemeris &g, const double *xyz, double t_rx, int32_t *tx_ms, double *tx_frac)
{
    double tau = 0.075, d[3] = {0, 0, 0};
    for (int it = 0; it < 8; ++it) {
        double X, Y, Z, c, s;
        fix_orbit(g, t_rx - tau, &X, &Y, &Z);
        fix_sincos(kFixOmegaE * tau, &c, &s);
        d[0] = c * X + s * Y - xyz[0], d[1] = c * Y - s * X - xyz[1], d[2] = Z - xyz[2];
        tau = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]) / kFixC;
    }
    if (!(d[0] * xyz[0] + d[1] * xyz[1] + d[2] * xyz[2] > 0.0)) return false;
    double dts = 0.0;
    for (int it = 0; it < 4; ++it) dts = fix_clock(g, t_rx - tau + dts);
    const double t_sv = t_rx - tau + dts;
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
    Heap(size_t n, bool on_, T fill) : v(on_ ? n : 0, fill), on(on_) {}
    T *ptr() { return on ? v.data() : nullptr; }
};

struct Scene {
    int E, K;
    std::vector<gat_ephemeris> ephs;
    std::vector<int32_t> tx_ms, rx_ms;
    std::vector<double> tx_frac, rx_frac, zenith;
    std::vector<gat_fix> fixes;
    std::vector<int> seen;
};

Scene scene(std::mt19937_64 &rng, int E, int K)
{
    std::uniform_real_distribution<double> u(-1.0, 1.0);
    Scene s;
    s.E = E, s.K = K, s.ephs = constellation(rng, K);
    s.tx_ms.assign((size_t)E * K, -1), s.tx_frac.assign((size_t)E * K, 0.0);
    s.rx_ms.assign((size_t)E, 0), s.rx_frac.assign((size_t)E, 0.0), s.zenith.assign((size_t)E * 2, 0.0);
    s.fixes.assign((size_t)E, gat_fix{}), s.seen.assign((size_t)E, 0);
    for (int e = 0; e < E; ++e) {
        const double lat = 1.4 * u(rng), lon = 3.1 * u(rng), r = 6371e3 + 1000.0 * u(rng);
        const double x[3] = {r * std::cos(lat) * std::cos(lon), r * std::cos(lat) * std::sin(lon), r * std::sin(lat)};
        const double t_rx = 208800.0 + 40000.0 * u(rng), bias = 1e-4 * u(rng);
        const double t_clock = t_rx + bias;
        s.rx_ms[(size_t)e] = (int32_t)std::floor(t_clock * 1e3);
        s.rx_frac[(size_t)e] = t_clock - s.rx_ms[(size_t)e] * 1e-3;
        if (s.rx_frac[(size_t)e] < 0) s.rx_frac[(size_t)e] = 0;
        for (int k = 0; k < K; ++k) {
            const size_t o = (size_t)e * K + k;
            if (measure(s.ephs[(size_t)k], x, t_rx, &s.tx_ms[o], &s.tx_frac[o])) s.seen[(size_t)e] += 1;
        }
        gat_fix &f = s.fixes[(size_t)e];
        f.x = x[0], f.y = x[1], f.z = x[2], f.clock_bias_s = bias, f.num_used = s.seen[(size_t)e];
        s.zenith[(size_t)e * 2] = 2.3 + 0.1 * u(rng), s.zenith[(size_t)e * 2 + 1] = 0.15 + 0.1 * u(rng);
    }
    return s;
}

struct Out {
    std::vector<double> frac, delay, geom;
    std::vector<uint8_t> ch;
    std::vector<int32_t> ep;
};
Out run(const Scene &s, const gat_atm_config &cfg, bool with_zenith = true)
{
    Out o;
    const size_t n = (size_t)s.E * s.K;
    o.frac.assign(n, -7.0), o.delay.assign(2 * n, -7.0), o.geom.assign(3 * n, -7.0), o.ch.assign(n, 0x77), o.ep.assign((size_t)s.E, -7);
    AtmPlan p{};
    const Refusal r = atm_plan(AtmCall{s.ephs.data(), s.tx_ms.data(), s.tx_frac.data(), s.rx_ms.data(), s.rx_frac.data(), s.fixes.data(), s.E, s.K, &cfg, o.frac.data()}, &p);
    CHECK(r.code == GAT_OK, "call refused");
    atm_host_run(p, s.ephs.data(), s.tx_ms.data(), s.tx_frac.data(), s.rx_ms.data(), s.rx_frac.data(), s.fixes.data(), with_zenith ? s.zenith.data() : nullptr,
                 o.frac.data(), o.delay.data(), o.geom.data(), o.ch.data(), o.ep.data());
    return o;
}

// the model in plain libm, for one corrected channel: (iono, tropo) from the twin's own geometry and the epoch's state
void by_libm(const gat_atm_config &cfg, const gat_fix &f, int32_t rx_ms, double rx_frac, const double *geom, double zd, double zw, double *iono, double *tropo)
{
    const double pi = kAtmPi;
    const double el = std::asin(geom[0]), az = std::atan2(geom[2], geom[1]);
    const double p = std::hypot(f.x, f.y);
    double lat = std::atan2(f.z, p * (1.0 - kVelE2));
    for (int i = 0; i < 30; ++i) {
        const double N = kVelA / std::sqrt(1.0 - kVelE2 * std::sin(lat) * std::sin(lat));
        lat = std::atan2(f.z + kVelE2 * N * std::sin(lat), p);
    }
    const double lon = std::atan2(f.y, f.x);
    const double E = el / pi, psi = 0.0137 / (E + 0.11) - 0.022;
    double phi_i = lat / pi + psi * std::cos(az);
    phi_i = std::fmin(std::fmax(phi_i, -0.416), 0.416);
    const double lam_i = lon / pi + psi * std::sin(az) / std::cos(pi * phi_i);
    const double phi_m = phi_i + 0.064 * std::cos(pi * (lam_i - 1.617));
    double t = 43200.0 * lam_i + (double)(rx_ms % 86400000) * 1e-3 + rx_frac - f.clock_bias_s;
    if (t >= 86400.0) t -= 86400.0;
    if (t < 0.0) t += 86400.0;
    const double F = 1.0 + 16.0 * std::pow(0.53 - E, 3);
    double per = 0.0, amp = 0.0;
    for (int i = 3; i >= 0; --i) per = per * phi_m + cfg.beta[i], amp = amp * phi_m + cfg.alpha[i];
    per = std::fmax(per, 72000.0), amp = std::fmax(amp, 0.0);
    const double xx = 2.0 * pi * (t - 50400.0) / per;
    const double T = std::fabs(xx) < 1.57 ? F * (5e-9 + amp * (1.0 - xx * xx / 2.0 + xx * xx * xx * xx / 24.0)) : F * 5e-9;
    *iono = kFixC * T * std::pow(kAtmL1 / cfg.carrier_hz, 2);
    *tropo = zd / (std::sin(el) + 0.00143 / (std::tan(el) + 0.0445)) + zw / (std::sin(el) + 0.00035 / (std::tan(el) + 0.017));
}

int twins(std::mt19937_64 &rng, int count, int *compared)
{
    int calls = 0;
    for (int n = 0; n < count; ++n) {
        const int K = n % 3 == 0 ? GAT_MAX_FIX_CHANNELS : 10 + (int)(rng() % 30);
        const int E = 6;
        Scene s = scene(rng, E, K);
        s.fixes[2].status = GAT_FIX_SINGULAR;                       // a failed fix
        s.fixes[4].status = GAT_FIX_NOT_CONVERGED | GAT_FIX_MASKED; // used as it stands
        const gat_atm_config cfg = atm_cfg();
        const Out full = run(s, cfg);
        const size_t cells = (size_t)E * K;
        for (unsigned outs = 0; outs < 32; ++outs) {
            Heap<double> frac(cells, true, -7.0), delay(2 * cells, outs & 1, -7.0), geom(3 * cells, outs & 2, -7.0), zen((size_t)E * 2, outs & 16, 0.0);
            Heap<uint8_t> ch(cells, outs & 4, 0x77);
            Heap<int32_t> ep((size_t)E, outs & 8, -7);
            Heap<int32_t> tx_ms(cells, true, 0), rx_ms((size_t)E, true, 0);
            Heap<double> tx_frac(cells, true, 0.0), rx_frac((size_t)E, true, 0.0);
            Heap<gat_ephemeris> eph((size_t)K, true, gat_ephemeris{});
            Heap<gat_fix> fixes((size_t)E, true, gat_fix{});
            tx_ms.v = s.tx_ms, rx_ms.v = s.rx_ms, tx_frac.v = s.tx_frac, rx_frac.v = s.rx_frac, eph.v = s.ephs, fixes.v = s.fixes;
            if (zen.on) zen.v = s.zenith;
            gat_atm_config c = cfg;
            if (!zen.on) c.zenith_dry_m = s.zenith[0], c.zenith_wet_m = s.zenith[1]; // epoch 0's pair for every epoch
            AtmPlan p{};
            const Refusal r = atm_plan(AtmCall{eph.ptr(), tx_ms.ptr(), tx_frac.ptr(), rx_ms.ptr(), rx_frac.ptr(), fixes.ptr(), E, K, &c, frac.ptr()}, &p);
            CHECK(r.code == GAT_OK, "twin call refused");
            atm_host_run(p, eph.ptr(), tx_ms.ptr(), tx_frac.ptr(), rx_ms.ptr(), rx_frac.ptr(), fixes.ptr(), zen.ptr(), frac.ptr(), delay.ptr(), geom.ptr(), ch.ptr(),
                         ep.ptr());
            ++calls;
            // an output has the bytes it has in the full call (with the array; without it epoch 0 alone has the same zenith delays)
            const size_t span = zen.on ? cells : (size_t)K;
            CHECK(std::memcmp(frac.v.data(), full.frac.data(), span * sizeof(double)) == 0, "outs %u: tx_frac_out", outs);
            if (delay.on) CHECK(std::memcmp(delay.v.data(), full.delay.data(), 2 * span * sizeof(double)) == 0, "outs %u: delay", outs);
            if (geom.on) CHECK(std::memcmp(geom.v.data(), full.geom.data(), 3 * cells * sizeof(double)) == 0, "outs %u: geom", outs);
            if (ch.on) CHECK(std::memcmp(ch.v.data(), full.ch.data(), span) == 0, "outs %u: channel_status", outs);
            if (ep.on) CHECK(std::memcmp(ep.v.data(), full.ep.data(), (size_t)E * sizeof(int32_t)) == 0, "outs %u: epoch_status", outs);
        }
        // what the full call says
        for (int e = 0; e < E; ++e) {
            CHECK(full.ep[(size_t)e] == (e == 2 ? GAT_ATM_NO_FIX : 0), "epoch %d: status %d", e, full.ep[(size_t)e]);
            int counted = 0;
            for (int k = 0; k < K; ++k) {
                const size_t o = (size_t)e * K + k;
                const uint8_t st = full.ch[o];
                if (e == 2 || s.tx_ms[o] < 0) {
                    CHECK(st == 0 && full.frac[o] == s.tx_frac[o] && full.delay[2 * o] == 0.0 && full.delay[2 * o + 1] == 0.0 && full.geom[3 * o] == 0.0,
                          "epoch %d channel %d: something without a frame or a measurement", e, k);
                    continue;
                }
                ++counted;
                CHECK(st == GAT_ATM_CH_CORRECTED || st == GAT_ATM_CH_LOW, "epoch %d channel %d: status %d", e, k, st);
                if (st != GAT_ATM_CH_CORRECTED) {
                    CHECK(full.geom[3 * o] < 0.0 && full.frac[o] == s.tx_frac[o] && full.delay[2 * o] == 0.0, "a low channel");
                    continue;
                }
                double iono, tropo;
                by_libm(cfg, s.fixes[(size_t)e], s.rx_ms[(size_t)e], s.rx_frac[(size_t)e], &full.geom[3 * o], s.zenith[(size_t)e * 2], s.zenith[(size_t)e * 2 + 1], &iono, &tropo);
                // the libm statement starts from the twin's rounded geometry: near the horizon 1e-16 of sin el are 1e-13 m of troposphere
                CHECK(std::fabs(full.delay[2 * o] - iono) <= 1e-9 && std::fabs(full.delay[2 * o + 1] - tropo) <= 1e-9, "epoch %d channel %d: iono %g (libm %g), tropo %g (libm %g)",
                      e, k, full.delay[2 * o], iono, full.delay[2 * o + 1], tropo);
                CHECK(full.frac[o] == s.tx_frac[o] + (full.delay[2 * o] + full.delay[2 * o + 1]) / kFixC, "the corrected fraction");
                ++*compared;
            }
            CHECK(counted == s.seen[(size_t)e] || e == 2, "epoch %d: %d counted, %d seen", e, counted, s.seen[(size_t)e]);
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

bool all_finite(const Out &o)
{
    for (double v : o.delay)
        if (!std::isfinite(v)) return false;
    for (double v : o.geom)
        if (!std::isfinite(v)) return false;
    return true;
}

// Hostile entries in designated epochs among clean ones: all defined, finite outputs but the passed-through fraction, the clean epochs
// untouched.
int hostile_entries(std::mt19937_64 &rng)
{
    const int K = 24, E = 9;
    const Scene calm = scene(rng, E, K);
    const gat_atm_config cfg = atm_cfg(GAT_ATM_IONO | GAT_ATM_TROPO, -1.0);
    const Out out0 = run(calm, cfg);
    int entries = 0;
    auto same_epoch = [&](const Out &o, int e) {
        const size_t a = (size_t)e * K;
        return std::memcmp(&o.frac[a], &out0.frac[a], sizeof(double) * K) == 0 && std::memcmp(&o.delay[2 * a], &out0.delay[2 * a], sizeof(double) * 2 * K) == 0 &&
               std::memcmp(&o.geom[3 * a], &out0.geom[3 * a], sizeof(double) * 3 * K) == 0 && std::memcmp(&o.ch[a], &out0.ch[a], (size_t)K) == 0 && o.ep[(size_t)e] == out0.ep[(size_t)e];
    };
    const double vals[] = {kNaN, kInf, -kInf, 0.0, -0.0, 1e300, -1e300, 5e-324};
    // the coefficients: every channel of every epoch is one thing or the other, nothing else changes
    for (int which = 0; which < 8; ++which)
        for (double v : vals) {
            gat_atm_config c = cfg;
            (which < 4 ? c.alpha[which] : c.beta[which - 4]) = v;
            const Out o = run(calm, c);
            CHECK(all_finite(o), "coefficient %d = %g: an output that is not finite", which, v);
            for (size_t i = 0; i < o.ch.size(); ++i) {
                CHECK(o.ch[i] == out0.ch[i] || (out0.ch[i] == GAT_ATM_CH_CORRECTED && o.ch[i] == GAT_ATM_CH_NONFINITE), "coefficient %d = %g: status %d", which, v, o.ch[i]);
                if (o.ch[i] == GAT_ATM_CH_NONFINITE) CHECK(o.frac[i] == calm.tx_frac[i] && o.delay[2 * i] == 0.0 && o.delay[2 * i + 1] == 0.0, "a channel that is not finite keeps something");
                if (!std::isfinite(v)) CHECK(out0.ch[i] != GAT_ATM_CH_CORRECTED || o.ch[i] == GAT_ATM_CH_NONFINITE, "coefficient %d = %g gives a delay", which, v);
            }
            CHECK(std::memcmp(o.geom.data(), out0.geom.data(), o.geom.size() * sizeof(double)) == 0, "coefficient %d = %g: the geometry changed", which, v);
            ++entries;
        }
    // the zenith delays of epochs 1 and 6
    for (int col = 0; col < 2; ++col)
        for (double v : vals) {
            Scene s = calm;
            s.zenith[(size_t)1 * 2 + col] = v, s.zenith[(size_t)6 * 2 + col] = v;
            const Out o = run(s, cfg);
            CHECK(all_finite(o), "zenith %d = %g: an output that is not finite", col, v);
            for (int e = 0; e < E; ++e)
                if (e != 1 && e != 6) CHECK(same_epoch(o, e), "zenith %d = %g: clean epoch %d changed", col, v, e);
            ++entries;
        }
    // the fix's state in epochs 1, 6 and 8
    for (int field = 0; field < 4; ++field)
        for (double v : vals) {
            Scene s = calm;
            for (int e : {1, 6, 8}) {
                gat_fix &f = s.fixes[(size_t)e];
                double *q[] = {&f.x, &f.y, &f.z, &f.clock_bias_s};
                *q[field] = v;
            }
            const Out o = run(s, cfg);
            CHECK(all_finite(o), "fix field %d = %g: an output that is not finite", field, v);
            for (int e = 0; e < E; ++e)
                if (e != 1 && e != 6 && e != 8) CHECK(same_epoch(o, e), "fix field %d = %g: clean epoch %d changed", field, v, e);
            if (!std::isfinite(v))
                for (int e : {1, 6, 8}) {
                    CHECK(o.ep[(size_t)e] == GAT_ATM_NO_FIX, "a fix that is not finite gives a frame");
                    for (int k = 0; k < K; ++k) CHECK(o.ch[(size_t)e * K + k] == 0 && o.frac[(size_t)e * K + k] == calm.tx_frac[(size_t)e * K + k], "an epoch without a fix writes something");
                }
            ++entries;
        }
    // every real field of one channel's ephemeris: only that channel may change
    int chan = 0;
    while (calm.tx_ms[(size_t)chan] < 0) ++chan;
    for (int f = 0; f < 21; ++f)
        for (double v : {kNaN, kInf, -kInf, 1e200}) {
            Scene s = calm;
            *real_field(s.ephs[(size_t)chan], f) = v;
            const Out o = run(s, cfg);
            CHECK(all_finite(o), "ephemeris field %d = %g: an output that is not finite", f, v);
            for (size_t i = 0; i < o.ch.size(); ++i)
                if ((int)(i % K) != chan) CHECK(o.ch[i] == out0.ch[i] && o.frac[i] == out0.frac[i] && o.delay[2 * i] == out0.delay[2 * i], "ephemeris field %d = %g: another channel changed", f, v);
            ++entries;
        }
    {   // the Earth's centre, below the mask radius, on the axis both ways, exactly on a satellite
        Scene s = calm;
        s.fixes[1].x = 0.0, s.fixes[1].y = 0.0, s.fixes[1].z = 0.0;
        s.fixes[3].x = 0.0, s.fixes[3].y = 0.0, s.fixes[3].z = 999999.0;
        s.fixes[5].x = 0.0, s.fixes[5].y = -0.0, s.fixes[5].z = 6356752.3;
        s.fixes[7].x = -0.0, s.fixes[7].y = 0.0, s.fixes[7].z = -6356752.3;
        int ch6 = 0;
        while (calm.tx_ms[(size_t)6 * K + ch6] < 0) ++ch6;
        const size_t o6 = (size_t)6 * K + ch6;
        const FixSat c = fix_sat(s.ephs[(size_t)ch6], s.tx_ms[o6], s.tx_frac[o6], s.rx_ms[6], s.rx_frac[6]);
        s.fixes[6].x = c.X, s.fixes[6].y = c.Y, s.fixes[6].z = c.Z;
        const Out o = run(s, cfg);
        CHECK(all_finite(o), "special states: an output that is not finite");
        for (int e : {0, 2, 4, 8}) CHECK(same_epoch(o, e), "special states: clean epoch %d changed", e);
        CHECK(o.ep[1] == GAT_ATM_NO_GEODETIC && o.ep[3] == GAT_ATM_NO_GEODETIC && o.ep[5] == 0 && o.ep[7] == 0 && o.ep[6] == 0, "special states: the epochs' status");
        CHECK(c.ok && (o.ch[o6] == GAT_ATM_CH_NONFINITE || o.ch[o6] == GAT_ATM_CH_CORRECTED || o.ch[o6] == GAT_ATM_CH_LOW), "on a satellite: status %d", o.ch[o6]);
        std::printf("a fix on a satellite: channel status %d\n", o.ch[o6]);
        entries += 5;
    }
    for (double floor : {-1.0, 0.0, 1.0, std::nextafter(1.0, 0.0), -5e-324, 1e300, -1e300}) {
        const gat_atm_config c = atm_cfg(GAT_ATM_IONO | GAT_ATM_TROPO, floor);
        const Out o = run(calm, c);
        CHECK(all_finite(o), "floor %g: an output that is not finite", floor);
        for (size_t i = 0; i < o.ch.size(); ++i)
            if (out0.ch[i] != 0) CHECK(o.ch[i] == (out0.geom[3 * i] >= floor ? out0.ch[i] : GAT_ATM_CH_LOW), "floor %g: status %d at sin el %g", floor, o.ch[i], out0.geom[3 * i]);
        ++entries;
    }
    return entries;
}

// the arctangent where a conversion or a division could go wrong
int arctangents()
{
    const double v[] = {0.0, -0.0, 5e-324, -5e-324, 1.0, -1.0, 1e308, -1e308, kInf, -kInf, kNaN, 0.0625, 0.03125, 0.09375, 1.0 - 0x1p-53, 1.0 + 0x1p-52};
    int n = 0;
    for (double y : v)
        for (double x : v) {
            const double a = atm_atan2(y, x);
            const bool number = !(std::isnan(y) || std::isnan(x) || (std::isinf(y) && std::isinf(x)));
            CHECK(number ? std::fabs(a - ((x == 0.0 && y == 0.0) ? 0.0 : std::atan2(y, x))) <= 1e-15 : std::isnan(a), "atan2(%g, %g) = %g", y, x, a);
            ++n;
        }
    return n;
}

// page 18: fields -> words -> a frame record -> fields
int pages(std::mt19937_64 &rng, int count)
{
    for (int n = 0; n < count; ++n) {
        gat_lnav_page18 p{};
        p.data_id = (int)(rng() % 4), p.sv_id = kPage18SvId, p.wnt = (int)(rng() % 256), p.wnlsf = (int)(rng() % 256), p.dn = (int)(rng() % 256);
        p.dt_ls = (int)(rng() % 256) - 128, p.dt_lsf = (int)(rng() % 256) - 128;
        const int ex_a[4] = {-30, -27, -24, -24}, ex_b[4] = {11, 14, 16, 16};
        for (int i = 0; i < 4; ++i) p.alpha[i] = std::ldexp((double)((int)(rng() % 256) - 128), ex_a[i]), p.beta[i] = std::ldexp((double)((int)(rng() % 256) - 128), ex_b[i]);
        p.a1 = std::ldexp((double)((int64_t)(rng() % (1u << 24)) - (1 << 23)), -50), p.a0 = std::ldexp((double)((int64_t)(rng() % (1ull << 32)) - (1ll << 31)), -30);
        p.tot = std::ldexp((double)(rng() % 256), 12);
        if (n == 0) p.a0 = kNaN, p.a1 = kInf, p.alpha[0] = 1e300; // no field's conversion may be undefined; what comes back is the encoder's
        std::vector<uint8_t> bits((size_t)kEphPayloadBits), again((size_t)kEphPayloadBits);
        page18_encode(&p, bits.data());
        gat_nav_frame fr{};
        fr.status = kEphLnavGood, fr.id = kPage18Subframe;
        for (int i = 0; i < kEphPayloadBits; ++i) fr.words[2 + i / 24] |= (uint32_t)bits[(size_t)i] << (29 - i % 24);
        gat_lnav_page18 q{};
        page18_decode(&fr, 1, &q);
        CHECK(q.valid == 1, "page %d not found", n);
        page18_encode(&q, again.data());
        CHECK(bits == again, "page %d: words -> fields -> words changes a bit", n);
        p.valid = 1;
        if (n > 0) CHECK(std::memcmp(&p, &q, sizeof p) == 0, "page %d: fields -> words -> fields changes a field", n);
        fr.id = 5;
        page18_decode(&fr, 1, &q);
        CHECK(q.valid == 0, "a page of subframe 5");
    }
    gat_lnav_page18 q{};
    page18_decode(nullptr, 0, &q);
    CHECK(q.valid == 0, "a page from no frames");
    return count;
}

} // namespace

int main()
{
    std::mt19937_64 rng(20261021);
    refusals();
    const int planned = plans(rng, 3000);
    int compared = 0;
    const int calls = twins(rng, 6, &compared);
    const int entries = hostile_entries(rng);
    const int angles = arctangents();
    const int coded = pages(rng, 200);
    std::printf("planned %d calls, ran the twin %d times, compared %d channels with libm, %d hostile entries, %d angles, %d pages, %d failures\n", planned, calls, compared,
                entries, angles, coded, failures);
    return failures || compared < 100 ? 1 : 0;
}
