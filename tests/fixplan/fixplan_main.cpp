// Stand-alone check of the position fix's pure plan (csrc/gat_fix_plan.h), of the host twin's loops over it (fix_host_run, the rule
// of csrc/gat_fix.h) and of the ephemeris table (csrc/gat_fix_eph.h).  A few thousand random plans must cover every (epoch,
// channel) exactly once through the workgroups, waves and lanes the kernel is launched with and stay inside a wave's LDS; every
// documented refusal must return its code with nothing planned.  The twin then runs on heap buffers of exactly the extents the
// call describes -- every subset of the optional outputs, with and without weights, epochs without measurements among good ones --
// so that AddressSanitizer sees any access outside them, and must find the receivers the transmit times were made for.  The
// ephemeris goes through the encoder and the decoder and must come back equal.  Built with -fsanitize=address,undefined,
// float-cast-overflow by tests/test_position_plan_host.py.  `fixplan sincos FILE` writes x, cos, sin of fix_sincos as raw doubles
// instead: a dense grid on [-72, 72], every multiple of pi/4 there, and +-2^k up to the largest double with their neighbours, where
// the sanitizer sees a quadrant taken by an out-of-range conversion.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "gat_fix.h"
#include "gat_fix_eph.h"
#include "gat_fix_plan.h"

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

gat_fix_config config(int max_iter = 10, double tol = 1e-4, double mask = -1.0)
{
    gat_fix_config c{};
    c.struct_size = sizeof(gat_fix_config);
    c.max_iter = max_iter, c.tol_m = tol, c.mask_sin = mask;
    return c;
}
FixCall call(int E, int K, const gat_fix_config *cfg) { return FixCall{kGiven, kGiven, kGiven, kGiven, kGiven, E, K, cfg, kGiven}; }

FixPlan untouched_plan()
{
    FixPlan p;
    std::memset(&p, 0x5a, sizeof p);
    return p;
}
void expect_refusal(const FixCall &a, int code, const char *what)
{
    FixPlan p = untouched_plan();
    const FixPlan q = untouched_plan();
    const Refusal r = fix_plan(a, &p);
    CHECK(r.code == code, "%s: got %d, want %d", what, r.code, code);
    CHECK(std::memcmp(&p, &q, sizeof p) == 0, "%s: the plan was written", what);
}

void refusals()
{
    const gat_fix_config good = config();
    FixCall a = call(3, 5, &good);
    const void **ptrs[] = {&a.eph, &a.tx_ms, &a.tx_frac, &a.rx_ms, &a.rx_frac, &a.fixes};
    for (const void **p : ptrs) {
        *p = nullptr;
        expect_refusal(a, GAT_ERR_ARG, "null pointer");
        *p = kGiven;
    }
    expect_refusal(call(3, 5, nullptr), GAT_ERR_ARG, "null config");
    gat_fix_config c = good;
    c.struct_size -= 4;
    expect_refusal(call(3, 5, &c), GAT_ERR_ARG, "struct_size");
    expect_refusal(call(0, 5, &good), GAT_ERR_ARG, "E = 0");
    expect_refusal(call(3, 0, &good), GAT_ERR_ARG, "K = 0");
    c = good, c.max_iter = 0;
    expect_refusal(call(3, 5, &c), GAT_ERR_ARG, "max_iter = 0");
    c = good, c.tol_m = 0.0;
    expect_refusal(call(3, 5, &c), GAT_ERR_ARG, "tol_m = 0");
    c = good, c.tol_m = std::numeric_limits<double>::quiet_NaN();
    expect_refusal(call(3, 5, &c), GAT_ERR_ARG, "tol_m NaN");
    c = good, c.mask_sin = std::numeric_limits<double>::quiet_NaN();
    expect_refusal(call(3, 5, &c), GAT_ERR_ARG, "mask_sin NaN");
    c = good, c.init_xyz[1] = std::numeric_limits<double>::infinity();
    expect_refusal(call(3, 5, &c), GAT_ERR_ARG, "init_xyz inf");
    c = good, c.flags = 1;
    expect_refusal(call(3, 5, &c), GAT_ERR_ARG, "flags");
    expect_refusal(call(3, GAT_MAX_FIX_CHANNELS + 1, &good), GAT_ERR_RANGE, "K = 65");
    expect_refusal(call(GAT_MAX_FIX_EPOCHS + 1, 5, &good), GAT_ERR_RANGE, "E = 2^24 + 1");
}

int plans(std::mt19937_64 &rng, int count)
{
    const gat_fix_config cfg = config();
    for (int n = 0; n < count; ++n) {
        const int E = n < 40 ? n + 1 : (int)std::ldexp(1.0, (int)(rng() % 25)) - (int)(rng() % 7 == 0 ? 0 : rng() % 1000);
        const int K = 1 + (int)(rng() % GAT_MAX_FIX_CHANNELS);
        if (E < 1 || E > GAT_MAX_FIX_EPOCHS) {
            --n;
            continue;
        }
        FixPlan p{};
        const Refusal r = fix_plan(call(E, K, &cfg), &p);
        CHECK(r.code == GAT_OK, "E %d K %d refused", E, K);
        gat_fix_plan rep{};
        fix_report(p, &rep);
        CHECK(rep.workgroups == p.groups && rep.threads == kFixThreads && rep.waves_per_workgroup == kFixWaves && rep.scratch_bytes == 0, "report");
        CHECK(p.groups * kFixWaves >= E && (p.groups - 1) * kFixWaves < E, "E %d: %lld groups", E, p.groups);
        CHECK(rep.lds_bytes == kFixWaves * kFixWaveDoubles * 8 && kFixTerms * kFixPitch + kFixTerms <= kFixWaveDoubles, "LDS");
        if (E > 20000) continue;
        // every (epoch, channel) once: lane k < K of the wave that fix_epoch_unit gives the epoch
        std::vector<uint8_t> seen((size_t)E * K, 0);
        for (long long g = 0; g < p.groups; ++g)
            for (int w = 0; w < kFixWaves; ++w) {
                int e;
                if (!fix_epoch_unit(g, w, E, &e)) continue;
                CHECK(e >= 0 && e < E, "epoch %d of %d", e, E);
                for (int lane = 0; lane < kFixWave; ++lane) {
                    if (lane >= K) continue;
                    const int top = (kFixTerms - 1) * kFixPitch + lane; // the lane's last term in the wave's LDS
                    CHECK(top < kFixTerms * kFixPitch, "LDS index");
                    seen[(size_t)e * K + lane] += 1;
                }
            }
        for (uint8_t s : seen) CHECK(s == 1, "a unit covered %d times (E %d K %d)", (int)s, E, K);
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
        g.wn = 77, g.iodc = 300 + k, g.iode = (300 + k) & 0xff, g.ura = 2, g.health = 0, g.fit = k & 1;
        g.toe = 208800.0, g.toc = 208784.0;
        g.af0 = 2e-4 * u(rng), g.af1 = 3e-12 * u(rng), g.af2 = 0.0, g.tgd = 8e-9 * u(rng);
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

int twins(std::mt19937_64 &rng, int count)
{
    std::uniform_real_distribution<double> u(-1.0, 1.0);
    int calls = 0;
    for (int n = 0; n < count; ++n) {
        const int K = n % 4 == 0 ? GAT_MAX_FIX_CHANNELS : 8 + (int)(rng() % 40);
        const int E = 1 + (int)(rng() % 6);
        const std::vector<gat_ephemeris> ephs = constellation(rng, K);
        std::vector<int32_t> tx_ms((size_t)E * K), rx_ms((size_t)E);
        std::vector<double> tx_frac((size_t)E * K), rx_frac((size_t)E), truth((size_t)E * 4);
        std::vector<int> seen((size_t)E, 0);
        const int dead = E > 2 ? (int)(rng() % E) : -1; // an epoch without a measurement
        for (int e = 0; e < E; ++e) {
            const double lat = 1.4 * u(rng), lon = 3.1 * u(rng), r = 6371e3 + 1000.0 * u(rng);
            double *x = &truth[(size_t)e * 4];
            x[0] = r * std::cos(lat) * std::cos(lon), x[1] = r * std::cos(lat) * std::sin(lon), x[2] = r * std::sin(lat), x[3] = 2e-4 * u(rng);
            rx_ms[(size_t)e] = 208800000 + (int32_t)(3000000.0 * u(rng)), rx_frac[(size_t)e] = 5e-4 * (1.0 + u(rng)) * 0.999;
            for (int k = 0; k < K; ++k) {
                const size_t o = (size_t)e * K + k;
                const bool ok = e != dead && measure(ephs[(size_t)k], x, rx_ms[(size_t)e], rx_frac[(size_t)e], x[3], &tx_ms[o], &tx_frac[o]);
                if (!ok) tx_ms[o] = -1, tx_frac[o] = 0.0;
                seen[(size_t)e] += ok ? 1 : 0;
            }
        }
        gat_fix_config cfg = config(12, 1e-6, n % 3 == 0 ? 0.17 : -1.0);
        for (unsigned outs = 0; outs < 16; ++outs)
            for (int wt = 0; wt < 2; ++wt) {
                Heap<double> sat((size_t)E * K * 4, outs & 1), resid((size_t)E * K, outs & 2), sel((size_t)E * K, outs & 4), w((size_t)E * K, wt);
                Heap<uint8_t> used((size_t)E * K, outs & 8);
                for (double &v : w.v) v = 1.0 + 0.5 * u(rng);
                std::vector<gat_fix> fixes((size_t)E);
                FixPlan p{};
                const Refusal r = fix_plan(FixCall{ephs.data(), tx_ms.data(), tx_frac.data(), rx_ms.data(), rx_frac.data(), E, K, &cfg, fixes.data()}, &p);
                CHECK(r.code == GAT_OK, "twin call refused");
                fix_host_run(p, ephs.data(), tx_ms.data(), tx_frac.data(), rx_ms.data(), rx_frac.data(), w.ptr(), fixes.data(), sat.ptr(), resid.ptr(),
                             sel.ptr(), used.ptr());
                ++calls;
                for (int e = 0; e < E; ++e) {
                    const gat_fix &f = fixes[(size_t)e];
                    const double *x = &truth[(size_t)e * 4];
                    CHECK(f.num_valid == seen[(size_t)e], "epoch %d: %d valid of %d seen", e, f.num_valid, seen[(size_t)e]);
                    if (seen[(size_t)e] < 4) {
                        CHECK(f.status == GAT_FIX_FEW_SATS && f.x == 0.0 && f.gdop == 0.0, "epoch %d: status %d", e, f.status);
                        continue;
                    }
                    if (seen[(size_t)e] < 6) continue; // too few for a bound on the geometry
                    const double err = std::sqrt((f.x - x[0]) * (f.x - x[0]) + (f.y - x[1]) * (f.y - x[1]) + (f.z - x[2]) * (f.z - x[2]));
                    CHECK((f.status & ~(GAT_FIX_MASKED | GAT_FIX_MASK_STARVED)) == 0, "epoch %d: status %d", e, f.status);
                    CHECK(err < 1e-3 && std::fabs(f.clock_bias_s - x[3]) < 1e-11, "epoch %d: %g m, %g s off", e, err, f.clock_bias_s - x[3]);
                    CHECK(f.num_used >= 4 && f.num_used <= f.num_valid && f.pdop > 0.0 && f.gdop >= f.pdop, "epoch %d: counts and dop", e);
                }
            }
    }
    return calls;
}

void ephemeris_table(std::mt19937_64 &rng)
{
    int count;
    const EphField *f = eph_fields(&count);
    // the fields of a subframe do not overlap and stay inside the payload
    for (int sf = 1; sf <= 3; ++sf) {
        int cover[kEphPayloadBits] = {};
        for (int n = 0; n < count; ++n) {
            if (f[n].sf != sf) continue;
            for (int i = 0; i < f[n].bits; ++i) {
                CHECK(f[n].first + i < kEphPayloadBits, "field %d leaves the payload", n);
                cover[f[n].first + i] += 1;
            }
            for (int i = 0; i < f[n].bits2; ++i) cover[f[n].first2 + i] += 1;
        }
        for (int i = 0; i < kEphPayloadBits; ++i) CHECK(cover[i] <= 1, "subframe %d bit %d in %d fields", sf, i, cover[i]);
    }
    for (int n = 0; n < 50; ++n) {
        gat_ephemeris g = constellation(rng, 1)[0];
        uint8_t bits[3 * kEphPayloadBits];
        eph_encode(&g, bits);
        gat_nav_frame frames[5] = {};
        for (int sf = 1; sf <= 3; ++sf) {
            gat_nav_frame &fr = frames[sf]; // frames 0 and 4 stay empty
            fr.status = kEphLnavGood, fr.id = sf;
            for (int i = 0; i < kEphPayloadBits; ++i) fr.words[2 + i / 24] |= (uint32_t)bits[(sf - 1) * kEphPayloadBits + i] << (29 - i % 24);
        }
        gat_ephemeris q1, q2;
        eph_decode(frames, 5, &q1);
        CHECK(q1.valid == 1 && q1.reason == GAT_EPH_OK, "decode: reason %d", q1.reason);
        eph_encode(&q1, bits);
        for (int sf = 1; sf <= 3; ++sf) {
            gat_nav_frame &fr = frames[sf];
            std::memset(fr.words, 0, sizeof fr.words);
            for (int i = 0; i < kEphPayloadBits; ++i) fr.words[2 + i / 24] |= (uint32_t)bits[(sf - 1) * kEphPayloadBits + i] << (29 - i % 24);
        }
        eph_decode(frames, 5, &q2);
        CHECK(std::memcmp(&q1, &q2, sizeof q1) == 0, "the quantised ephemeris does not come back");
        CHECK(std::fabs(q1.m0 - g.m0) < 2e-9 && std::fabs(q1.sqrt_a - g.sqrt_a) < 2e-6 && q1.iodc == g.iodc && q1.toe == g.toe, "quantisation");
        frames[2].status &= ~4; // a parity bit of subframe 2
        eph_decode(frames, 5, &q2);
        CHECK(q2.valid == 0 && q2.reason == GAT_EPH_MISSING, "bad parity: reason %d", q2.reason);
        eph_decode(frames, 0, &q2);
        CHECK(q2.valid == 0 && q2.reason == GAT_EPH_MISSING, "no frames: reason %d", q2.reason);
    }
}

int sincos_grid(const char *path)
{
    std::FILE *out = std::fopen(path, "wb");
    if (!out) return 2;
    auto put = [&](double x) {
        double v[3] = {x, 0.0, 0.0};
        fix_sincos(x, &v[1], &v[2]);
        std::fwrite(v, sizeof(double), 3, out);
    };
    auto around = [&](double x) { // x with four neighbours each side
        double lo = x, hi = x;
        put(x);
        for (int j = 0; j < 4; ++j) {
            lo = std::nextafter(lo, -std::numeric_limits<double>::infinity()), hi = std::nextafter(hi, std::numeric_limits<double>::infinity());
            put(lo), put(hi);
        }
    };
    const int n = 450000; // the density of the grid on [-64, 64] before it reached 72: Omega goes to +-69.3
    for (int i = 0; i <= n; ++i) put(-72.0 + 144.0 * (double)i / n);
    for (int k = -92; k <= 92; ++k) around((double)k * 0.78539816339744831); // the reduction's boundaries and its zeros
    // every power of two from 64 to the largest, both signs: a sine up to 2^20, defined (and equal in both builds) beyond, where the
    // quadrant's q passes 2^53, 2^63 and every other width a conversion could have; then what is not finite
    for (int k = 6; k <= 1023; ++k) around(std::ldexp(1.0, k)), around(-std::ldexp(1.0, k));
    put(std::numeric_limits<double>::infinity()), put(-std::numeric_limits<double>::infinity()), put(std::numeric_limits<double>::quiet_NaN());
    std::fclose(out);
    return 0;
}

} // namespace

int main(int argc, char **argv)
{
    if (argc == 3 && std::strcmp(argv[1], "sincos") == 0) return sincos_grid(argv[2]);
    std::mt19937_64 rng(20261020);
    refusals();
    const int planned = plans(rng, 3000);
    const int calls = twins(rng, 12);
    ephemeris_table(rng);
    std::printf("planned %d calls, ran the twin %d times, %d failures\n", planned, calls, failures);
    return failures ? 1 : 0;
}
