// Stand-alone check of the FFT acquisition search's pure plan (csrc/gat_acq_fft_plan.h) and of the host loops of its rule
// (csrc/gat_acq_fft.h), over a few thousand random calls.  Every planned call must take the transform length that minimises
// G F log2 F (or the forced one), cover the lag axis with its segments so that every bin has exactly one (segment, lag) owner and no
// lag outside [0, Jseg) is read, carve the scratch into disjoint aligned regions inside the 1 GiB bound that hold what the launch
// sequence puts there for every batch, and deal every (block, antenna) unit to exactly one (batch, step, group) in order; every
// refusal must return its code with nothing planned.  The host loops then run a sample of the planned calls on heap buffers sized
// to the descriptors' exact extents, so that AddressSanitizer sees any read before a block's first sample or past its last one or
// outside a code row, and a few bins are held to the contract's sum in long double.  Built with -fsanitize=address,undefined by
// tests/test_acquisition_fft_plan_host.py.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "gat_acq_fft.h"
#include "gat_acq_fft_plan.h"

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

AcqFftPlan untouched_plan()
{
    AcqFftPlan p;
    std::memset(&p, 0x5a, sizeof p);
    return p;
}
bool untouched(const AcqFftPlan &p)
{
    const AcqFftPlan q = untouched_plan();
    return std::memcmp(&p, &q, sizeof p) == 0;
}

gat_signal_desc desc(uintptr_t re, uintptr_t im, int layout, int M, long long N, long long as, long long bs)
{
    gat_signal_desc d{};
    d.re = reinterpret_cast<const void *>(re);
    d.im = layout == GAT_LAYOUT_PLANAR ? reinterpret_cast<const void *>(im) : nullptr;
    d.layout = layout;
    d.num_ants = M;
    d.num_samples = N;
    d.ant_stride = as;
    d.block_stride = bs;
    d.chan_stride = 0;
    return d;
}

gat_acq_config config(int D, int J, int s, long long first_shift, int Lc)
{
    gat_acq_config c{};
    c.struct_size = sizeof(gat_acq_config);
    c.num_doppler_bins = D;
    c.num_code_bins = J;
    c.code_step_samples = s;
    c.if_hz = 1000.0;
    c.code_freq_hz = 1.023e6;
    c.doppler_first_hz = -500.0;
    c.doppler_step_hz = 250.0;
    c.first_shift = first_shift;
    c.code_length = Lc;
    return c;
}

void expect_refusal(const gat_signal_desc *s, int B, int P, double fs, const gat_acq_config *c, AcqFftOptions o, int cus, int code, const char *what)
{
    AcqFftPlan p = untouched_plan();
    const Refusal r = acq_fft_plan(s, B, P, fs, c, o, cus, true, s ? &p : &p);
    CHECK(r.code == code, "%s: got %d, want %d", what, r.code, code);
    CHECK(r.code == GAT_OK || r.msg != nullptr, "%s: a refusal without a message", what);
    CHECK(untouched(p), "%s: a refused call planned something", what);
}

// everything a planned call promises
void check_plan(const AcqFftPlan &p, const gat_acq_config &c, const AcqFftOptions &o, int cus, bool own_power, int forced_log2)
{
    CHECK(p.F == (1ll << p.L) && p.F > p.N && p.L >= kAcqFftMinLog2 && p.L <= kAcqFftMaxLog2, "F 2^%d for N %lld", p.L, p.N);
    CHECK(p.Jseg == p.F - p.N + 1, "Jseg %lld", p.Jseg);
    const long long lags = (long long)p.s * (p.J - 1) + 1;
    CHECK((long long)p.G * p.Jseg >= lags && (long long)(p.G - 1) * p.Jseg < lags, "G %d of %lld lags, %lld a segment", p.G, lags, p.Jseg);
    if (forced_log2)
        CHECK(p.L == forced_log2, "forced 2^%d, planned 2^%d", forced_log2, p.L);
    else
        for (int v = kAcqFftMinLog2; v <= kAcqFftMaxLog2; ++v) {
            const long long F = 1ll << v, js = F - p.N + 1;
            if (F <= p.N) continue;
            const long long g = (lags + js - 1) / js;
            CHECK((long long)p.G * p.F * p.L < g * F * v || ((long long)p.G * p.F * p.L == g * F * v && p.L <= v), "2^%d is cheaper than the planned 2^%d", v, p.L);
        }
    CHECK(p.passes == (p.L <= 12 ? 1 : 2) && p.L1 + p.L2 == p.L && (p.passes == 1 ? p.L2 == 0 && p.tiles == 1 : p.L1 == (p.L + 1) / 2 && p.tiles == (int)(p.F >> 12)),
          "passes %d: %d + %d stages, %d tiles", p.passes, p.L1, p.L2, p.tiles);
    CHECK(p.passes == 1 || (p.L1 <= 9 && p.L2 >= 6 && p.L2 <= 9), "a pass of %d / %d stages: columns of a tile outside 8 .. 64", p.L1, p.L2);
    // groups and batches
    CHECK(p.units == (long long)p.B * p.M && p.Gu >= 1 && p.Gu <= p.units, "Gu %d of %lld units", p.Gu, p.units);
    CHECK(p.Ub >= p.Gu && p.Ub % p.Gu == 0, "a unit batch of %d is not whole steps of %d", p.Ub, p.Gu);
    CHECK(p.Db >= 1 && p.Db <= p.D, "Doppler batch %d of %d", p.Db, p.D);
    if (o.dbatch > 0) CHECK(p.Db == (o.dbatch < p.D ? o.dbatch : p.D), "forced Doppler batch %d, planned %d", o.dbatch, p.Db);
    if (o.groups == 0) {
        const double wgs = (double)p.P * p.D * p.G * p.tiles;
        if (wgs >= 2.0 * cus) CHECK(p.Gu == 1, "%g workgroups fill %d compute units, yet %d groups", wgs, cus, p.Gu);
    } else
        CHECK(p.Gu == o.groups, "forced %d groups, planned %d", o.groups, p.Gu);
    // the walk the entry point makes: every unit in exactly one (batch, step, group), in order within its group; blocks of a batch fit Bb
    std::vector<int> seen((size_t)p.units, 0);
    std::vector<long long> last((size_t)p.Gu, -1);
    for (long long ub = 0; ub < p.units; ub += p.Ub) {
        const long long un = p.Ub < p.units - ub ? p.Ub : p.units - ub;
        const long long b0 = ub / p.M, bn = (ub + un - 1) / p.M - b0 + 1;
        CHECK(bn >= 1 && bn <= p.Bb && b0 + bn <= p.B, "batch at unit %lld spans %lld blocks, Bb %d", ub, bn, p.Bb);
        for (long long us = ub; us < ub + un; us += p.Gu)
            for (int k = 0; k < p.Gu; ++k) {
                const long long u = us + k;
                if (u >= ub + un) continue;
                CHECK(u % p.Gu == k && u > last[(size_t)k], "unit %lld in group %d after %lld", u, k, last[(size_t)k]);
                last[(size_t)k] = u;
                ++seen[(size_t)u];
            }
    }
    for (size_t u = 0; u < seen.size(); ++u)
        if (seen[u] != 1) {
            CHECK(false, "unit %zu walked %d times", u, seen[u]);
            break;
        }
    for (int k = 0; k < p.Gu; ++k) CHECK(last[(size_t)k] >= 0, "group %d has no unit", k);
    // the carve-up: ordered, aligned, each region as large as its contents, inside the bound
    const size_t F8 = (size_t)p.F * 8, cells4 = (size_t)p.P * p.D * p.J * 4;
    const size_t offs[] = {p.off_res, p.off_pow, p.off_tw, p.off_C, p.off_W, p.off_Y, p.off_part, p.off_prn, p.bytes};
    const size_t need[] = {(size_t)p.P * sizeof(gat_acq_result), own_power ? cells4 : 0, F8 / 2, (size_t)p.P * p.Bb * p.G * F8, (size_t)p.Ub * p.Db * F8,
                           p.passes == 2 ? (size_t)p.Gu * p.P * p.Db * p.G * F8 : 0, p.Gu > 1 ? (size_t)p.Gu * cells4 : 0, (size_t)p.P * 4};
    for (int i = 0; i < 8; ++i) CHECK(offs[i] % 256 == 0 && offs[i + 1] >= offs[i] + need[i], "scratch region %d: [%zu, %zu) for %zu bytes", i, offs[i], offs[i + 1], need[i]);
    CHECK(p.bytes <= kAcqFftMaxScratch, "%zu bytes of scratch", p.bytes);
    (void)c;
}

// every bin has exactly one (segment, lag) owner, and the lags read are those of [0, Jseg)
void check_walk(const AcqFftPlan &p)
{
    std::vector<unsigned char> hits((size_t)p.J, 0);
    for (int g = 0; g < p.G; ++g) {
        CHECK(acq_fft_lag_bin(-1, g, p.Jseg, p.s, p.J) == -1 && acq_fft_lag_bin(p.Jseg, g, p.Jseg, p.s, p.J) == -1, "segment %d: a lag outside [0, Jseg) has a bin", g);
        for (long long l = 0; l < p.Jseg; ++l) {
            const int j = acq_fft_lag_bin(l, g, p.Jseg, p.s, p.J);
            if (j < 0) continue;
            CHECK(j < p.J && (long long)p.s * j == l + (long long)g * p.Jseg, "segment %d lag %lld owns bin %d", g, l, j);
            if (j < p.J) ++hits[(size_t)j];
        }
    }
    for (size_t j = 0; j < hits.size(); ++j)
        if (hits[j] != 1) {
            CHECK(false, "bin %zu has %d owners", j, (int)hits[j]);
            break;
        }
}

// the host loops on buffers of the exact extent; a few bins against the contract's sum in long double
void run_host_loop(std::mt19937_64 &rng, int li, int B, int M, long long N, long long as, long long bs, int D, int J, int s, long long first_shift, int Lc, int log2F, int groups)
{
    auto pick = [&](long long a, long long b) { return (long long)(rng() % (uint64_t)(b - a + 1)) + a; };
    const size_t in_samples = (size_t)((B - 1) * bs + (M - 1) * as + N), in_bytes = in_samples * layout_sample_bytes(li);
    std::vector<unsigned char> in_re(in_bytes), in_im(li == GAT_LAYOUT_PLANAR ? in_bytes : 0);
    if (li <= GAT_LAYOUT_INTERLEAVED) {
        for (size_t i = 0; i + 4 <= in_bytes; i += 4) {
            const float a = (float)pick(-1000, 1000) / 16.0f, b = (float)pick(-1000, 1000) / 16.0f;
            std::memcpy(&in_re[i], &a, 4);
            if (li == GAT_LAYOUT_PLANAR) std::memcpy(&in_im[i], &b, 4);
        }
    } else {
        for (auto &v : in_re) v = (unsigned char)pick(0, 255);
    }
    const int P = 2, rows = 3;
    std::vector<int8_t> codes((size_t)rows * Lc); // rows of exactly Lc chips: a chip index outside [0, Lc) of the last row is seen
    for (auto &v : codes) v = (int8_t)(pick(0, 1) ? 1 : -1);
    const int32_t prns[P] = {2, 0};
    const double fs = 2.0e6;
    const gat_signal_desc sg = desc(reinterpret_cast<uintptr_t>(in_re.data()), reinterpret_cast<uintptr_t>(in_im.data()), li, M, N, as, bs);
    const gat_acq_config c = config(D, J, s, first_shift, Lc);
    AcqFftPlan p = untouched_plan();
    const Refusal r = acq_fft_plan(&sg, B, P, fs, &c, AcqFftOptions{log2F, 0, 0, groups}, 1, false, &p);
    CHECK(r.code == GAT_OK, "host loop: a valid call was refused: %d %s", r.code, r.msg ? r.msg : "");
    if (r.code != GAT_OK) return;
    std::vector<float> out((size_t)P * D * J, -3.25f);
    acq_fft_host_run(&sg, codes.data(), Lc, prns, fs, c, p, out.data());
    const long double two_pi = 6.283185307179586476925286766559L;
    const double ratio = c.code_freq_hz / fs;
    for (int k = 0; k < 6; ++k) {
        const int pi = (int)pick(0, P - 1), i = (int)pick(0, D - 1), j = k == 0 ? 0 : k == 1 ? J - 1 : (int)pick(0, J - 1);
        const long double f = ((long double)c.if_hz + ((long double)c.doppler_first_hz + (long double)i * c.doppler_step_hz)) / fs;
        long double sum = 0, A2 = 0;
        for (int b = 0; b < B; ++b)
            for (int m = 0; m < M; ++m) {
                const double tau = std::fmod(ratio * (double)((long long)b * bs), (double)Lc);
                long double rr = 0, ri = 0, A = 0;
                for (long long n = 0; n < N; ++n) {
                    float xr, xi;
                    host_load_sample(&sg, (size_t)(b * bs + m * as + n), &xr, &xi);
                    const long long x = n + first_shift + (long long)s * j;
                    const double ph = ratio * (double)x + tau;
                    long long ip = (long long)std::floor(ph) % Lc;
                    if (ip < 0) ip += Lc;
                    const long double ch = codes[(size_t)prns[pi] * Lc + (size_t)ip], th = two_pi * (f * (long double)n - floorl(f * (long double)n));
                    const long double cc = cosl(th), ss = sinl(th);
                    rr += ch * (xr * cc + xi * ss);
                    ri += ch * (xi * cc - xr * ss);
                    A += fabsl(xr) + fabsl(xi);
                }
                sum += rr * rr + ri * ri;
                A2 += A * A;
            }
        // every R is within (about) 40 log2 F u A of the truth (three transforms and the carrier), so the power within 2 A times that
        const long double lim = 2.0L * 40.0L * p.L * 0x1p-24L * A2 + 1e-30L;
        const float got = out[((size_t)pi * D + i) * J + j];
        CHECK(fabsl(got - sum) <= lim, "host loop: bin (%d, %d, %d) off by %Lg of %Lg (power %Lg)", pi, i, j, fabsl(got - sum), lim, sum);
    }
}

} // namespace

int main()
{
    std::mt19937_64 rng(20261019);
    auto pick = [&](long long lo, long long hi) { return (long long)(rng() % (uint64_t)(hi - lo + 1)) + lo; };
    int planned = 0, two_pass = 0, grouped = 0, batched = 0, multi_seg = 0, ran = 0;
    const double fs = 2.0e6;
    for (int it = 0; it < 3000; ++it) {
        const int li = (int)pick(0, 3), Lc = (int)(it % 3 == 0 ? 1023 : pick(31, 10230));
        const int M = (int)(it % 5 == 0 ? pick(1, 16) : pick(1, 4)), B = (int)(it % 7 == 0 ? pick(1, 40) : pick(1, 3));
        const long long N = it % 4 == 0 ? pick(1, 2000) : it % 4 == 1 ? pick(2000, 20000) : it % 4 == 2 ? pick(20000, 70000) : pick(1, (1 << 18) - 1);
        const int s = (int)(it % 2 ? 1 : pick(1, kAcqMaxCodeStep));
        const int P = (int)(it % 6 == 0 ? pick(1, 32) : pick(1, 4)), D = (int)(it % 6 == 1 ? pick(1, 61) : pick(1, 5));
        const int J = (int)(it % 9 == 0 ? pick(1, 200000 / (P * D) + 1) : pick(1, 3000));
        const long long first_shift = pick(-5000, 5000);
        const long long bs = N + pick(0, 9), as = (B - 1) * bs + N + pick(0, 5);
        const gat_signal_desc sg = desc(0x100000000000ull, 0x300000000000ull, li, M, N, as, bs);
        const gat_acq_config c = config(D, J, s, first_shift, Lc);
        int forced = 0;
        if (it % 3 == 1) {
            int lo = kAcqFftMinLog2;
            while ((1ll << lo) <= N) ++lo;
            forced = (int)pick(lo, kAcqFftMaxLog2);
        }
        const AcqFftOptions o{forced, (int)(it % 5 == 2 ? pick(1, D + 2) : 0), (int)(it % 5 == 3 ? pick(1, M * B + 2) : 0), (int)(it % 8 == 5 ? pick(1, M * B) : 0)};
        const int cus = (int)(it % 2 ? 256 : pick(1, 304));
        const bool own = it % 2 == 0;
        AcqFftPlan p = untouched_plan();
        const Refusal r = acq_fft_plan(&sg, B, P, fs, &c, o, cus, own, &p);
        if (r.code == GAT_ERR_RANGE && r.msg && std::strstr(r.msg, "scratch")) { // short segments of a long grid: a refusal, with nothing planned
            CHECK(untouched(p), "a refused call planned something");
            continue;
        }
        CHECK(r.code == GAT_OK, "a valid call was refused: %d %s", r.code, r.msg ? r.msg : "");
        if (r.code != GAT_OK) continue;
        ++planned;
        two_pass += p.passes == 2, grouped += p.Gu > 1, batched += p.Db < p.D || p.Ub < p.units, multi_seg += p.G > 1;
        check_plan(p, c, o, cus, own, forced);
        if ((long long)p.G * p.Jseg <= 400000) check_walk(p);

        // the refusals, each from this valid call
        gat_signal_desc t = sg;
        gat_acq_config k = c;
        const AcqFftOptions z{0, 0, 0, 0};
        expect_refusal(nullptr, B, P, fs, &c, z, cus, GAT_ERR_ARG, "null signal");
        expect_refusal(&sg, B, P, fs, nullptr, z, cus, GAT_ERR_ARG, "null config");
        k = c, k.struct_size = 8;
        expect_refusal(&sg, B, P, fs, &k, z, cus, GAT_ERR_ARG, "struct_size");
        k = c, k.reserved = 1;
        expect_refusal(&sg, B, P, fs, &k, z, cus, GAT_ERR_ARG, "reserved");
        expect_refusal(&sg, B, 0, fs, &c, z, cus, GAT_ERR_ARG, "no PRNs");
        k = c, k.num_doppler_bins = 0;
        expect_refusal(&sg, B, P, fs, &k, z, cus, GAT_ERR_ARG, "no Doppler bins");
        k = c, k.num_code_bins = 0;
        expect_refusal(&sg, B, P, fs, &k, z, cus, GAT_ERR_ARG, "no code bins");
        k = c, k.code_step_samples = 0;
        expect_refusal(&sg, B, P, fs, &k, z, cus, GAT_ERR_ARG, "no code step");
        k = c, k.code_step_samples = kAcqMaxCodeStep + 1;
        expect_refusal(&sg, B, P, fs, &k, z, cus, GAT_ERR_RANGE, "code step above 31");
        k = c, k.num_doppler_bins = 4096, k.num_code_bins = 20000;
        expect_refusal(&sg, B, P, fs, &k, z, cus, GAT_ERR_RANGE, "above 2^26 bins");
        expect_refusal(&sg, B, P, 0.0, &c, z, cus, GAT_ERR_ARG, "no sampling frequency");
        k = c, k.code_freq_hz = -1.0;
        expect_refusal(&sg, B, P, fs, &k, z, cus, GAT_ERR_ARG, "negative code frequency");
        k = c, k.if_hz = NAN;
        expect_refusal(&sg, B, P, fs, &k, z, cus, GAT_ERR_ARG, "NaN frequency");
        k = c, k.if_hz = 3.0e12;
        expect_refusal(&sg, B, P, fs, &k, z, cus, GAT_ERR_RANGE, "carrier out of range");
        k = c, k.code_length = 0;
        expect_refusal(&sg, B, P, fs, &k, z, cus, GAT_ERR_ARG, "no code length");
        expect_refusal(&sg, 0, P, fs, &c, z, cus, GAT_ERR_ARG, "no blocks");
        t = sg, t.layout = 4;
        expect_refusal(&t, B, P, fs, &c, z, cus, GAT_ERR_ARG, "bad layout");
        t = sg, t.im = li == GAT_LAYOUT_PLANAR ? nullptr : t.re;
        expect_refusal(&t, B, P, fs, &c, z, cus, GAT_ERR_ARG, "signal planes");
        t = sg, t.num_samples = 0;
        expect_refusal(&t, B, P, fs, &c, z, cus, GAT_ERR_ARG, "no samples");
        t = sg, t.num_ants = 0;
        expect_refusal(&t, B, P, fs, &c, z, cus, GAT_ERR_ARG, "no antennas");
        t = sg, t.chan_stride = 8;
        expect_refusal(&t, B, P, fs, &c, z, cus, GAT_ERR_ARG, "chan_stride");
        t = sg, t.num_samples = 1 << kAcqFftMaxLog2;
        expect_refusal(&t, B, P, fs, &c, z, cus, GAT_ERR_RANGE, "N as long as the largest transform");
        if (N >= 1024) {
            int v = kAcqFftMinLog2;
            while ((2ll << v) <= N) ++v;
            expect_refusal(&sg, B, P, fs, &c, AcqFftOptions{v, 0, 0, 0}, cus, GAT_ERR_RANGE, "forced F <= N");
        }
        expect_refusal(&sg, B, P, fs, &c, AcqFftOptions{kAcqFftMinLog2 - 1, 0, 0, 0}, cus, GAT_ERR_RANGE, "forced log2 F = 9");
        expect_refusal(&sg, B, P, fs, &c, AcqFftOptions{kAcqFftMaxLog2 + 1, 0, 0, 0}, cus, GAT_ERR_RANGE, "forced log2 F = 19");
        expect_refusal(&sg, B, P, fs, &c, AcqFftOptions{0, -1, 0, 0}, cus, GAT_ERR_ARG, "negative Doppler batch");
        expect_refusal(&sg, B, P, fs, &c, AcqFftOptions{0, 0, 0, M * B + 1}, cus, GAT_ERR_ARG, "more groups than units");
        expect_refusal(&sg, B, P, fs, &c, z, 0, GAT_ERR_ARG, "no compute units");
        k = c, k.first_shift = 1ll << 30;
        expect_refusal(&sg, B, P, fs, &k, z, cus, GAT_ERR_RANGE, "first_shift beyond 2^30 samples");
        k = c, k.code_length = 3, k.first_shift = 20000000; // 2^21 laps of a three-chip code
        expect_refusal(&sg, B, P, fs, &k, z, cus, GAT_ERR_RANGE, "code phase span");
        if (M > 1) {
            t = sg, t.ant_stride = 0;
            expect_refusal(&t, B, P, fs, &c, z, cus, GAT_ERR_ARG, "zero ant_stride");
        }
        if (B > 1) {
            t = sg, t.block_stride = 0;
            expect_refusal(&t, B, P, fs, &c, z, cus, GAT_ERR_ARG, "zero block_stride");
        }
    }
    // the host loops, on small calls of every layout: odd sizes, blocks that do not abut, several segments and groups
    for (int it = 0; it < 400 && ran < 48; ++it) {
        const int li = it % 4, Lc = (int)(it % 3 == 0 ? 1023 : pick(31, 4000));
        const int M = (int)pick(1, 3), B = (int)pick(1, 3), D = (int)pick(1, 3), s = (int)pick(1, 4), J = (int)pick(1, 1500);
        const long long N = pick(1, 3000), first_shift = pick(-3000, 3000), bs = N + pick(0, 9), as = (B - 1) * bs + N + pick(0, 5);
        int lo = kAcqFftMinLog2;
        while ((1ll << lo) <= N) ++lo;
        const int log2F = lo + (int)pick(0, 1);
        const long long F = 1ll << log2F, Jseg = F - N + 1, G = ((long long)s * (J - 1) + Jseg) / Jseg;
        if ((double)F * ((double)M * B * D + 2.0 * B * G + 2.0 * D * G * M * B) > 1.0e6) continue;
        run_host_loop(rng, li, B, M, N, as, bs, D, J, s, first_shift, Lc, log2F, (int)pick(1, M * B)), ++ran;
    }
    // the scratch bound: two lags a segment over a long grid
    {
        const gat_signal_desc sg = desc(0x100000000000ull, 0x300000000000ull, 0, 1, 1023, 1023, 1023);
        const gat_acq_config c = config(1, 1 << 20, 31, 0, 1023);
        expect_refusal(&sg, 1, 32, fs, &c, AcqFftOptions{10, 0, 0, 0}, 256, GAT_ERR_RANGE, "spectra beyond 1 GiB");
    }
    CHECK(planned > 2500 && two_pass > 800 && grouped > 300 && batched > 100 && multi_seg > 300 && ran > 40,
          "the sweep lost its balance: %d planned, %d in two passes, %d with groups, %d batched, %d with several segments, %d run", planned, two_pass, grouped,
          batched, multi_seg, ran);
    std::printf("planned %d calls (%d in two passes, %d with unit groups, %d batched, %d with several segments), ran the host loops on %d, %d failures\n", planned,
                two_pass, grouped, batched, multi_seg, ran, failures);
    return failures ? 1 : 0;
}
