// Stand-alone check of the sample spectrum's pure plan (csrc/gat_spec_plan.h) and of the host loop of its rule (csrc/gat_spec.h),
// over a few thousand random calls.  Every planned call must cover each (block, antenna) pair exactly once through the rounds and
// teams the kernel walks, dealt to the grid exactly once, with the aligned load path chosen exactly under its rule and a geometry
// whose every LDS index and every sample read stay inside their arrays; every documented refusal must return its code with
// nothing planned.  The host loop then runs a sample of the planned calls on heap buffers sized to the descriptors' exact
// extents, so that AddressSanitizer sees any read before a block's first sample or past its last one, and a few bins are held to
// a long double DFT.  Built with -fsanitize=address,undefined by tests/test_spectrum_plan_host.py.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "gat_spec.h"
#include "gat_spec_plan.h"

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

const SpecPlan kUntouched = {true, -7, -7, -7, -7, -7, -7, -7, -7};
bool untouched(const SpecPlan &p)
{
    return p.aligned && p.log2F == -7 && p.R == -7 && p.team == -7 && p.teams == -7 && p.S == -7 && p.units == -7 && p.rounds == -7 && p.grid == -7;
}

const float *const kWindow = reinterpret_cast<const float *>(uintptr_t(0x9000));
float *const kPower = reinterpret_cast<float *>(uintptr_t(0x700000000000ull));

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

gat_spectrum_config config(int F, int H, uint32_t flags = 0)
{
    gat_spectrum_config c{};
    c.struct_size = sizeof(gat_spectrum_config);
    c.num_bins = F;
    c.hop = H;
    c.flags = flags;
    return c;
}

void expect_refusal(const gat_signal_desc *s, int B, const float *w, const gat_spectrum_config *c, const float *o, int code, const char *what)
{
    SpecPlan p = kUntouched;
    const Refusal r = spec_plan(s, B, w, c, o, 2048, &p);
    CHECK(r.code == code, "%s: got %d, want %d", what, r.code, code);
    CHECK(r.code == GAT_OK || r.msg != nullptr, "%s: a refusal without a message", what);
    CHECK(untouched(p), "%s: a refused call planned something", what);
}

// walks the plan as the kernel does: rounds dealt to the grid, a team a unit; then the geometry of one transform
void check_cover(const SpecPlan &p, int B, int M, int F, int H, long long N)
{
    CHECK(p.units == (long long)B * M && p.rounds == (p.units + p.teams - 1) / p.teams, "units %lld rounds %lld", p.units, p.rounds);
    CHECK(p.grid >= 1 && p.grid <= p.rounds, "grid %lld of %lld rounds", p.grid, p.rounds);
    CHECK((1 << p.log2F) == F && p.R == (F / 256 > 4 ? F / 256 : 4) && p.team * p.R == F && p.teams * p.team == kSpecThreads, "geometry of F %d", F);
    CHECK(p.S >= 1 && p.S <= GAT_MAX_SPECTRUM_SEGMENTS && (p.S - 1) * H + F <= N && p.S * H + F > N, "S %lld of N %lld", p.S, N);
    std::vector<unsigned char> hits((size_t)p.units, 0);
    for (long long g = 0; g < p.grid; ++g)
        for (long long rd = g; rd < p.rounds; rd += p.grid)
            for (int tm = 0; tm < p.teams; ++tm) {
                const long long u = rd * p.teams + tm;
                if (u >= p.units) continue;
                long long b;
                int m;
                spec_unit(u, M, &b, &m);
                CHECK(b >= 0 && b < B && m >= 0 && m < M && b * M + m == u, "unit %lld: block %lld antenna %d", u, b, m);
                ++hits[(size_t)u];
            }
    for (size_t i = 0; i < hits.size(); ++i)
        if (hits[i] != 1) {
            CHECK(false, "unit %zu covered %d times", i, (int)hits[i]);
            break;
        }
}

// every pass of the kernel's walk over one transform: each point held by exactly one (lane, register), every twiddle number
// inside its array and the one the rule names, the skew a bijection, and the last pass's registers the bins i * team + t
void check_passes(int F)
{
    const int L = spec_ilog2(F), R = spec_lane_points(F), r = spec_ilog2(R), team = F / R;
    const int passes = (L + r - 1) / r, r0 = L - r * (passes - 1);
    std::vector<unsigned char> seen((size_t)F);
    std::fill(seen.begin(), seen.end(), 0);
    for (unsigned p = 0; p < (unsigned)F; ++p) {
        const unsigned q = spec_skew(p);
        CHECK(q < (unsigned)F && !seen[q], "the skew of %u", p);
        if (q < (unsigned)F) seen[q] = 1;
    }
    CHECK(passes >= 2 && r0 >= 1 && r0 <= r, "F %d: %d passes, the first of %d stages", F, passes, r0);
    int j = 0;
    for (int ps = 0; ps < passes; ++ps) {
        const int rs = ps == 0 ? r0 : r;
        std::fill(seen.begin(), seen.end(), 0);
        for (unsigned t = 0; t < (unsigned)team; ++t)
            for (unsigned i = 0; i < (unsigned)R; ++i) {
                unsigned v, ii;
                const unsigned idx = spec_point_index(t, i, R, j, rs, &v, &ii);
                CHECK(idx < (unsigned)F && !seen[idx < (unsigned)F ? idx : 0], "F %d pass %d: lane %u register %u holds %u", F, ps, t, i, idx);
                if (idx < (unsigned)F) seen[idx] = 1;
                if (ps == passes - 1) CHECK(idx == i * (unsigned)team + t, "F %d: the last pass's register %u of lane %u is bin %u", F, i, t, idx);
                for (int q = 0; q < rs; ++q) {
                    if (i & (1u << q)) continue;
                    unsigned v2, i2;
                    const unsigned partner = spec_point_index(t, i | (1u << q), R, j, rs, &v2, &i2);
                    const unsigned h = 1u << (j + q), k = ((ii & ((1u << q) - 1u)) << j) | (v & ((1u << j) - 1u));
                    // stage j + q pairs (2hg + k, 2hg + k + h), h = 2^(j + q), with twiddle number k F / (2h)
                    CHECK(partner == idx + h, "F %d pass %d stage %d: partner %u of %u", F, ps, j + q, partner, idx);
                    CHECK(k == (idx & (h - 1u)) && (k << (L - 1 - j - q)) < (unsigned)F / 2, "F %d pass %d stage %d: twiddle %u of index %u", F, ps, j + q, k, idx);
                }
            }
        j += rs;
    }
    CHECK(j == L, "F %d: %d stages walked", F, j);
}

// the host loop on buffers of the descriptor's exact extent; a few bins against a long double DFT
void run_host_loop(std::mt19937_64 &rng, int li, int B, int M, long long N, long long as, long long bs, int F, int H)
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
    std::vector<float> w((size_t)F), out((size_t)B * M * F, -3.25f);
    for (auto &v : w) v = (float)pick(-64, 64) / 64.0f;
    const gat_signal_desc s = desc(reinterpret_cast<uintptr_t>(in_re.data()), reinterpret_cast<uintptr_t>(in_im.data()), li, M, N, as, bs);
    const gat_spectrum_config c = config(F, H);
    SpecPlan p = kUntouched;
    const Refusal r = spec_plan(&s, B, w.data(), &c, out.data(), 64, &p);
    CHECK(r.code == GAT_OK, "host loop: a valid call was refused: %d %s", r.code, r.msg ? r.msg : "");
    if (r.code != GAT_OK) return;
    spec_host_run(&s, B, w.data(), F, H, out.data());
    const long double two_pi = 6.283185307179586476925286766559L;
    for (int k = 0; k < 4; ++k) {
        const int b = (int)pick(0, B - 1), m = (int)pick(0, M - 1), f = (int)pick(0, F - 1);
        long double sum = 0, lim = 0;
        for (long long sg = 0; sg < p.S; ++sg) {
            long double xr = 0, xi = 0, A = 0;
            for (int n = 0; n < F; ++n) {
                float sr, si;
                host_load_sample(&s, (size_t)(b * bs + m * as + sg * H + n), &sr, &si);
                const long double ph = two_pi * (long double)(((long long)f * n) % F) / F, cc = cosl(ph), ss = sinl(ph);
                xr += (long double)w[(size_t)n] * (sr * cc + si * ss);
                xi += (long double)w[(size_t)n] * (si * cc - sr * ss);
                A += fabsl(w[(size_t)n]) * (fabsl(sr) + fabsl(si));
            }
            const long double u = 0x1p-24L, E = (11 * p.log2F + 1) * u * A;
            sum += xr * xr + xi * xi;
            lim += (2 * A + E) * E + 2 * u * (1 + u) * (A + E) * (A + E) + (long double)(p.S - 1) * u * 1.001L * (A + E) * (A + E);
        }
        const float got = out[((size_t)b * M + m) * F + f];
        CHECK(fabsl(got - sum) <= lim, "host loop: bin (%d, %d, %d) off by %Lg of %Lg", b, m, f, fabsl(got - sum), lim);
    }
}

} // namespace

int main()
{
    std::mt19937_64 rng(20261019);
    auto pick = [&](long long lo, long long hi) { return (long long)(rng() % (uint64_t)(hi - lo + 1)) + lo; };
    int planned = 0, aligned = 0, ran = 0, looped = 0;
    for (int F = GAT_MIN_SPECTRUM_BINS; F <= GAT_MAX_SPECTRUM_BINS; F *= 2) check_passes(F);

    for (int it = 0; it < 3000; ++it) {
        const int li = (int)pick(0, 3), F = 64 << pick(0, 6);
        const int M = (int)(it % 5 == 0 ? pick(1, 64) : pick(1, 9)), B = (int)(it % 7 == 0 ? pick(1, 400) : pick(1, 4));
        const long long vi = layout_vec_samples(li);
        const bool tidy = it % 2 == 0; // aligned bases, strides and hop: the 16-byte loads' candidates
        int H = (int)(it % 3 == 0 ? F : it % 3 == 1 ? F / 2 : pick(1, F));
        if (tidy) H = (int)((H + vi - 1) / vi * vi);
        const long long S = it % 11 == 0 ? pick(1, GAT_MAX_SPECTRUM_SEGMENTS) : pick(1, 6);
        const long long N = (S - 1) * H + F + pick(0, H - 1);
        const bool continuing = it % 4 == 1; // blocks that continue each other: block_stride = S * H
        long long bs = continuing ? S * H : N + pick(0, 9);
        if (tidy) bs = (bs + vi - 1) / vi * vi;
        long long as = (B - 1) * bs + N + (tidy ? 0 : pick(0, 5));
        if (tidy) as = (as + vi - 1) / vi * vi;
        const uintptr_t off = tidy ? 0 : (uintptr_t)pick(0, 3) * layout_sample_bytes(li);
        const gat_signal_desc s = desc(0x100000000000ull + off, 0x300000000000ull + off, li, M, N, as, bs);
        const gat_spectrum_config c = config(F, H);
        const long long want = pick(1, 3) == 1 ? pick(1, 64) : 2048;
        SpecPlan p = kUntouched;
        const Refusal r = spec_plan(&s, B, kWindow, &c, kPower, want, &p);
        CHECK(r.code == GAT_OK, "a valid call was refused: %d %s", r.code, r.msg ? r.msg : "");
        if (r.code != GAT_OK) continue;
        ++planned;
        const bool rule = blocks_aligned(&s, B) && H % vi == 0;
        CHECK(p.aligned == rule, "aligned %d, the rule says %d", (int)p.aligned, (int)rule);
        CHECK(!tidy || p.aligned, "an aligned call did not take the 16-byte loads");
        CHECK(p.S == S, "S %lld, want %lld", p.S, S);
        CHECK(p.grid <= want, "grid %lld above the %lld wanted", p.grid, want);
        aligned += p.aligned, looped += p.rounds > p.grid;
        check_cover(p, B, M, F, H, N);
        if (it % 8 == 3 && (double)B * M * (double)S * F <= 3.0e5) run_host_loop(rng, li, B, M, N, as, bs, F, H), ++ran;

        // the refusals, each from this valid call
        gat_signal_desc t = s;
        gat_spectrum_config k = c;
        expect_refusal(nullptr, B, kWindow, &c, kPower, GAT_ERR_ARG, "null signal");
        expect_refusal(&s, B, nullptr, &c, kPower, GAT_ERR_ARG, "null window");
        expect_refusal(&s, B, kWindow, nullptr, kPower, GAT_ERR_ARG, "null config");
        expect_refusal(&s, B, kWindow, &c, nullptr, GAT_ERR_ARG, "null output");
        k = c, k.struct_size = sizeof(gat_spectrum_config) + 8;
        expect_refusal(&s, B, kWindow, &k, kPower, GAT_ERR_ARG, "struct_size");
        expect_refusal(&s, 0, kWindow, &c, kPower, GAT_ERR_ARG, "no blocks");
        k = c, k.flags = 1u << pick(0, 31);
        expect_refusal(&s, B, kWindow, &k, kPower, GAT_ERR_ARG, "flags");
        k = c, k.num_bins = F / 2 < GAT_MIN_SPECTRUM_BINS ? 32 : F + F / 2;
        expect_refusal(&s, B, kWindow, &k, kPower, GAT_ERR_RANGE, "num_bins not a power of two, or below 64");
        k = c, k.num_bins = 2 * GAT_MAX_SPECTRUM_BINS;
        expect_refusal(&s, B, kWindow, &k, kPower, GAT_ERR_RANGE, "num_bins above 4096");
        k = c, k.num_bins = 0;
        expect_refusal(&s, B, kWindow, &k, kPower, GAT_ERR_RANGE, "no bins");
        k = c, k.hop = 0;
        expect_refusal(&s, B, kWindow, &k, kPower, GAT_ERR_RANGE, "no hop");
        k = c, k.hop = F + 1;
        expect_refusal(&s, B, kWindow, &k, kPower, GAT_ERR_RANGE, "hop above num_bins");
        t = s, t.num_samples = 0;
        expect_refusal(&t, B, kWindow, &c, kPower, GAT_ERR_ARG, "no samples");
        t = s, t.num_samples = F - 1;
        expect_refusal(&t, B, kWindow, &c, kPower, GAT_ERR_ARG, "a block shorter than a segment");
        t = s, t.num_ants = 0;
        expect_refusal(&t, B, kWindow, &c, kPower, GAT_ERR_ARG, "no antennas");
        t = s, t.ant_stride = -1;
        expect_refusal(&t, B, kWindow, &c, kPower, GAT_ERR_ARG, "negative ant_stride");
        t = s, t.block_stride = -1;
        expect_refusal(&t, B, kWindow, &c, kPower, GAT_ERR_ARG, "negative block_stride");
        t = s, t.layout = 4;
        expect_refusal(&t, B, kWindow, &c, kPower, GAT_ERR_ARG, "bad layout");
        t = s;
        t.im = li == GAT_LAYOUT_PLANAR ? nullptr : t.re;
        expect_refusal(&t, B, kWindow, &c, kPower, GAT_ERR_ARG, "signal planes");
        t = s, t.chan_stride = 8;
        expect_refusal(&t, B, kWindow, &c, kPower, GAT_ERR_UNSUPPORTED, "chan_stride");
        t = s, t.num_ants = GAT_MAX_ARRAY_ANTS + 1;
        expect_refusal(&t, B, kWindow, &c, kPower, GAT_ERR_RANGE, "too many antennas");
        t = s, t.num_samples = (long long)GAT_MAX_SPECTRUM_SEGMENTS * H + F;
        expect_refusal(&t, B, kWindow, &c, kPower, GAT_ERR_RANGE, "4097 segments");
        if (M > 1) {
            t = s, t.ant_stride = 0;
            expect_refusal(&t, B, kWindow, &c, kPower, GAT_ERR_ARG, "zero ant_stride");
        }
        if (B > 1) {
            t = s, t.block_stride = 0;
            expect_refusal(&t, B, kWindow, &c, kPower, GAT_ERR_ARG, "zero block_stride");
        }
        // overlap: the output starts on the last byte of either input plane, or ends one byte into one
        const uintptr_t in_bytes = (uintptr_t)((B - 1) * bs + (M - 1) * as + N) * layout_sample_bytes(li);
        const uintptr_t out_bytes = (uintptr_t)B * M * F * sizeof(float);
        expect_refusal(&s, B, kWindow, &c, reinterpret_cast<const float *>(reinterpret_cast<uintptr_t>(s.re) + in_bytes - 1), GAT_ERR_ARG, "the output starts on the input's last byte");
        expect_refusal(&s, B, kWindow, &c, reinterpret_cast<const float *>(reinterpret_cast<uintptr_t>(s.re) - out_bytes + 1), GAT_ERR_ARG, "the output ends on the input's first byte");
        if (li == GAT_LAYOUT_PLANAR)
            expect_refusal(&s, B, kWindow, &c, reinterpret_cast<const float *>(reinterpret_cast<uintptr_t>(s.im) + in_bytes - 1), GAT_ERR_ARG, "the output starts on the last byte of the im plane");
        // an output that ends where the input begins, or begins where it ends, is no overlap
        SpecPlan z = kUntouched;
        CHECK(spec_plan(&s, B, kWindow, &c, reinterpret_cast<const float *>(reinterpret_cast<uintptr_t>(s.re) - out_bytes), want, &z).code == GAT_OK, "an adjacent output was refused");
        if (li != GAT_LAYOUT_PLANAR)
            CHECK(spec_plan(&s, B, kWindow, &c, reinterpret_cast<const float *>(reinterpret_cast<uintptr_t>(s.re) + in_bytes), want, &z).code == GAT_OK, "an output behind the input was refused");
    }
    CHECK(planned == 3000 && aligned > 1000 && aligned < 2200 && ran > 100 && looped > 20, "the sweep lost its balance: %d planned, %d aligned, %d run, %d looped", planned, aligned, ran, looped);
    std::printf("planned %d calls (%d with 16-byte loads, %d with more rounds than workgroups), ran the host loop on %d, %d failures\n", planned, aligned, looped, ran, failures);
    return failures ? 1 : 0;
}
