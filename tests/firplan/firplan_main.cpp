// Stand-alone check of the sample filter's pure plan (csrc/gat_fir_plan.h) and of the host loop of its rule (csrc/gat_fir.h), over
// a few thousand random calls.  Every planned call must cover each (block, antenna, output) exactly once through the units and
// tiles the kernels walk, dealt to the grid exactly once, with the tiled kernel chosen exactly under the fast-path rule and a tile
// that fits its LDS; every documented refusal must return its code with nothing planned.  The host loop then runs a sample of the
// planned calls on heap buffers sized to the descriptors' exact extents, so that AddressSanitizer sees any read before a block's
// first sample or past its last one and any write outside the described outputs.  Built with -fsanitize=address,undefined by
// tests/test_filter_plan_host.py.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "gat_fir.h"
#include "gat_fir_plan.h"

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

const FirPlan kUntouched = {true, -7, -7, -7, -7, -7, -7, -7};
bool untouched(const FirPlan &p) { return p.tiled && p.tile == -7 && p.row == -7 && p.Q == -7 && p.chunk == -7 && p.chunks == -7 && p.units == -7 && p.grid == -7; }

const float *const kTaps = reinterpret_cast<const float *>(uintptr_t(0x9000));

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

gat_fir_config config(int T, int D, double step = 0.0, double phase = 0.0)
{
    gat_fir_config c{};
    c.struct_size = sizeof(gat_fir_config);
    c.num_taps = T;
    c.decimation = D;
    c.nco_step = step;
    c.nco_phase = phase;
    return c;
}

void expect_refusal(const gat_signal_desc *s, int B, const float *g_re, const float *g_im, const gat_fir_config *c, const gat_signal_desc *o, int code,
                    const char *what)
{
    FirPlan p = kUntouched;
    const Refusal r = fir_plan(s, B, g_re, g_im, c, o, 2048, &p);
    CHECK(r.code == code, "%s: got %d, want %d", what, r.code, code);
    CHECK(r.code == GAT_OK || r.msg != nullptr, "%s: a refusal without a message", what);
    CHECK(untouched(p), "%s: a refused call planned something", what);
}

// walks the plan as the kernels do and counts every (block, antenna, output); the tiled kernel's tiles and their LDS indices too
void check_cover(const FirPlan &p, int B, int M, int T, int D, long long N)
{
    const long long Q = p.Q;
    std::vector<unsigned char> hits((size_t)B * (size_t)M * (size_t)Q, 0), dealt((size_t)p.units, 0);
    CHECK(p.grid >= 1 && p.grid <= p.units, "grid %lld of %lld units", p.grid, p.units);
    CHECK(p.units == (long long)B * M * p.chunks && p.units < (1ll << 31), "units");
    CHECK(p.chunk > 0 && p.chunk % p.tile == 0, "chunk %lld of tiles of %d", p.chunk, p.tile);
    CHECK(p.tile >= 1 && p.tile <= kFirThreads * kFirLaneOutputs, "tile %d", p.tile);
    if (p.tiled) {
        CHECK((long long)p.row * D <= kFirLdsSamples && p.row >= p.tile + fir_halo_cols(T, D), "row %d for tile %d, T %d, D %d", p.row, p.tile, T, D);
    }
    for (long long g = 0; g < p.grid; ++g)
        for (long long u = g; u < p.units; u += p.grid) {
            ++dealt[(size_t)u];
            long long b, q0, q1;
            int m;
            fir_unit(u, p.chunks, p.chunk, Q, M, &b, &m, &q0, &q1);
            CHECK(b >= 0 && b < B && m >= 0 && m < M && q0 >= 0 && q0 < q1 && q1 <= Q, "unit %lld: block %lld antenna %d outputs [%lld, %lld)", u, b, m, q0, q1);
            if (!(b >= 0 && b < B && m >= 0 && m < M && q0 >= 0 && q1 <= Q)) continue;
            for (long long qt = q0; qt < q1; qt += p.tile) {
                const long long nt = q1 - qt < p.tile ? q1 - qt : p.tile;
                const long long p0 = qt * D, p1 = p0 + (nt - 1) * D + T; // the tile's samples
                CHECK(p1 <= N, "a tile reads sample %lld of %lld", p1 - 1, N);
                if (p.tiled) { // the last staged sample and the farthest read stay inside the rows
                    const long long rel = p1 - 1 - p0, col = rel / D;
                    CHECK(col < p.row && (rel % D) * p.row + col < kFirLdsSamples, "LDS index of sample %lld", rel);
                    CHECK((T - 1) / D + nt - 1 < p.row, "a lane reads column %lld of %d", (T - 1) / D + nt - 1, p.row);
                }
                for (long long q = qt; q < qt + nt; ++q) ++hits[((size_t)b * M + m) * (size_t)Q + (size_t)q];
            }
        }
    for (size_t i = 0; i < dealt.size(); ++i) CHECK(dealt[i] == 1, "unit %zu dealt %d times", i, (int)dealt[i]);
    for (size_t i = 0; i < hits.size(); ++i)
        if (hits[i] != 1) {
            CHECK(false, "output %zu covered %d times", i, (int)hits[i]);
            break;
        }
}

// the host loop on buffers of the descriptors' exact extents; the result against a long double restatement
void run_host_loop(std::mt19937_64 &rng, int li, int lo, int B, int M, long long N, long long ias, long long ibs, int T, int D, double step, double phase)
{
    auto pick = [&](long long a, long long b) { return (long long)(rng() % (uint64_t)(b - a + 1)) + a; };
    const long long Q = (N - T) / D + 1, obs = Q + pick(0, 2), oas = obs * B + pick(0, 2);
    const size_t in_samples = (size_t)((B - 1) * ibs + (M - 1) * ias + N), out_samples = (size_t)((B - 1) * obs + (M - 1) * oas + Q);
    const size_t in_bytes = in_samples * layout_sample_bytes(li), out_floats = out_samples * (lo == GAT_LAYOUT_PLANAR ? 1 : 2);
    std::vector<unsigned char> in_re(in_bytes), in_im(li == GAT_LAYOUT_PLANAR ? in_bytes : 0);
    std::vector<float> out_re(out_floats, -3.25f), out_im(lo == GAT_LAYOUT_PLANAR ? out_floats : 0, -3.25f);
    if (li <= GAT_LAYOUT_INTERLEAVED) {
        for (size_t i = 0; i + 4 <= in_bytes; i += 4) {
            const float a = (float)pick(-1000, 1000) / 16.0f, b = (float)pick(-1000, 1000) / 16.0f;
            std::memcpy(&in_re[i], &a, 4);
            if (li == GAT_LAYOUT_PLANAR) std::memcpy(&in_im[i], &b, 4);
        }
    } else {
        for (auto &v : in_re) v = (unsigned char)pick(0, 255);
    }
    std::vector<float> g_re((size_t)T), g_im((size_t)T);
    for (int t = 0; t < T; ++t) g_re[(size_t)t] = (float)pick(-64, 64) / 64.0f, g_im[(size_t)t] = (float)pick(-64, 64) / 64.0f;
    gat_signal_desc s = desc(reinterpret_cast<uintptr_t>(in_re.data()), reinterpret_cast<uintptr_t>(in_im.data()), li, M, N, ias, ibs);
    gat_signal_desc o = desc(reinterpret_cast<uintptr_t>(out_re.data()), reinterpret_cast<uintptr_t>(out_im.data()), lo, M, Q, oas, obs);
    const gat_fir_config c = config(T, D, step, phase);
    FirPlan p = kUntouched;
    const Refusal r = fir_plan(&s, B, g_re.data(), g_im.data(), &c, &o, 64, &p);
    CHECK(r.code == GAT_OK, "host loop: a valid call was refused: %d %s", r.code, r.msg ? r.msg : "");
    if (r.code != GAT_OK) return;
    fir_host_run(&s, B, g_re.data(), g_im.data(), T, D, step, phase, &o);
    // every described output was written, nothing else; a few outputs against the sum in long double
    std::vector<unsigned char> described(out_samples, 0);
    for (int b = 0; b < B; ++b)
        for (int m = 0; m < M; ++m)
            for (long long q = 0; q < Q; ++q) described[(size_t)(b * obs + m * oas + q)] = 1;
    for (size_t e = 0; e < out_samples; ++e) {
        const float yr = lo == GAT_LAYOUT_PLANAR ? out_re[e] : out_re[2 * e], yi = lo == GAT_LAYOUT_PLANAR ? out_im[e] : out_re[2 * e + 1];
        if (!described[e]) CHECK(yr == -3.25f && yi == -3.25f, "host loop: element %zu outside the outputs was written", e);
    }
    const FirNco nco = fir_nco(step, phase);
    for (int k = 0; k < 8; ++k) {
        const int b = (int)pick(0, B - 1), m = (int)pick(0, M - 1);
        const long long q = pick(0, Q - 1), pn = q * D + T - 1;
        long double zr = 0, zi = 0, S = 0;
        for (int t = 0; t < T; ++t) {
            float xr, xi;
            host_load_sample(&s, (size_t)(b * ibs + m * ias + pn - t), &xr, &xi);
            zr += (long double)g_re[(size_t)t] * xr - (long double)g_im[(size_t)t] * xi;
            zi += (long double)g_re[(size_t)t] * xi + (long double)g_im[(size_t)t] * xr;
            S += (fabsl(g_re[(size_t)t]) + fabsl(g_im[(size_t)t])) * (fabsl(xr) + fabsl(xi));
        }
        long double yr = zr, yi = zi;
        const long double P = (long double)(b * ibs + pn);
        if (nco.rotate) {
            long double th = P * (long double)nco.step + (long double)nco.phase;
            th -= rintl(th);
            const long double cc = cosl(6.283185307179586476925286766559L * th), ss = sinl(6.283185307179586476925286766559L * th);
            yr = cc * zr + ss * zi, yi = cc * zi - ss * zr;
        }
        const size_t e = (size_t)(b * obs + m * oas + q);
        const float gr = lo == GAT_LAYOUT_PLANAR ? out_re[e] : out_re[2 * e], gi = lo == GAT_LAYOUT_PLANAR ? out_im[e] : out_re[2 * e + 1];
        const long double lim = ((2 * T + 8) * 0x1p-24L + 6.283185307179586L * 0x1p-53L * (P / 2 + 2)) * S;
        CHECK(fabsl(gr - yr) <= lim && fabsl(gi - yi) <= lim, "host loop: output (%d, %d, %lld) off by %Lg, %Lg of %Lg", b, m, q, fabsl(gr - yr), fabsl(gi - yi), lim);
    }
}

} // namespace

int main()
{
    std::mt19937_64 rng(20261018);
    auto pick = [&](long long lo, long long hi) { return (long long)(rng() % (uint64_t)(hi - lo + 1)) + lo; };
    int planned = 0, tiled = 0, ran = 0, split = 0;

    for (int it = 0; it < 4000; ++it) {
        const int li = (int)pick(0, 3), lo = (int)pick(0, 1);
        const int M = (int)(it % 5 == 0 ? pick(1, 64) : pick(1, 9)), B = (int)(it % 7 == 0 ? pick(1, 40) : pick(1, 4));
        const int T = (int)(it % 3 == 0 ? pick(1, 256) : pick(1, 40)), D = (int)(it % 4 == 0 ? pick(1, 64) : pick(1, 8));
        const long long N = T + (it % 11 == 0 ? pick(0, 200000) / (B * M) : pick(0, 3000));
        const long long Q = (N - T) / D + 1;
        const bool tidy = it % 2 == 0; // aligned bases and strides: the tiled kernel's candidates
        const bool overlap_save = it % 3 == 1 && Q * D >= 1; // blocks that continue each other
        const long long vi = layout_vec_samples(li), vo = layout_vec_samples(lo);
        long long ibs = overlap_save ? Q * D : N + pick(0, 9);
        if (tidy) ibs = (ibs + vi - 1) / vi * vi;
        const long long obs = tidy ? (Q + vo - 1) / vo * vo : Q + pick(0, 9);
        long long ias = (B - 1) * ibs + N + (tidy ? 0 : pick(0, 5));
        if (tidy) ias = (ias + vi - 1) / vi * vi;
        const long long oas = obs * B + (tidy ? vo * pick(0, 3) : pick(0, 5));
        const uintptr_t ioff = tidy ? 0 : (uintptr_t)pick(0, 3) * layout_sample_bytes(li), ooff = tidy ? 0 : (uintptr_t)pick(0, 3) * layout_sample_bytes(lo);
        const gat_signal_desc s = desc(0x100000000ull + ioff, 0x200000000ull + ioff, li, M, N, ias, ibs);
        const gat_signal_desc o = desc(0x300000000ull + ooff, 0x400000000ull + ooff, lo, M, Q, oas, obs);
        const double step = it % 2 ? (double)pick(-1000, 1000) / 997.0 : 0.0, phase = it % 2 ? (double)pick(-5000, 5000) / 991.0 : 0.0;
        const gat_fir_config c = config(T, D, step, phase);
        const long long want = pick(1, 3) == 1 ? pick(1, 64) : 2048;
        FirPlan p = kUntouched;
        const Refusal r = fir_plan(&s, B, kTaps, kTaps, &c, &o, want, &p);
        CHECK(r.code == GAT_OK, "a valid call was refused: %d %s", r.code, r.msg ? r.msg : "");
        if (r.code != GAT_OK) continue;
        ++planned;
        const bool rule = blocks_aligned(&s, B) && blocks_aligned(&o, B);
        CHECK(p.tiled == rule, "tiled %d, the rule says %d", (int)p.tiled, (int)rule);
        CHECK(!tidy || p.tiled, "an aligned call did not run the tiled kernel");
        CHECK(p.Q == Q, "Q %lld, want %lld", p.Q, Q);
        tiled += p.tiled, split += p.chunks > 1;
        if ((long long)B * M * Q <= 400000) check_cover(p, B, M, T, D, N);
        if (it % 8 == 3 && (long long)B * M * Q * T <= 2000000) run_host_loop(rng, li, lo, B, M, N, ias, ibs, T, D, step, phase), ++ran;

        // the refusals, each from this valid pair
        gat_signal_desc t = s, v = o;
        gat_fir_config k = c;
        expect_refusal(nullptr, B, kTaps, kTaps, &c, &o, GAT_ERR_ARG, "null signal");
        expect_refusal(&s, B, kTaps, kTaps, &c, nullptr, GAT_ERR_ARG, "null output");
        expect_refusal(&s, B, nullptr, kTaps, &c, &o, GAT_ERR_ARG, "null taps_re");
        expect_refusal(&s, B, kTaps, nullptr, &c, &o, GAT_ERR_ARG, "null taps_im");
        expect_refusal(&s, B, kTaps, kTaps, nullptr, &o, GAT_ERR_ARG, "null config");
        k = c, k.struct_size = sizeof(gat_fir_config) + 8;
        expect_refusal(&s, B, kTaps, kTaps, &k, &o, GAT_ERR_ARG, "struct_size");
        expect_refusal(&s, 0, kTaps, kTaps, &c, &o, GAT_ERR_ARG, "no blocks");
        k = c, k.num_taps = 0;
        expect_refusal(&s, B, kTaps, kTaps, &k, &o, GAT_ERR_RANGE, "no taps");
        k = c, k.num_taps = GAT_MAX_FIR_TAPS + 1;
        expect_refusal(&s, B, kTaps, kTaps, &k, &o, GAT_ERR_RANGE, "too many taps");
        k = c, k.decimation = 0;
        expect_refusal(&s, B, kTaps, kTaps, &k, &o, GAT_ERR_RANGE, "no decimation");
        k = c, k.decimation = GAT_MAX_FIR_DECIMATION + 1;
        expect_refusal(&s, B, kTaps, kTaps, &k, &o, GAT_ERR_RANGE, "decimation too large");
        k = c, k.nco_step = NAN;
        expect_refusal(&s, B, kTaps, kTaps, &k, &o, GAT_ERR_ARG, "NaN step");
        k = c, k.nco_phase = -INFINITY;
        expect_refusal(&s, B, kTaps, kTaps, &k, &o, GAT_ERR_ARG, "infinite phase");
        t = s, t.num_samples = 0;
        expect_refusal(&t, B, kTaps, kTaps, &c, &o, GAT_ERR_ARG, "no samples");
        t = s, t.num_samples = T - 1;
        expect_refusal(&t, B, kTaps, kTaps, &c, &o, GAT_ERR_ARG, "a block shorter than the filter");
        t = s, t.num_ants = 0;
        expect_refusal(&t, B, kTaps, kTaps, &c, &o, GAT_ERR_ARG, "no antennas");
        t = s, t.ant_stride = -1;
        expect_refusal(&t, B, kTaps, kTaps, &c, &o, GAT_ERR_ARG, "negative ant_stride");
        v = o, v.block_stride = -1;
        expect_refusal(&s, B, kTaps, kTaps, &c, &v, GAT_ERR_ARG, "negative output block_stride");
        t = s, t.layout = 4;
        expect_refusal(&t, B, kTaps, kTaps, &c, &o, GAT_ERR_ARG, "bad layout");
        v = o, v.layout = -1;
        expect_refusal(&s, B, kTaps, kTaps, &c, &v, GAT_ERR_ARG, "bad output layout");
        t = s;
        t.im = li == GAT_LAYOUT_PLANAR ? nullptr : t.re;
        expect_refusal(&t, B, kTaps, kTaps, &c, &o, GAT_ERR_ARG, "signal planes");
        v = o;
        v.im = lo == GAT_LAYOUT_PLANAR ? nullptr : v.re;
        expect_refusal(&s, B, kTaps, kTaps, &c, &v, GAT_ERR_ARG, "output planes");
        v = o, v.num_ants = M + 1;
        expect_refusal(&s, B, kTaps, kTaps, &c, &v, GAT_ERR_ARG, "num_ants mismatch");
        v = o, v.num_samples = Q + 1;
        expect_refusal(&s, B, kTaps, kTaps, &c, &v, GAT_ERR_ARG, "num_samples is not Q");
        for (int l : {GAT_LAYOUT_INTERLEAVED_I16, GAT_LAYOUT_INTERLEAVED_I8}) {
            v = o, v.layout = l, v.im = nullptr;
            expect_refusal(&s, B, kTaps, kTaps, &c, &v, GAT_ERR_UNSUPPORTED, "an integer output");
        }
        t = s, t.chan_stride = 8;
        expect_refusal(&t, B, kTaps, kTaps, &c, &o, GAT_ERR_UNSUPPORTED, "signal chan_stride");
        v = o, v.chan_stride = 8;
        expect_refusal(&s, B, kTaps, kTaps, &c, &v, GAT_ERR_UNSUPPORTED, "output chan_stride");
        t = s, v = o, t.num_ants = v.num_ants = GAT_MAX_ARRAY_ANTS + 1;
        expect_refusal(&t, B, kTaps, kTaps, &c, &v, GAT_ERR_RANGE, "too many antennas");
        if (M > 1) {
            t = s, t.ant_stride = 0;
            expect_refusal(&t, B, kTaps, kTaps, &c, &o, GAT_ERR_ARG, "zero ant_stride");
            v = o, v.ant_stride = 0;
            expect_refusal(&s, B, kTaps, kTaps, &c, &v, GAT_ERR_ARG, "zero output ant_stride");
        }
        if (B > 1) {
            t = s, t.block_stride = 0;
            expect_refusal(&t, B, kTaps, kTaps, &c, &o, GAT_ERR_ARG, "zero block_stride");
            // the stream's span: (B - 1) * block_stride + N above 2^31
            t = s, t.block_stride = ((1ll << 31) - N) / (B - 1) + 1;
            expect_refusal(&t, B, kTaps, kTaps, &c, &o, GAT_ERR_RANGE, "a span above 2^31 samples");
        }
        // overlap: the output starts on the last byte of either input plane, or either output plane is an input plane
        const uintptr_t in_bytes = (uintptr_t)((B - 1) * ibs + (M - 1) * ias + N) * layout_sample_bytes(li);
        v = o, v.re = reinterpret_cast<const void *>(reinterpret_cast<uintptr_t>(s.re) + in_bytes - 1);
        expect_refusal(&s, B, kTaps, kTaps, &c, &v, GAT_ERR_ARG, "the output starts on the input's last byte");
        if (li == GAT_LAYOUT_PLANAR) {
            v = o, v.re = reinterpret_cast<const void *>(reinterpret_cast<uintptr_t>(s.im) + in_bytes - 1);
            expect_refusal(&s, B, kTaps, kTaps, &c, &v, GAT_ERR_ARG, "the output starts on the last byte of the input's im plane");
        }
        if (lo == GAT_LAYOUT_PLANAR) {
            v = o, v.im = s.re;
            expect_refusal(&s, B, kTaps, kTaps, &c, &v, GAT_ERR_ARG, "the output's im plane is the input's re plane");
        }
        expect_refusal(&s, B, kTaps, kTaps, &c, &s, li <= GAT_LAYOUT_INTERLEAVED ? GAT_ERR_ARG : GAT_ERR_UNSUPPORTED, "in place");
        // an output that ends where the input begins is no overlap
        const uintptr_t out_bytes = (uintptr_t)((B - 1) * obs + (M - 1) * oas + Q) * layout_sample_bytes(lo);
        if (lo != GAT_LAYOUT_PLANAR) {
            v = o, v.re = reinterpret_cast<const void *>(reinterpret_cast<uintptr_t>(s.re) - out_bytes);
            FirPlan z = kUntouched;
            CHECK(fir_plan(&s, B, kTaps, kTaps, &c, &v, want, &z).code == GAT_OK, "an adjacent output was refused");
        }
    }
    CHECK(planned == 4000 && tiled > 1000 && tiled < 3000 && ran > 200 && split > 100, "the sweep lost its balance: %d planned, %d tiled, %d run, %d split", planned, tiled, ran, split);
    std::printf("planned %d calls (%d tiled, %d with split blocks), ran the host loop on %d, %d failures\n", planned, tiled, split, ran, failures);
    return failures ? 1 : 0;
}
