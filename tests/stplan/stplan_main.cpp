// Stand-alone check of the pure plans of space-time adaptive processing (csrc/gat_st_plan.h) and of the host loop of the filter's
// rule (csrc/gat_st.h), over a few thousand random calls.  Every planned filter call must cover each (block, output) exactly once
// through the units and tiles the kernels walk, dealt to the grid exactly once, with the tiled kernel chosen exactly under its rule
// and a tile whose samples and halo fit its LDS and stay inside the block; the covariance's geometry must keep every staged
// column and every element a thread reads inside its LDS; every documented refusal must return its code with nothing planned.
// The host loop then runs on heap buffers sized to the descriptors' exact extents -- small shapes at the edges of every chunk,
// tile and halo among them --, so that AddressSanitizer sees any read before a block's first sample or past its last one and any
// write outside the described outputs.  Built with -fsanitize=address,undefined by tests/test_spacetime_plan_host.py.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "gat_st.h"
#include "gat_st_plan.h"

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

const StPlan kUntouched = {true, -7, -7, -7, -7, -7, -7, -7, -7};
bool untouched(const StPlan &p) { return p.tiled && p.tile == -7 && p.row == -7 && p.beams == -7 && p.outputs == -7 && p.chunk == -7 && p.chunks == -7 && p.units == -7 && p.grid == -7; }

const double *const kW = reinterpret_cast<const double *>(uintptr_t(0x9000));
float *const kCov = reinterpret_cast<float *>(uintptr_t(0xA000));

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

void expect_refusal(const gat_signal_desc *s, int B, const double *w_re, const double *w_im, int T, int J, const gat_signal_desc *o, int code, const char *what)
{
    StPlan p = kUntouched;
    const Refusal r = st_filter_plan(s, B, w_re, w_im, T, J, o, 2048, &p);
    CHECK(r.code == code, "%s: got %d, want %d", what, r.code, code);
    CHECK(r.code == GAT_OK || r.msg != nullptr, "%s: a refusal without a message", what);
    CHECK(untouched(p), "%s: a refused call planned something", what);
}

// walks the plan as the kernels do and counts every (block, output); the tiled kernel's tiles and their LDS indices too
void check_cover(const StPlan &p, int B, int M, int T, long long N)
{
    const long long No = p.outputs;
    std::vector<unsigned char> hits((size_t)B * (size_t)No, 0), dealt((size_t)p.units, 0);
    CHECK(No == N - T + 1, "outputs %lld", No);
    CHECK(p.grid >= 1 && p.grid <= p.units, "grid %lld of %lld units", p.grid, p.units);
    CHECK(p.units == (long long)B * p.chunks && p.units < (1ll << 31), "units");
    CHECK(p.tile >= 1 && p.tile <= kStThreads * kStLaneOutputs, "tile %d", p.tile);
    CHECK(p.chunk > 0 && p.chunk % p.tile == 0, "chunk %lld of tiles of %d", p.chunk, p.tile);
    if (p.tiled) CHECK(M <= kStTiledMaxAnts && p.row == p.tile + T - 1 && (long long)p.row * M <= kStLdsSamples, "row %d for tile %d, T %d, M %d", p.row, p.tile, T, M);
    for (long long g = 0; g < p.grid; ++g)
        for (long long u = g; u < p.units; u += p.grid) {
            ++dealt[(size_t)u];
            long long b, n0, n1;
            st_unit(u, p.chunks, p.chunk, No, &b, &n0, &n1);
            CHECK(b >= 0 && b < B && n0 >= 0 && n0 < n1 && n1 <= No, "unit %lld: block %lld outputs [%lld, %lld)", u, b, n0, n1);
            if (!(b >= 0 && b < B && n0 >= 0 && n1 <= No)) continue;
            for (long long nt0 = n0; nt0 < n1; nt0 += p.tile) {
                const long long nt = n1 - nt0 < p.tile ? n1 - nt0 : p.tile;
                const long long p1 = nt0 + nt + T - 1; // one past the tile's last sample
                CHECK(p1 <= N, "a tile reads sample %lld of %lld", p1 - 1, N);
                if (p.tiled) CHECK((long long)(M - 1) * p.row + (p1 - 1 - nt0) < kStLdsSamples, "LDS index of a tile's last sample");
                for (long long n = nt0; n < nt0 + nt; ++n) ++hits[(size_t)b * (size_t)No + (size_t)n];
            }
        }
    for (size_t i = 0; i < dealt.size(); ++i) CHECK(dealt[i] == 1, "unit %zu dealt %d times", i, (int)dealt[i]);
    for (size_t i = 0; i < hits.size(); ++i)
        if (hits[i] != 1) {
            CHECK(false, "output %zu covered %d times", i, (int)hits[i]);
            break;
        }
}

// the covariance kernel's LDS: every staged column and every element any thread reads of any snapshot of a chunk
void check_cov_geom(int M, int T)
{
    const StCovGeom g = st_cov_geom(M, T);
    const long long slots = (long long)g.cols * M + kStCovPad;
    CHECK(g.Q == M * T && g.nt * kStCovTile >= g.Q && (g.nt - 1) * kStCovTile < g.Q, "M %d T %d: nt %d", M, T, g.nt);
    CHECK(g.tiles == g.nt * (g.nt + 1) / 2 && g.phases >= 1 && g.phases * g.tiles <= kStCovThreads, "M %d T %d: tiles %d phases %d", M, T, g.tiles, g.phases);
    CHECK(g.per_phase >= 1 && g.chunk == g.phases * g.per_phase && g.cols == g.chunk + T - 1, "M %d T %d: chunk %d cols %d", M, T, g.chunk, g.cols);
    CHECK(g.lds_bytes >= (size_t)slots * 8 && g.lds_bytes >= (size_t)kStCovThreads * 64 && g.lds_bytes <= 65536, "M %d T %d: %zu bytes of LDS", M, T, g.lds_bytes);
    // the staging store of (column c, antenna m) and the reads z[-q], q < 4 nt, of snapshot n < chunk
    const long long lo_store = kStCovPad, hi_store = kStCovPad + (long long)(g.cols - 1) * M + (M - 1);
    CHECK(lo_store >= 0 && hi_store < slots, "M %d T %d: staging stores", M, T);
    const long long lo_read = kStCovPad + (long long)(0 + T) * M - 1 - (g.nt * kStCovTile - 1), hi_read = kStCovPad + (long long)(g.chunk - 1 + T) * M - 1;
    CHECK(lo_read >= 0 && hi_read < slots, "M %d T %d: reads [%lld, %lld] of %lld", M, T, lo_read, hi_read, slots);
    // element q < Q of snapshot n is sample (n + T - 1 - t) of antenna m: column n + T - 1 - t >= 0, stored at kStCovPad + c M + (M - 1 - m)
    for (int n : {0, g.chunk - 1})
        for (int q : {0, g.Q - 1}) {
            const int t = q / M, m = q % M, c = n + T - 1 - t;
            CHECK(c >= 0 && c < g.cols && kStCovPad + (long long)(n + T) * M - 1 - q == kStCovPad + (long long)c * M + (M - 1 - m), "M %d T %d: element %d of snapshot %d", M, T, q, n);
        }
}

// the host loop on buffers of the descriptors' exact extents; the result against a long double restatement
void run_host_loop(std::mt19937_64 &rng, int li, int lo, int B, int M, long long N, long long ias, long long ibs, int T, int J)
{
    auto pick = [&](long long a, long long b) { return (long long)(rng() % (uint64_t)(b - a + 1)) + a; };
    const int Q = M * T;
    const long long No = N - T + 1, obs = No + pick(0, 2), oas = obs * B + pick(0, 2);
    const size_t in_samples = (size_t)((B - 1) * ibs + (M - 1) * ias + N), out_samples = (size_t)((B - 1) * obs + (J - 1) * oas + No);
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
    std::vector<double> w_re((size_t)J * Q), w_im((size_t)J * Q);
    for (size_t i = 0; i < w_re.size(); ++i) w_re[i] = (double)pick(-4096, 4096) / 4099.0, w_im[i] = (double)pick(-4096, 4096) / 4093.0;
    gat_signal_desc s = desc(reinterpret_cast<uintptr_t>(in_re.data()), reinterpret_cast<uintptr_t>(in_im.data()), li, M, N, ias, ibs);
    gat_signal_desc o = desc(reinterpret_cast<uintptr_t>(out_re.data()), reinterpret_cast<uintptr_t>(out_im.data()), lo, J, No, oas, obs);
    StPlan p = kUntouched;
    const Refusal r = st_filter_plan(&s, B, w_re.data(), w_im.data(), T, J, &o, 64, &p);
    CHECK(r.code == GAT_OK, "host loop: a valid call was refused: %d %s", r.code, r.msg ? r.msg : "");
    if (r.code != GAT_OK) return;
    st_host_run(&s, B, w_re.data(), w_im.data(), T, J, &o);
    std::vector<unsigned char> described(out_samples, 0);
    for (int b = 0; b < B; ++b)
        for (int j = 0; j < J; ++j)
            for (long long n = 0; n < No; ++n) described[(size_t)(b * obs + j * oas + n)] = 1;
    for (size_t e = 0; e < out_samples; ++e) {
        const float yr = lo == GAT_LAYOUT_PLANAR ? out_re[e] : out_re[2 * e], yi = lo == GAT_LAYOUT_PLANAR ? out_im[e] : out_re[2 * e + 1];
        if (!described[e]) CHECK(yr == -3.25f && yi == -3.25f, "host loop: element %zu outside the outputs was written", e);
        else CHECK(!(yr == -3.25f && yi == -3.25f), "host loop: output %zu was not written", e);
    }
    for (int k = 0; k < 8; ++k) {
        const int b = (int)pick(0, B - 1), j = (int)pick(0, J - 1);
        const long long n = k == 0 ? 0 : k == 1 ? No - 1 : pick(0, No - 1);
        long double yr = 0, yi = 0, S = 0;
        for (int t = 0; t < T; ++t)
            for (int m = 0; m < M; ++m) {
                float xr, xi;
                host_load_sample(&s, (size_t)(b * ibs + m * ias + n + T - 1 - t), &xr, &xi);
                const long double wr = w_re[(size_t)j * Q + t * M + m], wi = w_im[(size_t)j * Q + t * M + m];
                yr += wr * xr + wi * xi;
                yi += wr * xi - wi * xr;
                S += hypotl(wr, wi) * hypotl(xr, xi);
            }
        const size_t e = (size_t)(b * obs + j * oas + n);
        const float gr = lo == GAT_LAYOUT_PLANAR ? out_re[e] : out_re[2 * e], gi = lo == GAT_LAYOUT_PLANAR ? out_im[e] : out_re[2 * e + 1];
        const long double lim = (4 * Q + 4) * 0x1p-24L * S;
        CHECK(hypotl(gr - yr, gi - yi) <= lim, "host loop: output (%d, %d, %lld) off by %Lg of %Lg", b, j, n, hypotl(gr - yr, gi - yi), lim);
    }
}

} // namespace

int main()
{
    std::mt19937_64 rng(20261019);
    auto pick = [&](long long lo, long long hi) { return (long long)(rng() % (uint64_t)(hi - lo + 1)) + lo; };
    int planned = 0, tiled = 0, ran = 0, split = 0;

    for (int M = 1; M <= GAT_MAX_ARRAY_ANTS; ++M)
        for (int T = 1; T <= GAT_MAX_ST_TAPS && M * T <= GAT_MAX_ARRAY_ANTS; ++T) check_cov_geom(M, T);

    for (int it = 0; it < 3000; ++it) {
        const int li = (int)pick(0, 3), lo = (int)pick(0, 1);
        const int T = (int)pick(1, GAT_MAX_ST_TAPS);
        const int M = (int)(it % 5 == 0 ? pick(1, GAT_MAX_ARRAY_ANTS / T) : pick(1, std::min<long long>(9, GAT_MAX_ARRAY_ANTS / T)));
        const int B = (int)(it % 7 == 0 ? pick(1, 40) : pick(1, 4)), J = (int)(it % 6 == 0 ? pick(1, 64) : pick(1, 9));
        const int tile = M <= kStTiledMaxAnts ? st_tile_outputs(M, T) : kStThreads;
        // lengths: anything; the edges of a tile and of the halo; long blocks that split
        long long N;
        switch (it % 6) {
        case 0: N = T + pick(0, 3000); break;
        case 1: N = T - 1 + tile * pick(1, 3) + pick(-1, 1); break;
        case 2: N = T + pick(0, 2); break;
        case 3: N = 2 * T - 1 + pick(0, 1); break;
        case 4: N = T + pick(0, 200000) / B; break;
        default: N = T - 1 + kStThreads * pick(1, 4) + pick(-1, 1); break;
        }
        const long long No = N - T + 1;
        const bool tidy = it % 2 == 0; // aligned bases and strides: the tiled kernel's candidates
        const bool overlap_save = it % 3 == 1; // blocks that continue each other
        const long long vi = layout_vec_samples(li), vo = layout_vec_samples(lo);
        long long ibs = overlap_save ? No : N + pick(0, 9);
        if (tidy) ibs = (ibs + vi - 1) / vi * vi;
        const long long obs = tidy ? (No + vo - 1) / vo * vo : No + pick(0, 9);
        long long ias = (B - 1) * ibs + N + (tidy ? 0 : pick(0, 5));
        if (tidy) ias = (ias + vi - 1) / vi * vi;
        const long long oas = obs * B + (tidy ? vo * pick(0, 3) : pick(0, 5));
        const uintptr_t ioff = tidy ? 0 : (uintptr_t)pick(0, 3) * layout_sample_bytes(li), ooff = tidy ? 0 : (uintptr_t)pick(0, 3) * layout_sample_bytes(lo);
        const gat_signal_desc s = desc(0x100000000ull + ioff, 0x200000000ull + ioff, li, M, N, ias, ibs);
        const gat_signal_desc o = desc(0x300000000ull + ooff, 0x400000000ull + ooff, lo, J, No, oas, obs);
        const long long want = pick(1, 3) == 1 ? pick(1, 64) : 2048;
        StPlan p = kUntouched;
        const Refusal r = st_filter_plan(&s, B, kW, kW, T, J, &o, want, &p);
        CHECK(r.code == GAT_OK, "a valid call was refused: %d %s", r.code, r.msg ? r.msg : "");
        if (r.code != GAT_OK) continue;
        ++planned;
        const bool rule = M <= kStTiledMaxAnts && blocks_aligned(&s, B) && blocks_aligned(&o, B);
        CHECK(p.tiled == rule, "tiled %d, the rule says %d", (int)p.tiled, (int)rule);
        CHECK(!tidy || M > kStTiledMaxAnts || p.tiled, "an aligned call did not run the tiled kernel");
        CHECK(p.beams == st_beam_tile(p.tiled, J) && p.beams >= 1 && (p.tiled ? p.beams <= kStTiledBeams : p.beams <= kStGeneralBeams), "beam tile %d", p.beams);
        tiled += p.tiled, split += p.chunks > 1;
        if ((long long)B * No <= 400000) check_cover(p, B, M, T, N);
        if (it % 4 != 0 && (long long)B * J * No * M * T <= 1500000) run_host_loop(rng, li, lo, B, M, N, ias, ibs, T, J), ++ran;
        CHECK(st_cov_plan(&s, B, 1, T, kCov, kCov).code == GAT_OK, "the covariance refused a valid signal");

        // the refusals, each from this valid pair
        gat_signal_desc t = s, v = o;
        expect_refusal(nullptr, B, kW, kW, T, J, &o, GAT_ERR_ARG, "null signal");
        expect_refusal(&s, B, kW, kW, T, J, nullptr, GAT_ERR_ARG, "null output");
        expect_refusal(&s, B, nullptr, kW, T, J, &o, GAT_ERR_ARG, "null w_re");
        expect_refusal(&s, B, kW, nullptr, T, J, &o, GAT_ERR_ARG, "null w_im");
        expect_refusal(&s, 0, kW, kW, T, J, &o, GAT_ERR_ARG, "no blocks");
        expect_refusal(&s, B, kW, kW, T, 0, &o, GAT_ERR_ARG, "no beams");
        expect_refusal(&s, B, kW, kW, 0, J, &o, GAT_ERR_RANGE, "no taps");
        expect_refusal(&s, B, kW, kW, GAT_MAX_ST_TAPS + 1, J, &o, GAT_ERR_RANGE, "too many taps");
        t = s, t.num_ants = GAT_MAX_ARRAY_ANTS / T + 1;
        expect_refusal(&t, B, kW, kW, T, J, &o, GAT_ERR_RANGE, "num_ants * num_taps above 64");
        CHECK(st_cov_plan(&t, B, 1, T, kCov, kCov).code == GAT_ERR_RANGE, "the covariance took num_ants * num_taps above 64");
        v = o, v.num_ants = GAT_MAX_ARRAY_ANTS + 1;
        expect_refusal(&s, B, kW, kW, T, GAT_MAX_ARRAY_ANTS + 1, &v, GAT_ERR_RANGE, "too many beams");
        t = s, t.num_samples = 0;
        expect_refusal(&t, B, kW, kW, T, J, &o, GAT_ERR_ARG, "no samples");
        if (T > 1) {
            t = s, t.num_samples = T - 1, v = o, v.num_samples = 1;
            expect_refusal(&t, B, kW, kW, T, J, &v, GAT_ERR_ARG, "a block shorter than the delay line");
            CHECK(st_cov_plan(&t, B, 1, T, kCov, kCov).code == GAT_ERR_ARG, "the covariance took a block shorter than the delay line");
        }
        t = s, t.num_ants = 0;
        expect_refusal(&t, B, kW, kW, T, J, &o, GAT_ERR_ARG, "no antennas");
        t = s, t.ant_stride = -1;
        expect_refusal(&t, B, kW, kW, T, J, &o, GAT_ERR_ARG, "negative ant_stride");
        v = o, v.block_stride = -1;
        expect_refusal(&s, B, kW, kW, T, J, &v, GAT_ERR_ARG, "negative output block_stride");
        t = s, t.layout = 4;
        expect_refusal(&t, B, kW, kW, T, J, &o, GAT_ERR_ARG, "bad layout");
        v = o, v.layout = -1;
        expect_refusal(&s, B, kW, kW, T, J, &v, GAT_ERR_ARG, "bad output layout");
        t = s;
        t.im = li == GAT_LAYOUT_PLANAR ? nullptr : t.re;
        expect_refusal(&t, B, kW, kW, T, J, &o, GAT_ERR_ARG, "signal planes");
        v = o;
        v.im = lo == GAT_LAYOUT_PLANAR ? nullptr : v.re;
        expect_refusal(&s, B, kW, kW, T, J, &v, GAT_ERR_ARG, "output planes");
        v = o, v.num_ants = J + 1;
        expect_refusal(&s, B, kW, kW, T, J, &v, GAT_ERR_ARG, "num_ants is not num_beams");
        v = o, v.num_samples = No + 1;
        expect_refusal(&s, B, kW, kW, T, J, &v, GAT_ERR_ARG, "num_samples is not N - T + 1");
        for (int l : {GAT_LAYOUT_INTERLEAVED_I16, GAT_LAYOUT_INTERLEAVED_I8}) {
            v = o, v.layout = l, v.im = nullptr;
            expect_refusal(&s, B, kW, kW, T, J, &v, GAT_ERR_UNSUPPORTED, "an integer output");
        }
        t = s, t.chan_stride = 8;
        expect_refusal(&t, B, kW, kW, T, J, &o, GAT_ERR_UNSUPPORTED, "signal chan_stride");
        CHECK(st_cov_plan(&t, B, 1, T, kCov, kCov).code == GAT_ERR_UNSUPPORTED, "the covariance took a chan_stride");
        v = o, v.chan_stride = 8;
        expect_refusal(&s, B, kW, kW, T, J, &v, GAT_ERR_UNSUPPORTED, "output chan_stride");
        if (M > 1) {
            t = s, t.ant_stride = 0;
            expect_refusal(&t, B, kW, kW, T, J, &o, GAT_ERR_ARG, "zero ant_stride");
        }
        if (J > 1) {
            v = o, v.ant_stride = 0;
            expect_refusal(&s, B, kW, kW, T, J, &v, GAT_ERR_ARG, "zero output ant_stride");
        }
        if (B > 1) {
            t = s, t.block_stride = 0;
            expect_refusal(&t, B, kW, kW, T, J, &o, GAT_ERR_ARG, "zero block_stride");
        }
        CHECK(st_cov_plan(&s, 0, 1, T, kCov, kCov).code == GAT_ERR_ARG && st_cov_plan(&s, B, 0, T, kCov, kCov).code == GAT_ERR_ARG &&
                  st_cov_plan(&s, B, 1, T, nullptr, kCov).code == GAT_ERR_ARG && st_cov_plan(nullptr, B, 1, T, kCov, kCov).code == GAT_ERR_ARG &&
                  st_cov_plan(&s, B, 1, GAT_MAX_ST_TAPS + 1, kCov, kCov).code == GAT_ERR_RANGE && st_cov_plan(&s, B, 1, 0, kCov, kCov).code == GAT_ERR_RANGE,
              "the covariance's refusals");
        // overlap: the output starts on the last byte of either input plane, or either output plane is an input plane
        const uintptr_t in_bytes = (uintptr_t)((B - 1) * ibs + (M - 1) * ias + N) * layout_sample_bytes(li);
        v = o, v.re = reinterpret_cast<const void *>(reinterpret_cast<uintptr_t>(s.re) + in_bytes - 1);
        expect_refusal(&s, B, kW, kW, T, J, &v, GAT_ERR_ARG, "the output starts on the input's last byte");
        if (lo == GAT_LAYOUT_PLANAR) {
            v = o, v.im = s.re;
            expect_refusal(&s, B, kW, kW, T, J, &v, GAT_ERR_ARG, "the output's im plane is the input's re plane");
        }
        // an output that ends where the input begins is no overlap
        const uintptr_t out_bytes = (uintptr_t)((B - 1) * obs + (J - 1) * oas + No) * layout_sample_bytes(lo);
        if (lo != GAT_LAYOUT_PLANAR) {
            v = o, v.re = reinterpret_cast<const void *>(reinterpret_cast<uintptr_t>(s.re) - out_bytes);
            StPlan z = kUntouched;
            CHECK(st_filter_plan(&s, B, kW, kW, T, J, &v, want, &z).code == GAT_OK, "an adjacent output was refused");
        }
    }
    CHECK(planned == 3000 && tiled > 700 && tiled < 2300 && ran > 500 && split > 100, "the sweep lost its balance: %d planned, %d tiled, %d run, %d split", planned, tiled, ran, split);
    std::printf("planned %d calls (%d tiled, %d with split blocks), ran the host loop on %d, %d failures\n", planned, tiled, split, ran, failures);
    return failures ? 1 : 0;
}
