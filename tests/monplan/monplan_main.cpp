// Stand-alone check of the tracking monitor's pure plan (csrc/gat_mon_plan.h) and of the host twin's loops over it (mon_host_run,
// the rule of csrc/gat_mon.h), over a few thousand random calls.  Every planned call must cover each (k, block), (k, window),
// (k, c, j), (k, c), k and (k, symbol) exactly once through the workgroups and threads the kernels are launched with, carve its
// scratch in disjoint, aligned parts within the planned bytes, and report the counts of the rule; every documented refusal must
// return its code with nothing planned.  The twin then runs on heap buffers of exactly the extents the call describes -- padded
// block strides, the last partial window, one block, every subset of the outputs --, so that AddressSanitizer sees any read
// outside the accumulators and any write outside an output.  Built with -fsanitize=address,undefined by
// tests/test_monitor_plan_host.py.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "gat_mon.h"
#include "gat_mon_plan.h"

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

gat_monitor_config config(int L, int l, int W, int Pd, int forced, long long fb, std::mt19937_64 &rng)
{
    gat_monitor_config c{};
    c.struct_size = sizeof(gat_monitor_config);
    c.num_taps = L, c.prompt_index = l, c.window_blocks = W, c.symbol_blocks = Pd, c.symbol_offset = forced, c.first_block = fb;
    for (int i = 0; i < 128; ++i) c.overlay[i] = i < Pd ? ((rng() & 1) ? 1 : -1) : 0; // beyond Pd: ignored, any value
    return c;
}

MonCall call(long long stride, int B, int K, int M, const gat_monitor_config *cfg, unsigned outs = 0xff, bool w = false)
{
    MonCall a{};
    a.acc_re = a.acc_im = kGiven;
    a.acc_block_stride = stride, a.B = B, a.K = K, a.M = M, a.cfg = cfg;
    a.w_re = a.w_im = w ? kGiven : nullptr;
    a.prompt_re = outs & 1 ? kGiven : nullptr, a.prompt_im = outs & 2 ? kGiven : nullptr, a.windows = outs & 4 ? kGiven : nullptr;
    a.energy = outs & 8 ? kGiven : nullptr, a.channels = outs & 16 ? kGiven : nullptr, a.sym_re = outs & 32 ? kGiven : nullptr;
    a.sym_im = outs & 64 ? kGiven : nullptr, a.sym_wbp = outs & 128 ? kGiven : nullptr;
    return a;
}

MonPlan untouched_plan()
{
    MonPlan p;
    std::memset(&p, 0x5a, sizeof p);
    return p;
}
bool untouched(const MonPlan &p)
{
    const MonPlan q = untouched_plan();
    return std::memcmp(&p, &q, sizeof p) == 0;
}

void expect_refusal(const MonCall &a, int code, const char *what)
{
    MonPlan p = untouched_plan();
    const Refusal r = mon_plan(a, &p);
    CHECK(r.code == code, "%s: got %d, want %d", what, r.code, code);
    CHECK(r.code == GAT_OK || r.msg != nullptr, "%s: a refusal without a message", what);
    CHECK(untouched(p), "%s: a refused call planned something", what);
}

// walks every launch as the kernels do and counts each unit
void check_cover(const MonPlan &p, unsigned outs)
{
    const long long B = p.B, K = p.K, Pd = p.Pd;
    CHECK(p.NW == (B + p.W - 1) / p.W && p.cap == B / Pd, "counts NW %lld cap %lld", p.NW, p.cap);
    CHECK(p.J == (B - Pd + 1 > 0 ? (B - Pd + 1) / Pd : 0), "J %lld", p.J);
    CHECK((p.J + 1) * Pd - 2 < B || p.J == 0, "the search's last symbol ends beyond the series");
    {
        std::vector<unsigned char> hit((size_t)(K * B), 0);
        CHECK(p.g_prompt >= 1, "no prompt launch");
        for (long long t = 0; t < p.g_prompt * kMonThreads; ++t) {
            int k, b;
            if (!mon_prompt_unit(t, p.B, p.K, &k, &b)) continue;
            CHECK(k >= 0 && k < K && b >= 0 && b < B, "prompt unit (%d, %d)", k, b);
            ++hit[(size_t)(k * B + b)];
        }
        for (unsigned char h : hit) CHECK(h == 1, "a (k, block) covered %d times", h);
    }
    CHECK((p.g_window > 0) == ((outs & 4) != 0), "window launch %lld", p.g_window);
    if (p.g_window) {
        std::vector<unsigned char> hit((size_t)(K * p.NW), 0), blocks((size_t)(K * B), 0);
        for (long long u = 0; u < p.g_window * kMonWindowWaves; ++u) {
            int k;
            long long v;
            if (!mon_window_unit(u, p.NW, p.K, &k, &v)) continue;
            CHECK(k >= 0 && k < K && v >= 0 && v < p.NW, "window unit (%d, %lld)", k, v);
            ++hit[(size_t)(k * p.NW + v)];
            for (long long b = v * p.W; b < (v + 1) * p.W && b < B; ++b) ++blocks[(size_t)(k * B + b)];
        }
        for (unsigned char h : hit) CHECK(h == 1, "a (k, window) covered %d times", h);
        for (unsigned char h : blocks) CHECK(h == 1, "a block in %d windows", h);
    }
    const bool sync = (outs & 0xf8) != 0;
    CHECK(p.do_sync == sync && (p.g_energy > 0) == sync && (p.g_pick > 0) == sync && (p.g_term > 0) == (sync && p.J > 0), "sync launches");
    if (p.g_term) {
        std::vector<unsigned char> hit((size_t)(K * Pd * p.J), 0);
        for (long long t = 0; t < p.g_term * kMonThreads; ++t) {
            int k, c;
            long long j;
            if (!mon_term_unit(t, p.J, p.Pd, p.K, &k, &j, &c)) continue;
            CHECK(k >= 0 && k < K && c >= 0 && c < Pd && j >= 0 && j < p.J, "term unit (%d, %d, %lld)", k, c, j);
            CHECK(t == (k * p.J + j) * Pd + c, "term %lld is not where the energies read it", t);
            CHECK(c + j * Pd + Pd <= B, "term (%d, %lld) reads beyond the series", c, j);
            ++hit[(size_t)((k * Pd + c) * p.J + j)];
        }
        for (unsigned char h : hit) CHECK(h == 1, "a (k, c, j) covered %d times", h);
    }
    if (p.g_energy) {
        std::vector<unsigned char> hit((size_t)(K * Pd), 0);
        for (long long t = 0; t < p.g_energy * kMonThreads; ++t) {
            int k, c;
            if (mon_energy_unit(t, p.Pd, p.K, &k, &c)) ++hit[(size_t)(k * Pd + c)];
        }
        for (unsigned char h : hit) CHECK(h == 1, "a (k, c) covered %d times", h);
        CHECK(p.g_pick * kMonThreads >= K && (p.g_pick - 1) * kMonThreads < K, "pick launch %lld", p.g_pick);
    }
    CHECK((p.g_symbol > 0) == ((outs & 0xe0) != 0 && p.cap > 0), "symbol launch %lld", p.g_symbol);
    if (p.g_symbol) {
        std::vector<unsigned char> hit((size_t)(K * p.cap), 0);
        for (long long t = 0; t < p.g_symbol * kMonThreads; ++t) {
            int k;
            long long j;
            if (!mon_symbol_unit(t, p.cap, p.K, &k, &j)) continue;
            CHECK(k >= 0 && k < K && j >= 0 && j < p.cap, "symbol unit (%d, %lld)", k, j);
            ++hit[(size_t)(k * p.cap + j)];
        }
        for (unsigned char h : hit) CHECK(h == 1, "a (k, symbol) covered %d times", h);
    }
    // the carve-up: the parts in use are aligned, disjoint, in order and inside the planned bytes
    struct Part {
        size_t off, bytes;
        bool used;
    } parts[] = {{p.off_pr, (size_t)(K * B * 8), p.own_pr},
                 {p.off_pi, (size_t)(K * B * 8), p.own_pi},
                 {p.off_terms, (size_t)(K * p.J * Pd * 8), sync},
                 {p.off_energy, (size_t)(K * Pd * 8), p.own_energy},
                 {p.off_chan, (size_t)K * sizeof(gat_monitor_channel), p.own_chan}};
    size_t end = 0;
    for (const Part &q : parts) {
        if (!q.used) continue;
        CHECK(q.off % 256 == 0 && q.off >= end && q.off + q.bytes <= p.bytes, "scratch part at %zu + %zu of %zu after %zu", q.off, q.bytes, p.bytes, end);
        end = q.off + q.bytes;
    }
    CHECK(p.own_pr == !(outs & 1) && p.own_pi == !(outs & 2) && p.own_energy == (sync && !(outs & 8)) && p.own_chan == (sync && !(outs & 16)), "ownership");
    CHECK(p.bytes <= kMonMaxScratch && p.bytes < end + 256, "planned bytes %zu for %zu", p.bytes, end);
    gat_monitor_plan rep{};
    mon_report(p, &rep);
    CHECK(rep.struct_size == sizeof rep && rep.num_windows == p.NW && rep.search_symbols == p.J && rep.symbol_capacity == p.cap &&
              rep.scratch_bytes == (int64_t)p.bytes && rep.term_workgroups == p.g_term,
          "report");
}

// an output on the heap at its exact extent (null when not asked for, or a zero extent still given as an address)
template <class T>
struct Out {
    std::vector<T> v;
    bool given;
    Out(size_t n, bool g) : v(g ? n : 0), given(g) {}
    T *ptr() { return given ? (v.empty() ? reinterpret_cast<T *>(uintptr_t(64)) : v.data()) : nullptr; }
};

void run_host(std::mt19937_64 &rng, int B, int K, int M, int L, int pad, int W, int Pd, int forced, long long fb, unsigned outs, bool weighted)
{
    const gat_monitor_config cfg = config(L, (int)(rng() % L), W, Pd, forced, fb, rng);
    const long long n = (long long)K * L * M, stride = n + pad;
    const size_t extent = (size_t)((B - 1) * stride + n);
    std::vector<float> re(extent), im(extent);
    std::uniform_real_distribution<float> u(-50.f, 50.f);
    for (size_t i = 0; i < extent; ++i) re[i] = u(rng), im[i] = u(rng);
    std::vector<double> w_re((size_t)K * M), w_im((size_t)K * M);
    for (size_t i = 0; i < w_re.size(); ++i) w_re[i] = u(rng) / 50.0, w_im[i] = u(rng) / 50.0;
    const long long NW = (B + W - 1) / W, cap = B / Pd;
    Out<double> pr((size_t)K * B, outs & 1), pi((size_t)K * B, outs & 2), en((size_t)K * Pd, outs & 8), sr((size_t)(K * cap), outs & 32),
        si((size_t)(K * cap), outs & 64), sw((size_t)(K * cap), outs & 128);
    Out<gat_monitor_window> win((size_t)(K * NW), outs & 4);
    Out<gat_monitor_channel> ch((size_t)K, outs & 16);
    MonCall a = call(B == 1 ? -7 : stride, B, K, M, &cfg, outs, weighted);
    a.acc_re = re.data(), a.acc_im = im.data();
    MonPlan p{};
    const Refusal r = mon_plan(a, &p);
    CHECK(r.code == GAT_OK, "host case refused: %s", r.msg ? r.msg : "");
    if (r.code != GAT_OK) return;
    check_cover(p, outs);
    mon_host_run(p, re.data(), im.data(), a.acc_block_stride, &cfg, weighted ? w_re.data() : nullptr, weighted ? w_im.data() : nullptr, pr.ptr(),
                 pi.ptr(), win.ptr(), en.ptr(), ch.ptr(), sr.ptr(), si.ptr(), sw.ptr());
    if (outs & 4) {
        long long blocks = 0;
        for (long long v = 0; v < NW; ++v) blocks += win.v[(size_t)v].blocks;
        CHECK(blocks == B && win.v[(size_t)(NW - 1)].blocks == B - (NW - 1) * W, "window blocks %lld of %d", blocks, B);
    }
    if (outs & 16)
        for (int k = 0; k < K; ++k) {
            const gat_monitor_channel &c = ch.v[(size_t)k];
            const long long J = p.J;
            if (forced >= 0)
                CHECK(c.symbol_offset == forced && c.start == mon_mod(forced - fb, Pd), "forced record %d %d", c.symbol_offset, c.start);
            else
                CHECK((J == 0) == (c.start == -1), "searched record start %d with J %lld", c.start, J);
            CHECK(c.start < 0 ? c.num_symbols == 0 && c.symbol_offset == -1 && c.e_max == 0.0 && c.e_second == 0.0
                              : c.num_symbols == (B >= c.start ? (B - c.start) / Pd : 0) && c.symbol_offset == mon_mod(fb + c.start, Pd),
                  "record of channel %d", k);
            CHECK(c.num_symbols <= cap && (Pd > 1 || c.e_second == 0.0), "symbols %d of %lld", c.num_symbols, cap);
            if (forced < 0 && (outs & 8) && J > 0)
                for (int i = 0; i < Pd; ++i) CHECK(en.v[(size_t)k * Pd + i] <= c.e_max && (i >= c.start || en.v[(size_t)k * Pd + i] < c.e_max), "c* is not the lowest largest");
        }
}

} // namespace

int main()
{
    std::mt19937_64 rng(20240611);
    auto pick = [&](long long lo, long long hi) { return (long long)(lo + rng() % (unsigned long long)(hi - lo + 1)); };

    // ---- random plans
    int planned = 0;
    for (int it = 0; it < 3000; ++it) {
        const int Pd = (int)(it % 5 == 0 ? pick(1, 128) : pick(1, 24));
        const int B = (int)(it % 7 == 0 ? pick(1, 3000) : it % 3 == 0 ? pick(1, 3 * Pd) : pick(1, 300));
        const int K = (int)(it % 11 == 0 ? pick(1, 40) : pick(1, 6)), M = (int)pick(1, 64), L = (int)pick(1, 7);
        const int W = (int)(it % 4 == 0 ? pick(1, B + 5) : pick(1, 40));
        const int forced = it % 2 ? -1 : (int)pick(0, Pd - 1);
        const gat_monitor_config cfg = config(L, (int)pick(0, L - 1), W, Pd, forced, pick(0, 1000000), rng);
        unsigned outs = (unsigned)pick(1, 255);
        MonPlan p = untouched_plan();
        const Refusal r = mon_plan(call((long long)K * L * M + pick(0, 9), B, K, M, &cfg, outs, it % 3 == 0), &p);
        CHECK(r.code == GAT_OK, "a valid call refused: %s", r.msg ? r.msg : "");
        if (r.code != GAT_OK) continue;
        check_cover(p, outs);
        ++planned;
    }
    // the limits are planned, and the call beyond the scratch bound is refused
    {
        const gat_monitor_config cfg = config(3, 1, 20, 20, -1, 0, rng);
        MonPlan p{};
        CHECK(mon_plan(call(3, GAT_MAX_MONITOR_BLOCKS, 1, 1, &cfg), &p).code == GAT_OK && p.bytes <= kMonMaxScratch, "2^20 blocks of one channel");
        CHECK(mon_plan(call(3 * 4096 * 64, 97, GAT_MAX_MONITOR_CHANNELS, GAT_MAX_ARRAY_ANTS, &cfg), &p).code == GAT_OK, "4096 channels of 64 antennas");
        expect_refusal(call(3 * 4096, GAT_MAX_MONITOR_BLOCKS, GAT_MAX_MONITOR_CHANNELS, 1, &cfg), GAT_ERR_RANGE, "scratch beyond 1 GiB");
    }

    // ---- refusals
    {
        const gat_monitor_config good = config(3, 1, 7, 10, -1, 0, rng);
        const long long n = 2 * 3 * 2;
        MonPlan p{};
        CHECK(mon_plan(call(n, 24, 2, 2, &good), &p).code == GAT_OK, "the base call");
        CHECK(mon_plan(call(n, 24, 2, 2, &good), nullptr).code == GAT_ERR_ARG, "null plan");
        MonCall a = call(n, 24, 2, 2, &good);
        a.acc_re = nullptr;
        expect_refusal(a, GAT_ERR_ARG, "null acc_re");
        a = call(n, 24, 2, 2, &good), a.acc_im = nullptr;
        expect_refusal(a, GAT_ERR_ARG, "null acc_im");
        expect_refusal(call(n, 24, 2, 2, nullptr), GAT_ERR_ARG, "null config");
        gat_monitor_config c = good;
        c.struct_size -= 8;
        expect_refusal(call(n, 24, 2, 2, &c), GAT_ERR_ARG, "struct_size");
        expect_refusal(call(n, 0, 2, 2, &good), GAT_ERR_ARG, "B = 0");
        expect_refusal(call(n, 24, 0, 2, &good), GAT_ERR_ARG, "K = 0");
        expect_refusal(call(n, 24, 2, 0, &good), GAT_ERR_ARG, "M = 0");
        c = good, c.num_taps = 0, c.prompt_index = 0;
        expect_refusal(call(n, 24, 2, 2, &c), GAT_ERR_ARG, "L = 0");
        expect_refusal(call(2 * 3 * 65, 24, 2, 65, &good), GAT_ERR_RANGE, "M = 65");
        expect_refusal(call(n, GAT_MAX_MONITOR_BLOCKS + 1, 2, 2, &good), GAT_ERR_RANGE, "B above 2^20");
        expect_refusal(call(4097 * 6, 24, 4097, 2, &good), GAT_ERR_RANGE, "K = 4097");
        c = good, c.prompt_index = 3;
        expect_refusal(call(n, 24, 2, 2, &c), GAT_ERR_RANGE, "prompt_index = L");
        c = good, c.prompt_index = -1;
        expect_refusal(call(n, 24, 2, 2, &c), GAT_ERR_RANGE, "prompt_index < 0");
        c = good, c.window_blocks = 0;
        expect_refusal(call(n, 24, 2, 2, &c), GAT_ERR_ARG, "W = 0");
        c = good, c.symbol_blocks = 0;
        expect_refusal(call(n, 24, 2, 2, &c), GAT_ERR_RANGE, "Pd = 0");
        c = good, c.symbol_blocks = 129;
        expect_refusal(call(n, 24, 2, 2, &c), GAT_ERR_RANGE, "Pd = 129");
        for (int v : {0, 2, -2}) {
            c = good, c.overlay[9] = (int8_t)v;
            expect_refusal(call(n, 24, 2, 2, &c), GAT_ERR_ARG, "overlay entry");
        }
        c = good, c.overlay[10] = 0; // beyond Pd: ignored
        CHECK(mon_plan(call(n, 24, 2, 2, &c), &p).code == GAT_OK, "an entry beyond Pd is ignored");
        c = good, c.symbol_offset = -2;
        expect_refusal(call(n, 24, 2, 2, &c), GAT_ERR_RANGE, "symbol_offset = -2");
        c = good, c.symbol_offset = 10;
        expect_refusal(call(n, 24, 2, 2, &c), GAT_ERR_RANGE, "symbol_offset = Pd");
        c = good, c.first_block = -1;
        expect_refusal(call(n, 24, 2, 2, &c), GAT_ERR_ARG, "first_block < 0");
        expect_refusal(call(n - 1, 24, 2, 2, &good), GAT_ERR_ARG, "stride below one block");
        expect_refusal(call(-n, 24, 2, 2, &good), GAT_ERR_ARG, "negative stride");
        CHECK(mon_plan(call(-n, 1, 2, 2, &good), &p).code == GAT_OK, "one block takes any stride");
        a = call(n, 24, 2, 2, &good, 0xff, true), a.w_im = nullptr;
        expect_refusal(a, GAT_ERR_ARG, "w_re alone");
        a = call(n, 24, 2, 2, &good, 0xff, true), a.w_re = nullptr;
        expect_refusal(a, GAT_ERR_ARG, "w_im alone");
        expect_refusal(call(n, 24, 2, 2, &good, 0), GAT_ERR_ARG, "every output null");
    }

    // ---- the host twin on exact extents
    int ran = 0;
    for (int Pd : {1, 2, 10, 20})
        for (int B : {1, Pd - 1, Pd, 2 * Pd - 2, 2 * Pd - 1, 2 * Pd, 97})
            for (int pad : {0, 5})
                for (int W : {1, 7, B, B + 3})
                    for (int forced : {-1, Pd / 2}) {
                        if (B < 1) continue;
                        const unsigned subsets[] = {0xff, 4, 0xe0, 16, 8, 1, 2, 32, 0xfc};
                        run_host(rng, B, (int)pick(1, 3), (int)pick(1, 3), (int)pick(1, 3), pad, W, Pd, forced, (ran % 2) * 13, subsets[ran % 9], ran % 3 == 0);
                        ++ran;
                    }
    for (int it = 0; it < 300; ++it) {
        const int Pd = (int)pick(1, 24), B = (int)pick(1, 200);
        run_host(rng, B, (int)pick(1, 4), (int)pick(1, 5), (int)pick(1, 4), (int)pick(0, 6), (int)pick(1, B + 4), Pd, it % 2 ? -1 : (int)pick(0, Pd - 1),
                 pick(0, 100000), (unsigned)pick(1, 255), it % 2 == 0);
        ++ran;
    }
    std::printf("planned %d calls, ran the host twin %d times, %d failures\n", planned, ran, failures);
    return failures ? 1 : 0;
}
