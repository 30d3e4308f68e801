// Stand-alone check of the navigation data layer's pure plan (csrc/gat_nav_plan.h) and of the host twin's loops over it
// (nav_host_run, the rule of csrc/gat_nav.h), over a few thousand random calls.  Every planned call must cover each (k, symbol),
// (k, candidate) and (k, frame) exactly once through the workgroups and threads the kernels are launched with, give a wave to every
// channel (quantiser, choice) and (channel, phase) (trellis), carve its scratch in disjoint, aligned parts within the planned
// bytes, and report the counts of the rule; every documented refusal must return its code with nothing planned.  The twin then
// runs on heap buffers of exactly the extents the call describes -- a capacity above the counts, counts from monitor records,
// every subset of the outputs, streams that hold frames at every offset --, so that AddressSanitizer sees any read outside the
// symbols and any write outside an output.  Built with -fsanitize=address,undefined by tests/test_navigation_plan_host.py.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "gat_nav.h"
#include "gat_nav_plan.h"

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

gat_nav_config config(int format, int cap, int max_frames, int min_frames)
{
    gat_nav_config c{};
    c.struct_size = sizeof(gat_nav_config);
    c.format = format, c.symbol_capacity = cap, c.max_frames = max_frames, c.min_frames = min_frames;
    return c;
}

NavCall call(int K, const gat_nav_config *cfg, unsigned outs = 0xf, bool mon = false)
{
    NavCall a{};
    a.sym_re = kGiven, a.mon = mon ? kGiven : nullptr, a.K = K, a.cfg = cfg;
    a.channels = outs & 1 ? kGiven : nullptr, a.frames = outs & 2 ? kGiven : nullptr, a.decoded = outs & 4 ? kGiven : nullptr;
    a.path_metric = outs & 8 ? kGiven : nullptr;
    return a;
}

NavPlan untouched_plan()
{
    NavPlan p;
    std::memset(&p, 0x5a, sizeof p);
    return p;
}
bool untouched(const NavPlan &p)
{
    const NavPlan q = untouched_plan();
    return std::memcmp(&p, &q, sizeof p) == 0;
}

void expect_refusal(const NavCall &a, int code, const char *what)
{
    NavPlan p = untouched_plan();
    const Refusal r = nav_plan(a, &p);
    CHECK(r.code == code, "%s: got %d, want %d", what, r.code, code);
    CHECK(r.code == GAT_OK || r.msg != nullptr, "%s: a refusal without a message", what);
    CHECK(untouched(p), "%s: a refused call planned something", what);
}

// walks every launch as the kernels do and counts each unit
void check_cover(const NavPlan &p, unsigned outs)
{
    const long long K = p.K, cap = p.cap;
    const bool cnav = p.format == GAT_NAV_CNAV, sync = (outs & 3) != 0;
    CHECK(p.P == (cnav ? 2 : 1) && p.bit_cap == p.cap / p.P && p.C == p.P * 600, "counts P %d bit_cap %d C %d", p.P, p.bit_cap, p.C);
    CHECK((p.g_slice > 0) == !cnav && p.g_quant == (cnav ? K : 0) && p.g_trellis == (cnav ? 2 * K : 0), "decode launches");
    if (p.g_slice) {
        std::vector<unsigned char> hit((size_t)(K * cap), 0);
        long long metric_units = 0;
        for (long long t = 0; t < p.g_slice * kNavThreads; ++t) {
            int k, j;
            metric_units += t < K;
            if (!nav_slice_unit(t, p.cap, p.K, &k, &j)) continue;
            CHECK(k >= 0 && k < K && j >= 0 && j < cap && t == k * cap + j, "slice unit (%d, %d)", k, j);
            ++hit[(size_t)t];
        }
        for (unsigned char h : hit) CHECK(h == 1, "a (k, symbol) covered %d times", h);
        CHECK(metric_units == K, "path_metric of %lld channels", metric_units);
    }
    CHECK(p.do_sync == sync && (p.g_score > 0) == sync && (p.g_pick > 0) == sync && (p.g_frame > 0) == ((outs & 2) != 0), "sync launches");
    if (p.g_score) {
        std::vector<unsigned char> hit((size_t)(K * p.C), 0);
        for (long long t = 0; t < p.g_score * kNavThreads; ++t) {
            int k, c, ph, o, pol;
            if (!nav_score_unit(t, p.C, p.K, &k, &c)) continue;
            nav_candidate(c, &ph, &o, &pol);
            CHECK(k >= 0 && k < K && ph >= 0 && ph < p.P && o >= 0 && o < 300 && (pol == 0 || pol == 1) && c == (ph * 300 + o) * 2 + pol, "candidate %d", c);
            ++hit[(size_t)t];
        }
        for (unsigned char h : hit) CHECK(h == 1, "a (k, candidate) covered %d times", h);
        CHECK(p.g_pick * kNavPickWaves >= K && (p.g_pick - 1) * kNavPickWaves < K, "pick launch %lld", p.g_pick);
    }
    if (p.g_frame) {
        std::vector<unsigned char> hit((size_t)(K * p.max_frames), 0);
        for (long long t = 0; t < p.g_frame * kNavThreads; ++t) {
            int k, f;
            if (!nav_frame_unit(t, p.max_frames, p.K, &k, &f)) continue;
            CHECK(k >= 0 && k < K && f >= 0 && f < p.max_frames && t == (long long)k * p.max_frames + f, "frame unit (%d, %d)", k, f);
            ++hit[(size_t)t];
        }
        for (unsigned char h : hit) CHECK(h == 1, "a (k, frame) covered %d times", h);
    }
    // the carve-up: the parts in use are aligned, disjoint, in order and inside the planned bytes
    struct Part {
        size_t off, bytes;
        bool used;
    } parts[] = {{p.off_q, (size_t)(K * cap), cnav},
                 {p.off_surv, (size_t)(K * 2 * p.bit_cap * 8), cnav},
                 {p.off_decoded, (size_t)(K * p.P * p.bit_cap), p.own_decoded},
                 {p.off_scores, (size_t)(K * p.C * 4), sync},
                 {p.off_chan, (size_t)K * sizeof(gat_nav_channel), p.own_chan}};
    size_t end = 0;
    for (const Part &q : parts) {
        if (!q.used) continue;
        CHECK(q.off % 256 == 0 && q.off >= end && q.off + q.bytes <= p.bytes, "scratch part at %zu + %zu of %zu after %zu", q.off, q.bytes, p.bytes, end);
        end = q.off + q.bytes;
    }
    CHECK(p.own_decoded == !(outs & 4) && p.own_chan == (sync && !(outs & 1)), "ownership");
    CHECK(p.bytes <= kNavMaxScratch && p.bytes < end + 256, "planned bytes %zu for %zu", p.bytes, end);
    // every trellis row lies inside its parts: T <= bit_cap steps of 8 bytes and one byte
    for (int ph = 0; ph < p.P; ++ph) CHECK(nav_bits(p.format, p.cap, ph) <= p.bit_cap && (!cnav || nav_bits(p.format, p.cap, ph) == 0 || ph + 2 * nav_bits(p.format, p.cap, ph) <= p.cap), "row of phase %d", ph);
    gat_nav_plan rep{};
    nav_report(p, &rep);
    CHECK(rep.struct_size == sizeof rep && rep.num_phases == p.P && rep.bit_capacity == p.bit_cap && rep.num_candidates == p.C &&
              rep.scratch_bytes == (int64_t)p.bytes && rep.trellis_workgroups == p.g_trellis && rep.frame_workgroups == p.g_frame,
          "report");
}

// ---- streams with frames in them, made with the rule's own pieces (the twin's answers are checked by the Python tests)
std::vector<uint8_t> lnav_frame_bits(std::mt19937_64 &rng, int tow)
{
    std::vector<uint8_t> b(300);
    for (auto &v : b) v = (uint8_t)(rng() & 1);
    const uint8_t pre[8] = {1, 0, 0, 0, 1, 0, 1, 1};
    std::memcpy(b.data(), pre, 8);
    for (int w = 0; w < 10; ++w) {
        if (w == 1) { // the HOW's source bits, sent XORed with the D30 the TLM word ended in: the count and subframe 3
            for (int i = 0; i < 17; ++i) b[30 + i] = (uint8_t)(((tow >> (16 - i)) & 1) ^ b[29]);
            b[30 + 19] = b[29], b[30 + 20] = (uint8_t)(1 ^ b[29]), b[30 + 21] = (uint8_t)(1 ^ b[29]);
        } // the parity of every word, by trial: 64 endings (the HOW: those that end in 00, over its two free bits)
        bool done = false;
        for (int free = 0; free < 4 && !done; ++free)
            for (int par = 0; par < 64 && !done; ++par) {
                if (w == 1) b[30 + 22] = (uint8_t)(free >> 1), b[30 + 23] = (uint8_t)(free & 1);
                for (int i = 0; i < 6; ++i) b[30 * w + 24 + i] = (uint8_t)((par >> (5 - i)) & 1);
                bool ok;
                nav_lnav_word(b.data(), 0, w, &ok);
                done = ok && (w != 1 || (par & 3) == 0);
            }
        CHECK(done, "no parity for word %d", w);
    }
    return b;
}
std::vector<uint8_t> cnav_frame_bits(std::mt19937_64 &rng, int tow)
{
    std::vector<uint8_t> b(300);
    for (auto &v : b) v = (uint8_t)(rng() & 1);
    const uint8_t pre[8] = {1, 0, 0, 0, 1, 0, 1, 1};
    std::memcpy(b.data(), pre, 8);
    for (int i = 0; i < 17; ++i) b[20 + i] = (uint8_t)((tow >> (16 - i)) & 1);
    const uint32_t crc = nav_crc24q_bits(b.data(), 0, 276);
    for (int i = 0; i < 24; ++i) b[276 + i] = (uint8_t)((crc >> (23 - i)) & 1);
    return b;
}
// symbols of `frames` frames after `prefix` random bits, inverted or not, after `phase` loose symbols (CNAV)
std::vector<double> stream(std::mt19937_64 &rng, int format, int prefix, int frames, int suffix, bool inverted, int phase, double sigma)
{
    std::vector<uint8_t> bits;
    for (int i = 0; i < prefix; ++i) bits.push_back((uint8_t)(rng() & 1));
    for (int f = 0; f < frames; ++f) {
        const std::vector<uint8_t> fr = format == GAT_NAV_CNAV ? cnav_frame_bits(rng, (100799 + f) % kNavTowModulus) : lnav_frame_bits(rng, (100799 + f) % kNavTowModulus);
        bits.insert(bits.end(), fr.begin(), fr.end());
    }
    for (int i = 0; i < suffix; ++i) bits.push_back((uint8_t)(rng() & 1));
    std::vector<uint8_t> sym;
    if (format == GAT_NAV_CNAV) {
        for (int i = 0; i < phase; ++i) sym.push_back(0);
        int s = 0;
        for (uint8_t u : bits) {
            int c1, c2;
            nav_fec_pair(s, u, &c1, &c2);
            sym.push_back((uint8_t)c1), sym.push_back((uint8_t)c2);
            s = (u << 5) | (s >> 1);
        }
    } else
        sym = bits;
    std::normal_distribution<double> noise(0.0, sigma);
    std::vector<double> x(sym.size());
    for (size_t i = 0; i < sym.size(); ++i) x[i] = ((sym[i] ? -1.0 : 1.0) + noise(rng)) * (inverted ? -1.0 : 1.0);
    return x;
}

// an output on the heap at its exact extent (null when not asked for, or a zero extent still given as an address)
template <class T>
struct Out {
    std::vector<T> v;
    bool given;
    Out(size_t n, bool g) : v(g ? n : 0), given(g) {}
    T *ptr() { return given ? (v.empty() ? reinterpret_cast<T *>(uintptr_t(64)) : v.data()) : nullptr; }
};

int synced_channels = 0, framed_channels = 0;

void run_host(std::mt19937_64 &rng, int format, int K, int cap, int max_frames, int min_frames, unsigned outs, bool records, int frames_sent)
{
    const gat_nav_config cfg = config(format, cap, max_frames, min_frames);
    std::vector<double> sym((size_t)K * cap, std::numeric_limits<double>::quiet_NaN());
    std::vector<gat_monitor_channel> mon((size_t)K);
    std::vector<int> want_offset((size_t)K, -2), count((size_t)K, cap);
    for (int k = 0; k < K; ++k) {
        const int prefix = (int)(rng() % 300), phase = format == GAT_NAV_CNAV ? (int)(rng() & 1) : 0;
        const std::vector<double> x = stream(rng, format, prefix, frames_sent, 40 + (int)(rng() % 50), (rng() & 1) != 0, phase, 0.2);
        const int n = records ? (int)((rng() % 3 == 0) ? rng() % (size_t)(cap + 1) : (x.size() < (size_t)cap ? x.size() : (size_t)cap)) : cap;
        for (int j = 0; j < cap; ++j)
            if ((size_t)j < x.size()) sym[(size_t)k * cap + j] = x[(size_t)j];
        count[(size_t)k] = n;
        mon[(size_t)k] = gat_monitor_channel{0, 0, records ? (k % 5 == 4 ? n + cap + 7 : n) : -9, 0, 1.0, 0.5}; // a count above the row is clamped
        if (records && k % 5 == 4) count[(size_t)k] = cap;
        const int bits_needed = (prefix + 300 * frames_sent + (format == GAT_NAV_CNAV ? GAT_NAV_TAIL_BITS : 0)) * (format == GAT_NAV_CNAV ? 2 : 1) + phase;
        if (frames_sent >= min_frames && count[(size_t)k] >= bits_needed && x.size() <= (size_t)cap) want_offset[(size_t)k] = prefix;
    }
    const int P = nav_phases(format), bit_cap = cap / P;
    Out<gat_nav_channel> ch((size_t)K, outs & 1);
    Out<gat_nav_frame> fr((size_t)K * max_frames, outs & 2);
    Out<uint8_t> dec((size_t)K * P * bit_cap, outs & 4);
    Out<int32_t> pm((size_t)K * P, outs & 8);
    NavCall a = call(K, &cfg, outs, records);
    NavPlan p{};
    const Refusal r = nav_plan(a, &p);
    CHECK(r.code == GAT_OK, "host case refused: %s", r.msg ? r.msg : "");
    if (r.code != GAT_OK) return;
    check_cover(p, outs);
    nav_host_run(p, cap ? sym.data() : reinterpret_cast<const double *>(uintptr_t(64)), records ? mon.data() : nullptr, ch.ptr(), fr.ptr(), dec.ptr(), pm.ptr());
    if (outs & 1)
        for (int k = 0; k < K; ++k) {
            const gat_nav_channel &c = ch.v[(size_t)k];
            CHECK(c.frame_offset >= -1 && c.frame_offset < 300 && c.num_frames >= 0 && c.num_frames <= max_frames && c.score >= c.second_score && c.second_score >= 0,
                  "record of channel %d", k);
            CHECK((c.frame_offset >= 0) == (c.score >= min_frames) && (c.frame_offset >= 0 || (c.num_frames == 0 && c.inverted == 0 && c.symbol_phase == 0)), "sync of channel %d", k);
            CHECK(c.num_bits == nav_bits(format, count[(size_t)k], c.symbol_phase), "bits of channel %d: %d", k, c.num_bits);
            if (want_offset[(size_t)k] >= 0) CHECK(c.frame_offset == want_offset[(size_t)k] && c.score >= frames_sent, "channel %d: offset %d, score %d", k, c.frame_offset, c.score);
            synced_channels += c.frame_offset >= 0;
            if ((outs & 2) && c.frame_offset >= 0) {
                ++framed_channels;
                for (int f = 0; f < max_frames; ++f) {
                    const gat_nav_frame &x = fr.v[(size_t)k * max_frames + f];
                    if (f >= c.num_frames) CHECK(x.status == 0 && x.tow == 0 && x.words[9] == 0, "a row beyond the frames is not zero");
                }
                if (want_offset[(size_t)k] >= 0 && frames_sent >= 2 && c.num_frames >= 2)
                    CHECK(fr.v[(size_t)k * max_frames].tow == 100799 && fr.v[(size_t)k * max_frames + 1].tow == 0 && c.tow_steps >= 1, "the week's last TOW step: format %d tows %d %d status %x %x steps %d frames_sent %d", format, fr.v[(size_t)k * max_frames].tow, fr.v[(size_t)k * max_frames + 1].tow, fr.v[(size_t)k * max_frames].status, fr.v[(size_t)k * max_frames + 1].status, c.tow_steps, frames_sent);
            }
        }
}

} // namespace

int main()
{
    std::mt19937_64 rng(20240917);
    auto pick = [&](long long lo, long long hi) { return (long long)(lo + rng() % (unsigned long long)(hi - lo + 1)); };

    // ---- random plans
    int planned = 0;
    for (int it = 0; it < 3000; ++it) {
        const int format = it & 1, K = (int)(it % 11 == 0 ? pick(1, 40) : pick(1, 6));
        const int cap = (int)(it % 7 == 0 ? pick(0, 7000) : it % 5 == 0 ? pick(0, 4) : pick(0, 700));
        const gat_nav_config cfg = config(format, cap, (int)pick(1, 30), (int)pick(1, 5));
        const unsigned outs = (unsigned)pick(1, 15);
        NavPlan p = untouched_plan();
        const Refusal r = nav_plan(call(K, &cfg, outs, it % 3 == 0), &p);
        CHECK(r.code == GAT_OK, "a valid call refused: %s", r.msg ? r.msg : "");
        if (r.code != GAT_OK) continue;
        check_cover(p, outs);
        ++planned;
    }
    // the limits are planned, and the call beyond the scratch bound is refused
    {
        NavPlan p{};
        gat_nav_config cfg = config(GAT_NAV_CNAV, GAT_MAX_MONITOR_BLOCKS, 1, 1);
        CHECK(nav_plan(call(64, &cfg), &p).code == GAT_OK && p.bytes <= kNavMaxScratch, "2^20 symbols of 64 channels");
        expect_refusal(call(GAT_MAX_MONITOR_CHANNELS, &cfg), GAT_ERR_RANGE, "scratch beyond 1 GiB");
        cfg = config(GAT_NAV_LNAV, 7000, 23, 1);
        CHECK(nav_plan(call(GAT_MAX_MONITOR_CHANNELS, &cfg), &p).code == GAT_OK, "4096 channels");
    }

    // ---- refusals
    {
        const gat_nav_config good = config(GAT_NAV_CNAV, 700, 2, 1);
        NavPlan p{};
        CHECK(nav_plan(call(3, &good), &p).code == GAT_OK, "the base call");
        CHECK(nav_plan(call(3, &good), nullptr).code == GAT_ERR_ARG, "null plan");
        NavCall a = call(3, &good);
        a.sym_re = nullptr;
        expect_refusal(a, GAT_ERR_ARG, "null sym_re");
        expect_refusal(call(3, nullptr), GAT_ERR_ARG, "null config");
        gat_nav_config c = good;
        c.struct_size -= 4;
        expect_refusal(call(3, &c), GAT_ERR_ARG, "struct_size");
        expect_refusal(call(0, &good), GAT_ERR_ARG, "K = 0");
        expect_refusal(call(-3, &good), GAT_ERR_ARG, "K < 0");
        c = good, c.symbol_capacity = -1;
        expect_refusal(call(3, &c), GAT_ERR_ARG, "capacity < 0");
        c = good, c.max_frames = 0;
        expect_refusal(call(3, &c), GAT_ERR_ARG, "max_frames = 0");
        c = good, c.min_frames = 0;
        expect_refusal(call(3, &c), GAT_ERR_ARG, "min_frames = 0");
        c = good, c.format = 2;
        expect_refusal(call(3, &c), GAT_ERR_ARG, "format = 2");
        c = good, c.format = -1;
        expect_refusal(call(3, &c), GAT_ERR_ARG, "format = -1");
        expect_refusal(call(3, &good, 0), GAT_ERR_ARG, "every output null");
        expect_refusal(call(GAT_MAX_MONITOR_CHANNELS + 1, &good), GAT_ERR_RANGE, "K = 4097");
        c = good, c.symbol_capacity = GAT_MAX_MONITOR_BLOCKS + 1;
        expect_refusal(call(3, &c), GAT_ERR_RANGE, "capacity above 2^20");
        c = good, c.max_frames = 0x7fffffff;
        expect_refusal(call(GAT_MAX_MONITOR_CHANNELS, &c), GAT_ERR_RANGE, "frame workgroups");
        c = good, c.symbol_capacity = 0;
        CHECK(nav_plan(call(3, &c), &p).code == GAT_OK && p.bit_cap == 0, "an empty capacity is planned");
    }

    // ---- the host twin on exact extents
    int ran = 0;
    for (int format : {GAT_NAV_LNAV, GAT_NAV_CNAV})
        for (int cap : {0, 1, 2, 3, 127, 128, 129, 257, 700, 1500})
            for (int sent : {0, 1, 2})
                for (int records : {0, 1}) {
                    const unsigned subsets[] = {0xf, 1, 2, 4, 8, 3, 0xa, 0xd};
                    run_host(rng, format, (int)pick(1, 3), cap * (format == GAT_NAV_CNAV && cap > 300 ? 2 : 1), (int)pick(1, 4), (int)pick(1, 2), subsets[ran % 8], records != 0, sent);
                    ++ran;
                }
    for (int it = 0; it < 120; ++it) {
        const int format = it & 1, sent = (int)pick(0, 3);
        run_host(rng, format, (int)pick(1, 4), (int)pick(0, 1300) * (format + 1), (int)pick(1, 5), (int)pick(1, 3), (unsigned)pick(1, 15), it % 3 != 0, sent);
        ++ran;
    }
    CHECK(synced_channels > 30 && framed_channels > 10, "too few synchronised channels: %d, %d", synced_channels, framed_channels);
    std::printf("planned %d calls, ran the host twin %d times (%d channels synchronised, %d with frames), %d failures\n", planned, ran, synced_channels, framed_channels, failures);
    return failures ? 1 : 0;
}
