// gat_nav.h -- the navigation data layer's rule (include/gat.h, "navigation data"): the symbol count of a channel, the hard bits and
// the (32,26) parity of the legacy message, the quantiser, the K = 7 rate-1/2 trellis and CRC-24Q of CNAV, a frame's hit and its
// record, and the choice among the candidates, written once for the device kernels (gat_nav.hip) and for the host twin
// (gat_nav_plan.h), as gat_mon.h is for the monitor.  Integer arithmetic throughout but for the quantiser's scale, which is double
// precision, sequential in the stated order and compiled without contraction in both builds: both give the same bits.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "gat.h"
#include "gat_hd.h"

namespace gat {

constexpr int kNavStates = 64;      // K = 7: six previous inputs, one state a lane
constexpr int kNavOffsets = GAT_NAV_FRAME_BITS;
constexpr int kNavLnavGood = 0x7ff; // preamble and ten words
constexpr int kNavCnavGood = 0x3;   // preamble and CRC
constexpr int kNavTowModulus = 100800;

// ---- common ------------------------------------------------------------------------------------------------------------------------
GAT_HD inline bool nav_finite(double x)
{
    uint64_t u;
    __builtin_memcpy(&u, &x, sizeof u);
    return ((u >> 52) & 0x7ff) != 0x7ff;
}
// a symbol as the rule reads it: a non-finite one counts as 0
GAT_HD inline double nav_value(double x) { return nav_finite(x) ? x : 0.0; }
GAT_HD inline int nav_phases(int format) { return format == GAT_NAV_CNAV ? 2 : 1; }
// n_k: the monitor's count on the device, clamped to the row, or the whole row
GAT_HD inline int nav_symbols(const gat_monitor_channel *mon, int k, int cap)
{
    if (!mon) return cap;
    const int n = mon[k].num_symbols;
    return n < 0 ? 0 : (n > cap ? cap : n);
}
// decoded bits of phase ph, and how many of them the frame search reads
GAT_HD inline int nav_bits(int format, int n, int ph) { return format == GAT_NAV_CNAV ? (n - ph > 0 ? (n - ph) / 2 : 0) : n; }
GAT_HD inline int nav_search_bits(int format, int bits)
{
    if (format != GAT_NAV_CNAV) return bits;
    return bits > GAT_NAV_TAIL_BITS ? bits - GAT_NAV_TAIL_BITS : 0;
}
GAT_HD inline int nav_parity32(uint32_t v)
{
    v ^= v >> 16, v ^= v >> 8, v ^= v >> 4, v ^= v >> 2, v ^= v >> 1;
    return (int)(v & 1u);
}
// 10001011 in the first eight bits of b, every bit XORed with p
GAT_HD inline bool nav_preamble(const uint8_t *b, int p)
{
    unsigned v = 0;
    for (int i = 0; i < 8; ++i) v = (v << 1) | (unsigned)((b[i] ^ p) & 1);
    return v == 0x8bu;
}
GAT_HD inline uint32_t nav_field(const uint8_t *b, int p, int first, int count)
{
    uint32_t v = 0;
    for (int i = 0; i < count; ++i) v = (v << 1) | (uint32_t)((b[first + i] ^ p) & 1);
    return v;
}

// ---- LNAV --------------------------------------------------------------------------------------------------------------------------
GAT_HD inline int nav_lnav_bit(double x) { return nav_value(x) < 0.0 ? 1 : 0; }
GAT_HD inline uint32_t nav_lnav_mask(int i)
{
    const uint32_t m[6] = {0xBB1F3480u, 0x5D8F9A40u, 0xAEC7CD00u, 0x5763E680u, 0x6BB1F340u, 0x8B7A89C0u};
    return m[i];
}
// Word w (0 .. 9) of the frame at b as 32 bits: D29* in bit 31, D30* in bit 30 (both 0 for word 1), the thirty received bits
// below.  *ok: the six parity bits agree.  Returns the word with D30* removed from its data bits.
GAT_HD inline uint32_t nav_lnav_word(const uint8_t *b, int p, int w, bool *ok)
{
    uint32_t x = nav_field(b, p, 30 * w, 30);
    if (w > 0) x |= nav_field(b, p, 30 * w - 2, 2) << 30;
    if (x & 0x40000000u) x ^= 0x3FFFFFC0u;
    uint32_t par = 0;
    for (int i = 0; i < 6; ++i) par = (par << 1) | (uint32_t)nav_parity32(x & nav_lnav_mask(i));
    *ok = par == (x & 0x3fu);
    return x;
}
GAT_HD inline int nav_lnav_id(uint32_t word2) { return (int)((word2 >> 8) & 7u); }
GAT_HD inline bool nav_lnav_hit(const uint8_t *b, int p)
{
    if (!nav_preamble(b, p)) return false;
    bool ok1, ok2;
    nav_lnav_word(b, p, 0, &ok1);
    const uint32_t w2 = nav_lnav_word(b, p, 1, &ok2);
    const int id = nav_lnav_id(w2);
    return ok1 && ok2 && (w2 & 3u) == 0 && id >= 1 && id <= 5;
}

// ---- CNAV --------------------------------------------------------------------------------------------------------------------------
GAT_HD inline uint32_t nav_crc24q_bit(uint32_t crc, int bit)
{
    crc ^= (uint32_t)(bit & 1) << 23;
    crc <<= 1;
    if (crc & 0x1000000u) crc ^= 0x1864CFBu;
    return crc;
}
GAT_HD inline uint32_t nav_crc24q_bits(const uint8_t *b, int p, int count)
{
    uint32_t crc = 0;
    for (int i = 0; i < count; ++i) crc = nav_crc24q_bit(crc, b[i] ^ p);
    return crc;
}
GAT_HD inline bool nav_cnav_hit(const uint8_t *b, int p) { return nav_preamble(b, p) && nav_crc24q_bits(b, p, GAT_NAV_FRAME_BITS) == 0; }

// the quantiser: unit from the sum of |x| (nav_value) over n symbols, q from x and unit
GAT_HD inline double nav_abs(double x)
{
    const double v = nav_value(x);
    return v < 0.0 ? -v : v;
}
GAT_HD inline int nav_quantise(double x, double unit)
{
    if (!nav_finite(unit) || !(unit > 0.0)) return 0;
    const double v = (nav_value(x) * 16.0) / unit;
    if (v >= 127.0) return 127;
    if (v <= -127.0) return -127;
    return (int)__builtin_rint(v);
}
// The code: s holds the six previous inputs, newest in bit 5; u is the input.  G1 = 171 taps delays 0 1 2 3 6, G2 = 133 delays
// 0 2 3 5 6 (octal, the MSB the input); G1's symbol is sent first.
GAT_HD inline void nav_fec_pair(int s, int u, int *c1, int *c2)
{
    *c1 = (u ^ (s >> 5) ^ (s >> 4) ^ (s >> 3) ^ s) & 1;
    *c2 = (u ^ (s >> 4) ^ (s >> 3) ^ (s >> 1) ^ s) & 1;
}
GAT_HD inline int nav_pred(int s_new, int b) { return ((s_new & 31) << 1) | b; }
// the branch metric into s_new from its predecessor b
GAT_HD inline int nav_branch(int s_new, int b, int q0, int q1)
{
    int c1, c2;
    nav_fec_pair(nav_pred(s_new, b), s_new >> 5, &c1, &c2);
    return (1 - 2 * c1) * q0 + (1 - 2 * c2) * q1;
}
// The two predecessors of a state differ in the oldest input, which both polynomials tap: both symbols of the branch flip, and the
// branch metric from b = 1 is the negative of the one from b = 0.  A step needs one of them.
GAT_HD inline int nav_branch0(int s_new, int q0, int q1) { return nav_branch(s_new, 0, q0, q1); }
// add-compare-select: the larger sum survives, a tie keeps b = 0
GAT_HD inline int nav_acs(int m0, int m1, int *dec)
{
    *dec = m1 > m0 ? 1 : 0;
    return m1 > m0 ? m1 : m0;
}
// one step back: the state before, from the survivor word of the step
GAT_HD inline int nav_back(int s, uint64_t word) { return nav_pred(s, (int)((word >> s) & 1u)); }

// ---- a frame's record -----------------------------------------------------------------------------------------------------------------
GAT_HD inline bool nav_hit(int format, const uint8_t *b, int p) { return format == GAT_NAV_CNAV ? nav_cnav_hit(b, p) : nav_lnav_hit(b, p); }
GAT_HD inline void nav_frame(int format, const uint8_t *b, int p, gat_nav_frame &fr)
{
    fr.status = nav_preamble(b, p) ? 1 : 0;
    if (format == GAT_NAV_CNAV) {
        if (nav_crc24q_bits(b, p, GAT_NAV_FRAME_BITS) == 0) fr.status |= 2;
        for (int w = 0; w < 10; ++w) fr.words[w] = nav_field(b, p, 30 * w, 30);
        fr.prn = (int32_t)nav_field(b, p, 8, 6);
        fr.id = (int32_t)nav_field(b, p, 14, 6);
        fr.tow = (int32_t)nav_field(b, p, 20, 17);
        return;
    }
    for (int w = 0; w < 10; ++w) {
        bool ok;
        fr.words[w] = nav_lnav_word(b, p, w, &ok) & 0x3FFFFFFFu;
        if (ok) fr.status |= 2 << w;
    }
    fr.tow = (int32_t)((fr.words[1] >> 13) & 0x1ffffu);
    fr.id = nav_lnav_id(fr.words[1]);
    fr.prn = 0;
}
GAT_HD inline bool nav_frame_good(int format, const gat_nav_frame &fr) { return fr.status == (format == GAT_NAV_CNAV ? kNavCnavGood : kNavLnavGood); }
GAT_HD inline bool nav_tow_step(int format, const gat_nav_frame &a, const gat_nav_frame &b)
{
    return nav_frame_good(format, a) && nav_frame_good(format, b) && b.tow == (a.tow + 1) % kNavTowModulus;
}

// ---- scores and the choice -------------------------------------------------------------------------------------------------------------
// candidate c of a channel = (ph * 300 + o) * 2 + p: the order of the choice's ties
GAT_HD inline int nav_candidates(int format) { return nav_phases(format) * kNavOffsets * 2; }
GAT_HD inline void nav_candidate(int c, int *ph, int *o, int *p) { *p = c & 1, *o = (c >> 1) % kNavOffsets, *ph = (c >> 1) / kNavOffsets; }
// whole frames from offset o inside `search` bits
GAT_HD inline int nav_whole_frames(int search, int o) { return search - o >= GAT_NAV_FRAME_BITS ? (search - o) / GAT_NAV_FRAME_BITS : 0; }
// bits: the decoded bits of the candidate's phase
GAT_HD inline int nav_score(int format, const uint8_t *bits, int search, int o, int p)
{
    const int F = nav_whole_frames(search, o);
    int s = 0;
    for (int f = 0; f < F; ++f) s += nav_hit(format, bits + o + (size_t)f * GAT_NAV_FRAME_BITS, p) ? 1 : 0;
    return s;
}
// The running choice: the largest score, a tie to the lowest candidate; second: the largest score of any other candidate.
struct NavBest {
    int score, cand, second;
};
GAT_HD inline NavBest nav_best_one(int score, int cand) { return NavBest{score, cand, -1}; }
GAT_HD inline NavBest nav_best_merge(const NavBest &a, const NavBest &b)
{
    const bool a_wins = a.score > b.score || (a.score == b.score && a.cand < b.cand);
    const NavBest &w = a_wins ? a : b, &l = a_wins ? b : a;
    return NavBest{w.score, w.cand, w.second > l.score ? w.second : l.score};
}
// the channel record but for tow_steps, from the choice; n: the channel's symbols
GAT_HD inline void nav_record(int format, const NavBest &best, int n, int max_frames, int min_frames, gat_nav_channel &ch)
{
    int ph, o, p;
    nav_candidate(best.cand, &ph, &o, &p);
    const bool sync = best.score >= min_frames;
    if (!sync) ph = 0, p = 0;
    const int bits = nav_bits(format, n, ph);
    const int F = sync ? nav_whole_frames(nav_search_bits(format, bits), o) : 0;
    ch.frame_offset = sync ? o : -1;
    ch.symbol_phase = ph;
    ch.inverted = p;
    ch.score = best.score;
    ch.second_score = best.second < 0 ? 0 : best.second;
    ch.num_frames = F < max_frames ? F : max_frames;
    ch.num_bits = bits;
    ch.tow_steps = 0;
}

} // namespace gat
