// gat_fix_eph.h -- the LNAV ephemeris of subframes 1 - 3 (include/gat.h gat_lnav_ephemeris_host, gat_lnav_ephemeris_words_host): the
// field layout stated once as a table, read by the decoder and written by the encoder.  Cold, integer extraction and scaling: host
// only, no HIP header; the entry points and a stand-alone test program (tests/fixplan) compile the same text.
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "gat.h"

namespace gat {

constexpr double kEphPi = 3.1415926535898; // semicircles to radians, as the interface specification has it
constexpr int kEphPayloadBits = 190;       // d1 .. d24 of words 3 .. 9 and d1 .. d22 of word 10
constexpr int kEphLnavGood = 0x7ff;

// A field: `bits` payload bits from `first` (bit 0 = d1 of word 3), continued by `bits2` bits from `first2` where it is split.
struct EphField {
    int sf, first, bits, first2, bits2;
    bool is_signed;
    int exp2;       // the scale is 2^exp2
    bool semi;      // semicircles: times kEphPi
    size_t offset;  // of the member of gat_ephemeris
    bool integer;   // an int32 member
};
#define GAT_EPH_D(sf, first, bits, f2, b2, sg, ex, semi, member) {sf, first, bits, f2, b2, sg, ex, semi, offsetof(gat_ephemeris, member), false}
#define GAT_EPH_I(sf, first, bits, f2, b2, member) {sf, first, bits, f2, b2, false, 0, false, offsetof(gat_ephemeris, member), true}
// payload bit of (word w = 3 .. 10, data bit d = 1 .. 24): 24 (w - 3) + d - 1
inline const EphField *eph_fields(int *count)
{
    static const EphField f[] = {
        GAT_EPH_I(1, 0, 10, 0, 0, wn),
        GAT_EPH_I(1, 12, 4, 0, 0, ura),
        GAT_EPH_I(1, 16, 6, 0, 0, health),
        GAT_EPH_I(1, 22, 2, 120, 8, iodc),
        GAT_EPH_D(1, 112, 8, 0, 0, true, -31, false, tgd),
        GAT_EPH_D(1, 128, 16, 0, 0, false, 4, false, toc),
        GAT_EPH_D(1, 144, 8, 0, 0, true, -55, false, af2),
        GAT_EPH_D(1, 152, 16, 0, 0, true, -43, false, af1),
        GAT_EPH_D(1, 168, 22, 0, 0, true, -31, false, af0),
        GAT_EPH_I(2, 0, 8, 0, 0, iode),
        GAT_EPH_D(2, 8, 16, 0, 0, true, -5, false, crs),
        GAT_EPH_D(2, 24, 16, 0, 0, true, -43, true, delta_n),
        GAT_EPH_D(2, 40, 32, 0, 0, true, -31, true, m0),
        GAT_EPH_D(2, 72, 16, 0, 0, true, -29, false, cuc),
        GAT_EPH_D(2, 88, 32, 0, 0, false, -33, false, e),
        GAT_EPH_D(2, 120, 16, 0, 0, true, -29, false, cus),
        GAT_EPH_D(2, 136, 32, 0, 0, false, -19, false, sqrt_a),
        GAT_EPH_D(2, 168, 16, 0, 0, false, 4, false, toe),
        GAT_EPH_I(2, 184, 1, 0, 0, fit),
        GAT_EPH_D(3, 0, 16, 0, 0, true, -29, false, cic),
        GAT_EPH_D(3, 16, 32, 0, 0, true, -31, true, omega0),
        GAT_EPH_D(3, 48, 16, 0, 0, true, -29, false, cis),
        GAT_EPH_D(3, 64, 32, 0, 0, true, -31, true, i0),
        GAT_EPH_D(3, 96, 16, 0, 0, true, -5, false, crc),
        GAT_EPH_D(3, 112, 32, 0, 0, true, -31, true, omega),
        GAT_EPH_D(3, 144, 24, 0, 0, true, -43, true, omega_dot),
        GAT_EPH_D(3, 176, 14, 0, 0, true, -43, true, idot),
    };
    *count = (int)(sizeof f / sizeof f[0]);
    return f;
}
#undef GAT_EPH_D
#undef GAT_EPH_I
constexpr int kEphIode3First = 168; // subframe 3's own IODE, word 10 d1 .. d8

inline double eph_scale(const EphField &f) { return ldexp(1.0, f.exp2) * (f.semi ? kEphPi : 1.0); }

// payload bit i of a frame record: words[2 + i / 24] holds d1 .. d24 in bits 29 .. 6
inline int eph_frame_bit(const gat_nav_frame &fr, int i) { return (int)((fr.words[2 + i / 24] >> (29 - i % 24)) & 1u); }
inline uint64_t eph_frame_bits(const gat_nav_frame &fr, int first, int bits)
{
    uint64_t v = 0;
    for (int i = 0; i < bits; ++i) v = (v << 1) | (uint64_t)eph_frame_bit(fr, first + i);
    return v;
}
inline uint64_t eph_field_raw(const gat_nav_frame &fr, const EphField &f)
{
    return (eph_frame_bits(fr, f.first, f.bits) << f.bits2) | eph_frame_bits(fr, f.first2, f.bits2);
}
inline bool eph_good(const gat_nav_frame &fr, int sf) { return fr.status == kEphLnavGood && fr.id == sf; }

inline void eph_decode(const gat_nav_frame *frames, int num_frames, gat_ephemeris *eph)
{
    memset(eph, 0, sizeof *eph);
    int count;
    const EphField *fields = eph_fields(&count);
    int newest[4] = {-1, -1, -1, -1};
    for (int i = 0; i < num_frames; ++i)
        for (int sf = 1; sf <= 3; ++sf)
            if (eph_good(frames[i], sf)) newest[sf] = i;
    if (newest[1] < 0 || newest[2] < 0 || newest[3] < 0) {
        eph->reason = GAT_EPH_MISSING;
        return;
    }
    // the newest complete set: subframe 1 from the newest back, each with the newest subframes 2 and 3 of its issue
    const gat_nav_frame *pick[4] = {nullptr, nullptr, nullptr, nullptr};
    for (int one = newest[1]; one >= 0 && !pick[1]; --one) {
        if (!eph_good(frames[one], 1)) continue;
        const int iode = (int)eph_frame_bits(frames[one], 120, 8); // the low 8 bits of IODC
        const gat_nav_frame *two = nullptr, *three = nullptr;
        for (int i = 0; i < num_frames; ++i) {
            if (eph_good(frames[i], 2) && (int)eph_frame_bits(frames[i], 0, 8) == iode) two = frames + i;
            if (eph_good(frames[i], 3) && (int)eph_frame_bits(frames[i], kEphIode3First, 8) == iode) three = frames + i;
        }
        if (two && three) pick[1] = frames + one, pick[2] = two, pick[3] = three;
    }
    if (!pick[1]) {
        eph->reason = GAT_EPH_IODE;
        return;
    }
    for (int n = 0; n < count; ++n) {
        const EphField &f = fields[n];
        const int width = f.bits + f.bits2;
        const uint64_t raw = eph_field_raw(*pick[f.sf], f);
        char *member = reinterpret_cast<char *>(eph) + f.offset;
        if (f.integer) {
            const int32_t v = (int32_t)raw;
            memcpy(member, &v, sizeof v);
            continue;
        }
        const int64_t v = f.is_signed && ((raw >> (width - 1)) & 1u) ? (int64_t)raw - ((int64_t)1 << width) : (int64_t)raw;
        const double d = (double)v * eph_scale(f);
        memcpy(member, &d, sizeof d);
    }
    eph->valid = 1;
    eph->reason = GAT_EPH_OK;
}

// the 190 payload bits of subframes 1, 2, 3, one bit a byte: bits[(sf - 1) * 190 + i]
inline void eph_encode(const gat_ephemeris *eph, uint8_t *bits)
{
    memset(bits, 0, 3 * (size_t)kEphPayloadBits);
    int count;
    const EphField *fields = eph_fields(&count);
    auto put = [&](int sf, int first, int n, uint64_t v) {
        for (int i = 0; i < n; ++i) bits[(size_t)(sf - 1) * kEphPayloadBits + first + i] = (uint8_t)((v >> (n - 1 - i)) & 1u);
    };
    for (int n = 0; n < count; ++n) {
        const EphField &f = fields[n];
        const int width = f.bits + f.bits2;
        const char *member = reinterpret_cast<const char *>(eph) + f.offset;
        int64_t v;
        if (f.integer) {
            int32_t i32;
            memcpy(&i32, member, sizeof i32);
            v = i32;
        } else {
            double d;
            memcpy(&d, member, sizeof d);
            const double q = rint(d / eph_scale(f));
            v = q == q && fabs(q) < 9.0e18 ? (int64_t)q : 0;
        }
        const uint64_t raw = (uint64_t)v & (width < 64 ? (((uint64_t)1 << width) - 1) : ~(uint64_t)0);
        put(f.sf, f.first, f.bits, raw >> f.bits2);
        put(f.sf, f.first2, f.bits2, raw & (((uint64_t)1 << f.bits2) - 1));
    }
    put(3, kEphIode3First, 8, (uint64_t)eph->iode & 0xffu);
}

} // namespace gat
