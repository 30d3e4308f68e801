// gat_atm_page18.h -- LNAV subframe 4, page 18 (include/gat.h gat_lnav_page18_host, gat_lnav_page18_words_host): the ionospheric and
// UTC fields' layout stated once as a table, read by the decoder and written by the encoder, as gat_fix_eph.h does for subframes
// 1 - 3 (whose bit access this uses).  Cold, integer extraction and scaling: host only, no HIP header.
#pragma once

#include "gat_fix_eph.h"

namespace gat {

constexpr int kPage18Subframe = 4;
constexpr int kPage18SvId = 56;

// A field: `bits` payload bits from `first` (bit 0 = d1 of word 3); a double member scaled by 2^exp2 or an int32 member.
struct Page18Field {
    int first, bits;
    bool is_signed;
    int exp2;
    size_t offset;
    bool integer;
};
#define GAT_P18_D(first, bits, sg, ex, member) {first, bits, sg, ex, offsetof(gat_lnav_page18, member), false}
#define GAT_P18_I(first, bits, sg, member) {first, bits, sg, 0, offsetof(gat_lnav_page18, member), true}
// payload bit of (word w = 3 .. 10, data bit d = 1 .. 24): 24 (w - 3) + d - 1
inline const Page18Field *page18_fields(int *count)
{
    static const Page18Field f[] = {
        GAT_P18_I(0, 2, false, data_id),
        GAT_P18_I(2, 6, false, sv_id),
        GAT_P18_D(8, 8, true, -30, alpha[0]),
        GAT_P18_D(16, 8, true, -27, alpha[1]),
        GAT_P18_D(24, 8, true, -24, alpha[2]),
        GAT_P18_D(32, 8, true, -24, alpha[3]),
        GAT_P18_D(40, 8, true, 11, beta[0]),
        GAT_P18_D(48, 8, true, 14, beta[1]),
        GAT_P18_D(56, 8, true, 16, beta[2]),
        GAT_P18_D(64, 8, true, 16, beta[3]),
        GAT_P18_D(72, 24, true, -50, a1),
        GAT_P18_D(96, 32, true, -30, a0), // words 7 and 8: contiguous in the payload
        GAT_P18_D(128, 8, false, 12, tot),
        GAT_P18_I(136, 8, false, wnt),
        GAT_P18_I(144, 8, true, dt_ls),
        GAT_P18_I(152, 8, false, wnlsf),
        GAT_P18_I(160, 8, false, dn),
        GAT_P18_I(168, 8, true, dt_lsf),
    };
    *count = (int)(sizeof f / sizeof f[0]);
    return f;
}
#undef GAT_P18_D
#undef GAT_P18_I

inline void page18_decode(const gat_nav_frame *frames, int num_frames, gat_lnav_page18 *page)
{
    memset(page, 0, sizeof *page);
    const gat_nav_frame *pick = nullptr;
    for (int i = 0; i < num_frames; ++i)
        if (eph_good(frames[i], kPage18Subframe) && (int)eph_frame_bits(frames[i], 2, 6) == kPage18SvId) pick = frames + i;
    if (!pick) return;
    int count;
    const Page18Field *fields = page18_fields(&count);
    for (int n = 0; n < count; ++n) {
        const Page18Field &f = fields[n];
        const uint64_t raw = eph_frame_bits(*pick, f.first, f.bits);
        const int64_t v = f.is_signed && ((raw >> (f.bits - 1)) & 1u) ? (int64_t)raw - ((int64_t)1 << f.bits) : (int64_t)raw;
        char *member = reinterpret_cast<char *>(page) + f.offset;
        if (f.integer) {
            const int32_t i32 = (int32_t)v;
            memcpy(member, &i32, sizeof i32);
        } else {
            const double d = (double)v * ldexp(1.0, f.exp2);
            memcpy(member, &d, sizeof d);
        }
    }
    page->valid = 1;
}

// the 190 payload bits, one bit a byte
inline void page18_encode(const gat_lnav_page18 *page, uint8_t *bits)
{
    memset(bits, 0, (size_t)kEphPayloadBits);
    int count;
    const Page18Field *fields = page18_fields(&count);
    for (int n = 0; n < count; ++n) {
        const Page18Field &f = fields[n];
        const char *member = reinterpret_cast<const char *>(page) + f.offset;
        int64_t v;
        if (f.integer) {
            int32_t i32;
            memcpy(&i32, member, sizeof i32);
            v = i32;
        } else {
            double d;
            memcpy(&d, member, sizeof d);
            const double q = rint(d / ldexp(1.0, f.exp2));
            v = q == q && fabs(q) < 9.0e18 ? (int64_t)q : 0;
        }
        const uint64_t raw = (uint64_t)v & (((uint64_t)1 << f.bits) - 1);
        for (int i = 0; i < f.bits; ++i) bits[f.first + i] = (uint8_t)((raw >> (f.bits - 1 - i)) & 1u);
    }
}

} // namespace gat
