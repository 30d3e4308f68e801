// gat_code_tables.h -- how a code table lies in device memory (gat_set_codes), as pure functions: the rows' strides, the refusals
// and the two packers.  The kernels depend on this layout; the correlator plan reads the strides (CorrTables, gat_corr_plan.h).
// No HIP call and no HIP header: the C-ABI layer, the host simulator and the stand-alone test programs (tests/chanrules,
// tests/corrplan) compile the same text.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "gat_sig_plan.h" // Refusal

namespace gat {

// Chip rows: 16-byte rows (dc_kernel stages them with 16-byte copies) with room for one more chip: every row carries its FIRST
// chip again at index Lc, so that "this chip and the next" are two reads without a wrap (the replica fill by quads).
constexpr int code_row_stride(int Lc) { return (Lc + 16) & ~15; } // bytes
// Sign-bit rows for the split-bf16 matrix kernel (a chip only flips signs there: 1/8 of the LDS), built only when every chip is
// +-1: bit i of a row = (chip i is -1), bit Lc repeats bit 0 -- see above --, and one whole dword of slack lies behind the last
// chip, so that the two dwords holding "this chip and the next" can always be read together.  A multiple of 4 dwords.
constexpr int code_bits_stride(int Lc) { return (((Lc + 1 + 32 + 31) / 32) + 3) & ~3; } // dwords

// the vector kernel keeps a workgroup's chip table in LDS next to one replica segment (~40 KB): 160 KB - that
constexpr int kMaxCodeLength = 120000;

inline Refusal check_code_table(int32_t code_length, int32_t num_prns)
{
    if (code_length < 1 || num_prns < 1) return {GAT_ERR_ARG, "sizes must be positive"};
    if (code_length > kMaxCodeLength) return {GAT_ERR_RANGE, "code table does not fit in LDS (max 120000 chips)"};
    return {GAT_OK, nullptr};
}

// codes: the caller's table, P rows of Lc chips
inline bool codes_all_pm1(const int8_t *codes, int Lc, int P)
{
    bool pm1 = true;
    for (size_t i = 0; i < (size_t)Lc * P && pm1; ++i) pm1 = codes[i] == 1 || codes[i] == -1;
    return pm1;
}

// rows: P * code_row_stride(Lc) bytes, every one of them written
inline void pack_code_rows(const int8_t *codes, int Lc, int P, int8_t *rows)
{
    const int stride = code_row_stride(Lc);
    for (int p = 0; p < P; ++p) {
        const int8_t *src = codes + (size_t)p * Lc;
        int8_t *row = rows + (size_t)p * stride;
        for (int i = 0; i < Lc; ++i) row[i] = src[i];
        row[Lc] = src[0];
        for (int i = Lc + 1; i < stride; ++i) row[i] = 0;
    }
}

// bits: P * code_bits_stride(Lc) dwords, every one of them written; for a table of +-1 chips (codes_all_pm1)
inline void pack_code_bits(const int8_t *codes, int Lc, int P, uint32_t *bits)
{
    const int stride = code_bits_stride(Lc);
    for (int p = 0; p < P; ++p) {
        const int8_t *src = codes + (size_t)p * Lc;
        uint32_t *row = bits + (size_t)p * stride;
        for (int w = 0; w < stride; ++w) row[w] = 0u;
        for (int i = 0; i < Lc; ++i)
            if (src[i] < 0) row[i >> 5] |= 1u << (i & 31);
        if (src[0] < 0) row[Lc >> 5] |= 1u << (Lc & 31);
    }
}

} // namespace gat
