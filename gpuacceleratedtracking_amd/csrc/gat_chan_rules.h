// gat_chan_rules.h -- which channel record a kernel can evaluate exactly, stated once for both sides.  The kernels poison (NaN) a
// record outside the set with the predicates below; the host entry points with host-resident records refuse the same set with the
// checks below, which are written as the predicates' negation: what passes here is not poisoned there.  No HIP call and no HIP
// header: the kernels (through gat_phase.h), the C-ABI layer, the pure plans and a stand-alone test program (tests/chanrules)
// compile the same text.  Files that include this header must be built with -ffp-contract=off: the span is a multiply followed by
// adds, and host and device must round it alike.
#pragma once

#include <cmath>

#include "gat_hd.h"
#include "gat_sig_plan.h" // Refusal

namespace gat {

// The bounds of the predicates below.  Only the two matrix-core kernels name them besides this header: they restate
// code_span_bad || mfma_wrap_bad term by term (gat_mfma.hip, gat_mfma_bf16.hip), because they compile to other code with the calls.
constexpr double kCodeSpanMax = 1073741824.0; // 2^30: |code phase| that the kernels' int32 / float-reciprocal chip index takes
constexpr double kCodeSpanLaps = 2097152.0;   // 2^21 laps of the table: what floormod_fast's float quotient resolves
constexpr double kMfmaWrapSamples = 32.0;     // the matrix-core kernels: at most one wrap of the table in this many samples

// Parameters floormod_fast / chip_index (gat_phase.h) cannot evaluate exactly: `reach` = the largest |sample + shift| of the call.
// The correlator kernels, the stand-alone replica and the materialising debug kernel all use this ONE predicate (they write
// NaN instead of indexing outside the chip table).
GAT_HD_FORCEINLINE bool code_span_bad(double ratio, double tau, double reach, int Lc)
{
    const double span = __builtin_fabs(tau) + __builtin_fabs(ratio) * reach + 1.0;
    return !(span < kCodeSpanMax) || !(span < kCodeSpanLaps * (double)Lc) || !(ratio >= 0.0);
}

// The carrier part of the same predicate: a carrier step f / fs or a carrier phase of 10^15 cycles or more, NaN or inf.
// Every correlator kernel poisons such a device-resident record with it.  (Below the bound carrier_reduce makes every record exact.)
GAT_HD_FORCEINLINE bool carrier_bad(double step, double phi)
{
    return !(__builtin_fabs(step) < 1.0e15) || !(__builtin_fabs(phi) < 1.0e15);
}

// The matrix-core kernels' own rule (gat_mfma.hip, gat_mfma_bf16.hip): they fill a lane's replica entries from one floored modulo
// and at most one wrap of the table per 32 samples.  The plan (plan_matrix, gat_corr_plan.h) keeps host records that break it
// away from them with this function; the kernels evaluate the same expression in their own text (see the constants above).
GAT_HD_FORCEINLINE bool mfma_wrap_bad(double ratio, int Lc)
{
    return !(ratio * kMfmaWrapSamples < (double)Lc);
}

// ---- the host's refusals: pure functions of values; the caller has checked fs > 0 (a bad fs is refused here too, as a bad record) ----

// The records of a correlator call, host-resident (gat_downconvert_and_correlate, gat_resident_correlate): P rows of Lc chips are
// bound, reach = N + max |shift|.  The first three refusals only name what the two predicates would refuse anyway.
inline Refusal check_channel_records(const gat_channel_params *params_host, size_t n, int32_t P, int Lc, double reach, double fs)
{
    for (size_t i = 0; i < n; ++i) {
        const gat_channel_params &p = params_host[i];
        if (p.prn < 0 || p.prn >= P) return {GAT_ERR_RANGE, "prn outside the code table"};
        if (!std::isfinite(p.code_freq_hz) || !std::isfinite(p.carrier_freq_hz) || !std::isfinite(p.code_phase_chips) ||
            !std::isfinite(p.carrier_phase_cycles))
            return {GAT_ERR_ARG, "non-finite channel parameter"};
        if (p.code_freq_hz < 0.0) return {GAT_ERR_RANGE, "negative code frequency"};
        if (carrier_bad(p.carrier_freq_hz / fs, p.carrier_phase_cycles)) return {GAT_ERR_RANGE, "carrier frequency / phase out of range"};
        if (code_span_bad(p.code_freq_hz / fs, p.code_phase_chips, reach, Lc)) return {GAT_ERR_RANGE, "code phase span too large"};
    }
    return {GAT_OK, nullptr};
}

// What the one-channel replica generators check alike behind their pointers and the bound table; exact_span: the generator
// evaluates the chip index exactly (gat_gen_code_replica), so the span bound holds for it as for code_replica_multi_kernel.
inline Refusal check_replica_call(int64_t count, int32_t prn, int32_t P, int Lc, double fc, double fs, double tau, int64_t first_shift,
                                  bool exact_span)
{
    if (count < 1) return {GAT_ERR_ARG, "count must be positive"};
    if (prn < 0 || prn >= P) return {GAT_ERR_RANGE, "prn outside the code table"};
    if (!(fs > 0.0) || !std::isfinite(fc) || !std::isfinite(tau)) return {GAT_ERR_ARG, "bad frequency / phase"};
    const long long shift = first_shift < 0 ? -(long long)first_shift : (long long)first_shift;
    if (count + shift >= (1ll << 30)) return {GAT_ERR_RANGE, "replica too long"};
    if (exact_span && code_span_bad(fc / fs, tau, (double)count + (double)shift, Lc)) return {GAT_ERR_RANGE, "code phase span too large"};
    return {GAT_OK, nullptr};
}

// The one record of gat_downconvert_and_accumulate over N samples and taps of at most max_shift (accumulate_debug_kernel).
inline Refusal check_accumulate_record(const gat_channel_params &p, int32_t P, int Lc, long long N, long long max_shift, double fs)
{
    if (p.prn < 0 || p.prn >= P) return {GAT_ERR_RANGE, "prn outside the code table"};
    if (!(fs > 0.0) || !std::isfinite(p.code_freq_hz) || !(p.code_freq_hz >= 0.0) || !std::isfinite(p.carrier_freq_hz) ||
        !std::isfinite(p.code_phase_chips) || !std::isfinite(p.carrier_phase_cycles))
        return {GAT_ERR_ARG, "bad frequency / phase"};
    if (N + max_shift >= (1ll << 30)) return {GAT_ERR_RANGE, "num_samples + |shift| must stay below 2^30"};
    if (code_span_bad(p.code_freq_hz / fs, p.code_phase_chips, (double)(N + max_shift), Lc)) return {GAT_ERR_RANGE, "code phase span too large"};
    return {GAT_OK, nullptr};
}

} // namespace gat
