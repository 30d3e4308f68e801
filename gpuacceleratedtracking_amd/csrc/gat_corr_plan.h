// gat_corr_plan.h -- the correlator call's launch plan as a value, and what host and kernels share about a launch.  No HIP
// call and no HIP header: the C-ABI layer (gat_planner.cpp enqueues what is planned here), the kernels (through gat_internal.h)
// and the stand-alone program tests/corrplan compile the same text.  First the constants, argument structs and constexpr geometry
// of the vector kernel (gat_dc.h), the resident correlator (gat_resident.h) and the matrix-core kernels (gat_mfma*.hip); then the
// plan's inputs (CorrKnobs, CorrTables, CorrCall) and output (CorrPlan); then the plan: corr_check_call, and corr_plan =
// corr_sort_taps, corr_pick_loads, plan_matrix or else plan_vector (size_tap_group per tap group); corr_plan_resident.
//
// Launch planning for the fused correlator (DESIGN.md "Kernels"):
//   ant_tile MT = largest of {4,3,2,1} dividing M          (register accumulators 2*MT*L <= 64)
//   vec      = 4 when every plane base/stride is 16-byte aligned, else 1
//   aw, kt   = antenna tiles (waves) and channels per workgroup: 16 antennas share one replica, up to 4 channels loop
//              over register-resident samples
//   nw       = waves per workgroup: 4, or 1 for short blocks of 1-2 antenna tiles in a long stream
//   splits   = workgroups per (block, channel, antenna tile): 1 once B*K*M/MT already fills the
//              chip (>= 8 workgroups per CU), otherwise the block's samples are split and a
//              finalize launch sums the per-split partials in fixed order.
//   matrix-core kernels where they measured faster (auto rule below).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "gat.h"
#include "gat_chan_rules.h" // mfma_wrap_bad: the matrix kernels' wrap rule, as they evaluate it
#include "gat_sig_plan.h" // the layout arithmetic (layout_sample_bytes, layout_vec_samples), blocks_aligned, Refusal

namespace gat {

constexpr int kThreads = 256;       // 4 wave64 per workgroup
constexpr int kMaxTapsPerLaunch = 8; // taps handled by one launch (register accumulators)
constexpr int kInlineParams = 4;     // channel parameter records of a host call that travel inside the kernel arguments
constexpr int kMaxAntTile = 4;       // antennas handled by one workgroup
constexpr int kFinalizeFewSplits = 32; // second stage: up to this many splits are summed by one thread per output element
constexpr int kMaxReplicaSpan = 512;  // tap span the LDS replica segment of a launch is sized for by default
constexpr int kMaxLaunchSpan = 2048;  // largest tap span one launch serves (the replica's LDS grows with the span beyond
                                      // kMaxReplicaSpan; wider tap lists are cut into several launches)

// Sample ownership of one lane per step in dc_kernel: G groups of S consecutive samples, one
// 16-byte load per plane and group (vec == 4: S = layout_vec_samples) or scalar loads (vec == 1: S = 1).
constexpr int dc_group_samples(int vec, int fmt) { return vec != 4 ? 1 : layout_vec_samples(fmt); }
constexpr int dc_groups(int vec, int fmt)
{
    return vec == 4 && fmt == GAT_LAYOUT_INTERLEAVED ? 2 : 1;
}
// samples one workgroup covers per step: the nw / aw waves that share an antenna tile, 64 lanes each (nw = 4 waves per
// workgroup, or 1: one-wave workgroups for short blocks, see gat_dc.h)
constexpr int dc_chunk(int vec, int fmt, int aw = 1, int nw = 4) { return (64 * nw / aw) * dc_group_samples(vec, fmt) * dc_groups(vec, fmt); }

// Arguments of the fused correlator kernel (passed by value in the kernarg segment).
struct DcArgs {
    const void *re;                   // planar: float re plane; interleaved formats: base pointer
    const void *im;                   // planar: float im plane; otherwise unused
    const gat_channel_params *params; // dev, [B*K], channel fastest; null: the records are in `inl` (B*K <= kInlineParams)
    const int8_t *codes;              // dev, [P][code_row_stride] (rows padded to 16 bytes)
    const uint32_t *code_bits;        // dev, [P][table_stride / 4]: sign bits of +-1 chips (bit i & 31 of dword i >> 5), or null:
                                      // the workgroups stage the int8 rows.  Long codes (GPS L5: 10 KB per PRN as int8) are staged as
                                      // bits -- 1.3 KB -- so that the LDS holds long replica segments and two channels' tables
    float *out_re;                    // dev, [B][K][Ltot][M]
    float *out_im;
    float *partial;                   // dev, [B*K][splits][Ltot*M*2] (splits > 1 only)
    unsigned *done_counter;           // dev, arrival counter of the launch's workgroups, or null: no completion flag
    unsigned *host_flag;              // pinned host memory (device address): the last workgroup stores flag_seq there
    unsigned flag_seq, total_wgs;     // total_wgs: workgroups that do work (num_tiles * KG)
    long long N, ant_stride, block_stride, chan_stride;
    double fs;
    int M, K, B, Lc, num_prns, code_row_stride;
    int table_stride;      // bytes of ONE channel's chip table in LDS and between rows of what is staged: code_row_stride (int8
                           // chips) or 4 * dwords per sign-bit row (code_bits != null); a multiple of 16
    int KG;                // channel groups: ceil(K / KT)
    int splits, chunks_per_split, total_chunks;
    int ant_groups;        // M / (MT * AW): antenna groups, one workgroup each
    int blocks_per_wg;     // consecutive integration blocks one workgroup loops over (splits == 1 only)
    int num_tiles;         // ceil(B / blocks_per_wg) * ant_groups * splits
    int Ltot;              // taps of the whole call (output indexing)
    int max_abs_shift;     // max |shift| over ALL taps of the call (range check)
    int rep_span;          // shifts[last] - shifts[0] of THIS launch's taps (replica halo)
    int seg_steps;         // steps per segment (replica produced at once), <= dc_segment_steps()
    int rep_copy_stride;   // floats between the replica and its copy shifted by one entry (taps at odd offsets), 0: one copy
    int rep_chan_floats;   // floats of LDS per channel replica (one-wave workgroups: sized for this launch's taps; four-wave
                           // ones: for the segment the host chose, <= dc_rep_chan_floats())
    int keep_l2;           // 1: plain loads (several channel groups share the tile through L2), 0: non-temporal
    int n_vec;             // samples of a block the vector path covers: N - N % (samples per 16-byte load); N for scalar loads
    int align_head;        // 1: workgroups walk a block from the 128-byte line its first sample lies in (gat_dc.h)
    int fill_quads;        // 1: replica producers write four consecutive entries at a time where the code rate allows (gat_dc_body.inc)
    unsigned flags;
    int shifts[kMaxTapsPerLaunch];    // ascending
    int tap_off[kMaxTapsPerLaunch];   // float offset of tap l's chips from the lane's group base: even (8-byte aligned reads)
    int tap_index[kMaxTapsPerLaunch]; // position of each tap in the caller's list
    // host-parameter calls of up to kInlineParams records (the single-block call of a receiver loop, the reference's
    // kernel_algorithm with scalar arguments): no 40-byte upload in front of the launch (3.3 us of a 15 us call)
    gat_channel_params inl[kInlineParams];
};

// Arguments of dc_tail_kernel (gat_kernels.hip): the N % S samples at the end of every block that the vector path of
// dc_kernel leaves out when the block length is no multiple of the samples S one 16-byte load holds.
struct DcTailArgs {
    const void *re, *im;
    const gat_channel_params *params; // dev [B*K], or null: the records are in `inl`
    const int8_t *codes;
    float *out_re, *out_im;           // [B][K][L][M]: the tail's sums are ADDED to what dc_kernel (+ second stage) wrote
    unsigned *done_counter, *host_flag;
    unsigned flag_seq;
    long long N, ant_stride, block_stride, chan_stride;
    double fs;
    int M, K, B, L, Lc, num_prns, code_row_stride, format, n_vec, max_abs_shift;
    int shifts[GAT_MAX_TAPS];         // in the caller's order
    gat_channel_params inl[kInlineParams];
};

struct DcLaunch {
    int ant_tile; // MT: antennas per wave
    int aw;       // antenna tiles (waves) per workgroup: 1, 2, 4
    int kt;       // channels per workgroup: 1, 2, 4
    int nw;       // waves per workgroup: 4, or 1 (short blocks: one wave per block, no workgroup barrier to wait at)
    int depth;    // register sets of samples per wave (steps in flight): 1, or 2 (dc_depth_max)
    int taps;     // L of this launch
    int vec;      // 4 or 1
    int format;   // GAT_LAYOUT_*
    unsigned grid;
    unsigned lds_bytes;
};
// ---- resident correlator (gat_resident.h): calls without a launch ----------------------------------------------------
// One bounded-lifetime kernel stays on the device and serves single-block calls that the host rings in through a
// doorbell in pinned host memory; every workgroup posts its sums to pinned host memory as result lines.
// Doorbell: one 64-byte line per channel (K <= kResMaxChannels lines, written by the host in descending order, line 0 last):
//   dword 0 seq | 1 reserved | 2..11 gat_channel_params | 12..13 block offset in samples (int64) | 14 check | 15 seq
// check = XOR of dwords 0..13: a poll that catches a line half-written fails the check and is repeated.
// Result lines: workgroup `slot` (tile * KG + channel group, the body's decode of blockIdx) owns ceil(2 MT L / 14) lines of
//   14 values | check = XOR of the 14 values and seq | seq
// its value o is the sum for (tap l, antenna m of its tile, re / im) = (o / 2 / MT, o / 2 % MT, o % 2).  Written with plain
// stores and no fence: the host takes a call's results when every line carries the call's number and passes its check.
constexpr int kBellDwords = 16;
constexpr int kResMaxChannels = 16;    // channels (doorbell lines) of a resident correlator: four 256-byte loads of one wave
constexpr unsigned kBellQuit = 0xffffffffu; // never a call's sequence number
constexpr int kResLinePayload = 14;
struct ResidentArgs {
    const unsigned *host_bell; // the doorbell the HOST writes: [bell_copies][kResMaxChannels][16] -- device memory that the host reaches
                               // through the PCIe BAR (bell_copies = 8: one per blockIdx % 8), or pinned host memory (1 copy)
    int bell_copies;
    unsigned *host_lines;      // pinned host: [workgroups][lines per workgroup][16]
    unsigned *host_state;      // pinned host: [0] why the kernel ended (0: it runs), [1] calls the master served
    unsigned *dev_quit;        // device: set by the master when it leaves (every workgroup polls the host: forward == 0)
    unsigned *dev_bell;        // device: [8][K lines] copies of the doorbell written by the master (forward != 0)
    int forward;               // 1: only the master polls the host and forwards; 0: every workgroup polls the host
    unsigned start_seq;        // sequence number of the last call served before this launch
    unsigned max_calls;        // the kernel ends after this many calls ...
    long long idle_ticks;      // ... or this long without one (100 MHz wall clock) ...
    long long life_ticks;      // ... or this long after its start, whatever happens
};
enum ResidentExit : unsigned { kResidentRuns = 0, kResidentQuit = 1, kResidentIdle = 2, kResidentLife = 3, kResidentCalls = 4 };

// carrier table of one segment: [steps <= kUcarSteps][samples of a lane's groups, G * S <= 8][re, im] floats per channel
constexpr int kUcarSteps = 8;
constexpr int kUcarFloats = kUcarSteps * 8 * 2;
// Most steps whose code replica one workgroup produces at once (a "segment").  One channel per workgroup: ~8192 entries
// (39 KB of LDS) when a wave carries 3-4 antennas -- those instances are limited to 3 workgroups per CU by registers
// anyway, and longer segments mean fewer barriers (configs[1]: 0.846 vs 0.822 of HBM) --, ~4096 entries (25 KB) for 1-2
// antennas per wave, where LDS is what limits the workgroups per CU; ~8192 entries over the channels of a channel-
// looping workgroup.  The host may ask for fewer (short blocks).
constexpr int dc_segment_steps(int chunk, int kt, int mt)
{
    const int s = (kt == 1 ? (mt >= 3 ? 8192 : 4096) : 8192 / kt) / chunk;
    return s < 2 ? 2 : (s > kUcarSteps ? kUcarSteps : s);
}
// Floats of LDS per channel for one segment's replica: entry i <-> sample (segment start) + shifts[0] + i, linear, so
// that the chips of a lane's S consecutive samples are ONE 8-byte-aligned vector read per tap (ds_read2_b64).  Taps at
// an odd distance from the first read a second copy shifted by one entry (rep_copy_stride floats further); the host
// then halves the segment so that both fit here.  Room: segment samples + kMaxReplicaSpan taps + one entry per
// producer thread of overshoot; at least one step with two copies.
constexpr int dc_rep_copy_floats(int steps, int chunk, int span, int threads = kThreads) { return (steps * chunk + span + threads + 2 + 1) & ~1; }
constexpr int dc_rep_chan_floats_steps(int steps, int chunk, int span = kMaxReplicaSpan)
{
    const int one = dc_rep_copy_floats(steps, chunk, span);
    const int two = 2 * dc_rep_copy_floats(1, chunk, span);
    return ((one > two ? one : two) + 7) & ~7;
}
constexpr int dc_rep_chan_floats(int chunk, int kt, int mt) { return dc_rep_chan_floats_steps(dc_segment_steps(chunk, kt, mt), chunk); }
// dynamic LDS of one four-wave dc_kernel workgroup: per-channel constants, reduction scratch, carrier table, one segment's
// replica (chan_floats per channel: the host may size it for fewer steps than dc_segment_steps), chip tables
constexpr size_t dc_lds_bytes_floats(int kt, int code_row_stride, int chan_floats)
{
    return (size_t)kt * 32 + (size_t)kt * 4 * 64 * sizeof(float) + (size_t)kt * kUcarFloats * sizeof(float) +
           (size_t)kt * chan_floats * sizeof(float) + (size_t)kt * code_row_stride;
}
constexpr size_t dc_lds_bytes(int kt, int mt, int code_row_stride, int chunk)
{
    return dc_lds_bytes_floats(kt, code_row_stride, dc_rep_chan_floats(chunk, kt, mt));
}
// Samples of a group handled at once in the one-channel step (chips, phasors and wipe-off products of SB samples live
// together): the whole group, half of the eight-sample groups of int8 pairs (a fourth wave per SIMD, round 3), and two of
// four for the tiles with 25-40 accumulator registers (four antennas x five taps: 145 -> 128 registers, round 4).
constexpr int dc_sub_batch(int s, int mt, int l, int kt, int aw = 1)
{
    if (aw == 2 && mt == 2 && kt == 2 && s == 4) return 2; // the two-channel 2 x 2 tile: two-sample passes (chips of both channels live)
    return s > 4 ? 4 : (s == 4 && kt == 1 && 2 * mt * l > 24 && 2 * mt * l <= 40 ? 2 : s);
}
// Occupancy hints (__launch_bounds__ of dc_kernel; the host sizes the LDS segment for the same number of workgroups per
// CU).  scripts/kernel_resources.sh prints what every instance needs; a bound tighter than that spills into the step loop
// (1.2-3x slower, rounds 1-2).  Round 4 took the per-lane phasor state and three hoisted fill addresses out of every
// instance: see the rule below; the channel-looping instances with more than 40 accumulator registers -> two waves
// (<= 256 registers, no AGPR copies), without spills for float and int16 samples.  The int8 forms (eight samples per
// group) keep round 3's bounds: 13-92 registers over 256 in their channel-looping instances (AGPR copies, one wave per
// SIMD; by default such shapes run on the split-bf16 matrix kernel).
constexpr int dc_min_waves(int mt, int l, int kt, int d, int fmt, int aw = 1)
{
    // the two-channel 2 x 2 tile: four waves per SIMD up to five taps (127 registers at five; three waves measured no faster than
    // the one-channel tile, profiles/r05/ab_kt2.txt), three beyond
    // (ComplexF32 pairs: two two-sample groups per lane and step cost ~20 registers more -- four waves up to three taps)
    if (mt == 2 && aw == 2)
        return fmt == GAT_LAYOUT_INTERLEAVED_I8 ? 2 : fmt == GAT_LAYOUT_INTERLEAVED ? (l <= 3 ? 4 : l <= 6 ? 3 : 2) : (l <= 5 ? 4 : 3);
    const int accs = 2 * mt * l * kt;
    const bool i8 = fmt == GAT_LAYOUT_INTERLEAVED_I8;
    if (accs > 40) return i8 ? 1 : (accs <= 48 && kt == 2 ? 3 : 2); // (four antennas x three taps x two channels: 167 registers)
    if (d != 1 || i8 || kt != 1) return 3;
    // one channel, one sample set: four waves where the step fits 128 registers -- up to 24 accumulator registers in every
    // format, up to 40 where the step runs in two-sample passes (dc_sub_batch: four-sample groups, i.e. planar float and
    // int16 samples; the four-antenna five-tap planar instance spills two registers outside its step loop for it)
    const int s = dc_group_samples(4, fmt);
    return accs <= 24 || dc_sub_batch(s, mt, l, kt) < s ? 4 : 3;
}
// one-wave workgroups: steps per segment and LDS bytes (replica sized for the launch's own tap span)
constexpr int kOneWaveSegSteps = 4;
// Deepest sample prefetch an instance family is built with.  Two register sets (steps c+1 and c+2 in flight) exist for
// the four-antenna, <= 3-tap, one-channel tile only -- the configs[1] family, streaming every byte once at the HBM rate:
// measured + 1.3 % there on fast and slow boxes alike; every other family measured no gain or a loss.
constexpr int dc_depth_max(int mt, int l, int aw, int kt, int nw)
{
    // (round 4: and the one-antenna one-wave tile of short blocks in a long stream -- 6-7 waves per SIMD with ONE step of 2 KB
    // in flight each are 13.5 KB per SIMD, 0.78 of the HBM rate by Little's law at 2.2 us: what that shape measured, 0.74)
    return (nw == 4 && aw == 1 && kt == 1 && mt == 4 && l <= 3) || (nw == 1 && aw == 1 && kt == 1 && mt == 1 && l <= 3) ? 2 : 1;
}
constexpr size_t dc_lds_bytes_one_wave(int rep_chan_floats, int code_row_stride)
{
    return 32 + 64 * sizeof(float) + kUcarFloats * sizeof(float) + (size_t)rep_chan_floats * sizeof(float) + (size_t)code_row_stride;
}

// Which instances carry the replica fill by quads / from sign-bit chip tables (the host asks for them nowhere else: every
// form costs an instance scalar registers whether it runs or not)
constexpr bool dc_fill_quads(int aw, int kt, int nw) { return nw == 4 && aw == 2 && kt == 2; }
constexpr bool dc_bit_tables(int nw) { return nw == 4; }

// Which instances exist.  Register accumulators 2 * MT * L * KT <= 64; antenna-parallel waves (AW > 1) need full
// 4-antenna tiles; unaligned input (VEC == 1, scalar loads) is served one antenna per workgroup.
constexpr bool dc_instance(int mt, int l, int vec, int aw, int kt, int nw = 4, int depth = 1)
{
    if (depth != 1 && !(vec == 4 && depth == dc_depth_max(mt, l, aw, kt, nw))) return false;
    // one-wave workgroups: short blocks of one- and two-antenna tiles
    if (nw != 4 && !(nw == 1 && vec == 4 && aw == 1 && kt == 1 && mt <= 2)) return false;
#ifdef GAT_DC_DEV // development builds: only the instances the BASELINE shapes use (compiles in seconds)
    if (!((mt == 1 || mt == 4 || mt == 2) && (l == 3 || l == 5) && vec == 4)) return false;
#endif
    if (mt < 1 || mt > kMaxAntTile || l < 1 || l > kMaxTapsPerLaunch) return false;
    if (vec != 4) return vec == 1 && mt == 1 && aw == 1 && kt == 1;
    // the two-channel 2 x 2 tile: two waves of two antennas each on the same samples, two sample sub-chunks, two channels per
    // workgroup (the one-channel form of it measured 4-12 % slower than one wave of four antennas at 4, 5 and 6 waves per SIMD:
    // profiles/r05/ab_aw2.txt -- it does not exist)
    if (mt == 2 && aw == 2) return kt == 2 && nw == 4 && depth == 1;
    if (aw != 1 && (mt != 4 || aw != 4)) return false;
    // several channels per workgroup only with antenna-parallel waves: measured on MI355X, a channel loop over one
    // antenna tile never beat separate channel workgroups sharing the tile through L2 (M = 1, 4; K = 8, 12)
    if (kt != 1 && aw != 4) return false;
    return (kt == 1 || kt == 2 || kt == 4) && mt * l * kt <= 48;
}
constexpr bool dc_resident_instance(int mt, int l) { return dc_instance(mt, l, 4, 1, 1, 4, 1); }

// Arguments of the matrix-core kernel (gat_mfma.hip): 16-antenna tiles, planar f32 input.
constexpr int kMfmaMaxTaps = 16;     // 2 * CT * L <= 32 columns with CT >= 1
constexpr int kMfmaMaxSpan = 768;    // replica halo served per 256-sample step
struct MfArgs {
    const void *re; // planar f32: re plane; interleaved formats (split-bf16 kernel only): base pointer
    const void *im; // planar f32: im plane; otherwise null
    const gat_channel_params *params;
    const int8_t *codes;
    const uint32_t *code_bits; // split-bf16 kernel: sign-bit tables [P][code_bits_stride]
    const void *zeros;         // split-bf16 kernel: 16 zero bytes (target of out-of-range sample loads)
    float *out_re;
    float *out_im;
    float *partial;
    long long N, ant_stride, block_stride;
    double fs;
    int M, K, B, L, Lc, num_prns, code_row_stride;
    int CT;              // f32 kernel: channels per 32-column tile = 16 / L
    int nslots;          // split-bf16 kernel: channel slots per workgroup (columns packed flat)
    int chan_groups;     // ceil(ceil(K / CT) / NCT)
    int ant_tiles;       // M / 16 (f32 kernel) or M / (16 * rt) (split-bf16 kernel)
    int splits, steps_per_split, total_steps, num_tiles;
    int max_abs_shift, rep_span, rep_stride;
    int code_bits_stride; // dwords per sign-bit row (multiple of 4)
    int codes_in_lds;    // 1: the workgroup's chip tables are staged in LDS (they fit)
    int rep_ring;        // split-bf16 kernel: entries of a channel slot's chip-sign ring (a multiple of the tile, >= rep_span + 2 tiles; rep_stride >= rep_ring + rep_span + tile)
    int mb_mode;         // split-bf16 kernel: MbMode of this launch (the host's choice: mb_mode(), or kMbThree on request for int16)
    unsigned flags;
    int shifts[kMfmaMaxTaps];    // ascending
    int tap_index[kMfmaMaxTaps]; // position in the caller's list
};
// Geometry of the matrix-core kernels that the host's planner and the kernels share (gat_mfma.hip, gat_mfma_bf16.hip).
// split-bf16 kernel: workgroup size -- 4 consumer waves + 12 producer waves (4 per SIMD, 128 VGPRs) where the instance fits
// that register budget, otherwise + 8 producer waves (3 per SIMD, 168 VGPRs)
constexpr int mb_threads(int RT, int NCT) { return ((RT == 2 && NCT == 1) || (RT == 4 && NCT == 2)) ? 768 : 1024; }
// consumer waves: one per SIMD
constexpr int mb_consumer_waves(int, int) { return 4; }
constexpr int mb_producer_threads(int RT, int NCT) { return mb_threads(RT, NCT) - 64 * mb_consumer_waves(RT, NCT); }
constexpr int kMbMaxChain = 8192;  // samples per accumulation chain (f32 rounding of the running sum)
constexpr int kMbMaxSlots = 24;    // channel slots per workgroup (header size)
constexpr int kMbHeader = 1536;    // ChanInfoB[<= 20] (64 B each) + slack, 16-byte aligned
constexpr int mb_tile_samples(int RT, int NCT)
{
    const int t = 32 * (4 / NCT), cap = 128 / RT;
    return t < cap ? t : cap;
}
constexpr int mb_slots(int nct, int L, int K)
{ // upper bound of the channels a workgroup's 32 * nct flat columns touch
    const int s = (32 * nct + 2 * L - 1) / (2 * L) + 1;
    return s < K ? s : K;
}
// How the split-bf16 kernel lays the cross products along the MFMA's 16 reduction slots (per 32-lane half: 8 slots):
//   kMbThree  float / int16 samples: x = hi + mid + lo, w = hi + mid + lo, 8 products per sample  -> 1 sample per half and MFMA
//   kMbOne    int8 samples: exact in ONE bf16 term, 3 products + a zero slot per sample          -> 2 samples per half and MFMA
//   kMbTwo    int16 samples, round 5: exact in TWO bf16 terms (a = x rounded to 8 significant bits, b = x - a: at most 7 bits,
//             |b| <= 2^-8 |a|), 5 products per sample {a h, a m, a l, b h, b m} (b * lo(w) is 2^-24 of the product: below f32), laid as a
//             STREAM of slots across consecutive MFMAs: 8 samples per half every 5 MFMAs -- 1.6 samples per half and MFMA.
//             Needs the half's sample count per step (T / consumer waves per tile / 2) to be a multiple of 8.
enum MbMode : int { kMbThree = 0, kMbOne = 1, kMbTwo = 2 };
constexpr int mb_mode(int rt, int nct, int fmt, bool force_three = false)
{
    if (fmt == GAT_LAYOUT_INTERLEAVED_I8) return kMbOne;
    const int wpt = mb_consumer_waves(rt, nct) / nct, hs = mb_tile_samples(rt, nct) / (wpt > 0 ? wpt : 1) / 2;
    return fmt == GAT_LAYOUT_INTERLEAVED_I16 && !force_three && wpt > 0 && hs >= 8 && hs % 8 == 0 ? kMbTwo : kMbThree;
}
// two-term path: bytes of one LDS row of slot-ordered bf16 terms (10 bytes per sample), an odd multiple of 16 (rows of one
// 16-lane group of a 16-byte read then start on distinct bank quads)
constexpr int mb_two_row_bytes(int T) { return ((10 * T + 15) / 16 * 16) | 16; }
// chip-sign ring of the split-bf16 kernel: ring length and the least row length for a tap span (gat_mfma_bf16.hip, s_rep)
// (instances of two or four row tiles; those of one keep two buffers of span + T entries and copy the overlap)
constexpr bool mb_rep_ring_rows(int rt) { return rt >= 2; }
constexpr int mb_rep_ring(int rt, int T, int span) { return mb_rep_ring_rows(rt) ? (span + 2 * T + T - 1) / T * T : 0; }
constexpr int mb_rep_row(int rt, int T, int span) { return mb_rep_ring_rows(rt) ? mb_rep_ring(rt, T, span) + span + T : span + T; }
constexpr size_t mb_lds_bytes(int rt, int nct, int fmt, int nslots, int rep_stride, int code_bits_stride, int mode = -1)
{
    if (mode < 0) mode = mb_mode(rt, nct, fmt);
    const bool x1 = mode == kMbOne;
    const int T = mb_tile_samples(rt, nct);
    const int xs = x1 ? T + 2 : T + 1, wbytes = x1 ? 8 : 16;
    const size_t xw = mode == kMbTwo ? (size_t)2 * rt * 32 * mb_two_row_bytes(T) + (size_t)2 * (2 * nslots + 1) * mb_two_row_bytes(T)
                                     : (size_t)2 * rt * 32 * xs * 8 + (size_t)2 * (2 * nslots + 1) * xs * wbytes;
    return (size_t)kMbHeader + xw + (size_t)(((mb_rep_ring_rows(rt) ? 1 : 2) * nslots * rep_stride + 3) & ~3) * 4 + (size_t)nslots * code_bits_stride * 4;
}
// f32-MFMA kernel: 256-sample tiles, 32 planes per row tile
constexpr int kMfTile = 256;
constexpr int kMfXStride = kMfTile + 1; // floats per plane row in LDS: odd (bank spread)
constexpr size_t mf_lds_bytes(int nct, int ct, int rep_stride, int code_row_stride, int codes_in_lds)
{
    return (size_t)1024 + (size_t)2 * 32 * kMfXStride * sizeof(float) + (size_t)2 * nct * ct * rep_stride * sizeof(float) +
           (codes_in_lds ? (size_t)nct * ct * code_row_stride + 16 : 0);
}

// ---- the plan's inputs and output -------------------------------------------------------------------------------------------
// The kernel-selection and launch-geometry options of a context (gat_ctx::knobs): what each means, and its range, is the table
// kOptions of gat_api.cpp.  A recorded launch bakes them in: key_put_ctx (gat_api.cpp) keys every member.
struct CorrKnobs {
    long long one_wave_min = -1;                                // option dc_one_wave_min
    int mc_mode = 1;                                            // GAT_MC_* kernel selection (gat_set_matrix_core)
    int mc_nct = 0, mc_i16_terms = 2;                           // options mc_nct / mc_i16_terms
    int max_ant_tile = kMaxAntTile;                             // option max_ant_tile
    int max_aw = 4, max_kt = 4, max_bpw = 16;                   // options dc_aw / dc_kt / dc_bpw (and gat_set_vector_tiling)
    int force_bpw = 0, wgs_per_cu = 0;                          // options dc_bpw_force / dc_wgs_per_cu
    int one_wave = 1, one_wave_seg = kOneWaveSegSteps;          // options dc_one_wave / dc_ow_seg
    int max_depth = 2, keep_l2 = -1, quads = -1;                // options dc_depth / dc_keep_l2 / dc_quads
    int bit_tables = 1, aw2 = -1, seg_cap = 0, align_head = 1;  // options dc_bits / dc_aw2 / dc_seg / dc_align
};
// The context's code tables and device, as a call finds them (corr_tables, gat_ctx.h)
struct CorrTables {
    const int8_t *d_codes;
    const uint32_t *d_code_bits;
    const void *d_zeros;
    int Lc, P, code_row_stride, code_bits_stride, num_cus;
};
// a correlator call's arguments (params_dev: [B*K] records on the device, or null with params_inline: host records)
struct CorrCall {
    const gat_signal_desc *sig;
    const gat_channel_params *params_dev, *params_inline;
    int B, K, L;
    const int32_t *shifts;
    double fs;
    float *out_re, *out_im;
    uint32_t flags;
};
// What a call launches.  Planning fills every argument it knows; the enqueue adds the scratch, the uploaded records and
// the completion flag.  (a and cfg carry no initialiser on purpose: only the tap groups in use are written)
struct CorrPlan {
    int kind = 0; // 0: the vector kernel, 1: the f32-MFMA kernel, 2: the split-bf16 kernel
    // matrix-core kernels
    MfArgs m{};
    int rt = 1, nct = 1;
    unsigned grid = 0, lds = 0;
    // vector kernel: one launch per tap group
    int groups = 0; // tap groups (a resident plan sizes the first only)
    DcArgs a[GAT_MAX_TAPS];
    DcLaunch cfg[GAT_MAX_TAPS];
    int splits = 1;
    bool finalize = false, tail = false; // a second stage / a tail launch follows
    gat_launch_info info{};
};
constexpr Refusal kPlanned{GAT_OK, nullptr};

// validation (the null checks of the records and outputs are the caller's: a resident correlator has neither)
inline Refusal corr_check_call(const CorrTables &c, const CorrCall &call)
{
    const gat_signal_desc *sig = call.sig;
    if (!c.d_codes) return {GAT_ERR_STATE, "gat_set_codes has not been called"};
    const int fmt = sig->layout;
    if (fmt < GAT_LAYOUT_PLANAR || fmt > GAT_LAYOUT_INTERLEAVED_I8) return {GAT_ERR_ARG, "unknown signal layout"};
    const bool planar = fmt == GAT_LAYOUT_PLANAR;
    if (!sig->re || (planar && !sig->im) || (!planar && sig->im)) return {GAT_ERR_ARG, "signal pointers do not match the layout"};
    if (call.B < 1 || call.K < 1 || sig->num_ants < 1 || sig->num_samples < 1) return {GAT_ERR_ARG, "sizes must be positive"};
    if (call.L < 1 || call.L > GAT_MAX_TAPS) return {GAT_ERR_RANGE, "num_taps outside 1..GAT_MAX_TAPS"};
    if (!(call.fs > 0.0) || !std::isfinite(call.fs)) return {GAT_ERR_ARG, "sampling frequency must be positive"};
    if (call.flags & ~GAT_FLAG_ATOMIC) return {GAT_ERR_ARG, "unknown flag bits"};
    long long max_shift = 0;
    for (int l = 0; l < call.L; ++l) max_shift = std::max<long long>(max_shift, std::llabs((long long)call.shifts[l]));
    if (sig->num_samples + max_shift >= (1ll << 30)) return {GAT_ERR_RANGE, "num_samples + |shift| must stay below 2^30"};
    if (sig->ant_stride < 0 || sig->block_stride < 0 || sig->chan_stride < 0) return {GAT_ERR_ARG, "negative stride"};
    return kPlanned;
}

// ---- the tap order and the launch groups --------------------------------------------------------------------------------------
// the taps sorted by shift (stable: equal shifts keep the caller's order) and cut into the vector kernel's launches:
// groups of <= kMaxTapsPerLaunch whose span fits the LDS replica segment (a single-tap group always fits: span 0)
struct CorrTaps {
    int order[GAT_MAX_TAPS], sorted[GAT_MAX_TAPS], begin[GAT_MAX_TAPS + 1]; // group g: sorted taps begin[g] .. begin[g + 1] - 1
    int groups;
    int max_taps; // taps of the widest launch (register accumulators 2 * MT * taps * kt)
    int span;
    long long max_shift;
};
inline void corr_sort_taps(const CorrCall &call, CorrTaps &t)
{
    const int L = call.L;
    t.groups = 0;
    t.max_taps = 1;
    for (int l = 0; l < L; ++l) t.order[l] = l;
    std::stable_sort(t.order, t.order + L, [&](int x, int y) { return call.shifts[x] < call.shifts[y]; });
    for (int l = 0; l < L; ++l) t.sorted[l] = call.shifts[t.order[l]];
    for (int t0 = 0; t0 < L;) {
        int t1 = t0 + 1;
        while (t1 < L && t1 - t0 < kMaxTapsPerLaunch && (long long)t.sorted[t1] - t.sorted[t0] <= kMaxLaunchSpan) ++t1;
        t.begin[t.groups++] = t0;
        t.max_taps = std::max(t.max_taps, t1 - t0);
        t0 = t1;
    }
    t.begin[t.groups] = L;
    t.span = t.sorted[L - 1] - t.sorted[0];
    t.max_shift = std::max(std::llabs((long long)t.sorted[0]), std::llabs((long long)t.sorted[L - 1]));
}

// ---- the load width and the antenna tile ----------------------------------------------------------------------------------------
struct CorrLoads {
    int vec, MT;
    int spv;               // samples one 16-byte load holds (4 / 2 / 4 / 8 by format)
    long long plane_bytes; // bytes of one sample in one plane
};
inline CorrLoads corr_pick_loads(const CorrKnobs &c, const gat_signal_desc *sig, int B)
{
    const int M = sig->num_ants, fmt = sig->layout;
    const long long N = sig->num_samples;
    int MT = 1;
    for (int mt = c.max_ant_tile; mt >= 1; --mt)
        if (M % mt == 0) {
            MT = mt;
            break;
        }
    // 16-byte vector loads need every group start 16-byte aligned: plane bases and all strides
    // multiples of the samples one 16-byte load holds (4 / 2 / 4 / 8 by format)
    const int spv = dc_group_samples(4, fmt);
    const long long plane_bytes = layout_sample_bytes(fmt);
    int vec = 1;
    // ... in a block that a 32-bit descriptor length can describe.  The block LENGTH may be anything (the reference
    // bounds each thread by num_samples, src/algorithms.jl:170): lanes beyond the last whole group read zeros through
    // the buffer range check and the N % spv samples behind it are taken one per lane after the step loop.
    // (a stride that is never applied -- one antenna, one block -- does not matter)
    if (blocks_aligned(sig, B) && sig->chan_stride % spv == 0 && N * plane_bytes < (1ll << 31)) vec = 4;
    if (vec != 4) MT = 1; // unaligned input (scalar loads) is served one antenna per wave
    // the vector kernel reaches a wave's MT antennas through ONE descriptor per plane (antenna = scalar offset): the
    // tile's span of bytes must stay below 2^31 (a lane offset of 2^31 then means "beyond every record")
    while (MT > 1 && ((long long)(MT - 1) * sig->ant_stride + N) * plane_bytes >= (1ll << 31)) {
        int next = 1;
        for (int mt = MT - 1; mt >= 1; --mt)
            if (M % mt == 0) { next = mt; break; }
        MT = next;
    }
    return {vec, MT, spv, plane_bytes};
}

// ---- matrix-core paths: antenna-rich shapes whose (channel, tap) columns fill a useful part of
// a 32-column tile run on the matrix cores -- the split-bf16 kernel (gat_mfma_bf16.hip) by default,
// the f32-MFMA kernel (gat_mfma.hip) on request; everything else takes the vector kernel below.

// split-bf16 kernel: a consumer lane reads the chip-sign word of its column's (channel slot, tap) -- dword slot * rs + shift
// + const -- 32 lanes (columns of one tile) per LDS access, 32 banks: choose the row stride rs (odd, in [base, base + 32))
// under which the fewest of a tile's distinct words share a bank (rows 1 apart at taps -49 / 0 / +49: slot s + 2's early
// tap sits on slot s's late tap's bank, every read a 2-way conflict)
inline int pick_rep_stride(int base, int tiles, int K, int L, const int *sorted)
{
    int best_rs = base + 1;
    long long best_cost = -1;
    for (int rs = base + 1; rs < base + 32; rs += 2) {
        long long cost = 0;
        for (int tl = 0; tl < tiles; ++tl) {
            int words[32], nw = 0; // distinct words of the tile
            for (int r = 0; r < 32; r += 2) { // columns (k, l, re / im): the pair reads one word
                const int col = 32 * tl + r, k = col / (2 * L), l = (col - 2 * L * k) >> 1;
                if (k >= K) break;
                words[nw++] = k * rs + (sorted[l] - sorted[0]);
            }
            for (int i = 0; i < nw; ++i)
                for (int j = 0; j < i; ++j) cost += ((words[i] - words[j]) & 31) == 0 && words[i] != words[j];
        }
        if (best_cost < 0 || cost < best_cost) {
            best_cost = cost;
            best_rs = rs;
        }
    }
    return best_rs;
}

// Says whether a matrix-core kernel takes the call (p.kind != 0 behind it), and fills p.m, p.rt, p.nct, p.grid, p.lds, p.splits,
// p.finalize and p.info if so.
inline Refusal plan_matrix(const CorrKnobs &c, const CorrTables &t, const CorrCall &call, const CorrTaps &taps, const CorrLoads &ld, CorrPlan &p)
{
    const gat_signal_desc *sig = call.sig;
    const int B = call.B, K = call.K, L = call.L, M = sig->num_ants, fmt = sig->layout, vec = ld.vec, spv = ld.spv, span = taps.span;
    const long long N = sig->num_samples;
    const int *sorted = taps.sorted;
    const int CT = L <= kMfmaMaxTaps ? 16 / L : 0;
    // Both matrix-core kernels fill a lane's replica entries from one floored modulo and at most one wrap of the table
    // per 32 samples, and poison (NaN) a channel whose code rate breaks that (mfma_wrap_bad).  Tables of fewer than 64
    // chips (where a rate below two chips per sample can break it), and host-side records that break it, take the vector
    // kernel instead (a one-chip table under GAT_MC_F32 returned NaN for a valid call).
    bool wraps_ok = t.Lc >= 64;
    if (call.params_inline)
        for (long long i = 0; i < (long long)B * K && wraps_ok; ++i) wraps_ok = !mfma_wrap_bad(call.params_inline[i].code_freq_hz / call.fs, t.Lc);
    const bool shape_any = c.mc_mode != 0 && vec == 4 && N % spv == 0 /* whole load groups */ && M % 16 == 0 && sig->chan_stride == 0 && CT >= 1 &&
                           span <= kMfmaMaxSpan && 2 * std::min(K, CT) * L >= 12 /* >= 3/8 of the columns */ && wraps_ok;
    const bool shape_ok = shape_any && fmt == GAT_LAYOUT_PLANAR; // the f32-MFMA kernel reads planar f32 only
    const int nct_total = shape_ok ? (K + CT - 1) / CT : 1;
    int nct = nct_total >= 4 ? 4 : (nct_total >= 2 ? 2 : 1);
    while (nct > 1 && nct * CT > 20) nct >>= 1; // both kernels keep at most 20 channel slots per workgroup
    // split-bf16 kernel: columns packed flat (2 L per channel), 32 per tile; rt_max 16-antenna row tiles per workgroup.
    // Column tiles per workgroup: a workgroup of nct tiles costs the same whether its last tiles are live or dead, so
    // the launch costs (groups x nct) tile SLOTS -- at two tiles per workgroup a slot costs w2 x what it costs at four
    // (more sample splitting per column, the 12-wave instance at 64 antennas; profiles/r05/mfma_nct_scan_*.txt:
    // 1.13-1.41 by layout and row tiles).  Three tiles: 4 slots either way -> one workgroup of four (0.55 vs 0.74 ms
    // at 64 antennas x 16 channels of int16); five or six: 6 x w2 slots vs 8 -> mostly two per workgroup (0.62 vs
    // 0.75 ms at 32 x 32 int16, 0.86 vs 0.93 float); nine or more: four.
    const bool int8_in = fmt == GAT_LAYOUT_INTERLEAVED_I8;
    const bool two_term = fmt == GAT_LAYOUT_INTERLEAVED_I16 && c.mc_i16_terms != 3;
    const int tiles_b = (2 * L * K + 31) / 32;
    const int rt_max = (M / 16) % 4 == 0 ? 4 : ((M / 16) % 2 == 0 ? 2 : 1);
    int n_first = tiles_b >= 4 ? 4 : (tiles_b >= 2 ? 2 : 1);
    const double w2 = int8_in ? (rt_max == 4 ? 1.41 : 1.22) : two_term ? (rt_max == 4 ? 1.30 : 1.13) : (rt_max == 4 ? 1.26 : 1.235);
    if (tiles_b >= 3) n_first = ((tiles_b + 1) / 2 * 2) * w2 < (tiles_b + 3) / 4 * 4 ? 2 : 4;
    // kernel choice: 3 / 1 (auto) -> split-bf16 when its tile fits in LDS, 2 -> f32 MFMA.  GAT_MC_AUTO picks a matrix
    // kernel only where it measured faster than the vector kernel (scripts/r05_i16_planner_scan.sh, profiles/r05/
    // mfma_planner_scan_*.txt: N = 50 000, 3 taps, 16-64 antennas x 4-32 channels; round 2's scan: profiles/r02/).  What
    // decides is the share of the launch's tile slots that carry live columns, u = 2 L K / (32 x slots x slot cost): the
    // vector kernel's time grows with K, the matrix kernel's with the slots.  Float samples (three bf16 terms): the
    // matrix kernel wins from u = 0.70 on at four row tiles (64 x 16: 0.76 vs 0.90 ms, 64 x 32: 1.48 vs 1.69; 64 x 24
    // at u = 0.60: 1.48 vs 1.30) and only with nearly full slots at two (32 x 32, u = 0.81: 0.88 vs 0.85; 32 x 64 wins);
    // int16 samples (two exact terms, 5/8 of the MFMAs): from u = 0.5 on (32 x 8: 0.22 vs 0.27 ms, 64 x 12: 0.55 vs
    // 0.74, 64 x 32: 1.12 vs 1.81; a single tile -- 4 channels -- loses); one row tile (M = 16, 48) never wins; tap
    // counts beyond three were not scanned again: round 2's rule (M >= 32, K >= 32, M K >= 2048) stays for them.
    // From int8 pairs (single-term path) it wins from 24 (channel, tap, re/im) columns on at every M.  The f32-MFMA
    // kernel is never chosen by itself any more: the round-2 vector kernel is faster everywhere (configs[4]: 2.45 vs
    // 4.19 ms, 64 antennas x 32 channels: 0.58 vs 0.92 ms); it runs on request (GAT_MC_F32).
    const int slots_first = (tiles_b + n_first - 1) / n_first * n_first;
    const double slot_cost = n_first == 4 ? 1.0 : n_first == 2 ? w2 : 1.8;
    const double util = 2.0 * L * K / (32.0 * slots_first * slot_cost);
    const double util_min = rt_max == 1 ? 2.0 : two_term ? (rt_max == 4 ? 0.50 : 0.53) : (rt_max == 4 ? 0.70 : 0.90);
    const bool round2_rule = M >= 32 && K >= 32 && (long long)M * K >= 2048;
    const bool auto_bf16 = 2ll * L * K >= 24 && (int8_in || (L <= 3 ? util >= util_min : round2_rule));
    const bool want_bf16 = c.mc_mode == 3 || (c.mc_mode == 1 && auto_bf16);
    const bool want_f32 = c.mc_mode == 2;
    int kind = 0, rt = 1, rep_stride_m = 0;
    int nslots_b = 0, nct_b = 1;
    if (shape_any && want_bf16 && t.d_code_bits && t.d_zeros && N % spv == 0 && spv <= 8) {
        if (c.mc_nct > 0) n_first = c.mc_nct; // A/B runs
        for (int n = n_first; n >= 1 && !kind; n >>= 1) {
            rt = (rt_max == 4 && n == 1) ? 2 : rt_max; // <4,1> does not fit the VGPR budget of a 12-wave workgroup
            const int T = mb_tile_samples(rt, n);
            // chip-sign rows: a ring + the copy of its first window (gat_mfma_bf16.hip, s_rep); odd: channel rows land on different banks
            int rs = ((mb_rep_row(rt, T, span) + 31) / 32) * 32 + 1;
            const int ns = mb_slots(n, L, K);
            // at most one (slot, sample pair) item per producer thread
            if (ns * T / 2 > mb_producer_threads(rt, n) || ns > kMbMaxSlots) continue;
            const int mode_n = mb_mode(rt, n, fmt, c.mc_i16_terms == 3);
            // ... and the taps of neighbouring channels too, where the longer rows still fit
            const int rs_tuned = pick_rep_stride(rs - 1, tiles_b, K, L, sorted);
            if (mb_lds_bytes(rt, n, fmt, ns, rs_tuned, t.code_bits_stride, mode_n) <= 160 * 1024) rs = rs_tuned;
            if (mb_lds_bytes(rt, n, fmt, ns, rs, t.code_bits_stride, mode_n) <= 160 * 1024) {
                if (c.mc_mode == 1) {
                    // GAT_MC_AUTO: the kernel's set-up (sign tables and the first replica into LDS, three sample loads
                    // ahead) is paid per workgroup, and a launch is cut into ~2 workgroups per CU: with few steps per
                    // workgroup the vector kernel is faster whatever the shape (ONE 50 MHz block of 64 antennas x 32
                    // int16 channels: 10 steps each, 0.056 vs 0.050 ms; round 4's rule sent it here).  Crossovers:
                    // 10-14 steps with int16 pairs, 25-40 with float samples (profiles/r05/mfma_blocks_scan_*.txt).
                    const long long steps_total = (N + T - 1) / T;
                    const long long groups = (long long)B * (M / (16 * rt)) * ((tiles_b + n - 1) / n);
                    const long long cut = std::min<long long>(steps_total, std::max<long long>(1, (2ll * t.num_cus + groups - 1) / groups));
                    const long long steps_each = (steps_total + cut - 1) / cut;
                    if (steps_each < (two_term || int8_in ? 16 : 32)) break; // -> the vector kernel
                }
                kind = 2;
                nct_b = n;
                nslots_b = ns;
                rep_stride_m = rs;
            }
        }
    }
    if (shape_ok && !kind && want_f32) {
        rep_stride_m = ((256 + span + 31) / 32) * 32 + 1;
        if (mf_lds_bytes(nct, CT, rep_stride_m, t.code_row_stride, 0) <= 160 * 1024) kind = 1;
    }
    if (!kind) return kPlanned;
    if (kind == 2) nct = nct_b;
    const int T = kind == 2 ? mb_tile_samples(rt, nct) : 256;
    MfArgs &m = p.m;
    m.re = sig->re;
    m.im = sig->im;
    m.params = call.params_dev; // null: the host records are uploaded at the enqueue
    m.codes = t.d_codes;
    m.out_re = call.out_re;
    m.out_im = call.out_im;
    m.N = N;
    m.ant_stride = sig->ant_stride;
    m.block_stride = sig->block_stride;
    m.fs = call.fs;
    m.M = M; m.K = K; m.B = B; m.L = L; m.Lc = t.Lc; m.num_prns = t.P; m.code_row_stride = t.code_row_stride;
    m.CT = CT;
    m.chan_groups = kind == 2 ? (tiles_b + nct - 1) / nct : (nct_total + nct - 1) / nct;
    m.nslots = nslots_b;
    m.ant_tiles = kind == 2 ? M / (16 * rt) : M / 16;
    m.total_steps = (int)((N + T - 1) / T);
    const long long groups_m = (long long)B * m.ant_tiles * m.chan_groups;
    // the split-bf16 kernel runs one 8-wave workgroup per CU (its LDS tile): 2 rounds fill the chip
    const long long want = (kind == 2 ? 2ll : 4ll) * t.num_cus;
    long long sp = std::max<long long>(1, (want + groups_m - 1) / groups_m);
    sp = std::min<long long>(sp, m.total_steps);
    m.steps_per_split = (int)((m.total_steps + sp - 1) / sp);
    if (kind == 2) m.steps_per_split = std::min(m.steps_per_split, std::max(1, kMbMaxChain / T));
    m.splits = (m.total_steps + m.steps_per_split - 1) / m.steps_per_split;
    if (kind == 2 && m.splits > 1) {
        // one workgroup per CU at a time: prefer a split count whose workgroups fill whole rounds of the chip
        // (735 workgroups on 256 CUs idle 13 % of the third round; 768 do not)
        int best = m.splits;
        double best_eff = 0.0;
        for (int sp2 = m.splits; sp2 <= std::min<long long>(m.total_steps, (long long)m.splits + m.splits / 4 + 8); ++sp2) {
            const int sps = (m.total_steps + sp2 - 1) / sp2;
            const int real = (m.total_steps + sps - 1) / sps; // split count that step size really gives
            const long long wgs = groups_m * real;
            const long long rounds = (wgs + t.num_cus - 1) / t.num_cus;
            const double eff = (double)wgs / (double)(rounds * t.num_cus);
            if (eff > best_eff + 1e-9) {
                best_eff = eff;
                best = real;
            }
        }
        m.steps_per_split = (m.total_steps + best - 1) / best;
        m.splits = (m.total_steps + m.steps_per_split - 1) / m.steps_per_split;
    }
    m.num_tiles = B * m.ant_tiles * m.splits;
    m.max_abs_shift = (int)taps.max_shift;
    m.rep_span = span;
    m.rep_stride = rep_stride_m;
    m.rep_ring = kind == 2 ? mb_rep_ring(rt, T, span) : 0;
    m.flags = call.flags;
    for (int l = 0; l < kMfmaMaxTaps; ++l) {
        m.shifts[l] = sorted[std::min(l, L - 1)];
        m.tap_index[l] = taps.order[std::min(l, L - 1)];
    }
    const long long grid_m = ((long long)(m.num_tiles + 7) / 8) * 8 * m.chan_groups;
    if (grid_m >= (1ll << 31)) return {GAT_ERR_RANGE, "grid too large"};
    if (kind == 2) {
        m.codes_in_lds = 1; // sign-bit tables, always staged
        m.code_bits = t.d_code_bits;
        m.zeros = t.d_zeros;
        m.code_bits_stride = t.code_bits_stride;
        // int16 samples: two exact bf16 terms per value (5 products per sample), or the float path's three on request
        m.mb_mode = mb_mode(rt, nct, fmt, c.mc_i16_terms == 3);
        p.lds = (unsigned)mb_lds_bytes(rt, nct, fmt, m.nslots, m.rep_stride, t.code_bits_stride, m.mb_mode);
    } else {
        m.codes_in_lds = mf_lds_bytes(nct, CT, m.rep_stride, t.code_row_stride, 1) <= 160 * 1024;
        p.lds = (unsigned)mf_lds_bytes(nct, CT, m.rep_stride, t.code_row_stride, m.codes_in_lds);
    }
    p.kind = kind;
    p.rt = rt;
    p.nct = nct;
    p.grid = (unsigned)grid_m;
    p.splits = m.splits;
    p.finalize = !(call.flags & GAT_FLAG_ATOMIC) && m.splits > 1;
    // (gat.h order: workgroups, threads, splits, ant_tile, vec, lds_bytes, finalize_launched, matrix_core, channels_per_wg,
    // blocks_per_wg, prefetch_depth, bf16_terms)
    p.info = {(int32_t)grid_m, kind == 2 ? mb_threads(rt, nct) : 2 * kThreads, m.splits, kind == 2 ? 16 * rt : 16, 4, (int32_t)p.lds,
              p.finalize ? 1 : 0, kind, kind == 2 ? m.nslots : nct * CT, 1, 0, kind == 2 ? (m.mb_mode == kMbOne ? 1 : m.mb_mode == kMbTwo ? 2 : 3) : 0};
    return kPlanned;
}

// ---- vector kernel (gat_dc.h): launch geometry ---------------------------------------------------------
// One tap group's launch: e and ec arrive as the call's common arguments and geometry; its taps, replica layout, segment, depth
// and LDS are set here.  seg_max: most steps per segment of this geometry; deep_ok: two sample sets are allowed.
inline Refusal size_tap_group(const CorrTaps &tp, int g, long long chunk, long long cps, int tab_bytes, int seg_max, bool deep_ok, DcArgs &e, DcLaunch &ec)
{
    const int MT = ec.ant_tile, aw = ec.aw, kt = ec.kt, nw = ec.nw, vec = ec.vec, fmt = ec.format;
    const int t0 = tp.begin[g], taps = tp.begin[g + 1] - t0;
    ec.taps = taps;
    // Taps in any order: tap_index maps each tap of a launch back to its position in the caller's list.
    for (int l = 0; l < kMaxTapsPerLaunch; ++l) {
        e.shifts[l] = tp.sorted[t0 + std::min(l, taps - 1)];
        e.tap_index[l] = tp.order[t0 + std::min(l, taps - 1)];
    }
    e.rep_span = e.shifts[taps - 1] - e.shifts[0];
    // Replica layout in LDS (gat_dc.h): linear, one 8-byte-aligned vector read per tap and 4 samples.  Taps at an
    // even distance from the first read the replica itself; any tap at an odd distance needs the copy stored one
    // entry further, and the segment shrinks so that both fit the channel's share of LDS.
    bool odd = false;
    for (int l = 0; l < taps; ++l) odd |= ((e.shifts[l] - e.shifts[0]) & 1) != 0;
    int seg = seg_max;
    ec.depth = 1;
    if (nw == 1) { // the replica's LDS is sized for this launch: segment + tap span + one entry per producer lane
        e.seg_steps = (int)std::min<long long>(seg, cps);
        if (deep_ok && seg >= 2 && dc_instance(MT, taps, vec, aw, kt, nw, 2)) {
            ec.depth = 2; // whole groups of two steps per segment; the kernel pads the block's last group
            e.seg_steps = (int)std::min<long long>(seg - seg % 2, (cps + 1) / 2 * 2);
        }
        const int one = dc_rep_copy_floats(e.seg_steps, (int)chunk, e.rep_span, 64);
        e.rep_copy_stride = odd ? one : 0;
        e.rep_chan_floats = ((odd ? 2 : 1) * one + 7) & ~7;
        ec.lds_bytes = (unsigned)dc_lds_bytes_one_wave(e.rep_chan_floats, tab_bytes);
    } else {
        // An instance that holds four waves per SIMD (dc_min_waves) needs four workgroups per CU to get them: with
        // 10 KB chip tables (GPS L5) the full eight-step segment makes a workgroup 47 KB -- three per CU.  Such launches
        // take a segment short enough for 40 KB (configs[2]: six steps; 1.151 -> 1.106 ms together with the two-sample
        // passes that bring the five-tap instance to 128 registers, profiles/r04/r04g_c2_four_waves.txt).
        // (a tap span beyond the default sizing -- seven taps half a chip apart at 262 MHz span 768 samples -- gets the
        // room it needs in the same launch instead of a second launch: 22.8 -> 17 us for that call)
        const int span_sz = std::max(kMaxReplicaSpan, e.rep_span);
        const int want_waves = dc_min_waves(MT, taps, kt, 1, fmt, aw);
        if (want_waves >= 4 || (aw == 2 && want_waves >= 3))
            while (seg > 2 && dc_lds_bytes_floats(kt, tab_bytes, dc_rep_chan_floats_steps(seg, (int)chunk, span_sz)) > (size_t)(160 / want_waves) * 1024) --seg;
        if (span_sz > kMaxReplicaSpan)
            while (seg > 1 && dc_lds_bytes_floats(kt, tab_bytes, dc_rep_chan_floats_steps(seg, (int)chunk, span_sz)) > 64 * 1024) --seg;
        const int chan_floats = dc_rep_chan_floats_steps(seg, (int)chunk, span_sz);
        if (dc_lds_bytes_floats(kt, tab_bytes, chan_floats) > 160 * 1024)
            return {GAT_ERR_RANGE, "tap span and code table do not fit the LDS of one workgroup"};
        e.rep_chan_floats = chan_floats;
        ec.lds_bytes = (unsigned)dc_lds_bytes_floats(kt, tab_bytes, chan_floats);
        if (odd)
            while (seg > 1 && 2 * dc_rep_copy_floats(seg, (int)chunk, e.rep_span) > chan_floats) --seg;
        if (deep_ok && seg >= 2 && dc_instance(MT, taps, vec, aw, kt, nw, 2)) {
            ec.depth = 2;
            seg -= seg % 2; // whole groups of two steps per segment; the kernel pads the block's last group
        }
        e.seg_steps = (int)std::min<long long>(seg, (cps + ec.depth - 1) / ec.depth * ec.depth);
        e.rep_copy_stride = odd ? dc_rep_copy_floats(e.seg_steps, (int)chunk, e.rep_span) : 0;
    }
    for (int l = 0; l < kMaxTapsPerLaunch; ++l) {
        const int d = e.shifts[l] - e.shifts[0];
        e.tap_off[l] = (d & 1) ? e.rep_copy_stride + d - 1 : d;
    }
    return kPlanned;
}

// The vector kernel's launches of a call: p.a / p.cfg of every tap group, p.splits, p.finalize, p.tail, p.info.  resident_wgs > 0:
// the ONE vector launch a resident correlator would be (corr_plan_resident): one antenna tile and one channel per workgroup on
// four waves, one sample set, the block's samples split over about resident_wgs workgroups, walked from the line; only the first
// tap group is sized.
inline Refusal plan_vector(const CorrKnobs &c, const CorrTables &t, const CorrCall &call, const CorrTaps &taps, const CorrLoads &ld, long long resident_wgs, CorrPlan &p)
{
    const bool resident = resident_wgs > 0;
    const gat_signal_desc *sig = call.sig;
    const int B = call.B, K = call.K, L = call.L, M = sig->num_ants, fmt = sig->layout, vec = ld.vec, spv = ld.spv, max_taps = taps.max_taps;
    const long long N = sig->num_samples, plane_bytes = ld.plane_bytes, max_shift = taps.max_shift;
    int MT = ld.MT;
    // aw: antenna tiles (waves) per workgroup -- 16 antennas on 4 waves walk the same samples, so carrier and replica
    //     are produced once per workgroup; kt: channels a workgroup loops over with the samples held in registers.
    // The two-channel 2 x 2 tile (round 5): a four-antenna tile as TWO waves of two antennas on the same samples, each wave
    // looping over TWO channels on its register-resident samples -- half the sample loads per channel of the one-wave-of-four
    // tile at the same registers per wave.  Several channels on one signal were bound by the CU's load path (L2 -> L1 -> registers:
    // 12 channel workgroups re-read every tile), not by HBM or the vector pipe: configs[2] 1.14 -> 1.02 ms, four antennas x
    // eight channels at 20 MHz 0.305 -> 0.253 ms, eight antennas x four channels 0.368 -> 0.291 ms
    // (profiles/r05/ab_aw2_rule.txt).  Not for int8 pairs (eight-sample groups: the two-channel step spills), not for tiles of
    // 16 antennas (AW = 4 with up to four channels per workgroup), not in the latency regime (too few workgroups to matter;
    // + 6 % there), not for one signal per channel.  Option dc_aw2: -1 this rule, 0 never, 1 wherever an instance exists.
    const long long pairs_wgs = (long long)B * ((K + 1) / 2) * (M / 4);
    // (ComplexF32 pairs beyond five taps: the instance drops to two waves per SIMD)
    const bool aw2_rule = fmt != GAT_LAYOUT_INTERLEAVED_I8 && !(fmt == GAT_LAYOUT_INTERLEAVED && max_taps > 5) && K >= 2 && sig->chan_stride == 0 &&
                          pairs_wgs >= 2ll * t.num_cus;
    const bool aw4_tile = (M / MT) % 4 == 0 && c.max_aw >= 4; // sixteen antennas on four waves (with up to four channels per workgroup)
    // LDS: two workgroups per CU at least (80 KB each); a chip table that does not even fit alone is an error
    // chip tables in LDS: int8 rows, or -- long codes (GPS L5: 10 KB per PRN) whose chips are all +-1 -- sign-bit rows (1.3 KB):
    // room for long replica segments and for a second channel's table (option dc_bits: 0 never, 1 long codes, 2 always)
    bool bit_tables = t.d_code_bits && t.code_bits_stride > 0 && (c.bit_tables == 2 || (c.bit_tables == 1 && t.code_row_stride > 2048));
    int tab_bytes = bit_tables ? t.code_bits_stride * 4 : t.code_row_stride;
    // (the 2 x 2 tile only where its two channels' tables fit: a long int8 table -- chips not all +-1, 20 000 and more --
    // would leave it one channel, and there is no instance of that)
    const bool aw2 = (c.aw2 == 1 || (c.aw2 < 0 && aw2_rule)) && !resident && vec == 4 && MT == 4 && !aw4_tile && c.max_kt >= 2 &&
                     c.max_aw >= 2 && K >= 2 && sig->chan_stride == 0 && dc_instance(2, max_taps, 4, 2, 2) &&
                     dc_lds_bytes(2, 2, tab_bytes, dc_chunk(vec, fmt, 2)) <= 80 * 1024;
    if (aw2) MT = 2;
    const int AT = M / MT;
    int aw = 1, kt = 1;
    if (vec == 4 && MT == 4) aw = AT % 4 == 0 ? 4 : (AT % 2 == 0 ? 2 : 1);
    if (aw2) aw = 2;
    aw = std::min(aw, c.max_aw);
    if (vec == 4 && aw == 4 && sig->chan_stride == 0 && K > 1) kt = K >= 3 ? 4 : 2;
    if (aw2 && sig->chan_stride == 0 && K > 1) kt = 2; // the 2 x 2 tile: two channels on the wave's two antennas (half the loads per channel)
    kt = std::min(kt, c.max_kt);
    if (resident) aw = 1, kt = 1;
    while (kt > 1 && !dc_instance(MT, max_taps, vec, aw, kt)) kt >>= 1;
    while (aw > 1 && !dc_instance(MT, max_taps, vec, aw, kt)) aw >>= 1;
    auto lds_of = [&](int kt_, int aw_) { return dc_lds_bytes(kt_, MT, tab_bytes, dc_chunk(vec, fmt, aw_)); };
    while (kt > 1 && lds_of(kt, aw) > 80 * 1024) kt >>= 1;
    if (lds_of(kt, aw) > 160 * 1024) return {GAT_ERR_RANGE, "code table too long for the LDS-resident chip table of the vector kernel"};
    if (!dc_instance(MT, max_taps, vec, aw, kt)) return {GAT_ERR_UNSUPPORTED, "no kernel instance for this shape"};
    const int AG = AT / aw;
    const int KG = (K + kt - 1) / kt;

    const long long groups = (long long)B * KG * AG;
    // One-wave workgroups: short blocks (a few steps of a four-wave workgroup) of one- or two-antenna tiles in a stream
    // long enough to fill the chip with single waves.  Per block the set-up (parameters, rotations, walk constants) is
    // then done by one wave instead of four, and no wave waits at a workgroup barrier.
    int nw = 4;
    if (c.one_wave && !resident && vec == 4 && aw == 1 && kt == 1 && MT <= 2 && t.code_row_stride <= 2048 &&
        (N + dc_chunk(vec, fmt, 1) - 1) / dc_chunk(vec, fmt, 1) <= 8 &&
        groups >= (c.one_wave_min >= 0 ? c.one_wave_min : 32ll * t.num_cus) &&
        c.max_aw >= 4 /* the (1, 1, 1) tiling of the A/B tests keeps the four-wave geometry */ &&
        dc_instance(MT, max_taps, vec, 1, 1, 1))
        nw = 1;
    if (!dc_bit_tables(nw)) bit_tables = false, tab_bytes = t.code_row_stride; // (one-wave workgroups read int8 rows)
    const long long chunk = dc_chunk(vec, fmt, aw, nw);
    // Workgroups per CU the split aims for: 8 -- except for the channel-looping instances (KT >= 2: 170-250 registers,
    // two workgroups resident per CU), where a finer split only adds partial sums, a second launch and workgroup starts
    // (configs[3] shard, 512 tiles: 2 / 4 / 8 per CU = 0.667 / 0.675 / 0.687 ms, profiles/r03/r03a_c4_split.txt).
    const int per_cu = c.wgs_per_cu > 0 ? c.wgs_per_cu : (kt >= 2 ? 2 : 8);
    const long long target = resident ? resident_wgs : (long long)per_cu * t.num_cus * (nw == 1 ? 4 : 1);
    long long chunks = 0, splits = 1, cps = 1, bpw = 1;
    auto plan = [&](long long slack) { // slack: virtual samples in front of a block (line alignment, below)
        chunks = (N + slack + chunk - 1) / chunk;
        splits = std::max<long long>(1, (target + groups - 1) / groups);
        splits = std::min(splits, chunks);
        // tiny blocks (latency regime): a second launch costs more than a few serial steps
        // (a resident correlator has no second launch: its workgroups post their sums to the host, which adds them)
        if (chunks <= 4 && !(call.flags & GAT_FLAG_ATOMIC) && !resident) splits = 1;
        cps = (chunks + splits - 1) / splits;
        splits = (chunks + cps - 1) / cps;
    };
    plan(0);
    // short blocks in a long stream: one workgroup loops over several consecutive blocks (chip table, channel set-up
    // and the workgroup launch are paid once) while the chip stays filled 16 workgroups deep per CU
    if (splits == 1 && c.max_bpw > 1) {
        const long long by_fill = std::max<long long>(1, groups / (16ll * t.num_cus * (nw == 1 ? 4 : 1)));
        const long long by_len = std::max<long long>(1, (nw == 1 ? 64 : 16) / chunks);
        bpw = std::min<long long>(std::min(by_fill, by_len), c.max_bpw);
        if (c.force_bpw > 0) bpw = std::min<long long>(c.force_bpw, B); // A/B runs: option dc_bpw_force
    }
    // Line alignment (gat_dc.h): where a block of some antenna may start off a 128-byte line -- the base pointer or a stride
    // that is applied is no multiple of 128 bytes (N = 50 000 floats: every other block) -- workgroups walk each block from
    // the line its first sample lies in: up to 112 bytes of virtual samples in front of the block, hence the slack in the
    // chunk count.  Four-wave workgroups that own one block each (several short blocks per workgroup keep their walk across
    // block boundaries instead); option dc_align = 0 turns it off for A/B runs.
    // (a resident correlator is told the block's offset with every call: it always walks from the line)
    const bool align_head = c.align_head && vec == 4 && nw == 4 && bpw == 1 &&
                            (resident || (reinterpret_cast<uintptr_t>(sig->re) & 127u) != 0 || (B > 1 && (sig->block_stride * plane_bytes) % 128 != 0) ||
                             (M > MT && (sig->ant_stride * plane_bytes * MT) % 128 != 0) || (sig->chan_stride * plane_bytes) % 128 != 0);
    if (align_head) plan(112 / plane_bytes);
    const long long BG = (B + bpw - 1) / bpw;
    const long long tiles = BG * AG * splits;
    const long long grid_wgs = ((tiles + 7) / 8) * 8 * KG;
    if (grid_wgs >= (1ll << 31)) return {GAT_ERR_RANGE, "grid too large"};

    DcArgs a{};
    a.re = sig->re;
    a.im = sig->im;
    a.params = call.params_dev;
    if (!call.params_dev && call.params_inline) std::memcpy(a.inl, call.params_inline, (size_t)B * K * sizeof(gat_channel_params));
    a.codes = t.d_codes;
    a.out_re = call.out_re;
    a.out_im = call.out_im;
    a.total_wgs = (unsigned)(tiles * KG);
    a.N = N;
    a.ant_stride = sig->ant_stride;
    a.block_stride = sig->block_stride;
    a.chan_stride = sig->chan_stride;
    a.fs = call.fs;
    a.M = M;
    a.K = K;
    a.B = B;
    a.Lc = t.Lc;
    a.num_prns = t.P;
    a.code_row_stride = t.code_row_stride;
    a.code_bits = bit_tables ? t.d_code_bits : nullptr;
    a.table_stride = tab_bytes;
    a.KG = KG;
    a.splits = (int)splits;
    a.chunks_per_split = (int)cps;
    a.total_chunks = (int)chunks;
    a.ant_groups = AG;
    a.blocks_per_wg = (int)bpw;
    a.num_tiles = (int)tiles;
    a.Ltot = L;
    a.flags = call.flags;
    a.keep_l2 = c.keep_l2 >= 0 ? c.keep_l2 : (KG > 1 && sig->chan_stride == 0);
    a.n_vec = (int)(vec == 4 ? N - N % spv : N);
    a.align_head = align_head ? 1 : 0;
    // replica fill by quads: where two channels share a wave's samples (the 2 x 2 tile) the fill's instructions are on the critical
    // resource; the one-channel tiles measured no gain (option dc_quads: -1 by rule, 0 never, 1 wherever the code rate allows)
    a.fill_quads = dc_fill_quads(aw, kt, nw) && (c.quads >= 0 ? c.quads : 1) ? 1 : 0;
    a.max_abs_shift = (int)max_shift;

    DcLaunch cfg{};
    cfg.ant_tile = MT;
    cfg.aw = aw;
    cfg.kt = kt;
    cfg.nw = nw;
    cfg.vec = vec;
    cfg.format = fmt;
    cfg.grid = (unsigned)grid_wgs;
    // Two register sets of samples (steps c+1 and c+2 in flight): the streaming regime of the four-antenna <= 3-tap tile
    // only -- every byte read once (one channel group), a workgroup owns whole blocks (no split), >= 2 steps per block.
    // (float samples: with int16 / int8 pairs the conversions make the step vector-bound and the third wave per SIMD that
    // the second set costs is worth more: 0.206 -> 0.209 ms, 0.169 -> 0.170 ms)
    const bool deep_ok = !resident && c.max_depth >= 2 && vec == 4 && splits == 1 && KG == 1 && c.keep_l2 != 1 && sig->chan_stride == 0 && chunks >= 2 &&
                         (fmt == GAT_LAYOUT_PLANAR || fmt == GAT_LAYOUT_INTERLEAVED);
    int seg_max = nw == 1 ? c.one_wave_seg : dc_segment_steps((int)chunk, kt, MT);
    if (nw == 4 && c.seg_cap > 0) seg_max = std::max(1, std::min(seg_max, c.seg_cap));

    const int sized = resident ? 1 : taps.groups; // (corr_plan_resident refuses a second group)
    for (int g = 0; g < sized; ++g) {
        p.a[g] = a;
        p.cfg[g] = cfg;
        const Refusal rg = size_tap_group(taps, g, chunk, cps, tab_bytes, seg_max, deep_ok, p.a[g], p.cfg[g]);
        if (rg.code != GAT_OK) return rg;
    }
    p.splits = (int)splits;
    p.finalize = !(call.flags & GAT_FLAG_ATOMIC) && splits > 1;
    // a block length that is no multiple of the load group: the N % spv samples behind the last whole group are added
    // by dc_tail_kernel, one more (tiny) launch behind the vector kernel and its second stage
    p.tail = vec == 4 && N % spv != 0;
    const DcLaunch &last = p.cfg[sized - 1];
    p.info = {(int32_t)last.grid, 64 * nw, (int32_t)splits, MT * aw, vec, (int32_t)last.lds_bytes, p.finalize ? 1 : 0, 0, kt, (int32_t)bpw, last.depth, 0};
    return kPlanned;
}

// The launch plan of a validated call: a value that touches neither the device nor the context.
inline Refusal corr_plan(const CorrKnobs &c, const CorrTables &t, const CorrCall &call, CorrPlan &p)
{
    CorrTaps taps;
    corr_sort_taps(call, taps);
    p.groups = taps.groups;
    const CorrLoads ld = corr_pick_loads(c, call.sig, call.B);
    const Refusal r = plan_matrix(c, t, call, taps, ld, p);
    return r.code != GAT_OK || p.kind ? r : plan_vector(c, t, call, taps, ld, 0, p);
}

// The resident correlator's launch plan (gat_resident_open): the call's validation and every restriction of a resident
// launch.  a, cfg: the arguments and geometry of the ONE vector launch that would serve the call -- one block, 16-byte
// aligned, no tail; four-wave workgroups, one antenna tile and one channel each (the resident instances), about max_wgs
// of them.  GAT_ERR_UNSUPPORTED where the call is no such launch.
inline Refusal corr_plan_resident(const CorrKnobs &c, const CorrTables &t, const gat_signal_desc *sig, int32_t K, int32_t L, const int32_t *shifts, double fs,
                                  long long max_wgs, DcArgs *a, DcLaunch *cfg)
{
    const CorrCall call{sig, nullptr, nullptr, 1, K, L, shifts, fs, nullptr, nullptr, 0u};
    Refusal r = corr_check_call(t, call);
    if (r.code != GAT_OK) return r;
    CorrPlan p;
    CorrTaps taps;
    corr_sort_taps(call, taps);
    p.groups = taps.groups;
    r = plan_vector(c, t, call, taps, corr_pick_loads(c, sig, 1), max_wgs, p);
    if (r.code != GAT_OK) return r;
    *a = p.a[0];
    *cfg = p.cfg[0];
    if (p.groups > 1) return {GAT_ERR_UNSUPPORTED, "resident correlator: the taps need more than one launch"};
    if (cfg->vec != 4 || p.tail) return {GAT_ERR_UNSUPPORTED, "resident correlator: block starts must be 16-byte aligned and num_samples a multiple of the load group"};
    if (cfg->depth != 1 || cfg->nw != 4) return {GAT_ERR_UNSUPPORTED, "resident correlator: no instance for this geometry"};
    if (!dc_resident_instance(cfg->ant_tile, cfg->taps)) return {GAT_ERR_UNSUPPORTED, "resident correlator: no kernel instance for this shape"};
    a->keep_l2 = 0; // the resident instances read the signal with non-temporal loads
    return kPlanned;
}

} // namespace gat
