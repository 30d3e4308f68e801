// corr_launch_contract.h -- what the correlator's kernels ASSUME of a launch (LDS carve-up, replica room, grid decode, descriptor
// spans, tap tables), stated once: the host simulator's stand-in launchers (tests/hostsim/fake_kernels.cpp) and the stand-alone plan
// program (tests/corrplan) check every planned launch against it.  Each check takes the launch's arguments as the launcher gets
// them and `broken`, called with the condition's text and a printf message for every assumption that does not hold (REQUIRE
// calls whatever is named `broken` where it stands: the checks' parameter here, the user's own function in its other checks).
#pragma once

#include "gat_corr_plan.h"

namespace gat {
typedef void (*Broken)(const char *cond, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
#define REQUIRE(cond, ...) do { if (!(cond)) broken(#cond, __VA_ARGS__); } while (0)

inline void check_dc(const DcArgs &a, const DcLaunch &cfg, bool resident, Broken broken)
{
    const int fmt = cfg.format, vec = cfg.vec, nw = cfg.nw, kt = cfg.kt, aw = cfg.aw, MT = cfg.ant_tile, L = cfg.taps;
    const long long chunk = dc_chunk(vec, fmt, aw, nw);
    const int spv = dc_group_samples(vec, fmt);
    const long long plane_bytes = fmt == GAT_LAYOUT_PLANAR ? 4 : fmt == GAT_LAYOUT_INTERLEAVED ? 8 : fmt == GAT_LAYOUT_INTERLEAVED_I16 ? 4 : 2;
    const char *tag = resident ? "resident" : "launch";
    REQUIRE(dc_instance(MT, L, vec, aw, kt, nw, cfg.depth), "%s: no instance <%d,%d,%d,aw %d,kt %d,nw %d,d %d>", tag, MT, L, vec, aw, kt, nw, cfg.depth);
    REQUIRE(a.M % (MT * aw) == 0 && a.ant_groups == a.M / (MT * aw), "%s: antenna tiling M %d MT %d aw %d groups %d", tag, a.M, MT, aw, a.ant_groups);
    REQUIRE(a.KG == (a.K + kt - 1) / kt, "%s: channel groups %d for K %d kt %d", tag, a.KG, a.K, kt);
    REQUIRE(a.splits >= 1 && a.chunks_per_split >= 1 && (long long)a.splits * a.chunks_per_split >= a.total_chunks &&
                (long long)(a.splits - 1) * a.chunks_per_split < a.total_chunks,
            "%s: splits %d x %d chunks for %d", tag, a.splits, a.chunks_per_split, a.total_chunks);
    const long long head = a.align_head ? 112 / plane_bytes : 0;
    REQUIRE((long long)a.total_chunks * chunk >= a.n_vec + (vec == 4 ? head : 0) && (long long)(a.total_chunks - 1) * chunk < a.n_vec + head + chunk,
            "%s: %d chunks of %lld for n_vec %d (+%lld)", tag, a.total_chunks, chunk, a.n_vec, head);
    REQUIRE(a.blocks_per_wg >= 1 && (a.blocks_per_wg == 1 || a.splits == 1), "%s: blocks per workgroup %d with %d splits", tag, a.blocks_per_wg, a.splits);
    const long long BG = (a.B + a.blocks_per_wg - 1) / a.blocks_per_wg;
    REQUIRE(a.num_tiles == BG * a.ant_groups * a.splits && a.total_wgs == (unsigned)(a.num_tiles * a.KG), "%s: tiles %d wgs %u", tag, a.num_tiles, a.total_wgs);
    REQUIRE(cfg.grid % 8 == 0 && cfg.grid >= a.total_wgs && cfg.grid == (unsigned)(((a.num_tiles + 7) / 8) * 8 * a.KG), "%s: grid %u for %d tiles x %d", tag, cfg.grid, a.num_tiles, a.KG);
    REQUIRE(vec == 4 ? (a.n_vec % spv == 0 && a.n_vec <= a.N && a.N - a.n_vec < spv) : a.n_vec == a.N, "%s: n_vec %d of N %lld", tag, a.n_vec, a.N);
    if (vec == 4) {
        REQUIRE(((long long)(MT - 1) * a.ant_stride + a.N) * plane_bytes < (1ll << 31), "%s: tile span beyond a descriptor", tag);
        REQUIRE((reinterpret_cast<uintptr_t>(a.re) & 15u) == 0, "%s: vector loads from an unaligned plane", tag);
        REQUIRE(a.M == 1 || a.ant_stride % spv == 0, "%s: antenna stride %lld", tag, a.ant_stride);
    } else {
        REQUIRE(MT == 1 && aw == 1 && kt == 1, "%s: scalar loads with a tile", tag);
    }
    // taps
    REQUIRE(L >= 1 && L <= kMaxTapsPerLaunch, "%s: %d taps", tag, L);
    for (int l = 1; l < L; ++l) REQUIRE(a.shifts[l] >= a.shifts[l - 1], "%s: taps not ascending", tag);
    REQUIRE(a.rep_span == a.shifts[L - 1] - a.shifts[0] && a.rep_span <= kMaxLaunchSpan, "%s: tap span %d", tag, a.rep_span);
    for (int l = 0; l < L; ++l) {
        const int d = a.shifts[l] - a.shifts[0];
        REQUIRE(a.tap_index[l] >= 0 && a.tap_index[l] < a.Ltot, "%s: tap index %d of %d", tag, a.tap_index[l], a.Ltot);
        REQUIRE(a.tap_off[l] % 2 == 0 && a.tap_off[l] == ((d & 1) ? a.rep_copy_stride + d - 1 : d), "%s: tap offset %d for distance %d", tag, a.tap_off[l], d);
        REQUIRE(!(d & 1) || a.rep_copy_stride > 0, "%s: odd tap distance without the shifted copy", tag);
    }
    // LDS: what the kernel carves must fit what the launch gives it; the replica must hold a segment + taps + the producers' overshoot
    const int threads = 64 * nw, rpc = threads / kt;
    REQUIRE(a.seg_steps >= 1 && a.seg_steps <= kUcarSteps && a.seg_steps % cfg.depth == 0, "%s: %d steps per segment (depth %d)", tag, a.seg_steps, cfg.depth);
    const size_t carve = nw == 1 ? dc_lds_bytes_one_wave(a.rep_chan_floats, a.table_stride) : dc_lds_bytes_floats(kt, a.table_stride, a.rep_chan_floats);
    REQUIRE(carve <= cfg.lds_bytes && cfg.lds_bytes <= 160 * 1024, "%s: LDS carve %zu of %u", tag, carve, cfg.lds_bytes);
    const long long seg_entries = (long long)a.seg_steps * chunk + a.rep_span;
    const long long filled = (seg_entries + rpc - 1) / rpc * rpc; // every producer takes the same number of steps
    if (a.rep_copy_stride) {
        REQUIRE(a.rep_copy_stride >= filled + 1 - 1 && (long long)a.rep_copy_stride - 1 + filled <= a.rep_chan_floats,
                "%s: replica + copy: stride %d, %lld entries, room %d", tag, a.rep_copy_stride, filled, a.rep_chan_floats);
    } else {
        REQUIRE(filled <= a.rep_chan_floats, "%s: replica: %lld entries, room %d", tag, filled, a.rep_chan_floats);
    }
    REQUIRE((long long)a.N + a.max_abs_shift < (1ll << 30), "%s: sample range", tag);
    REQUIRE(a.code_row_stride % 16 == 0 && a.code_row_stride >= a.Lc && a.codes != nullptr, "%s: chip table", tag);
    REQUIRE(a.table_stride % 16 == 0 && (a.code_bits ? a.table_stride * 8 >= a.Lc : a.table_stride == a.code_row_stride), "%s: staged table of %d bytes (%s) for %d chips",
            tag, a.table_stride, a.code_bits ? "sign bits" : "int8", a.Lc);
    if (!resident) {
        REQUIRE(a.params != nullptr || (long long)a.B * a.K <= kInlineParams, "launch: %d x %d records without a buffer", a.B, a.K);
        REQUIRE(a.out_re != nullptr && a.out_im != nullptr, "launch: no outputs");
        REQUIRE(a.splits == 1 || (a.flags & GAT_FLAG_ATOMIC) || a.partial != nullptr, "launch: split without a partial buffer");
        REQUIRE((a.done_counter == nullptr) == (a.host_flag == nullptr) && (a.done_counter == nullptr || a.flag_seq != 0), "launch: completion flag half set");
        REQUIRE(cfg.depth == 1 || (a.splits == 1 && a.KG == 1 && !a.keep_l2), "launch: two sample sets outside the streaming regime");
    } else {
        REQUIRE(a.B == 1 && kt == 1 && aw == 1 && nw == 4 && cfg.depth == 1 && vec == 4 && a.n_vec == a.N && a.K <= kResMaxChannels, "resident: geometry");
    }
}
inline void check_mf_common(const MfArgs &a, unsigned grid, int T, const char *tag, Broken broken)
{
    REQUIRE(a.re && a.params && a.codes && a.out_re && a.out_im, "%s: null pointer", tag);
    REQUIRE(a.total_steps == (a.N + T - 1) / T && a.steps_per_split >= 1 && (long long)a.splits * a.steps_per_split >= a.total_steps &&
                (long long)(a.splits - 1) * a.steps_per_split < a.total_steps,
            "%s: %d splits x %d steps for %d", tag, a.splits, a.steps_per_split, a.total_steps);
    REQUIRE(a.num_tiles == a.B * a.ant_tiles * a.splits && grid == (unsigned)(((a.num_tiles + 7) / 8) * 8 * a.chan_groups), "%s: tiles %d grid %u", tag, a.num_tiles, grid);
    REQUIRE(a.splits == 1 || (a.flags & GAT_FLAG_ATOMIC) || a.partial != nullptr, "%s: split without a partial buffer", tag);
    REQUIRE(a.L >= 1 && a.L <= kMfmaMaxTaps && a.rep_span == a.shifts[a.L - 1] - a.shifts[0] && a.rep_span <= kMfmaMaxSpan, "%s: taps %d span %d", tag, a.L, a.rep_span);
    for (int l = 1; l < a.L; ++l) REQUIRE(a.shifts[l] >= a.shifts[l - 1], "%s: taps not ascending", tag);
    for (int l = 0; l < a.L; ++l) REQUIRE(a.tap_index[l] >= 0 && a.tap_index[l] < a.L, "%s: tap index", tag);
    REQUIRE(a.rep_stride >= T + a.rep_span && (a.rep_stride & 1), "%s: replica row %d for a tile of %d + %d", tag, a.rep_stride, T, a.rep_span);
    REQUIRE((reinterpret_cast<uintptr_t>(a.re) & 15u) == 0 && a.ant_stride % 2 == 0, "%s: alignment", tag);
}
inline void check_mfma(const MfArgs &a, int nct, unsigned grid, unsigned lds_bytes, Broken broken)
{
    REQUIRE((nct == 1 || nct == 2 || nct == 4) && a.CT >= 1 && a.CT == 16 / a.L && nct * a.CT <= 20, "f32 mfma: nct %d CT %d L %d", nct, a.CT, a.L);
    REQUIRE(a.M % 16 == 0 && a.ant_tiles == a.M / 16 && a.im != nullptr, "f32 mfma: antennas %d tiles %d", a.M, a.ant_tiles);
    REQUIRE(a.chan_groups == ((a.K + a.CT - 1) / a.CT + nct - 1) / nct, "f32 mfma: channel groups %d", a.chan_groups);
    REQUIRE(lds_bytes == mf_lds_bytes(nct, a.CT, a.rep_stride, a.code_row_stride, a.codes_in_lds) && lds_bytes <= 160 * 1024, "f32 mfma: LDS %u", lds_bytes);
    check_mf_common(a, grid, kMfTile, "f32 mfma", broken);
}
inline void check_mfma_bf16(const MfArgs &a, int rt, int nct, int fmt, unsigned grid, unsigned lds_bytes, Broken broken)
{
    const bool inst = (rt == 1 || rt == 2 || rt == 4) && (nct == 1 || nct == 2 || nct == 4) && !(rt == 4 && nct == 1);
    REQUIRE(inst && fmt >= 0 && fmt <= 3, "bf16 mfma: instance rt %d nct %d fmt %d", rt, nct, fmt);
    const int T = mb_tile_samples(rt, nct), spv = dc_group_samples(4, fmt);
    REQUIRE(a.M % (16 * rt) == 0 && a.ant_tiles == a.M / (16 * rt), "bf16 mfma: antennas %d rt %d tiles %d", a.M, rt, a.ant_tiles);
    REQUIRE(a.N % spv == 0, "bf16 mfma: N %lld is no multiple of the load group", a.N);
    const int tiles = (2 * a.L * a.K + 31) / 32;
    REQUIRE(a.chan_groups == (tiles + nct - 1) / nct, "bf16 mfma: %d column tiles in %d groups of %d", tiles, a.chan_groups, nct);
    REQUIRE(a.nslots == mb_slots(nct, a.L, a.K) && a.nslots <= kMbMaxSlots && a.nslots * T / 2 <= mb_threads(rt, nct) - 64 * mb_consumer_waves(rt, nct),
            "bf16 mfma: %d slots x %d samples for %d producers", a.nslots, T, mb_threads(rt, nct) - 64 * mb_consumer_waves(rt, nct));
    REQUIRE((long long)a.steps_per_split * T <= kMbMaxChain || a.steps_per_split == 1, "bf16 mfma: chain of %d x %d samples", a.steps_per_split, T);
    REQUIRE(a.code_bits && a.zeros && a.code_bits_stride % 4 == 0 && a.code_bits_stride * 32 >= a.Lc, "bf16 mfma: sign-bit tables");
    REQUIRE(a.mb_mode == mb_mode(rt, nct, fmt) || (fmt == GAT_LAYOUT_INTERLEAVED_I16 && a.mb_mode == kMbThree), "bf16 mfma: operand split %d for layout %d", a.mb_mode, fmt);
    if (mb_rep_ring_rows(rt))
        REQUIRE(a.rep_ring % T == 0 && a.rep_ring >= a.rep_span + 2 * T && a.rep_stride >= a.rep_ring + a.rep_span + T, "bf16 mfma: chip-sign ring %d in rows of %d for span %d, tile %d", a.rep_ring, a.rep_stride, a.rep_span, T);
    else
        REQUIRE(a.rep_ring == 0 && a.rep_stride >= a.rep_span + T, "bf16 mfma: chip-sign rows of %d for span %d, tile %d", a.rep_stride, a.rep_span, T);
    REQUIRE(a.mb_mode != kMbTwo || a.nslots * T / 4 <= mb_threads(rt, nct) - 64 * mb_consumer_waves(rt, nct), "bf16 mfma: two-term items");
    REQUIRE(lds_bytes == mb_lds_bytes(rt, nct, fmt, a.nslots, a.rep_stride, a.code_bits_stride, a.mb_mode) && lds_bytes <= 160 * 1024, "bf16 mfma: LDS %u", lds_bytes);
    check_mf_common(a, grid, T, "bf16 mfma", broken);
}
} // namespace gat
