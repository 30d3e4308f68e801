// gat_ctx.h -- what the translation units of the C-ABI layer share: the context, error helpers, the entry preamble, scratch and
// graph housekeeping, the planner's entry points.  The layer: gat_api.cpp (contexts, operators, options, the closed loop),
// gat_planner.cpp (the correlator call: the enqueue of what the pure plan of gat_corr_plan.h plans from the context's knobs
// -- gat_ctx::knobs -- and tables -- corr_tables), gat_group.cpp (device groups), gat_resident_api.cpp (the resident
// correlator's host side), gat_acq_api.cpp (acquisition), gat_array_api.cpp (antenna arrays), gat_beam_api.cpp (beams of the raw
// samples), gat_cond_api.cpp (sample conditioning), gat_st_api.cpp (space-time processing).  What the operators over raw samples
// share is gat_sig_plan.h (through gat_internal.h); the work split of those that reduce blocks to estimates is gat_est_plan.h, filled
// in by the pure plans cov_plan (gat_array_plan.h), stats_plan (gat_cond_plan.h) and st_cov_plan (gat_st_plan.h) and walked by
// enqueue_estimates below.  What the two acquisition searches (gat_acq_api.cpp, gat_acq_fft_api.cpp) share is a header of its own,
// gat_acq_frame.h: the checks before planning, the common kernel arguments and the frame around each search's launches, over the
// pure plans of gat_acq_plan.h and gat_acq_fft_plan.h.  Which host-resident channel record an entry point accepts is gat_chan_rules.h
// (pure: the negation of the predicates the kernels poison with); how gat_set_codes lays a table out is gat_code_tables.h.
#pragma once

#include <cmath>
#include <string>
#include <vector>

#include "gat_chan_rules.h"  // the host's checks of channel records: the negation of the kernels' predicates
#include "gat_code_tables.h" // the layout behind d_codes and d_code_bits
#include "gat_est_plan.h"  // the launches that enqueue_estimates walks
#include "gat_internal.h"

struct gat_ctx;

// A resident correlator (gat_resident_open): one bounded-lifetime kernel serving single-block calls rung in through
// pinned host memory (gat_resident.h).  Owned by its context's list until gat_resident_close.
struct gat_resident {
    gat_ctx *ctx = nullptr;
    hipStream_t stream = nullptr;  // its own non-blocking stream: the kernel runs next to the context's work
    gat::DcArgs a{};
    gat::DcLaunch cfg{};
    gat::ResidentArgs r{};
    unsigned char *h_block = nullptr; // pinned: doorbell lines | state | result lines
    unsigned *h_bell = nullptr, *h_state = nullptr, *h_lines = nullptr, *h_init = nullptr;
    unsigned *d_quit = nullptr;       // device: the master's "I am leaving" word | eight forwarded doorbells
    unsigned *d_bell = nullptr;       // device (fine-grained, host-writable through the BAR): the doorbell's copies, or null: it is in h_block
    int bell_copies = 1;
    int wgs = 0, lines_per_wg = 0, nval = 0; // working workgroups, result lines and values of each
    int blocks_per_cu = 1;                   // workgroups of its kernel instance one compute unit holds at once
    std::vector<int> val_src, val_dst; // value pair (re, im) i of a workgroup: word of its lines holding re | tap * M + antenna of the tile it adds to
    unsigned seq = 0;                 // sequence number of the last call
    bool running = false;             // a kernel was started and has not been seen to end
    bool stale = false;               // the code table changed: the correlator has to be opened again
    int K = 0, L = 0, M = 0, spv = 1;
    long long N = 0;
    double fs = 0.0;
    uint32_t idle_us = 0, life_ms = 0, max_calls = 0;
    long long ticks_per_us = 100;
    unsigned last_exit = 0;
    uint64_t launches = 0, calls = 0;
};

struct gat_ctx {
    std::vector<gat_resident *> residents; // open resident correlators (parked before device-wide waits)
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    int8_t *d_codes = nullptr;
    // gat_tracking_run with GAT_FLAG_GRAPH: the launch sequence of the last such call, instantiated (replayed when the
    // next call has the same arguments: a receiver cycling through one ring buffer).  Which members of the context a
    // recorded launch bakes in is known in ONE place, key_put_ctx (gat_api.cpp): whatever changes one of them without
    // being part of that key must call drop_loop_graphs.
    struct LoopGraph {
        std::vector<unsigned char> key;
        hipGraphExec_t exec = nullptr;
        unsigned long long last_use = 0;
    };
    std::vector<LoopGraph> loop_graphs; // small LRU (kMaxLoopGraphs): e.g. the a/b parameter order of odd block counts
    unsigned long long loop_graph_clock = 0;
    void *d_zeros = nullptr;         // 64 zero bytes (out-of-range sample loads of the split-bf16 kernel read these)
    uint32_t *d_code_bits = nullptr; // bit i of row p = (chip i of PRN p is -1); only when every chip is +-1
    int code_bits_stride = 0;        // dwords per row, a multiple of 4
    int Lc = 0, P = 0, code_row_stride = 0; // rows padded to a multiple of 16 bytes
    float *d_partial = nullptr;
    size_t partial_bytes = 0;
    // completion flag (latency regime): small launches of the vector kernel end by storing a sequence number into pinned
    // host memory; gat_sync spins on it instead of going through hipStreamSynchronize (~5 us sooner)
    unsigned *h_flag = nullptr;      // pinned, host address
    unsigned *d_flag = nullptr;      // the same word, device address
    unsigned *d_done = nullptr;      // device: arrival counter of a launch's workgroups
    unsigned flag_seq = 0;           // last sequence number handed to a launch
    unsigned wait_seq = 0;           // != 0: the newest work on the stream is a flagged launch with this number
    int flag_max_wgs = 1024;         // option sync_flag_wgs
    gat_channel_params *d_params = nullptr; // parameter scratch: the records of a host call, the tap list of gat_downconvert_and_accumulate
    size_t params_bytes = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool timer_running = false;
    std::vector<hipEvent_t> lap_events; // gat_timer_lap: pool, grows to the most laps ever outstanding
    size_t laps = 0;                    // laps recorded since the last gat_timer_laps
    int num_cus = 256;
    gat::CorrKnobs knobs; // the correlator plan's kernel-selection and launch-geometry options (gat_corr_plan.h; kOptions of gat_api.cpp)
    int acq_fft_log2 = 0, acq_fft_dbatch = 0, acq_fft_ubatch = 0; // options acq_fft_log2 / acq_fft_doppler_batch / acq_fft_unit_batch (0: the plan's choice)
    std::string err;
    gat_launch_info last{};
};

namespace gat {

inline int32_t fail(gat_ctx *c, int32_t code, const char *msg)
{
    if (c) c->err = msg;
    return code;
}

inline int32_t hipfail(gat_ctx *c, hipError_t e, const char *where)
{
    if (c) {
        c->err = std::string(where) + ": " + hipGetErrorString(e);
    }
    return -(int32_t)e;
}

#define GAT_HIP(c, call)                                      \
    do {                                                      \
        hipError_t e_ = (call);                               \
        if (e_ != hipSuccess) return hipfail((c), e_, #call); \
    } while (0)

// Tracing ranges around the library's launch sequences (the reference wraps every launch of kernel_algorithm in
// NVTX.@range, src/algorithms.jl:953 ...): roctxRangePush / Pop, resolved at the first use (gat_api.cpp).  RAII; a null
// name opens nothing.
struct TraceRange {
    explicit TraceRange(const char *name);
    ~TraceRange();
    TraceRange(const TraceRange &) = delete;
    TraceRange &operator=(const TraceRange &) = delete;
    const void *rx;
};

// The start of every entry point that enqueues on the context's stream, AFTER its validation (a refused call leaves
// wait_seq alone), in this order: select the device; clear wait_seq -- what follows is newer work than a flagged launch,
// so gat_sync must wait on the stream (spinning on the older launch's flag would return before the newer work is done) --;
// open the trace range `range` of the calling scope (null: the entry point has none).  No allocation: this is on the path
// of the single-block latency.  Entry points that enqueue nothing keep a bare hipSetDevice.
#define GAT_ENTER(c, range)                \
    GAT_HIP(c, hipSetDevice(c->device));   \
    (c)->wait_seq = 0;                     \
    const gat::TraceRange trace_(range)

// scratch and graph housekeeping shared by the planner, the operators and the loop (gat_api.cpp)
void drop_loop_graphs(gat_ctx *c);
// Room for `bytes` in a library-owned device buffer; in_graphs: recorded graphs bake its pointer in and go when it moves.
int32_t grow_scratch(gat_ctx *c, void **buf, size_t *cap_bytes, size_t bytes, bool in_graphs);
inline int32_t ensure_partial(gat_ctx *c, size_t bytes) { return grow_scratch(c, reinterpret_cast<void **>(&c->d_partial), &c->partial_bytes, bytes, true); }
inline int32_t ensure_params(gat_ctx *c, size_t bytes) { return grow_scratch(c, reinterpret_cast<void **>(&c->d_params), &c->params_bytes, bytes, false); }
int32_t upload_params(gat_ctx *c, const gat_channel_params *params_host, size_t n);

// The enqueue loop of the operators that reduce blocks to estimates (gat_spatial_covariance, gat_sample_stats,
// gat_spacetime_covariance).  What CovArgs and StatsArgs share, for launch t of a plan over sig: the planes from the launch's first block on.
template <class Args>
Args estimate_args(const gat_signal_desc *sig, const EstimateLaunches &t)
{
    const size_t off = block_offset_bytes(sig, t.b0);
    Args a{};
    a.re = static_cast<const char *>(sig->re) + off;
    a.im = sig->im ? static_cast<const char *>(sig->im) + off : nullptr;
    a.M = sig->num_ants;
    a.B = t.bn;
    a.bpe = t.bpe;
    a.E = t.en;
    a.G = (int)t.G;
    a.splits = (int)t.splits;
    a.N = t.plan.N;
    a.ant_stride = sig->ant_stride;
    a.block_stride = sig->block_stride;
    a.seg_len = t.seg_len;
    return a;
}
// Walks the plan's launches: room for each one's slices in c->d_partial, then launch(args, t) enqueues its kernel and its finish
// (what it returns but GAT_OK ends the walk).
template <class Args, class F>
int32_t enqueue_estimates(gat_ctx *c, const gat_signal_desc *sig, const EstimatePlan &plan, F &&launch)
{
    for (EstimateLaunches t(plan); t.next();) {
        int32_t rc = ensure_partial(c, t.scratch_bytes);
        if (rc == GAT_OK) rc = launch(estimate_args<Args>(sig, t), t);
        if (rc != GAT_OK) return rc;
    }
    return GAT_OK;
}
// What gat_last_launch_info reports after an entry point whose launch is told by these five: scalar loads (vec 1), the rest zero.
inline void set_last_launch(gat_ctx *c, long long workgroups, int32_t threads, int32_t splits, int32_t ant_tile, int32_t lds_bytes)
{
    c->last = gat_launch_info{};
    c->last.workgroups = (int32_t)workgroups;
    c->last.threads = threads;
    c->last.splits = splits;
    c->last.ant_tile = ant_tile;
    c->last.vec = 1;
    c->last.lds_bytes = lds_bytes;
}
// validation of a loop configuration (gat_tracking_update and the weighted update)
int32_t check_loop_config(gat_ctx *c, const gat_loop_config *cfg);

// Where the closed loop's block b reads its records and writes its successor's: the ping-pong pair alternating (b set; block 0
// reads a), or rows b and b + 1 of one array of K records a row (b null: the history run).
struct LoopRecords {
    gat_channel_params *a, *b;
    gat_channel_params *of(int32_t block, int32_t K) const { return b ? ((block & 1) ? b : a) : a + (size_t)block * (size_t)K; }
};
// The closed loop's block sequence (gat_api.cpp), the one enqueue of gat_tracking_run, gat_tracking_run_weighted and
// gat_tracking_run_history: per block the correlator call, then gat_tracking_update_weighted (w_re / w_im null: gat_tracking_update).
int32_t tracking_run_enqueue(gat_ctx *c, const gat_signal_desc *sig, int32_t num_blocks, int32_t K, int32_t L, const int32_t *shifts, double fs,
                             const gat_loop_config *cfg, gat_loop_state *state, LoopRecords rec, float *acc_re, float *acc_im,
                             int64_t acc_block_stride, uint32_t flags, const double *w_re, const double *w_im);
// gat_tracking_run and gat_tracking_run_weighted (gat_array_api.cpp): validation, the eager sequence, the graph cache; w_re / w_im
// (null: the unweighted run) belong to the key of a recorded graph.
int32_t tracking_run_shared(gat_ctx *c, const gat_signal_desc *sig, int32_t num_blocks, int32_t K, int32_t L, const int32_t *shifts,
                            double fs, const gat_loop_config *cfg, gat_loop_state *state, gat_channel_params *params_a,
                            gat_channel_params *params_b, float *acc_re, float *acc_im, int64_t acc_block_stride, uint32_t flags,
                            int32_t *current_is_b, const double *w_re, const double *w_im);

// params_dev: [B*K] records on the device -- or null with params_inline: B*K <= kInlineParams validated HOST records that
// travel inside the vector kernel's arguments (uploaded after all if a matrix-core kernel takes the call)
int32_t correlate_impl(gat_ctx *c, const gat_signal_desc *sig, const gat_channel_params *params_dev, int32_t B, int32_t K, int32_t L,
                       const int32_t *shifts, double fs, float *out_re, float *out_im, uint32_t flags,
                       const gat_channel_params *params_inline = nullptr);
// what the correlator plans (corr_plan, corr_plan_resident: gat_corr_plan.h) read of the context besides its knobs, built per call
inline CorrTables corr_tables(const gat_ctx &c)
{
    return {c.d_codes, c.d_code_bits, c.d_zeros, c.Lc, c.P, c.code_row_stride, c.code_bits_stride, c.num_cus};
}
// the context's resident correlators (gat_resident_api.cpp): asked to leave before anything that waits for the whole device
// (hipFree, a new code table, the context's end); freed with the context
void park_residents(gat_ctx *c);
void resident_free(gat_resident *res);

} // namespace gat
