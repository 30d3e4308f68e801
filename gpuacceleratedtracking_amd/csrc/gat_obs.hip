// gat_obs.hip -- the observables' kernels (include/gat.h gat_observables) for gfx950.  The arithmetic is gat_obs.h (the host twin
// runs the same text), the geometry and the scratch layout gat_obs_plan.h.
//
// Two exact integer prefix sums over B x K records of 40 bytes and a gather at the epochs: memory-bound.  A workgroup is rows x
// lanes over one chunk of blocks and one group of channels; the lanes of a row read consecutive records, a thread walks its run
// of consecutive blocks and keeps the record it read as the next block's predecessor.
//   obs_sum_kernel      forms w, c and the bad flag of every block, keeps every thread's run sums in the scratch and adds them
//                       per channel through LDS in row order: the chunk's totals.
//   obs_channel_kernel  a wave a channel: scans the chunk totals into exclusive prefixes, reads n at the frame block and at epoch
//                       0 (the chunk's prefix plus the wraps of the chunk's blocks before it), resolves the channel's record.
//   obs_anchor_kernel   one wave: the anchor of the reception times.
//   obs_epoch_kernel    the sum kernel's walk again from the chunk's prefix plus the run sums of the rows before, writing the
//                       epochs it passes.
// Integers only in every sum, no atomics: the same bits every call.
#include "gat_obs_kernels.h"

namespace gat {

namespace {

struct ObsWhere {
    int chunk, k, kg, lane, row;
};
__device__ inline ObsWhere obs_where(const ObsArgs &a)
{
    ObsWhere w;
    int gi;
    obs_workgroup(a.groups, blockIdx.x, &w.chunk, &gi);
    obs_thread(a.lanes, (int)threadIdx.x, &w.lane, &w.row);
    w.kg = obs_group_channels(a.rule.K, a.group, gi);
    w.k = gi * a.group + w.lane;
    return w;
}

__global__ __launch_bounds__(kObsThreads) void obs_sum_kernel(ObsArgs a)
{
    __shared__ ObsSum lds_sum[kObsThreads];
    __shared__ int32_t lds_bad[kObsThreads];
    const ObsRule &o = a.rule;
    const ObsWhere at = obs_where(a);
    const size_t K = (size_t)o.K;
    ObsSum s{0, 0};
    bool bad = false;
    long long i0, i1;
    if (at.lane < at.kg && obs_run(o.B, a.run, at.chunk, at.row, &i0, &i1)) {
        gat_channel_params cur = a.hist[(size_t)i0 * K + at.k];
        int e;
        for (long long i = i0; i < i1; ++i) {
            const gat_channel_params nxt = a.hist[(size_t)(i + 1) * K + at.k];
            if (!obs_record_finite(cur)) bad = true;
            if (obs_epoch_at(o, i, &e) && !obs_tau_inside(o, cur.code_phase_chips)) bad = true;
            int64_t w, c;
            obs_wraps(o, cur, nxt, &w, &c, &bad);
            s.w += w, s.c += c;
            cur = nxt;
        }
        if (i1 == o.B) { // the last run owns record B
            if (!obs_record_finite(cur)) bad = true;
            if (obs_epoch_at(o, i1, &e) && !obs_tau_inside(o, cur.code_phase_chips)) bad = true;
        }
    }
    const int t = (int)threadIdx.x;
    lds_sum[t] = s;
    lds_bad[t] = bad ? 1 : 0;
    a.runs[(size_t)blockIdx.x * kObsThreads + t] = s;
    __syncthreads();
    if (t < at.kg) { // row 0: t is the lane
        ObsSum tot{0, 0};
        int32_t b = 0;
        for (int r = 0; r < a.rows; ++r) {
            const ObsSum v = lds_sum[r * a.lanes + t];
            tot.w += v.w, tot.c += v.c;
            b |= lds_bad[r * a.lanes + t];
        }
        a.totals[(size_t)at.chunk * K + at.k] = tot;
        a.bad[(size_t)at.chunk * K + at.k] = b;
    }
}

__device__ inline int64_t obs_wave_sum(int64_t v)
{
    for (int d = kObsWave / 2; d > 0; d /= 2) v += __shfl_xor((long long)v, d, kObsWave);
    return v;
}

// n (the code periods) below record `target` of channel k, before the totals become prefixes: the exclusive prefix of the chunk
// from the lane that owns it, plus the wraps of the chunk's blocks below the record.  The same value in every lane.
__device__ inline int64_t obs_wave_n(const ObsArgs &a, int k, long long target, int per, int lane, int64_t lane_excl_w)
{
    const ObsRule &o = a.rule;
    const size_t K = (size_t)o.K;
    const int cg = obs_chunk_of(a.chunks, target), owner = cg / per;
    int64_t pre = lane_excl_w;
    if (lane == owner)
        for (int c = owner * per; c < cg; ++c) pre += a.totals[(size_t)c * K + k].w;
    pre = __shfl((long long)pre, owner, kObsWave);
    int64_t part = 0;
    for (long long i = (long long)cg * kObsChunk + lane; i < target; i += kObsWave) {
        int64_t w, c;
        bool bad = false;
        obs_wraps(o, a.hist[(size_t)i * K + k], a.hist[(size_t)(i + 1) * K + k], &w, &c, &bad);
        part += w;
    }
    return pre + obs_wave_sum(part);
}

__global__ __launch_bounds__(kObsWave *kObsChanWaves) void obs_channel_kernel(ObsArgs a)
{
    const ObsRule &o = a.rule;
    const int wave = (int)threadIdx.x / kObsWave, lane = (int)threadIdx.x % kObsWave;
    const long long kk = (long long)blockIdx.x * kObsChanWaves + wave;
    if (kk >= o.K) return; // the whole wave: no barrier follows
    const int k = (int)kk;
    const size_t K = (size_t)o.K;
    // the lane's chunks and their sum; the lanes' exclusive scan
    const int per = (a.chunks + kObsWave - 1) / kObsWave;
    const int c0 = lane * per < a.chunks ? lane * per : a.chunks, c1 = c0 + per < a.chunks ? c0 + per : a.chunks;
    ObsSum s{0, 0};
    int bad_i = 0;
    for (int c = c0; c < c1; ++c) {
        const ObsSum v = a.totals[(size_t)c * K + k];
        s.w += v.w, s.c += v.c;
        bad_i |= a.bad[(size_t)c * K + k];
    }
    ObsSum incl = s;
    for (int d = 1; d < kObsWave; d *= 2) {
        const int64_t uw = __shfl_up((long long)incl.w, d, kObsWave), uc = __shfl_up((long long)incl.c, d, kObsWave);
        if (lane >= d) incl.w += uw, incl.c += uc;
    }
    const ObsSum excl{incl.w - s.w, incl.c - s.c};
    const bool bad = __ballot(bad_i != 0) != 0;

    const ObsSync sync = obs_sync(o, a.mon[k], a.nav[k], a.frames + (size_t)k * (size_t)o.max_frames);
    const bool inside = sync.synced && !(sync.status & GAT_OBS_FRAME_OUTSIDE);
    const int64_t n_g = inside ? obs_wave_n(a, k, sync.g, per, lane, excl.w) : 0;
    const double tau_g = inside ? a.hist[(size_t)sync.g * K + k].code_phase_chips : 0.0;
    const int64_t n_first = obs_wave_n(a, k, o.first, per, lane, excl.w);
    const gat_obs_channel ch = obs_channel(o, sync, bad, n_g, tau_g);
    ObsChan c{};
    c.status = ch.status, c.frame0_ms = ch.frame0_ms, c.pstar = ch.edge_period;
    obs_tx(o, c, a.hist[(size_t)o.first * K + k], n_first, &c.tx0_ms, &c.tx0_frac);
    if (lane == 0) {
        a.chan[k] = c;
        if (a.out.channels) a.out.channels[k] = ch;
    }
    // the totals become exclusive prefixes (every n above is read: the shuffles of obs_wave_n are behind us)
    ObsSum run = excl;
    for (int c2 = c0; c2 < c1; ++c2) {
        const ObsSum v = a.totals[(size_t)c2 * K + k];
        a.totals[(size_t)c2 * K + k] = run;
        run.w += v.w, run.c += v.c;
    }
}

// a lane's candidate for the anchor
struct ObsCand {
    int k; // -1: none
    int32_t ms;
    double frac;
};
__device__ inline ObsCand obs_cand_shfl_xor(const ObsCand &c, int d)
{
    ObsCand r;
    r.k = __shfl_xor(c.k, d, kObsWave);
    r.ms = __shfl_xor(c.ms, d, kObsWave);
    r.frac = __shfl_xor(c.frac, d, kObsWave);
    return r;
}

__global__ __launch_bounds__(kObsWave) void obs_anchor_kernel(ObsArgs a)
{
    const ObsRule &o = a.rule;
    const int lane = (int)threadIdx.x;
    if (o.rx_mode == GAT_OBS_RX_GIVEN) {
        if (lane == 0) *a.anchor = ObsAnchor{o.rx0_ms, 0, o.rx0_frac};
        return;
    }
    // the first measured channel
    int first = 0x7fffffff;
    for (int k = lane; k < o.K; k += kObsWave)
        if (a.chan[k].tx0_ms >= 0) {
            first = k;
            break;
        }
    for (int d = kObsWave / 2; d > 0; d /= 2) {
        const int other = __shfl_xor(first, d, kObsWave);
        first = other < first ? other : first;
    }
    if (first == 0x7fffffff) {
        if (lane == 0) *a.anchor = ObsAnchor{-1, o.first, 0.0};
        return;
    }
    const int32_t ref_ms = a.chan[first].tx0_ms;
    // the latest of the lane's channels, the lowest on a tie; then of the lanes'
    ObsCand best{-1, 0, 0.0};
    for (int k = lane; k < o.K; k += kObsWave) {
        const ObsChan c = a.chan[k];
        if (c.tx0_ms < 0) continue;
        if (best.k < 0 || obs_later(ref_ms, c.tx0_ms, c.tx0_frac, best.ms, best.frac)) best = ObsCand{k, c.tx0_ms, c.tx0_frac};
    }
    for (int d = kObsWave / 2; d > 0; d /= 2) {
        const ObsCand other = obs_cand_shfl_xor(best, d);
        const bool take = other.k >= 0 && (best.k < 0 || obs_later(ref_ms, other.ms, other.frac, best.ms, best.frac) ||
                                           (!obs_later(ref_ms, best.ms, best.frac, other.ms, other.frac) && other.k < best.k));
        if (take) best = other;
    }
    if (lane == 0) *a.anchor = obs_anchor_from(o, best.ms, best.frac);
}

__global__ __launch_bounds__(kObsThreads) void obs_epoch_kernel(ObsArgs a)
{
    __shared__ ObsSum lds_sum[kObsThreads];
    const ObsRule &o = a.rule;
    const ObsWhere at = obs_where(a);
    const size_t K = (size_t)o.K;
    lds_sum[threadIdx.x] = a.runs[(size_t)blockIdx.x * kObsThreads + threadIdx.x];
    __syncthreads();
    long long i0, i1;
    if (!(at.lane < at.kg && obs_run(o.B, a.run, at.chunk, at.row, &i0, &i1))) return;
    ObsSum base = a.totals[(size_t)at.chunk * K + at.k];
    for (int r = 0; r < at.row; ++r) {
        const ObsSum v = lds_sum[r * a.lanes + at.lane];
        base.w += v.w, base.c += v.c;
    }
    const ObsChan ch = a.chan[at.k];
    const bool writes_rx = at.k == 0 && (a.out.rx_ms || a.out.rx_frac);
    const ObsAnchor an = writes_rx ? *a.anchor : ObsAnchor{-1, 0, 0.0};
    auto emit = [&](long long i, const gat_channel_params &r) {
        int e;
        if (!obs_epoch_at(o, i, &e)) return;
        obs_emit(o, a.out, ch, r, e, at.k, base.w, base.c);
        if (writes_rx) {
            int32_t ms;
            double frac;
            obs_rx(o, an, e, &ms, &frac);
            if (a.out.rx_ms) a.out.rx_ms[e] = ms;
            if (a.out.rx_frac) a.out.rx_frac[e] = frac;
        }
    };
    gat_channel_params cur = a.hist[(size_t)i0 * K + at.k];
    for (long long i = i0; i < i1; ++i) {
        const gat_channel_params nxt = a.hist[(size_t)(i + 1) * K + at.k];
        emit(i, cur);
        int64_t w, c;
        bool bad = false;
        obs_wraps(o, cur, nxt, &w, &c, &bad);
        base.w += w, base.c += c;
        cur = nxt;
    }
    if (i1 == o.B) emit(i1, cur); // the last run owns record B
}

} // namespace

hipError_t launch_obs(const ObsArgs &a, const ObsPlan &p, hipStream_t st)
{
    if (p.chunk_groups < 1 || p.chunk_groups > 0x7fffffffll || p.chan_groups < 1 || p.chan_groups > 0x7fffffffll) return hipErrorInvalidValue;
    hipLaunchKernelGGL(obs_sum_kernel, dim3((unsigned)p.chunk_groups), dim3(kObsThreads), 0, st, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(obs_channel_kernel, dim3((unsigned)p.chan_groups), dim3(kObsWave * kObsChanWaves), 0, st, a);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(obs_anchor_kernel, dim3(1), dim3(kObsWave), 0, st, a);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(obs_epoch_kernel, dim3((unsigned)p.chunk_groups), dim3(kObsThreads), 0, st, a);
    return hipGetLastError();
}

} // namespace gat
