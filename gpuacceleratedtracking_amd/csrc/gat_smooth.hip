// gat_smooth.hip -- the carrier smoothing's kernels (include/gat.h gat_smooth_observables) for gfx950.  The arithmetic is
// gat_smooth.h (the host twin runs the same text), the geometry and the scratch layout gat_smooth_plan.h.
//
// Three integer prefix scans over E x K observables (C = scan of q, SS = scan of C, a = max-scan of the arc starts) and a gather:
// memory-bound.  A workgroup is rows x lanes over one chunk of epochs; the lanes of a row read consecutive elements of the [E][K]
// arrays, a thread walks its run of consecutive epochs and keeps the epoch it read as the next one's predecessor.
//   sm_sum_kernel      forms q and the reset flags of every epoch, reduces every thread's run to a segment (gat_smooth.h SmSeg),
//                      keeps it in the scratch and combines the runs per channel through LDS in row order: the chunk's segment.
//   sm_channel_kernel  a wave a channel: scans the chunks' segments into exclusive prefixes and writes the channel's record.
//   sm_emit_kernel     the sum kernel's walk again from the chunk's prefix combined with the runs of the rows before, writing C,
//                      SS and a(e) of every (epoch, channel) to the scratch, and the status.
//   sm_output_kernel   a thread an (epoch, channel): gathers SS at e - n and C at a(e) and writes the outputs.
// Integers only in every sum, no atomics, every store a plain vector store: the same bits every call.
#include "gat_smooth_kernels.h"

namespace gat {

namespace {

// the thread's run of the chunk reduced to a segment; with Emit, the scans written on the way from `base`
template <bool Emit>
__device__ inline SmSeg sm_walk(const SmArgs &a, int lane, int e0, int e1, SmSeg s)
{
    const SmRule &r = a.rule;
    SmEpoch prev = e0 > 0 ? sm_load(r, a.in, a.K, e0 - 1, lane) : SmEpoch{};
    for (int e = e0; e < e1; ++e) {
        const SmEpoch cur = sm_load(r, a.in, a.K, e, lane);
        int64_t q;
        const int st = sm_step(r, e == 0, prev, cur, &q);
        sm_push(&s, e, q, st);
        if (Emit) {
            const size_t o = (size_t)e * (size_t)a.K + (size_t)lane;
            a.C[o] = s.Q, a.SS[o] = s.S, a.arc[o] = cur.measured ? s.reset : -1;
            if (a.out.status) a.out.status[o] = (uint8_t)st;
        }
        prev = cur;
    }
    return s;
}

__global__ __launch_bounds__(kSmThreads) void sm_sum_kernel(SmArgs a)
{
    __shared__ SmSeg lds[kSmThreads];
    const int chunk = (int)blockIdx.x, t = (int)threadIdx.x;
    int lane, row, e0, e1;
    sm_thread(a.lanes, t, &lane, &row);
    SmSeg s = sm_empty();
    if (lane < a.K && sm_run(a.E, a.run, chunk, row, &e0, &e1)) s = sm_walk<false>(a, lane, e0, e1, s);
    lds[t] = s;
    a.runs[(size_t)chunk * kSmThreads + t] = s;
    __syncthreads();
    if (t < a.K) { // row 0: t is the lane
        SmSeg tot = sm_empty();
        for (int r = 0; r < a.rows; ++r) tot = sm_combine(tot, lds[r * a.lanes + t]);
        a.totals[(size_t)chunk * (size_t)a.K + t] = tot;
    }
}

__device__ inline SmSeg sm_shfl_up(const SmSeg &s, int d)
{
    SmSeg r;
    r.Q = (uint64_t)__shfl_up((long long)s.Q, d, kSmWave);
    r.S = (uint64_t)__shfl_up((long long)s.S, d, kSmWave);
    r.len = __shfl_up(s.len, d, kSmWave);
    r.reset = __shfl_up(s.reset, d, kSmWave);
    for (int i = 0; i < 4; ++i) r.cnt[i] = __shfl_up(s.cnt[i], d, kSmWave);
    return r;
}

__global__ __launch_bounds__(kSmWave *kSmChanWaves) void sm_channel_kernel(SmArgs a)
{
    const int wave = (int)threadIdx.x / kSmWave, lane = (int)threadIdx.x % kSmWave;
    const long long kk = (long long)blockIdx.x * kSmChanWaves + wave;
    if (kk >= a.K) return; // the whole wave: no barrier follows
    const int k = (int)kk;
    const size_t K = (size_t)a.K;
    // the lane's chunks and their segment; the lanes' scan
    const int per = (a.chunks + kSmWave - 1) / kSmWave;
    const int c0 = lane * per < a.chunks ? lane * per : a.chunks, c1 = c0 + per < a.chunks ? c0 + per : a.chunks;
    SmSeg s = sm_empty();
    for (int c = c0; c < c1; ++c) s = sm_combine(s, a.totals[(size_t)c * K + k]);
    SmSeg incl = s;
    for (int d = 1; d < kSmWave; d *= 2) {
        const SmSeg u = sm_shfl_up(incl, d);
        if (lane >= d) incl = sm_combine(u, incl);
    }
    SmSeg excl = sm_shfl_up(incl, 1);
    if (lane == 0) excl = sm_empty();
    if (lane == kSmWave - 1 && a.out.channels) a.out.channels[k] = gat_smooth_channel{incl.cnt[0], incl.cnt[1], incl.cnt[2], incl.cnt[3]};
    // the totals become exclusive prefixes
    SmSeg run = excl;
    for (int c = c0; c < c1; ++c) {
        const SmSeg v = a.totals[(size_t)c * K + k];
        a.totals[(size_t)c * K + k] = run;
        run = sm_combine(run, v);
    }
}

__global__ __launch_bounds__(kSmThreads) void sm_emit_kernel(SmArgs a)
{
    __shared__ SmSeg lds[kSmThreads];
    const int chunk = (int)blockIdx.x, t = (int)threadIdx.x;
    int lane, row, e0, e1;
    sm_thread(a.lanes, t, &lane, &row);
    lds[t] = a.runs[(size_t)chunk * kSmThreads + t];
    __syncthreads();
    if (!(lane < a.K && sm_run(a.E, a.run, chunk, row, &e0, &e1))) return;
    SmSeg base = a.totals[(size_t)chunk * (size_t)a.K + lane];
    for (int r = 0; r < row; ++r) base = sm_combine(base, lds[r * a.lanes + lane]);
    sm_walk<true>(a, lane, e0, e1, base);
}

__global__ __launch_bounds__(kSmThreads) void sm_output_kernel(SmArgs a)
{
    int e, k;
    if (!sm_unit(blockIdx.x, (int)threadIdx.x, a.cells, a.K, &e, &k)) return; // no barrier follows
    const size_t K = (size_t)a.K, o = (size_t)e * K + (size_t)k;
    const int arc = a.arc[o];
    const int back = arc < 0 ? -1 : e - sm_count(a.rule, e, arc);
    sm_emit(a.rule, a.out, o, e, a.in.tx_frac[o], arc, a.C[o], a.SS[o], back >= 0 ? a.SS[(size_t)back * K + k] : 0, arc < 0 ? 0 : a.C[(size_t)arc * K + k]);
}

} // namespace

hipError_t launch_smooth(const SmArgs &a, const SmPlan &p, hipStream_t st)
{
    if (p.chunks < 1 || p.chan_groups < 1 || p.chan_groups > 0x7fffffffll || p.out_groups < 1 || p.out_groups > 0x7fffffffll) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sm_sum_kernel, dim3((unsigned)p.chunks), dim3(kSmThreads), 0, st, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(sm_channel_kernel, dim3((unsigned)p.chan_groups), dim3(kSmWave * kSmChanWaves), 0, st, a);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(sm_emit_kernel, dim3((unsigned)p.chunks), dim3(kSmThreads), 0, st, a);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(sm_output_kernel, dim3((unsigned)p.out_groups), dim3(kSmThreads), 0, st, a);
    return hipGetLastError();
}

} // namespace gat
