// gat_nav.hip -- the navigation data layer's kernels (include/gat.h gat_nav_decode) for gfx950.  The arithmetic is gat_nav.h (the host
// twin runs the same text), the geometry and the decoding of a work unit gat_nav_plan.h.  Everything but the quantiser's scale is
// integer arithmetic, and that scale meets the same operands in the same order whichever lane holds them: no atomics, no
// data-dependent order.
//
// The trellis is the hot path.  One wave runs a (channel, phase) pair and lane s holds the metric of state s.  A step is a
// dependent chain -- two cross-lane reads of the predecessors' metrics (ds_bpermute through __shfl, the index vectors constant),
// an add each, a compare and a select -- and its 64 survivor decisions are one __ballot word.  The symbols of 64 steps are loaded
// once, a pair a lane, and handed to the step by v_readlane; the 64 survivor words of those steps gather across the lanes (lane i
// keeps the word of step i) and leave in one coalesced 512-byte store.  The traceback reloads 64 words a time the same way and
// walks them with the state in scalar registers (the state is wave-uniform), so no step waits for memory; the 64 bits of a chunk
// leave in one coalesced store.  The occupancy is 2 K waves, one to a workgroup so that they spread over the compute units.
#include "gat_nav_kernels.h"

namespace gat {

namespace {

__device__ inline long long nav_thread() { return (long long)blockIdx.x * kNavThreads + threadIdx.x; }

// LNAV, one thread per (k, j): the hard bit, 0 beyond the channel's symbols
__global__ __launch_bounds__(kNavThreads) void nav_slice_kernel(NavArgs a)
{
    const long long t = nav_thread();
    if (t < a.K && a.path_metric) a.path_metric[t] = 0;
    int k, j;
    if (!nav_slice_unit(t, a.cap, a.K, &k, &j)) return;
    const int n = nav_symbols(a.mon, k, a.cap);
    a.decoded[t] = (uint8_t)(j < n ? nav_lnav_bit(a.sym_re[t]) : 0);
}

// CNAV, one wave per channel: lane l adds |x[l]|, |x[l + 64]|, ..; every lane adds the 64 partial sums in lane order
__global__ __launch_bounds__(kNavWave) void nav_quantise_kernel(NavArgs a)
{
    const int k = blockIdx.x, lane = threadIdx.x;
    const int n = nav_symbols(a.mon, k, a.cap);
    const double *x = a.sym_re + (size_t)k * a.cap;
    int8_t *q = a.q + (size_t)k * a.cap;
    double s = 0.0;
    for (int j = lane; j < n; j += kNavWave) s += nav_abs(x[j]);
    double S = 0.0;
    for (int l = 0; l < kNavWave; ++l) S += __shfl(s, l);
    const double unit = S / (double)n;
    for (int j = lane; j < a.cap; j += kNavWave) q[j] = (int8_t)(j < n ? nav_quantise(x[j], unit) : 0);
}

// CNAV, one wave per (k, ph): the forward pass, the final state, the traceback
__global__ __launch_bounds__(kNavWave) void nav_trellis_kernel(NavArgs a)
{
    const int k = blockIdx.x >> 1, ph = blockIdx.x & 1, lane = threadIdx.x;
    const int n = nav_symbols(a.mon, k, a.cap);
    const int T = nav_bits(GAT_NAV_CNAV, n, ph);
    const size_t row = ((size_t)k * 2 + ph) * (size_t)a.bit_cap;
    const int8_t *q = a.q + (size_t)k * a.cap + ph;
    unsigned long long *surv = a.surv + row;
    uint8_t *bits = a.decoded + row;
    const int p0 = nav_pred(lane, 0), p1 = nav_pred(lane, 1);

    int m = 0;
    for (int t0 = 0; t0 < T; t0 += kNavWave) {
        const int steps = T - t0 < kNavWave ? T - t0 : kNavWave;
        int pair = 0; // q0 in the low half, q1 in the high half
        if (lane < steps) pair = (int)(((unsigned)q[2 * (t0 + lane)] & 0xffffu) | ((unsigned)q[2 * (t0 + lane) + 1] << 16));
        unsigned long long mine = 0; // lane i keeps the survivor word of step i
        for (int i = 0; i < steps; ++i) {
            const int qi = __builtin_amdgcn_readlane(pair, i);
            const int bm = nav_branch0(lane, (short)(qi & 0xffff), qi >> 16);
            int dec;
            m = nav_acs(__shfl(m, p0) + bm, __shfl(m, p1) - bm, &dec);
            const unsigned long long word = __ballot(dec);
            if (lane == i) mine = word;
        }
        if (lane < steps) surv[t0 + lane] = mine;
    }
    // the largest metric, the lowest state on a tie: every lane ends with the same pair
    int best = m, state = lane;
    for (int off = kNavWave / 2; off > 0; off >>= 1) {
        const int om = __shfl_xor(best, off), os = __shfl_xor(state, off);
        if (om > best || (om == best && os < state)) best = om, state = os;
    }
    if (lane == 0 && a.path_metric) a.path_metric[(size_t)k * 2 + ph] = best;
    __syncthreads(); // the survivor words are read by other lanes than wrote them

    int s = __builtin_amdgcn_readfirstlane(state);
    for (int t0 = (T - 1) / kNavWave * kNavWave; T > 0 && t0 >= 0; t0 -= kNavWave) {
        const int steps = T - t0 < kNavWave ? T - t0 : kNavWave;
        const unsigned long long w = lane < steps ? surv[t0 + lane] : 0ull;
        const int lo = (int)(unsigned)w, hi = (int)(unsigned)(w >> 32);
        int mine = 0;
        for (int i = steps - 1; i >= 0; --i) {
            const unsigned long long wi = ((unsigned long long)(unsigned)__builtin_amdgcn_readlane(hi, i) << 32) | (unsigned)__builtin_amdgcn_readlane(lo, i);
            if (lane == i) mine = s >> 5;
            s = nav_back(s, wi);
        }
        if (lane < steps) bits[t0 + lane] = (uint8_t)mine;
    }
    for (int j = T + lane; j < a.bit_cap; j += kNavWave) bits[j] = 0;
}

// one thread per (k, candidate): its hitting frames; neighbouring lanes read neighbouring bits
__global__ __launch_bounds__(kNavThreads) void nav_score_kernel(NavArgs a)
{
    const long long t = nav_thread();
    int k, c, ph, o, p;
    if (!nav_score_unit(t, a.C, a.K, &k, &c)) return;
    nav_candidate(c, &ph, &o, &p);
    const int search = nav_search_bits(a.format, nav_bits(a.format, nav_symbols(a.mon, k, a.cap), ph));
    a.scores[t] = nav_score(a.format, a.decoded + ((size_t)k * a.P + ph) * (size_t)a.bit_cap, search, o, p);
}

__device__ inline NavBest nav_best_xor(const NavBest &b, int off)
{
    return NavBest{__shfl_xor(b.score, off), __shfl_xor(b.cand, off), __shfl_xor(b.second, off)};
}

// One wave per channel: lane l takes candidates l, l + 64, ..; the lanes' choices merge by the rule's order (gat_nav.h), which does
// not depend on how they pair up.  The frames of the choice are decoded once more, a neighbouring pair a lane, for tow_steps.
__global__ __launch_bounds__(kNavThreads) void nav_pick_kernel(NavArgs a)
{
    const int k = blockIdx.x * kNavPickWaves + threadIdx.x / kNavWave, lane = threadIdx.x % kNavWave;
    if (k >= a.K) return;
    const int32_t *scores = a.scores + (size_t)k * a.C;
    NavBest best = nav_best_one(scores[lane], lane); // C >= 600: every lane has a candidate
    for (int c = lane + kNavWave; c < a.C; c += kNavWave) best = nav_best_merge(best, nav_best_one(scores[c], c));
    for (int off = kNavWave / 2; off > 0; off >>= 1) best = nav_best_merge(best, nav_best_xor(best, off));
    gat_nav_channel ch;
    nav_record(a.format, best, nav_symbols(a.mon, k, a.cap), a.max_frames, a.min_frames, ch);
    const uint8_t *bits = a.decoded + ((size_t)k * a.P + ch.symbol_phase) * (size_t)a.bit_cap + (ch.frame_offset < 0 ? 0 : ch.frame_offset);
    int steps = 0;
    for (int f = lane; f + 1 < ch.num_frames; f += kNavWave) {
        gat_nav_frame x, y;
        nav_frame(a.format, bits + (size_t)f * GAT_NAV_FRAME_BITS, ch.inverted, x);
        nav_frame(a.format, bits + (size_t)(f + 1) * GAT_NAV_FRAME_BITS, ch.inverted, y);
        steps += nav_tow_step(a.format, x, y) ? 1 : 0;
    }
    for (int off = kNavWave / 2; off > 0; off >>= 1) steps += __shfl_xor(steps, off);
    ch.tow_steps = steps;
    if (lane == 0) a.chan[k] = ch;
}

// one thread per (k, f): frame f of the choice the record in device memory names, zeros beyond its frames
__global__ __launch_bounds__(kNavThreads) void nav_frame_kernel(NavArgs a)
{
    const long long t = nav_thread();
    int k, f;
    if (!nav_frame_unit(t, a.max_frames, a.K, &k, &f)) return;
    const gat_nav_channel ch = a.chan[k];
    gat_nav_frame fr{};
    if (f < ch.num_frames && ch.frame_offset >= 0)
        nav_frame(a.format, a.decoded + ((size_t)k * a.P + ch.symbol_phase) * (size_t)a.bit_cap + ch.frame_offset + (size_t)f * GAT_NAV_FRAME_BITS,
                  ch.inverted, fr);
    a.frames[t] = fr;
}

template <class Kernel>
hipError_t launch(Kernel kernel, const NavArgs &a, long long grid, int threads, hipStream_t st)
{
    if (grid < 1 || grid > 0x7fffffffll) return hipErrorInvalidValue;
    hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(threads), 0, st, a);
    return hipGetLastError();
}

} // namespace

hipError_t launch_nav_slice(const NavArgs &a, long long grid, hipStream_t st) { return launch(nav_slice_kernel, a, grid, kNavThreads, st); }
hipError_t launch_nav_quantise(const NavArgs &a, long long grid, hipStream_t st) { return launch(nav_quantise_kernel, a, grid, kNavWave, st); }
hipError_t launch_nav_trellis(const NavArgs &a, long long grid, hipStream_t st) { return launch(nav_trellis_kernel, a, grid, kNavWave, st); }
hipError_t launch_nav_score(const NavArgs &a, long long grid, hipStream_t st) { return launch(nav_score_kernel, a, grid, kNavThreads, st); }
hipError_t launch_nav_pick(const NavArgs &a, long long grid, hipStream_t st) { return launch(nav_pick_kernel, a, grid, kNavThreads, st); }
hipError_t launch_nav_frames(const NavArgs &a, long long grid, hipStream_t st) { return launch(nav_frame_kernel, a, grid, kNavThreads, st); }

} // namespace gat
