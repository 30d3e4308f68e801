// gat_mon.hip -- the tracking monitor's kernels (include/gat.h gat_track_monitor) for gfx950.  The arithmetic is gat_mon.h (the host
// twin runs the same text), the geometry and the decoding of a work unit gat_mon_plan.h.  Every value meets the same operands
// in the same order whichever lane holds it: no atomics, no reduction tree, no data-dependent order.  The per-channel series
// (prompts [K][B], terms [K][J][Pd], energies [K][Pd]) are contiguous in the index neighbouring lanes differ in, so the scans
// read coalesced.
#include "gat_mon_kernels.h"

namespace gat {

namespace {

__device__ inline long long mon_thread() { return (long long)blockIdx.x * kMonThreads + threadIdx.x; }

// one thread per (k, b): the loop's prompt tap of block b
__global__ __launch_bounds__(kMonThreads) void mon_prompt_kernel(MonArgs a)
{
    int k, b;
    if (!mon_prompt_unit(mon_thread(), a.B, a.K, &k, &b)) return;
    const size_t o = (size_t)b * (size_t)a.acc_block_stride;
    double re, im;
    tap_sum(a.acc_re + o, a.acc_im + o, k, a.L, a.prompt, a.M, a.w_re, a.w_im, re, im);
    a.pr[(size_t)k * a.B + b] = re;
    a.pi[(size_t)k * a.B + b] = im;
}

// One wave per (k, window): its 64 lanes stage 64 blocks' prompts in LDS with one coalesced load each, lane 0 adds them in block
// order (the sums are sequential by rule).  The trip count is the same for every wave, so the barriers are uniform.
__global__ __launch_bounds__(kMonThreads) void mon_window_kernel(MonArgs a)
{
    __shared__ double s_i[kMonWindowWaves][kMonWave], s_q[kMonWindowWaves][kMonWave];
    const int wave = threadIdx.x / kMonWave, lane = threadIdx.x % kMonWave;
    int k = 0;
    long long v = 0;
    const bool live = mon_window_unit((long long)blockIdx.x * kMonWindowWaves + wave, a.NW, a.K, &k, &v);
    const long long b0 = v * a.W;
    const long long n = !live ? 0 : (a.B - b0 < a.W ? a.B - b0 : a.W); // the last window takes what is left
    const long long span = a.W < a.B ? a.W : a.B;
    const double *pr = a.pr + (size_t)k * a.B + b0, *pi = a.pi + (size_t)k * a.B + b0;
    gat_monitor_window w;
    mon_window_begin(w);
    for (long long c0 = 0; c0 < span; c0 += kMonWave) {
        if (c0 + lane < n) {
            s_i[wave][lane] = pr[c0 + lane];
            s_q[wave][lane] = pi[c0 + lane];
        }
        __syncthreads();
        if (lane == 0) {
            const int m = n - c0 < kMonWave ? (int)(n - c0) : kMonWave;
            for (int i = 0; i < m; ++i) mon_window_add(w, s_i[wave][i], s_q[wave][i]);
        }
        __syncthreads();
    }
    if (live && lane == 0) a.windows[(size_t)k * a.NW + v] = w;
}

// one thread per (k, j, c): |S|^2 of symbol j from the candidate start c; neighbouring lanes read neighbouring blocks
__global__ __launch_bounds__(kMonThreads) void mon_term_kernel(MonArgs a)
{
    const long long t = mon_thread();
    int k, c;
    long long j;
    if (!mon_term_unit(t, a.J, a.Pd, a.K, &k, &j, &c)) return;
    a.terms[t] = mon_symbol_energy(a.pr + (size_t)k * a.B, a.pi + (size_t)k * a.B, c, j, a.Pd, a.overlay);
}

// one thread per (k, c): E = the terms added in j order (neighbouring lanes read neighbouring terms of one j)
__global__ __launch_bounds__(kMonThreads) void mon_energy_kernel(MonArgs a)
{
    int k, c;
    if (!mon_energy_unit(mon_thread(), a.Pd, a.K, &k, &c)) return;
    double e = 0.0;
    for (long long j = 0; j < a.J; ++j) e += a.terms[((size_t)k * a.J + j) * a.Pd + c];
    a.energy[(size_t)k * a.Pd + c] = e;
}

// one thread per channel: the symbol start and the channel record
__global__ __launch_bounds__(kMonThreads) void mon_pick_kernel(MonArgs a)
{
    const long long k = mon_thread();
    if (k >= a.K) return;
    gat_monitor_channel ch;
    mon_pick(a.energy + (size_t)k * a.Pd, a.Pd, a.B, a.J, a.forced, a.first_block, ch);
    a.chan[k] = ch;
}

// one thread per (k, symbol of the capacity): the symbols from the start the choice left in device memory, 0 beyond them
__global__ __launch_bounds__(kMonThreads) void mon_symbol_kernel(MonArgs a)
{
    const long long t = mon_thread();
    int k;
    long long j;
    if (!mon_symbol_unit(t, a.cap, a.K, &k, &j)) return;
    const int c = a.chan[k].start;
    double sr = 0.0, si = 0.0, wbp = 0.0;
    if (c >= 0 && j < a.chan[k].num_symbols) mon_symbol(a.pr + (size_t)k * a.B, a.pi + (size_t)k * a.B, c + j * a.Pd, a.Pd, a.overlay, sr, si, wbp);
    if (a.sym_re) a.sym_re[t] = sr;
    if (a.sym_im) a.sym_im[t] = si;
    if (a.sym_wbp) a.sym_wbp[t] = wbp;
}

template <class Kernel>
hipError_t launch(Kernel kernel, const MonArgs &a, long long grid, hipStream_t st)
{
    if (grid < 1 || grid > 0x7fffffffll) return hipErrorInvalidValue;
    hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(kMonThreads), 0, st, a);
    return hipGetLastError();
}

} // namespace

hipError_t launch_mon_prompts(const MonArgs &a, long long grid, hipStream_t st) { return launch(mon_prompt_kernel, a, grid, st); }
hipError_t launch_mon_windows(const MonArgs &a, long long grid, hipStream_t st) { return launch(mon_window_kernel, a, grid, st); }
hipError_t launch_mon_terms(const MonArgs &a, long long grid, hipStream_t st) { return launch(mon_term_kernel, a, grid, st); }
hipError_t launch_mon_energies(const MonArgs &a, long long grid, hipStream_t st) { return launch(mon_energy_kernel, a, grid, st); }
hipError_t launch_mon_pick(const MonArgs &a, long long grid, hipStream_t st) { return launch(mon_pick_kernel, a, grid, st); }
hipError_t launch_mon_symbols(const MonArgs &a, long long grid, hipStream_t st) { return launch(mon_symbol_kernel, a, grid, st); }

} // namespace gat
