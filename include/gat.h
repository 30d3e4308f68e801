/*
 * gat.h -- C ABI of libgat, the MI355X (gfx950) GNSS tracking correlator.
 *
 * Drop-in boundary for ONE path of coezmaden/GPUAcceleratedTracking: downconvert + correlate
 * (carrier wipe-off, PRN code replica, multi-tap multiply over antennas, reduction).  The
 * reference has no FFI layer -- its boundary is Julia multiple dispatch -- so every entry point
 * below names the reference interface it stands in for (paths relative to the reference tree).
 * INTEGRATION.md shows the Julia `ccall` shim that binds them.
 *
 * Conventions
 *   - plain C, no exceptions cross the ABI; every function returns int32 status:
 *       0 = GAT_OK, > 0 = argument/state error (GAT_ERR_*), < 0 = -(hipError_t).
 *     gat_last_error(ctx) returns a human-readable message for the last failure on that ctx.
 *   - "dev" pointers are device (HBM) addresses valid on the ctx's device; "host" pointers are
 *     ordinary host memory, read/written only during the call.
 *   - all work is enqueued on the ctx's HIP stream; calls are asynchronous unless stated.
 *     A ctx is not thread-safe; distinct ctxs are independent.
 *   - arrays are column-major as in the reference: signal [N x M] (sample fastest,
 *     src/gen_signal.jl:179), codes [Lc x P] (src/algorithms.jl:185), correlator outputs
 *     [M x L x K x B] (antenna fastest, src/algorithms.jl:628), planar re / im
 *     (StructArray{ComplexF32}).
 *   - indices are 0-based here (sample n = 0 is the reference's sample_idx = 1; prn is the
 *     0-based column of the code table, i.e. reference prn - 1).
 */
#ifndef GAT_H_
#define GAT_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(GAT_BUILD)
#define GAT_API __attribute__((visibility("default")))
#else
#define GAT_API
#endif

/* ---- status codes ----------------------------------------------------------------------- */
#define GAT_OK 0
#define GAT_ERR_ARG 1         /* null pointer, non-positive size, bad enum                    */
#define GAT_ERR_RANGE 2       /* prn / phase / size outside the supported range               */
#define GAT_ERR_STATE 3       /* e.g. correlate before gat_set_codes                          */
#define GAT_ERR_UNSUPPORTED 4 /* valid request this build has no kernel for                   */
#define GAT_ERR_NOMEM 5

/* ---- flags for gat_downconvert_and_correlate ------------------------------------------- */
#define GAT_FLAG_ATOMIC 1u /* single-pass float atomics (reference alg. 4/5,                */
                           /* src/algorithms.jl:625-632); default = deterministic two-stage */

#define GAT_FLAG_GRAPH 2u  /* gat_tracking_run and gat_downconvert_and_correlate_dev: replay the call's launch sequence */
                           /* as an instantiated hipGraph when it repeats with the same arguments and buffers (needs a  */
                           /* non-default stream; else stays eager).  Not for the host-parameter entry point.          */

/* ---- signal layouts ---------------------------------------------------------------------- */
#define GAT_LAYOUT_PLANAR 0          /* float32 re[] and im[] planes (reference StructArray)   */
#define GAT_LAYOUT_INTERLEAVED 1     /* ComplexF32 {re,im} pairs; .im must be NULL             */
#define GAT_LAYOUT_INTERLEAVED_I16 2 /* {int16 re, int16 im} pairs (front-end "sc16"), 4 B/sample */
#define GAT_LAYOUT_INTERLEAVED_I8 3  /* {int8 re, int8 im} pairs (front-end "sc8"), 2 B/sample  */

#define GAT_MAX_TAPS 32 /* correlator taps per call (L), any order; reference uses 3 and 7 */

typedef struct gat_ctx gat_ctx;

/* One satellite channel in one integration block.  Replaces the scalar arguments
 * (prn, code_frequency, carrier_frequency, start_code_phase, carrier_phase) of
 * Tracking.downconvert_and_correlate! (call site src/benchmarks.jl:63-79) and of
 * downconvert_and_correlate_kernel_1330! (src/algorithms.jl:142-159). */
typedef struct gat_channel_params {
    int32_t prn;                 /* 0-based column of the code table                         */
    int32_t reserved;            /* must be 0                                                */
    double code_freq_hz;         /* code_frequency (chips/s), incl. code Doppler             */
    double carrier_freq_hz;      /* carrier_frequency = IF + Doppler (Hz)                    */
    double code_phase_chips;     /* start_code_phase at sample 0                             */
    double carrier_phase_cycles; /* carrier_phase at sample 0, in CYCLES (algorithms.jl:172) */
} gat_channel_params;
/* Accepted records (the correlate entry points and the resident correlator; host records outside this set return
 * GAT_ERR_RANGE / GAT_ERR_ARG, device records outside it get NaN outputs): 0 <= prn < num_prns; code_freq_hz >= 0;
 * |code_phase_chips| + code_freq_hz / fs * (num_samples + max|shift|) + 1 below both 2^30 and 2^21 * code_length;
 * |carrier_freq_hz / fs| < 1e15 and |carrier_phase_cycles| < 1e15, any carrier within that, above Nyquist included.  Every
 * value is finite.  The kernels reduce the carrier phase modulo 1 and the carrier step f / fs modulo 1 exactly, so results
 * meet the 1e-5 contract over the whole carrier range.  The matrix-core kernels also need code_freq_hz / fs * 32 < code_length
 * (see gat_set_matrix_core). */

/* Device-resident antenna signal; replaces signal.re / signal.im (CuArray{Float32,2} or ,3)
 * handed to kernel_algorithm (src/algorithms.jl:887-888) -- element (n, m, b, k) lives at
 *   n + m*ant_stride + b*block_stride + k*chan_stride          (in samples). */
/* Fast path requirements (checked per call; a signal that misses them is still correlated, by the scalar-load kernel --
 * one antenna per wave, a double-precision sincos per sample, typically 5-10x slower; gat_launch_info.vec tells which ran):
 * plane base pointers 16-byte aligned, and ant_stride, block_stride and chan_stride multiples of the samples one 16-byte
 * load holds -- 4 (planar float), 2 (ComplexF32 pairs), 4 (int16 pairs), 8 (int8 pairs) --, i.e. every block of every
 * antenna STARTS on a 16-byte boundary.  num_samples itself may be anything (N = 2046 at fs = 2 x 1.023 MHz, N = 2500 as
 * int8 pairs ...): a receiver with such a block length pads block_stride to the next multiple, nothing else. */
typedef struct gat_signal_desc {
    const void *re;       /* dev; planar: float real plane. interleaved formats: base pointer */
    const void *im;       /* dev; planar: float imaginary plane. interleaved formats: NULL    */
    int32_t layout;       /* GAT_LAYOUT_*                                                     */
    int32_t num_ants;     /* M                                                                */
    int64_t num_samples;  /* N per integration block                                          */
    int64_t ant_stride;   /* samples between antennas (>= extent of one antenna's stream)     */
    int64_t block_stride; /* samples between consecutive integration blocks (normally N)     */
    int64_t chan_stride;  /* 0: every channel reads the same signal; != 0: one signal per     */
                          /* channel as in _3d_4431! (src/algorithms.jl:668)                 */
} gat_signal_desc;

/* ---- context ------------------------------------------------------------------------------
 * Replaces the implicit CUDA.jl task-local device + default stream (CUDA.@sync at
 * src/benchmarks.jl:120).  `hip_stream` is a hipStream_t the caller keeps alive (e.g. PyTorch's
 * current stream); NULL is the HIP default (null) stream -- which is also what PyTorch's default
 * stream is; GAT_OWN_STREAM asks the library to create (and own) a non-blocking stream. */
#define GAT_OWN_STREAM ((void *)(intptr_t)-1)
GAT_API int32_t gat_create(int32_t device, void *hip_stream, gat_ctx **out_ctx);
GAT_API int32_t gat_destroy(gat_ctx *ctx);
GAT_API int32_t gat_set_stream(gat_ctx *ctx, void *hip_stream);
GAT_API int32_t gat_sync(gat_ctx *ctx); /* CUDA.@sync equivalent: wait for the ctx stream  */
GAT_API const char *gat_last_error(const gat_ctx *ctx);
/* "libgat <version> (gfx950) git:<short commit of the kernel sources>[+dirty] flags:<-D flags beyond the product recipe | none>":
 * which library a result came from (the reference tags saved results with its commit: @tagsave,
 * scripts/run_benchmarks_gpsl1.jl:24-27).  A product build says "flags:none"; development builds (-DGAT_DEV: A/B knobs
 * from the environment, -DGAT_DC_DEV: a reduced instance set) name theirs. */
GAT_API const char *gat_version(void);

/* Device properties used for metadata (add_metadata!, src/benchmarks.jl:11-32: GPU_model, CUDA
 * version).  name_buf receives the device name; *runtime_version the HIP runtime version. */
GAT_API int32_t gat_device_info(gat_ctx *ctx, char *name_buf, size_t name_len,
                                int32_t *runtime_version, int32_t *num_cus);

/* ---- code tables --------------------------------------------------------------------------
 * Replaces `system.codes` (GNSSSignals.jl; src/benchmarks.jl:93, src/algorithms.jl:185):
 * int8 chips, column-major [code_length x num_prns], copied to the device once.  Any int8 value is
 * accepted (a chip multiplies the sample as it is), 1 to 120000 chips per row (more: GAT_ERR_RANGE),
 * any number of rows.  Tables whose chips are all +-1 also get sign-bit rows: the vector kernel
 * stages those for rows of 2048 chips and more, and the split-bf16 matrix kernel needs them.  Any
 * other table is staged as int8 rows and runs on the vector kernel or, on request (GAT_MC_F32),
 * the f32 matrix kernel -- never on the split-bf16 kernel. */
GAT_API int32_t gat_set_codes(gat_ctx *ctx, const int8_t *codes_host, int32_t code_length,
                              int32_t num_prns);

/* Host-side PRN generators standing in for GNSSSignals.GPSL1()/GPSL5() (src/
 * GPUAcceleratedTracking.jl:39-42).  system = "GPSL1" (1023 chips, 1.023 Mcps, PRN 1..37) or
 * "GPSL5" (I5, 10230 chips, 10.23 Mcps, PRN 1..37).  out_codes may be NULL to query sizes. */
GAT_API int32_t gat_gen_codes(const char *system, int32_t num_prns, int8_t *out_codes_host,
                              int32_t *code_length, double *code_freq_hz);

/* get_correlator_sample_shifts(system, correlator, fs, preferred_code_shift)
 * (src/benchmarks.jl:105-107): s = max(1, round(spacing*fs/fc)); shifts[l] = (l - L/2)*s. */
GAT_API int32_t gat_sample_shifts(int32_t num_taps, double sampling_freq_hz, double code_freq_hz,
                                  double spacing_chips, int32_t *shifts_host);

/* ---- the hot path -------------------------------------------------------------------------
 * Tracking.downconvert_and_correlate!(system, signal, correlator, code_replica, code_phase,
 *   carrier_replica, carrier_phase, downconverted_signal, code_frequency,
 *   correlator_sample_shifts, carrier_frequency, sampling_frequency, start_sample,
 *   num_samples, prn)                                           (src/benchmarks.jl:63-79)
 * == kernel_algorithm(..., ::KernelAlgorithm{1330|1331|1431|2xxx|3431|4431|5431})
 *                                                               (src/algorithms.jl:869-1545)
 * == downconvert_and_correlate_kernel_3d_4431! for num_channels > 1 (src/algorithms.jl:637).
 *
 *   R[m,l,k,b] = sum_{n<N} x[n,m,b] * conj(exp(j2pi(n*f/fs + phi))) * c[floor(fc/fs*(n+shift_l)+tau) mod Lc]
 *
 * One fused launch (plus a tiny finalize launch when one block's samples are split over
 * several workgroups).  Outputs are OVERWRITTEN (the reference's `+=` into stale buffers,
 * src/algorithms.jl:207, is not reproduced).  params: [num_channels x num_blocks], channel
 * fastest.  out_re/out_im: dev float [M x L x K x B].  The replica / carrier / downconverted
 * scratch arguments of the reference call do not exist: nothing is materialised.
 * params_host is validated (GAT_ERR_RANGE / GAT_ERR_ARG instead of NaN results) and consumed before the call returns: up
 * to 4 records (num_blocks * num_channels <= 4: the single-block call of a receiver loop, the reference's kernel_algorithm
 * with scalar arguments) travel inside the kernel arguments -- no upload in front of the launch --, more are copied to a
 * context-owned device buffer on the context's stream. */
GAT_API int32_t gat_downconvert_and_correlate(gat_ctx *ctx, const gat_signal_desc *signal,
                                              const gat_channel_params *params_host,
                                              int32_t num_blocks, int32_t num_channels,
                                              int32_t num_taps, const int32_t *shifts_host,
                                              double sampling_freq_hz, float *out_re_dev,
                                              float *out_im_dev, uint32_t flags);

/* Same, with the per-(block, channel) parameters already resident on the device (a tracking
 * loop that produces them on-GPU; also the form bench.py times). */
GAT_API int32_t gat_downconvert_and_correlate_dev(gat_ctx *ctx, const gat_signal_desc *signal,
                                                  const gat_channel_params *params_dev,
                                                  int32_t num_blocks, int32_t num_channels,
                                                  int32_t num_taps, const int32_t *shifts_host,
                                                  double sampling_freq_hz, float *out_re_dev,
                                                  float *out_im_dev, uint32_t flags);

/* ---- stand-alone operators on the same path ---------------------------------------------- */

/* Tracking.gen_code_replica!(code_replica, system, code_frequency, sampling_frequency,
 *   start_code_phase, start_sample, num_samples, correlator_sample_shifts, prn)
 *   (scripts/code_replica_experiment.jl:70) == gen_code_replica_kernel! (src/algorithms.jl:13)
 * rep[i] = c[floor(fc/fs*(i + first_shift) + tau) mod Lc], i = 0..count-1, as float32 +-1. */
GAT_API int32_t gat_gen_code_replica(gat_ctx *ctx, float *replica_dev, int64_t count, int32_t prn,
                                     double code_freq_hz, double sampling_freq_hz,
                                     double code_phase_chips, int64_t first_shift);

/* gen_code_replica_texture_mem_kernel! (src/algorithms.jl:121-140): the same replica addressed
 * through a Float32 NORMALISED coordinate (phase / code_length rounded to float32, wrap, nearest
 * texel) -- an emulation of the arithmetic behind the texture path's code-phase error
 * (paper/paper.tex:318-331; scripts/code_replica_experiment.jl).  Study use only: the
 * correlator never uses it. */
GAT_API int32_t gat_gen_code_replica_f32coord(gat_ctx *ctx, float *replica_dev, int64_t count,
                                              int32_t prn, double code_freq_hz,
                                              double sampling_freq_hz, double code_phase_chips,
                                              int64_t first_shift);

/* The same study with the texture unit's FIXED-POINT addressing modelled (paper/paper.tex:322-331 reports min 0 / mean
 * 0.03 / median 0.02 / max 3.17 % relative code-phase error; Float32 rounding of the coordinate alone gives 1/16 of the
 * mean and 1/25 of the maximum).  From the Float32 normalised coordinate u = float32(phase / code_length), wrapped to
 * w = u - floor(u):
 *   coord_frac_bits > 0 : w is TRUNCATED to that many fractional bits (the unit's fixed-point normalised coordinate);
 *   x = w * code_length, exact (no Float32 rounding of the product);
 *   texel_frac_bits >= 0: x is ROUNDED to nearest at that many fractional bits (a fixed-point texel address; 8 = the
 *                         sub-texel precision CUDA documents for its filter weights); -1: left as it is;
 *   chip = floor(x).
 * (0, -1) is Float32 rounding of the coordinate alone with an exact product.  Study use only
 * (scripts/code_replica_experiment.py runs the reference's sweep over these modes). */
GAT_API int32_t gat_gen_code_replica_texaddr(gat_ctx *ctx, float *replica_dev, int64_t count, int32_t prn,
                                             double code_freq_hz, double sampling_freq_hz, double code_phase_chips,
                                             int64_t first_shift, int32_t coord_frac_bits, int32_t texel_frac_bits);

/* gen_code_replica_texture_mem_strided_nsat_kernel! (src/algorithms.jl:78-98): the replicas of num_channels
 * satellite channels in ONE call -- row k (row_stride floats apart) = channel k with its own prn, code_freq_hz and
 * code_phase_chips (params_dev[k]; the carrier fields are ignored); rep[k][i] = c_k[floor(fc_k/fs*(i + first_shift)
 * + tau_k) mod Lc].  Exact index arithmetic (prn is a table column here, not the reference's normalised texture
 * coordinate, SURVEY defect D5).  A prn outside the table poisons its row with NaN. */
GAT_API int32_t gat_gen_code_replica_multi(gat_ctx *ctx, float *replica_dev, int64_t count, int64_t row_stride,
                                           int32_t num_channels, const gat_channel_params *params_dev,
                                           double sampling_freq_hz, int64_t first_shift);

/* downconvert_and_accumulate_strided_kernel! (src/algorithms.jl:828-866), the materialising middle stage of the
 * reference's algorithm 2, as a DEBUG export: for one integration block (planar float signal) and one channel it
 * writes what the fused correlator never materialises -- carrier replica [N], downconverted signal [N x M]
 * (sample fastest) and the per-sample products [N x M x L] -- so that the reference's test of that stage
 * (test/algorithms.jl:1438-1514: prompt products == 1, column sums == [1476 2500 1476]) has a counterpart.
 * Any output pointer may be NULL.  Not a fast path: 8*N*(1 + M + M*L) bytes of stores for 8*N*M bytes of signal. */
GAT_API int32_t gat_downconvert_and_accumulate(gat_ctx *ctx, const gat_signal_desc *signal,
                                               const gat_channel_params *params_host, int32_t num_taps,
                                               const int32_t *shifts_host, double sampling_freq_hz,
                                               float *carrier_re_dev, float *carrier_im_dev, float *dw_re_dev,
                                               float *dw_im_dev, float *accum_re_dev, float *accum_im_dev);

/* gen_signal! (src/gen_signal.jl:53-175): noise-free synthetic IF signal, identical on every
 * antenna.  Writes, for every block b, x[n,m,b] = sum_k c_k[floor(fc_k/fs*n + tau_kb) mod Lc]
 *   * (cos, sin)(float32(2pi*n*f_kb/fs + phase_kb)).  NOTE: for THIS call the
 * carrier_phase_cycles field is interpreted in RADIANS, as start_carrier_phase is in the
 * reference (src/gen_signal.jl:88).  params_dev: [num_channels x num_blocks].  `amplitude`
 * scales the sum (1.0 = the reference); the integer layouts store rint(amplitude * x),
 * saturated -- e.g. amplitude 2000 for int16, 40 for int8. */
GAT_API int32_t gat_gen_signal(gat_ctx *ctx, void *re_dev, void *im_dev, int32_t layout,
                               int64_t num_samples, int32_t num_ants, int64_t ant_stride,
                               int64_t block_stride, int32_t num_blocks, int32_t num_channels,
                               const gat_channel_params *params_dev, double sampling_freq_hz,
                               double amplitude);

/* The same generator with what a receiver's input has and the reference's noise-free one lacks (paper/paper.tex:116;
 * SURVEY section 8-d "build additions"): a unit-modulus steering phase per antenna (steering_cycles_dev: M floats in cycles on
 * the device, or NULL: identical antennas) and complex white Gaussian noise of standard deviation noise_sigma per component
 * (in units of one satellite's amplitude; scaled by `amplitude` like the signal).  The noise of sample (block, antenna, n) is a
 * pure function of (seed, block, antenna, n) -- counter-based, independent of the launch geometry and of the layout. */
GAT_API int32_t gat_gen_signal_noisy(gat_ctx *ctx, void *re_dev, void *im_dev, int32_t layout,
                                     int64_t num_samples, int32_t num_ants, int64_t ant_stride,
                                     int64_t block_stride, int32_t num_blocks, int32_t num_channels,
                                     const gat_channel_params *params_dev, double sampling_freq_hz,
                                     double amplitude, const float *steering_cycles_dev, double noise_sigma,
                                     uint64_t seed);

/* reduce_cplx_multi_3/4/5 two-pass sum (src/reduction.jl:93, :331, :548; launch sequence
 * src/algorithms.jl:914-922): column sums of a planar complex [n x num_cols] array.
 * Deterministic; no single-block second pass limit (SURVEY defect D6). */
GAT_API int32_t gat_reduce_cplx_multi(gat_ctx *ctx, const float *in_re_dev, const float *in_im_dev,
                                      int64_t n, int32_t num_cols, float *out_re_dev,
                                      float *out_im_dev);

/* ---- closed tracking-loop step ------------------------------------
 * What Tracking.jl's `track` does around the correlator (the reference touches that layer only
 * to borrow buffers: TrackingState, src/benchmarks.jl:54-61): discriminators + loop filters turn
 * the accumulators of the block just correlated into the parameters of the next block, ON THE
 * DEVICE, so a receiver loop is {correlate, update} with no host round trip.  Textbook loop
 * (Kaplan & Hegarty ch. 5; the same structure Tracking.jl uses):
 *   prompt/early/late = sum over antennas of R[m, tap]                      (identical antennas;
 *                       the *_weighted entry points below form sum_m conj(w_m) R[m, tap] instead)
 *   PLL: Costas arctan discriminator atan(Q/I)/2pi [cycles] -> 3rd-order bilinear loop filter
 *   DLL: (2-d)/2 * (|L|-|E|)/(|E|+|L|) [chips], d = E-L spacing in chips -> 2nd-order bilinear
 *        filter, carrier aided (code_doppler += carrier_doppler * code_freq / carrier_center)
 *   next block: carrier_phase += carrier_freq * T, code_phase += code_freq * T (mod code_length),
 *               carrier_freq = if_hz + doppler, code_freq = nominal + code_doppler
 * No reference implementation of this step is available here (Tracking.jl is un-vendored):
 * parity is against the oracle's restatement of the same equations only ("unpinned"). */
typedef struct gat_loop_config {
    double block_seconds;        /* T = N / fs                                                 */
    double pll_bandwidth_hz;     /* carrier loop noise bandwidth (e.g. 18 Hz)                  */
    double dll_bandwidth_hz;     /* code loop noise bandwidth (e.g. 1 Hz)                      */
    double code_freq_nominal_hz; /* e.g. 1.023e6                                               */
    double carrier_center_hz;    /* RF centre frequency for carrier aiding (e.g. 1575.42e6)    */
    double if_hz;                /* intermediate frequency of the sampled signal               */
    double early_late_spacing_chips; /* d: distance between the early and the late tap in chips */
    int32_t code_length;
    int32_t num_taps, early_index, prompt_index, late_index; /* positions in the tap list      */
} gat_loop_config;

typedef struct gat_loop_state { /* one per channel, device-resident; zero everything but      */
    double init_carrier_doppler_hz; /* ... this: the acquisition estimate the loop starts from */
    double carrier_doppler_hz;  /* out: current carrier Doppler estimate                       */
    double code_doppler_hz;     /* out: current code Doppler estimate                          */
    double pll_acc1, pll_acc2;  /* loop-filter integrators                                     */
    double dll_acc;
    double last_pll_error_cycles, last_dll_error_chips; /* diagnostics                         */
    double prompt_power;        /* |P|^2 of the last block                                     */
} gat_loop_state;

/* acc_re/acc_im: dev float [M x L x K] of ONE block (as written by the correlator);
 * cur/next: dev gat_channel_params[K] (may alias); state: dev gat_loop_state[K]. */
GAT_API int32_t gat_tracking_update(gat_ctx *ctx, const float *acc_re_dev, const float *acc_im_dev,
                                    int32_t num_channels, int32_t num_ants,
                                    const gat_loop_config *config_host, gat_loop_state *state_dev,
                                    const gat_channel_params *cur_dev, gat_channel_params *next_dev);

/* The same update on the HOST (the same arithmetic: csrc/gat_loop.h), for a receiver that takes its correlator outputs on
 * the host -- from a resident correlator, below -- and closes its loops there, as Tracking.jl does.  All pointers are host
 * memory; next_host may alias cur_host.  Needs no context and no device. */
GAT_API int32_t gat_tracking_update_host(const float *acc_re_host, const float *acc_im_host, int32_t num_channels,
                                         int32_t num_ants, const gat_loop_config *config_host, gat_loop_state *state_host,
                                         const gat_channel_params *cur_host, gat_channel_params *next_host);

/* num_blocks consecutive integration blocks of a device-resident signal (block b starts b * sig->block_stride
 * samples in) through {correlate, tracking update} with the parameters ping-ponging between params_a (current at
 * entry) and params_b: 2 * num_blocks launches enqueued from native code, no host round trip and no
 * synchronisation (a per-block call from a scripting host is launch-bound: ~16 us per 1 ms block).  Block b's
 * accumulators go to acc_re/acc_im + b * acc_block_stride floats ([M x L x K] each; stride 0 keeps only the last
 * block's).  *current_is_b tells which buffer holds the parameters for the block after the last one.
 * flags: GAT_FLAG_ATOMIC as for the correlator; GAT_FLAG_GRAPH: the first call with a given argument set runs
 * eagerly and records the sequence, later calls with the same arguments replay it with one hipGraphLaunch. */
GAT_API int32_t gat_tracking_run(gat_ctx *ctx, const gat_signal_desc *sig, int32_t num_blocks, int32_t num_channels,
                                 int32_t num_taps, const int32_t *shifts_host, double sampling_freq_hz,
                                 const gat_loop_config *config_host, gat_loop_state *state_dev,
                                 gat_channel_params *params_a_dev, gat_channel_params *params_b_dev,
                                 float *acc_re_dev, float *acc_im_dev, int64_t acc_block_stride, uint32_t flags,
                                 int32_t *current_is_b);

/* ---- memory + timing helpers (for hosts without their own HIP array type) ---------------- */
GAT_API int32_t gat_malloc(gat_ctx *ctx, size_t bytes, void **out_dev);
GAT_API int32_t gat_free(gat_ctx *ctx, void *dev);
GAT_API int32_t gat_memcpy_h2d(gat_ctx *ctx, void *dst_dev, const void *src_host, size_t bytes);
GAT_API int32_t gat_memcpy_d2h(gat_ctx *ctx, void *dst_host, const void *src_dev, size_t bytes);
GAT_API int32_t gat_memset(gat_ctx *ctx, void *dst_dev, int32_t value, size_t bytes);

/* hipEvent pair on the ctx stream (the reference times with BenchmarkTools around CUDA.@sync,
 * src/benchmarks.jl:120; CUDA.@elapsed in test/algorithms.jl:1242).  stop() synchronises. */
GAT_API int32_t gat_timer_start(gat_ctx *ctx);
GAT_API int32_t gat_timer_stop(gat_ctx *ctx, float *elapsed_ms);
/* Per-call statistics as the reference's harness keeps them (BenchmarkTools stores every sample's time: Minimum / Median /
 * Mean / sigma / Maximum + RawTimes, src/benchmarks.jl:1-9): gat_timer_lap records ONE event on the ctx stream -- call it
 * before the first timed launch and after every launch --; gat_timer_laps waits for the newest lap and returns the
 * intervals between consecutive laps in milliseconds (laps - 1 of them, at most `capacity`), then forgets the laps.  The
 * events come from a pool the context owns (it grows to the largest number of laps ever outstanding). */
GAT_API int32_t gat_timer_lap(gat_ctx *ctx);
GAT_API int32_t gat_timer_laps(gat_ctx *ctx, float *intervals_ms, int32_t capacity, int32_t *num_intervals);

/* Measurement aid ("also report vs the measured read ceiling"): a kernel that ONLY reads -- every lane
 * one 16-byte load per step over `bytes` of device memory (a multiple of 16), summed into a value nobody stores -- launched
 * `launches` times on the ctx stream, each launch timed by its own event pair (ms_each_host[launches]).  `variant` picks
 * the reader: bits 0-1 workgroups per CU (0: 8, 1: 16, 2: 32, 3: 64), bit 2 plain instead of non-temporal loads, bit 3
 * four instead of eight loads in flight per lane.  What the best variant reaches over the correlator's own stream is the
 * memory system's ceiling for a read-once kernel on this device, in this process, at this moment (bench.py:
 * roofline.read_ceiling_GBps; tests: the box-tolerant performance guard).  Not part of the reference's surface. */
GAT_API int32_t gat_debug_read_stream(gat_ctx *ctx, const void *dev, size_t bytes, int32_t variant, int32_t launches,
                                      float *ms_each_host);

/* Kernel selection.  By default (GAT_MC_AUTO) the library runs the split-bf16 matrix-core kernel (gat_mfma_bf16.hip:
 * both operands as hi+mid+lo bf16 terms, f32-equivalent accuracy; every sample format) where it measured faster than
 * the vector kernel -- M % 16 == 0 and at least 24 (channel, tap, re/im) columns, then by the share of the kernel's
 * 32-column tile slots that carry live columns: float samples (three bf16 terms per value) from 0.70 on at M % 64 == 0
 * (64 antennas x 16 or 32 channels) and 0.90 at M % 32 == 0; int16 pairs (two exact terms, 5/8 of the matrix work: round 5)
 * from 0.5 on at M % 32 == 0 (32 antennas x 8 channels); int8 pairs always; and only launches long enough to give each of
 * the kernel's ~2 workgroups per CU 16 steps (int16, int8) or 32 (float) of 32-128 samples: ONE 1 ms block stays on the
 * vector kernel whatever its shape --, everything else on the vector kernel.
 * GAT_MC_VECTOR forces the vector kernel (A/B measurements, bit-comparisons), GAT_MC_F32 the
 * f32-MFMA kernel (gat_mfma.hip), GAT_MC_BF16_SPLIT the split-bf16 kernel only (shapes neither
 * matrix kernel takes fall through to the vector kernel in every mode). */
#define GAT_MC_VECTOR 0
#define GAT_MC_AUTO 1
#define GAT_MC_F32 2
#define GAT_MC_BF16_SPLIT 3
GAT_API int32_t gat_set_matrix_core(gat_ctx *ctx, int32_t enable);

/* Caps on the vector kernel's workgroup tiling (0 = leave a cap unchanged).  By default a workgroup covers up to 4
 * antenna tiles (16 antennas: carrier and replica are produced once per workgroup), loops over up to 4 channels with
 * the samples held in registers, and over several consecutive short blocks.  (1, 1, 1) gives one antenna tile, one
 * channel and one block per workgroup -- the round-1 geometry; used by A/B measurements and by the parity tests,
 * which run every tiling against the oracle. */
GAT_API int32_t gat_set_vector_tiling(gat_ctx *ctx, int32_t max_antenna_tiles, int32_t max_channels,
                                      int32_t max_blocks);

/* Launch-geometry options by name, for tests (force a code path on a small case) and A/B measurements; none changes a
 * result beyond summation order.  The library reads NO environment variable that selects kernels or geometry (development
 * builds, -DGAT_DEV, map GAT_<NAME> onto these).  Names: "sync_flag_wgs" (largest launch in workgroups that carries the
 * completion flag; 0: never), "max_ant_tile", "dc_aw", "dc_kt", "dc_bpw" (the caps of gat_set_vector_tiling),
 * "dc_bpw_force", "dc_wgs_per_cu", "dc_one_wave", "dc_one_wave_min", "dc_ow_seg", "dc_depth", "dc_keep_l2", "dc_align",
 * "dc_aw2", "dc_quads", "dc_bits", "dc_seg" (round 5: the two-channel tile and its replica fill), "mc_i16_terms" (split-bf16
 * kernel, int16 samples: 2 = the exact two-term split, the default; 3 = the float path's three terms: bit-comparisons),
 * "mc_nct" (32-column tiles per workgroup of the split-bf16 kernel to try first; 0 = by rule), "acq_fft_log2",
 * "acq_fft_doppler_batch", "acq_fft_unit_batch" (gat_acquire_fft below: the transform length, which moves a bin by rounding, and
 * the batches, which change no bit; 0 = the plan's choice).
 * GAT_ERR_ARG: unknown name; GAT_ERR_RANGE: value outside the option's range. */
GAT_API int32_t gat_set_option(gat_ctx *ctx, const char *name, int64_t value);

/* Launch geometry chosen for the last correlate call, or the last gat_beamform_samples call (diagnostics / DESIGN.md tables). */
typedef struct gat_launch_info {
    int32_t workgroups, threads, splits, ant_tile, vec, lds_bytes, finalize_launched;
    int32_t matrix_core; /* 0: the vector kernel ran, 1: the f32-MFMA kernel, 2: the split-bf16 MFMA kernel */
    int32_t channels_per_wg; /* channels one workgroup loops over (signal held in registers / LDS meanwhile)  */
    int32_t blocks_per_wg;   /* consecutive integration blocks one workgroup loops over                       */
    int32_t prefetch_depth;  /* vector kernel: register sets of samples per wave (steps in flight); else 0      */
    int32_t bf16_terms;      /* split-bf16 kernel: bf16 terms per sample value (1: int8, 2: int16, 3: float); else 0 */
} gat_launch_info;
/* struct_size = sizeof(gat_launch_info) of the CALLER's header: the struct grows at its end between versions and the
 * library copies no more than the caller has room for. */
GAT_API int32_t gat_last_launch_info(const gat_ctx *ctx, gat_launch_info *out, size_t struct_size);

/* ---- resident correlator: single-block calls without a kernel launch -------------------------------------------
 * The reference's benchmark is ONE 1 ms block per call, synchronised (`@benchmark CUDA.@sync kernel_algorithm(...)`,
 * src/benchmarks.jl:120-146), and its receiver loop consumes every block's correlator outputs on the host
 * (Tracking.jl's discriminators).  Through gat_downconvert_and_correlate + gat_sync such a call costs a kernel launch and
 * the wait for its end: 7 us on this platform before the kernel has done anything.  A resident correlator keeps ONE
 * kernel on the device for a fixed call geometry; a call rings a doorbell (the channel records and the block's position
 * travel with the ring), every workgroup of the kernel correlates its share and posts its sums to pinned host memory
 * stamped with the call's number, the host adds them in a fixed order: no launch, no stream wait, outputs already on
 * the host (2 MHz .. 8 MHz blocks: 5-6 us instead of 10.5-13.5; a 20 MHz block of four antennas and twelve channels:
 * 9 us instead of 16 -- DESIGN.md 4.2b).
 *
 * Lifetime is bounded on the DEVICE side, whatever the host does: the kernel ends by itself after `idle_us` without a
 * call, after `life_ms` in total, or after `max_calls` calls; the next call starts it again (that call then costs a
 * launch).  It occupies one workgroup slot per workgroup it uses (info.workgroups: about max_workgroups at most) and polls
 * its doorbell while it waits (in host memory: from up to `host_pollers` of them).  Other work of the process runs next to it on other streams; calls that
 * synchronise the whole device (hipDeviceSynchronize, hipFree) wait until it has ended: gat_free, gat_set_codes and
 * gat_destroy therefore ask every resident correlator of the context to leave first (gat_set_codes: for good -- the
 * correlator answers GAT_ERR_STATE afterwards and has to be opened again).
 *
 * Geometry (fixed at open): `signal` describes ONE block (num_samples, num_ants, ant_stride, layout; block_stride and
 * chan_stride as for the correlator) at the START of a device buffer; every call names its block by an offset in
 * samples from there (a ring buffer of blocks, or always 0).  Supported: what gat_downconvert_and_correlate would run as
 * ONE launch of the vector kernel -- any sample layout, block starts 16-byte aligned and num_samples a multiple of the
 * samples one 16-byte load holds (4 / 2 / 4 / 8 by layout), num_channels <= 16, at most 8 taps within a span of 2048
 * samples -- else GAT_ERR_UNSUPPORTED (use the ordinary call).  The caller makes sure the block's samples are in
 * device memory before the call (e.g. gat_sync after the copy that brought them); the kernel reads them past its caches.
 * Results: host arrays [M x L x K], the ordinary call's layout for one block; same values as the ordinary call up to the
 * summation order of the per-workgroup partial sums. */
typedef struct gat_resident gat_resident;
typedef struct gat_resident_config {
    uint32_t struct_size;    /* sizeof(gat_resident_config) of the caller's header                               */
    uint32_t idle_us;        /* the kernel ends after this long without a call          (0: default, 5 000 us)   */
    uint32_t life_ms;        /* ... and after this long whatever happens                (0: default, 2 000 ms)   */
    uint32_t max_calls;      /* ... and after this many calls                           (0: no limit)            */
    uint32_t max_workgroups; /* workgroups one block's samples may be split over   (0: default, 128 -- 64 with the    */
                             /* doorbell in host memory; at most the device's compute units: all of them have to be  */
                             /* on the device at once)                                                           */
    uint32_t host_pollers;   /* doorbell in host memory: up to this many workgroups poll it themselves; with more, one     */
                             /* does and forwards the ring through device memory        (0: default, 20)         */
    uint32_t doorbell;       /* where the doorbell lives: 0 device memory written through the PCIe BAR where the device   */
                             /* has a large BAR, else pinned host memory; 1 pinned host memory; 2 device memory          */
} gat_resident_config;
typedef struct gat_resident_info {
    int32_t workgroups;  /* workgroups of the resident kernel (sample splits x antenna tiles x channels)          */
    int32_t splits;      /* sample splits of one block                                                            */
    int32_t running;     /* 1: a kernel has been started and has not been seen to end                             */
    int32_t last_exit;   /* why the last kernel that ended did: 0 none yet, 1 asked to, 2 idle, 3 lifetime, 4 calls */
    uint64_t launches;   /* kernels started so far (1 + the restarts)                                             */
    uint64_t calls;      /* calls served                                                                          */
} gat_resident_info;
GAT_API int32_t gat_resident_open(gat_ctx *ctx, const gat_signal_desc *signal, int32_t num_channels, int32_t num_taps,
                                  const int32_t *shifts_host, double sampling_freq_hz, const gat_resident_config *config,
                                  gat_resident **out_resident);
/* One call = gat_downconvert_and_correlate(..., num_blocks = 1, ...) + gat_sync + the copy of the outputs to the host.
 * params_host: num_channels records, validated as by the host entry point.  block_offset_samples: >= 0, a multiple of
 * the samples one 16-byte load holds.  Blocks until the results are in out_re_host / out_im_host. */
GAT_API int32_t gat_resident_correlate(gat_resident *resident, const gat_channel_params *params_host,
                                       int64_t block_offset_samples, float *out_re_host, float *out_im_host);
/* The receiver loop with the host in it, from native code: num_blocks consecutive integration blocks (block b starts
 * first_block_offset + b * block_stride_samples samples into the correlator's buffer; the caller has put all of them on
 * the device) through {gat_resident_correlate, gat_tracking_update_host} -- Tracking.jl's structure: correlate on the
 * accelerator, discriminators and loop filters on the CPU -- without a trip through the scripting host per block.
 * params_host[K]: in the first block's parameters, out those for the block after the last; state_host[K] as for
 * gat_tracking_update_host.  Block b's accumulators go to acc_re/acc_im_host + b * acc_block_stride floats ([M x L x K]
 * each; stride 0 keeps only the last block's).  An error ends the run at the block it occurred in: params_host and
 * state_host then hold the loop's state in front of that block. */
GAT_API int32_t gat_resident_tracking_run(gat_resident *resident, int32_t num_blocks, int64_t first_block_offset,
                                          int64_t block_stride_samples, const gat_loop_config *config_host,
                                          gat_loop_state *state_host, gat_channel_params *params_host,
                                          float *acc_re_host, float *acc_im_host, int64_t acc_block_stride);
GAT_API int32_t gat_resident_info_get(const gat_resident *resident, gat_resident_info *out, size_t struct_size);
/* asks the kernel to leave and waits until it has (bounded by the kernel's own limits); the next call starts it again */
GAT_API int32_t gat_resident_park(gat_resident *resident);
/* the same for every resident correlator of the context: call it before anything that waits for the WHOLE device
 * (hipDeviceSynchronize, torch.cuda.synchronize(), hipFree of a foreign allocation) -- such a call otherwise sits out the
 * resident kernels' idle limit (5 ms by default).  gat_free, gat_set_codes and gat_destroy do it themselves. */
GAT_API int32_t gat_resident_park_all(gat_ctx *ctx);
/* (a correlator that is still open when its context is destroyed is closed by gat_destroy: its handle dies with the context) */
GAT_API int32_t gat_resident_close(gat_resident *resident);

/* ---- several devices from one host thread --------------------------------------------------
 * The reference is single-device (its only device call is CUDA.CuDevice(0) for the GPU's name, src/benchmarks.jl:24;
 * "parallelization over multiple channels can be easily extended", paper/paper.tex:114).  Satellite channels are
 * independent given the antenna signal, so they shard with NO collective: every device holds the full signal
 * (replicated by peer copies -- xGMI between the GPUs of one node; 6.4 MB per ms at 16 antennas x 50 MHz is 4 % of one
 * link) and correlates a contiguous slice of the channels; outputs are disjoint.  A group is a set of ordinary
 * contexts (one per member, each with its own stream: the members' launches of one call overlap); a member's context
 * is available for every single-device function above (allocation, gat_gen_signal, timers ...).  The same device
 * may appear several times (two members on device 0 rehearse the whole path on a one-GPU box). */
typedef struct gat_group gat_group;
GAT_API int32_t gat_device_count(int32_t *count);
/* devices: num_members device ordinals, or NULL for 0 .. num_members-1 */
GAT_API int32_t gat_group_create(int32_t num_members, const int32_t *devices, gat_group **out_group);
GAT_API int32_t gat_group_destroy(gat_group *group);
GAT_API int32_t gat_group_size(const gat_group *group, int32_t *num_members);
GAT_API int32_t gat_group_ctx(gat_group *group, int32_t rank, gat_ctx **ctx); /* borrowed: destroyed with the group */
GAT_API const char *gat_group_last_error(const gat_group *group);
/* the contiguous channel slice of member `rank`: channels [first, first + count) of num_channels (count may be 0) */
GAT_API int32_t gat_group_shard(const gat_group *group, int32_t num_channels, int32_t rank, int32_t *first,
                                int32_t *count);
GAT_API int32_t gat_group_set_codes(gat_group *group, const int8_t *codes_host, int32_t code_length,
                                    int32_t num_prns);
/* dst (on dst_ctx's device) <- src (on src_ctx's device), asynchronous: the copy runs on dst_ctx's stream after
 * everything enqueued so far on src_ctx's stream (hipMemcpyPeerAsync; a plain device copy when both are one device),
 * and work enqueued on src_ctx's stream AFTER this call waits for the copy: the source buffer may be refilled on its
 * own stream right away (a receiver replicating every millisecond needs no group-wide sync between blocks). */
GAT_API int32_t gat_memcpy_peer(gat_ctx *dst_ctx, void *dst_dev, gat_ctx *src_ctx, const void *src_dev, size_t bytes);
/* bufs_dev[r] (r != src_rank) <- bufs_dev[src_rank], `bytes` each: the ingest device's signal to its peers */
GAT_API int32_t gat_group_replicate(gat_group *group, int32_t src_rank, void *const *bufs_dev, size_t bytes);
/* gat_downconvert_and_correlate over the group: params_host [num_channels x num_blocks] (channel fastest) for ALL
 * channels; member r correlates its slice on signals[r] (its own copy of the signal) into out_*_dev[r], a device
 * buffer [M x L x count_r x B] on ITS device.  Asynchronous on every member's stream. */
GAT_API int32_t gat_group_correlate(gat_group *group, const gat_signal_desc *signals,
                                    const gat_channel_params *params_host, int32_t num_blocks, int32_t num_channels,
                                    int32_t num_taps, const int32_t *shifts_host, double sampling_freq_hz,
                                    float *const *out_re_dev, float *const *out_im_dev, uint32_t flags);
/* the members' outputs concatenated along the channel axis into host arrays [M x L x K x B]; synchronises */
GAT_API int32_t gat_group_gather(gat_group *group, float *const *out_re_dev, float *const *out_im_dev,
                                 int32_t num_blocks, int32_t num_channels, int32_t num_taps, int32_t num_ants,
                                 float *out_re_host, float *out_im_host);
GAT_API int32_t gat_group_sync(gat_group *group);

/* ---- signal acquisition: the search that seeds the tracking loops --------------------------------------------------
 * Acquisition.jl's `acquire(system, signal, sampling_frequency, prns; interm_freq, max_doppler, dopplers, ...)` (the
 * reference starts every track from an estimate its own code never produces: init_carrier_doppler_hz above,
 * src/benchmarks.jl:54-61 builds its TrackingState from fixed values).  For every PRN p, Doppler bin i < D and code bin
 * j < J the search computes
 *   P[p,i,j] = sum_b sum_m | R[b, (p,i), j, m] |^2
 * where R is exactly what gat_downconvert_and_correlate returns for the channel record
 *   {prn p, code_freq fc, carrier_freq if_hz + f_i, code_phase tau_b, carrier_phase 0}
 * with f_i = doppler_first_hz + i * doppler_step_hz, tau_b = fmod(fc/fs * (double)(b * block_stride), Lc) (the code phase
 * continues from block to block) and the tap shift Delta_j = first_shift + s * j samples: coherent over one block's N
 * samples, non-coherent over antennas and blocks.  Bin j's code phase at sample 0 of block 0 is fc/fs * Delta_j mod Lc, the
 * convention of gat_channel_params.code_phase_chips.  Code Doppler is neglected (every bin uses fc, so one replica serves
 * every Doppler bin): a signal at Doppler f_d drifts by fc * |f_d| / f_carrier * B * N / fs chips over the search (GPS L1,
 * 5 kHz, 10 ms: 0.03 chip).
 * power: dev float [P x D x J] (code bin fastest), deterministic (no float atomics; the same call gives the same bits). */
typedef struct gat_acq_config {
    uint32_t struct_size;       /* sizeof(gat_acq_config) of the caller's header                                    */
    int32_t num_doppler_bins;   /* D >= 1                                                                          */
    double if_hz;               /* intermediate frequency of the sampled signal                                     */
    double code_freq_hz;        /* fc: nominal code frequency (chips/s)                                             */
    double doppler_first_hz;    /* f_0                                                                             */
    double doppler_step_hz;     /* f_{i+1} - f_i                                                                   */
    int64_t first_shift;        /* Delta_0 in samples (any sign): a fine search starts its code window here         */
    int32_t code_step_samples;  /* s: 1 .. 31 samples between code bins                                             */
    int32_t num_code_bins;      /* J >= 1                                                                          */
    double min_peak_ratio;      /* detection threshold on peak / second (0: default 2.0)                            */
    int32_t code_length;        /* Lc in chips: gat_acquire 0 = the bound table's; gat_acq_stats_host: required     */
    int32_t reserved;           /* must be 0                                                                       */
} gat_acq_config;

/* Per-PRN result.  Peak (i*, j*) = the largest bin (the first in [D x J] order on ties).  The Doppler and the code phase
 * are refined by a three-point parabola on power through the peak's neighbours along that axis, clamped to +-0.5 bin; a
 * peak on the grid's edge (or a neighbourhood that is not concave) keeps the bin centre.  The code phase is wrapped into
 * [0, Lc).  The noise set = every bin, in every Doppler row, whose circular code distance from the peak's code phase is
 * more than 1.5 chips; with fewer than 64 such bins (a narrow fine search) noise_power, second_power, peak_to_second and
 * cn0_dbhz are NaN and detected = -1. */
typedef struct gat_acq_result {
    int32_t prn;                /* the code-table column searched (gat_acq_stats_host: the row index p)             */
    int32_t detected;           /* 1: peak_to_second >= min_peak_ratio, 0: not, -1: no noise estimate                 */
    int32_t doppler_bin;        /* i*                                                                              */
    int32_t code_bin;           /* j*                                                                              */
    double peak_power;          /* P[p, i*, j*]                                                                    */
    double noise_power;         /* mean over the noise set                                                         */
    double second_power;        /* maximum over the noise set                                                      */
    double peak_to_second;      /* peak_power / second_power                                                       */
    double cn0_dbhz;            /* 10 log10((peak - noise) / (noise * N / fs))                                     */
    double carrier_doppler_hz;  /* f_0 + (i* + di) * doppler_step_hz                                              */
    double code_phase_chips;    /* fc/fs * (first_shift + s * (j* + dj)) mod Lc                                    */
    int64_t num_noise_bins;     /* size of the noise set                                                           */
} gat_acq_result;

/* The search on the device for num_prns PRNs (prns_host: code-table columns) over num_blocks blocks of `signal` (any
 * layout, any alignment, any N; chan_stride must be 0).  power_dev: dev float [num_prns x D x J] that receives the grid,
 * or NULL (the grid stays in the context's scratch).  results_host: num_prns results.  Synchronises: the results are on the
 * host when the call returns.  Bounds: num_prns * D * J <= 2^26 bins, N + |first_shift| + s * J < 2^30 samples, else
 * GAT_ERR_RANGE; GAT_ERR_STATE before gat_set_codes. */
GAT_API int32_t gat_acquire(gat_ctx *ctx, const gat_signal_desc *signal, int32_t num_blocks, const int32_t *prns_host,
                            int32_t num_prns, double sampling_freq_hz, const gat_acq_config *config, float *power_dev,
                            gat_acq_result *results_host);

/* The same statistics on the HOST over a grid power_host [num_prns x D x J] (the arithmetic is csrc/gat_acq.h, shared with
 * the device): N and sampling_freq_hz enter the C/N0 only.  Needs no context and no device. */
GAT_API int32_t gat_acq_stats_host(const float *power_host, int32_t num_prns, int32_t num_doppler_bins, int32_t num_code_bins,
                                   const gat_acq_config *config, double sampling_freq_hz, int64_t num_samples,
                                   gat_acq_result *results_host);

/* ---- FFT acquisition: every code phase of a block by fast correlation ------------------------------------------------------
 * The same grid P[p,i,j] under the same contract, arguments, results, synchronisation and error codes as gat_acquire, computed by
 * transforms instead of one sum per bin.  The replica is a plain (non-circular) window of the code, so R is a LINEAR correlation
 * and zero padding gives it exactly: with F = 2^L > N, w the wiped samples padded with zeros to F, c_g the F chips from sample
 * first_shift + g * Jseg on, W = FFT(w) and C_g = FFT(c_g),
 *   R[l] = IFFT(C_g[q] * W[(F - q) mod F])[l]   for every lag 0 <= l < Jseg = F - N + 1,
 * and the lag axis first_shift .. first_shift + s (J - 1) is covered by G = ceil((s (J - 1) + 1) / Jseg) such segments; with s > 1
 * the grid keeps every s-th lag.  The cost is G transforms of F points per (PRN, Doppler bin, block, antenna) whatever s is, so
 * the method pays at sample spacing (s = 1) and for long codes, and loses to gat_acquire on coarse grids (large s) -- DESIGN.md
 * 4.6 has the measured ratios.  The arithmetic is one fixed sequence of float32 operations (csrc/gat_acq_fft.h) shared with
 * gat_acquire_fft_host: the device's grid equals the twin's bit for bit, for the same transform length and unit-group count.
 * It is deterministic (no float atomics) and within the same 1e-5 of the FP64 contract as gat_acquire, not bit-equal to it.
 * Refusals beyond gat_acquire's: N >= 2^18 samples (the largest transform), a forced transform length 2^v <= N (option
 * acq_fft_log2), and a search whose spectra do not fit 1 GiB of scratch at the smallest batches: all GAT_ERR_RANGE.
 * Options (gat_set_option): acq_fft_log2 (0 = the plan's choice: the F that minimises G F log2 F; else 10 .. 18),
 * acq_fft_doppler_batch and acq_fft_unit_batch (0 = the plan's choice; how many Doppler bins / (block, antenna) units are
 * transformed at a time: scratch and launch count, never the bits). */
GAT_API int32_t gat_acquire_fft(gat_ctx *ctx, const gat_signal_desc *signal, int32_t num_blocks, const int32_t *prns_host,
                                int32_t num_prns, double sampling_freq_hz, const gat_acq_config *config, float *power_dev,
                                gat_acq_result *results_host);

/* What gat_acquire_fft would do with a call, without a device.  unit_groups: the (block, antenna) units are dealt to this many
 * groups, each summed in unit order and the groups then in group order, where (PRN, Doppler, segment) alone gives fewer than two
 * workgroups per compute unit: the one plan parameter besides fft_log2 that enters the bits. */
typedef struct gat_acq_fft_plan {
    uint32_t struct_size;    /* sizeof(gat_acq_fft_plan), set by the caller                                       */
    int32_t fft_log2;        /* L: the transform has F = 2^L points                                               */
    int32_t num_segments;    /* G                                                                                 */
    int32_t segment_lags;    /* Jseg = F - N + 1                                                                  */
    int32_t passes;          /* 1: the transform stays in one workgroup (F <= 4096); 2: two passes through memory  */
    int32_t doppler_batch;   /* Doppler bins transformed at a time                                                */
    int32_t unit_batch;      /* (block, antenna) units whose spectra are held at a time                            */
    int32_t unit_groups;     /* Gu                                                                                */
    int64_t scratch_bytes;   /* of the context's scratch buffer                                                   */
} gat_acq_fft_plan;
/* config->code_length must be set (there is no bound table to take it from); fft_log2, doppler_batch, unit_batch: the options'
 * values (0 = the plan's choice); num_cus: the device's compute units (gat_device_info); own_power: 1 when the call would pass
 * power_dev = NULL.  Returns the refusal gat_acquire_fft would return for the same call, or GAT_OK with *plan filled. */
GAT_API int32_t gat_acquire_fft_plan(const gat_signal_desc *signal, int32_t num_blocks, int32_t num_prns, double sampling_freq_hz,
                                     const gat_acq_config *config, int32_t fft_log2, int32_t doppler_batch, int32_t unit_batch,
                                     int32_t num_cus, int32_t own_power, gat_acq_fft_plan *plan);

/* The twin: the same grid on the HOST, bit for bit what gat_acquire_fft writes when fft_log2 and unit_groups are the device
 * plan's (gat_acquire_fft_plan).  signal: a descriptor of host memory; codes_host: [rows x code_row_stride] chips, prns_host: rows;
 * fft_log2 10 .. 18 with 2^fft_log2 > N, 1 <= unit_groups <= num_blocks * num_ants; power_host: [num_prns x D x J].  Plain loops:
 * meant for small shapes. */
GAT_API int32_t gat_acquire_fft_host(const gat_signal_desc *signal, int32_t num_blocks, const int8_t *codes_host, int32_t code_length,
                                     int32_t code_row_stride, const int32_t *prns_host, int32_t num_prns, double sampling_freq_hz,
                                     const gat_acq_config *config, int32_t fft_log2, int32_t unit_groups, float *power_host);

/* ---- antenna-array processing: spatial covariance, beamformer weights, beamformed samples, accumulators and loop ----
 * The correlators return accumulators per antenna; what an array receiver does with its antennas happens here.
 * Correlation is linear -- w^H (sum_n x_n c_n) = sum_n (w^H x_n) c_n -- so a beam or a null is applied to the
 * accumulators the correlators already produce: one pass over the raw samples estimates the spatial covariance, a small
 * FP64 solver turns it into weights, and the weights enter where the loop forms its antenna sum.  The reference has no
 * counterpart (its antennas are identical and only summed). */
#define GAT_MAX_ARRAY_ANTS 64    /* antennas of the array functions                                            */
#define GAT_BF_CONVENTIONAL 0    /* w = a / (a^H a)                                                            */
#define GAT_BF_MVDR 1            /* w = R'^-1 a / (a^H R'^-1 a)                                                */
#define GAT_BF_POWER_INVERSION 2 /* w = R'^-1 e0 / (e0^H R'^-1 e0): no steering vector, antenna 0 is the reference */

/* Spatial covariance of the raw samples, one estimate per blocks_per_estimate consecutive blocks (the last estimate
 * takes what is left): E = ceil(num_blocks / blocks_per_estimate),
 *   R_e[i][j] = sum_{b in e} sum_{n<N} x[n,i,b] * conj(x[n,j,b])                      (a plain sum, not a mean)
 * cov_re/cov_im: dev float [E][M][M] planar.  Every sample layout, 1 <= M <= GAT_MAX_ARRAY_ANTS (else GAT_ERR_RANGE),
 * any N, base alignment and strides; chan_stride must be 0 (GAT_ERR_UNSUPPORTED).  M <= 8 with every block of every
 * antenna starting on a 16-byte boundary (the correlator's fast-path rule) streams the samples once with 16-byte loads
 * and keeps the upper triangle in registers; everything else is staged through LDS and tiled over the upper triangle.
 * The result is exactly Hermitian (only the upper triangle is computed; the mirror is its conjugate, the diagonal's
 * imaginary part is +0) and deterministic (workgroups write partial sums to slices of the context's scratch, a second
 * kernel adds them in a fixed order; no float atomics).  Sums are float32 in two levels; integer samples whose sums stay
 * below 2^24 (int8 pairs up to N = 256) come back exact. */
GAT_API int32_t gat_spatial_covariance(gat_ctx *ctx, const gat_signal_desc *signal, int32_t num_blocks,
                                       int32_t blocks_per_estimate, float *cov_re_dev, float *cov_im_dev);

/* Beamformer weights w [K][M] (planar, FP64) from ONE covariance [M][M] (planar float32, as gat_spatial_covariance
 * writes it; the lower triangle and the diagonal's real part are read) and K steering vectors a [K][M] (planar, FP64),
 * by `mode` (GAT_BF_*).  Diagonal loading: R' = R + loading * trace(R) / M * I, loading >= 0.  FP64 Cholesky R' = L L^H
 * (done once, shared by the K channels) and two triangular solves per channel.  GAT_BF_CONVENTIONAL reads no covariance
 * (cov_* may be NULL); GAT_BF_POWER_INVERSION reads no steering vector (steer_* may be NULL) and gives every channel the
 * same weights.  A covariance that is not positive definite (or a steering vector of zeros): NaN weights from the device
 * entry point -- the convention of bad channel records --, GAT_ERR_RANGE from the host one. */
GAT_API int32_t gat_array_weights(gat_ctx *ctx, const float *cov_re_dev, const float *cov_im_dev, int32_t num_ants,
                                  const double *steer_re_dev, const double *steer_im_dev, int32_t num_channels,
                                  int32_t mode, double loading, double *w_re_dev, double *w_im_dev);
/* The same arithmetic on the HOST (csrc/gat_array.h, shared with the device); all pointers are host memory.  Needs no
 * context and no device. */
GAT_API int32_t gat_array_weights_host(const float *cov_re_host, const float *cov_im_host, int32_t num_ants,
                                       const double *steer_re_host, const double *steer_im_host, int32_t num_channels,
                                       int32_t mode, double loading, double *w_re_host, double *w_im_host);

/* Beamformed accumulators: y[b][k][l] = sum_m conj(w[k][m]) * acc[b][k][l][m].  acc: dev float [B][K][L][M] (what the
 * correlators write), w: dev double [K][M] planar, out: dev float [B][K][L] planar. */
GAT_API int32_t gat_beamform(gat_ctx *ctx, const float *acc_re_dev, const float *acc_im_dev, int32_t num_blocks,
                             int32_t num_channels, int32_t num_taps, int32_t num_ants, const double *w_re_dev,
                             const double *w_im_dev, float *out_re_dev, float *out_im_dev);

/* Beams of the raw samples: y[n, j, b] = sum_m conj(w[j][m]) * x[n, m, b], 0 <= j < num_beams.
 * signal: any layout, 1 <= M <= GAT_MAX_ARRAY_ANTS, any N, base alignment and strides; chan_stride must be 0.
 * w: dev double [num_beams][M] planar, as gat_array_weights writes it; 1 <= num_beams <= GAT_MAX_ARRAY_ANTS.
 * out: describes device memory the call WRITES: layout GAT_LAYOUT_PLANAR or GAT_LAYOUT_INTERLEAVED (float32),
 *      num_ants == num_beams, num_samples == signal->num_samples, its own ant_stride and block_stride, chan_stride 0;
 *      beam j, block b, sample n goes to n + j*ant_stride + b*block_stride.  Nothing outside those elements is written.
 * The output descriptor can be handed unchanged to gat_acquire, gat_spatial_covariance and the correlators: as given it is
 * a num_beams-antenna signal; with num_ants = 1 and chan_stride = ant_stride it is one signal per channel (per-satellite
 * beams, each channel correlated on ONE stream instead of M).  This is how a null reaches the acquisition search, which
 * adds its antennas non-coherently and so takes a jammer at full strength.
 * Arithmetic: the weights are narrowed to float32 once; the sum runs in antenna order 0 .. M-1 with one FMA per real
 * product, in float32: |y - y64| <= (4M + 4) * 2^-24 * sum_m |w_m| |x_m| per sample.  The bits depend neither on the
 * kernel nor on the work split; integer samples convert exactly; NaN weights (what gat_array_weights writes for a
 * covariance that is not positive definite) give NaN samples and no error.  M <= 8 with every block of every antenna and of
 * every beam starting on a 16-byte boundary streams the samples once with 16-byte loads and stores for up to 4 beams (a
 * further pass per 4 more); everything else runs the scalar-load kernel (8 beams a pass).  gat_last_launch_info afterwards
 * describes this call: vec = 4 (streaming) or 1, workgroups, threads, splits (chunks of a block), ant_tile = M.
 * Enqueues on the context's stream and does not synchronise.  Refusals, all before any launch: GAT_ERR_ARG for null
 * pointers, num_blocks or num_beams < 1, negative strides, out->num_ants != num_beams, out->num_samples !=
 * signal->num_samples, a planar output without im or an interleaved one with im, and an output whose byte extent (either
 * plane, computed from the descriptor) overlaps the input's; GAT_ERR_RANGE for M or num_beams above 64;
 * GAT_ERR_UNSUPPORTED for an integer output layout or chan_stride != 0 on either side. */
GAT_API int32_t gat_beamform_samples(gat_ctx *ctx, const gat_signal_desc *signal, int32_t num_blocks,
                                     const double *w_re_dev, const double *w_im_dev, int32_t num_beams,
                                     const gat_signal_desc *out);

/* gat_tracking_update / gat_tracking_update_host / gat_tracking_run with the antenna sum of prompt, early and late
 * replaced by sum_m conj(w[k][m]) * R[m, tap]; w: double [K][M] planar (device memory for the device entry points, host
 * memory for the host one).  w_re = w_im = NULL is the unweighted call: the same code path and the same bits.  The
 * graph cache of gat_tracking_run is shared (the weight pointers are part of a recorded sequence's key). */
GAT_API int32_t gat_tracking_update_weighted(gat_ctx *ctx, const float *acc_re_dev, const float *acc_im_dev,
                                             int32_t num_channels, int32_t num_ants, const gat_loop_config *config_host,
                                             gat_loop_state *state_dev, const gat_channel_params *cur_dev,
                                             gat_channel_params *next_dev, const double *w_re_dev, const double *w_im_dev);
GAT_API int32_t gat_tracking_update_host_weighted(const float *acc_re_host, const float *acc_im_host, int32_t num_channels,
                                                  int32_t num_ants, const gat_loop_config *config_host,
                                                  gat_loop_state *state_host, const gat_channel_params *cur_host,
                                                  gat_channel_params *next_host, const double *w_re_host,
                                                  const double *w_im_host);
GAT_API int32_t gat_tracking_run_weighted(gat_ctx *ctx, const gat_signal_desc *sig, int32_t num_blocks, int32_t num_channels,
                                          int32_t num_taps, const int32_t *shifts_host, double sampling_freq_hz,
                                          const gat_loop_config *config_host, gat_loop_state *state_dev,
                                          gat_channel_params *params_a_dev, gat_channel_params *params_b_dev,
                                          float *acc_re_dev, float *acc_im_dev, int64_t acc_block_stride, uint32_t flags,
                                          int32_t *current_is_b, const double *w_re_dev, const double *w_im_dev);

/* ---- sample conditioning: level statistics, pulse blanking, AGC, requantisation ----------------------------------------
 * A stream-in, stream-out stage in front of everything else: measure the level of each antenna with pulses excluded
 * (gat_sample_stats), turn the measurement into a scale, a DC estimate and a blanking threshold on the device
 * (gat_agc_update), and write a conditioned stream, blanked and requantised (gat_condition_samples), that the search, the
 * covariance, the beamformer and the correlators take as a signal.  The fastest kernels read int8 pairs; this is what
 * produces them from a float front end.  The rule below is written so that the device, the host twin and a float32
 * restatement give the same bits.
 *   Blanking: a sample of antenna m is KEPT iff fabsf(re) <= T_m && fabsf(im) <= T_m on the raw sample (integer samples
 *     convert exactly).  A NaN component blanks its sample at any threshold, +inf included; a component equal to T is kept.
 *     With GAT_COND_BLANK_ALL_ANTS sample n is blanked on every antenna if it is blanked on any.
 *   A kept component: t = x - dc, then y = t * scale: one float32 subtraction, one float32 multiplication, never fused.
 *   Float outputs (planar, ComplexF32): y as is; a blanked sample is +0.0, +0.0.
 *   Integer outputs (int16 / int8 pairs): y rounded to nearest, ties to even, then clamped to +-32767 / +-127 (the most
 *     negative code is never written); a component whose rounded value was outside that range counts as clipped; a NaN y
 *     (NaN parameters only) writes 0 and counts as clipped; a blanked sample is 0, 0. */
typedef struct gat_cond_params { /* one per antenna, device- or host-resident */
    float scale;                 /* y = (x - dc) * scale */
    float dc_re, dc_im;
    float threshold;             /* on the RAW sample: blanked unless |re| <= T and |im| <= T; +inf: no blanking */
} gat_cond_params;
#define GAT_COND_BLANK_ALL_ANTS 1u /* a sample blanked on one antenna is blanked on all of them */

/* The conditioned stream.  signal: any layout, 1 <= M <= GAT_MAX_ARRAY_ANTS, any N, base alignment and strides,
 * chan_stride 0.  out: describes device memory the call WRITES, as in gat_beamform_samples: the same num_ants and
 * num_samples, its own layout (any of the four, the input's included) and strides; nothing outside the described elements
 * is written.  params_dev: M records.  counts_dev: uint64 [M][2] = {blanked samples, clipped components} of this call,
 * ADDED to what is there (the caller zeroes it; integer atomics, so the order does not matter), or NULL.
 * M <= 8 with every block of every antenna starting on a 16-byte boundary on both sides streams with 16-byte non-temporal
 * loads and 16-byte stores (a lane owns 4, or with an int8 side 8, consecutive samples of all antennas); everything else
 * runs one sample per lane with scalar loads and stores.  The bits are the same.  gat_last_launch_info afterwards: vec = 4
 * (streaming) or 1, workgroups, threads, splits (chunks of a block), ant_tile = M.  Enqueues on the context's stream and
 * does not synchronise; it allocates nothing.  Refusals, all before any launch: GAT_ERR_ARG for null pointers, num_blocks <
 * 1, sizes < 1, negative (or, where more than one antenna / block is described, zero) strides, unknown flags, out->num_ants
 * or out->num_samples different from the signal's, a planar side without im or an interleaved one with im, and an output
 * whose byte extent overlaps the input's unless the two descriptors are identical element for element (in place: the same
 * layout, planes and strides); GAT_ERR_RANGE for M above 64 or an extent beyond 9e15 samples; GAT_ERR_UNSUPPORTED for
 * chan_stride != 0 on either side. */
GAT_API int32_t gat_condition_samples(gat_ctx *ctx, const gat_signal_desc *signal, int32_t num_blocks,
                                      const gat_cond_params *params_dev, uint32_t flags, const gat_signal_desc *out,
                                      uint64_t *counts_dev);
/* The same rule in a plain loop on the HOST (csrc/gat_cond.h, shared with the device): every pointer is host memory; needs
 * no context and no device.  The bit-exact reference of the device call, with the same refusals. */
GAT_API int32_t gat_condition_samples_host(const gat_signal_desc *signal, int32_t num_blocks, const gat_cond_params *params_host,
                                           uint32_t flags, const gat_signal_desc *out, uint64_t *counts_host);

/* Level statistics, one record per (estimate, antenna): E = ceil(num_blocks / blocks_per_estimate) as in
 * gat_spatial_covariance, stats_dev [E][M].  The blanking rule is the one above; only `threshold` of the records is read,
 * params_dev == NULL keeps every sample without a NaN component.  The samples cross HBM once (M <= 8; more antennas run in
 * tiles of 8, and with GAT_COND_BLANK_ALL_ANTS a tile reads the other tiles' samples again for the verdict).  Every lane
 * sums in FP64; workgroups write their sums to slices of the context's scratch and a second kernel adds them in a fixed
 * order: no float atomics, the same bits on every call.  Counts and max_abs are exact; |sum - exact| <= 1e-5 * sum |x| per
 * component and sum_pow to a relative 1e-5 hold with a wide margin (integer samples: exact below 2^53). */
typedef struct gat_sample_stats_t {
    int64_t kept, blanked;
    double sum_re, sum_im, sum_pow; /* over kept samples: sum x, sum |x|^2 */
    float max_abs;                  /* largest |component| among kept samples; 0 if none */
    float pad_;
} gat_sample_stats_t;
GAT_API int32_t gat_sample_stats(gat_ctx *ctx, const gat_signal_desc *signal, int32_t num_blocks, int32_t blocks_per_estimate,
                                 const gat_cond_params *params_dev, uint32_t flags, gat_sample_stats_t *stats_dev);

/* One estimate's statistics [num_ants] into the next records [num_ants], on the device: sigma = sqrt(sum_pow / (2 kept))
 * (the RMS per component), scale = target_rms / sigma, dc = sum / kept if remove_dc else 0, threshold = blank_factor *
 * sigma (blank_factor <= 0: +inf).  FP64 throughout, narrowed once.  kept == 0 or sigma == 0 (or not finite): scale = 0,
 * dc = 0, threshold = +inf.  gat_sample_stats, gat_agc_update, gat_sample_stats again is the robust iteration: a pulse
 * inflates the first sigma, the second pass excludes it.  After a first call has sized the scratch, the three calls and
 * gat_condition_samples neither allocate nor read on the host: they can be captured in a stream graph. */
typedef struct gat_agc_config {
    uint32_t struct_size; /* sizeof(gat_agc_config) */
    double target_rms;    /* finite, >= 0 */
    double blank_factor;
    int32_t remove_dc;
} gat_agc_config;
GAT_API int32_t gat_agc_update(gat_ctx *ctx, const gat_sample_stats_t *stats_dev, int32_t num_ants, const gat_agc_config *cfg,
                               gat_cond_params *params_dev);
/* The same arithmetic on the HOST (csrc/gat_cond.h, shared with the device), to the last bit. */
GAT_API int32_t gat_agc_update_host(const gat_sample_stats_t *stats_host, int32_t num_ants, const gat_agc_config *cfg,
                                    gat_cond_params *params_host);

/* ---- sample filtering: complex FIR, decimation and an oscillator over the raw samples ------------------------------------
 * A stream-in, stream-out stage that changes a stream's band and rate: a notch against a CW tone, a channeliser from a
 * wideband front end down to the rate the search and the correlators are fast at.  For block b, antenna m and output
 * sample q (0 <= q < Q), with T complex float32 taps g, decimation D and blocks of N input samples:
 *     Q     = (N - T) / D + 1                    (integer division; N >= T)
 *     p     = q*D + (T-1)                        newest input sample of output q
 *     z     = sum_{t=0}^{T-1} g[t] * x[p - t]    "valid" convolution: nothing outside the block is read
 *     P     = b*block_stride(signal) + p         position in the antenna's stream
 *     theta = fma((double)P, step, phase)        cycles; step - rint(step) and phase - floor(phase) first (exact, but for
 *                                                a negative phase above -2^-53, which becomes 1.0)
 *     y     = (c - j s) * z                      (c, s): the library's float polynomial of exp(j 2 pi theta)
 * The sum runs in float32 in tap order from +0, per tap zr = fma(g_re, x_re, zr), zr = fma(-g_im, x_im, zr), zi =
 * fma(g_re, x_im, zi), zi = fma(g_im, x_re, zi); y_re = fma(s, z_im, c*z_re), y_im = fma(-s, z_re, c*z_im).  nco_step == 0
 * && nco_phase == 0 is the plain filter: y = z bit for bit.  Integer samples convert exactly; NaN and inf propagate by the
 * IEEE rules.  The bits depend neither on the kernel nor on the work split, and the host twin gives the same ones:
 *     |y - y64| <= [(2T + 8) * 2^-24 + 2 pi * 2^-53 * (P/2 + 2)] * sum_t (|g_re| + |g_im|)(|x_re| + |x_im|)  per component.
 * There is no state between calls: a continuous stream is described by overlapping blocks (overlap-save by descriptor:
 * input num_samples = Q*D + T - 1 and block_stride = Q*D, output block_stride = Q), and because the oscillator runs on the
 * stream position P every partition of one stream into blocks gives the same bits.  "Mix down by nu cycles/sample, then
 * low-pass with h" is this rule with g[t] = h[t] * exp(+j 2 pi nu t) and nco_step = nu: one sincos per output.
 * signal: any layout, 1 <= M <= GAT_MAX_ARRAY_ANTS, any base alignment and strides, overlapping blocks included,
 * chan_stride 0.  taps: T floats each, device memory (the host twin: host memory).  out: describes device memory the call
 * WRITES: GAT_LAYOUT_PLANAR or GAT_LAYOUT_INTERLEAVED float32, num_ants == M, num_samples == Q, its own strides; nothing
 * outside the described elements is written.  gat_acquire, gat_spatial_covariance, gat_beamform_samples, gat_sample_stats,
 * gat_condition_samples and the correlators take it unchanged.
 * With every block of every antenna starting on a 16-byte boundary on both sides a workgroup stages its samples through
 * LDS with 16-byte loads (the tiled kernel); everything else runs one output per lane with scalar loads.
 * gat_last_launch_info afterwards: vec = 1 (general) or the samples of a 16-byte load (tiled), workgroups, threads, splits
 * (chunks of a (block, antenna) pair's outputs), ant_tile = 1.  Enqueues on the context's stream, does not synchronise and
 * allocates nothing.  Refusals, all before any launch: GAT_ERR_ARG for null pointers, a wrong struct_size, num_blocks < 1,
 * bad sizes or strides, N < T, out->num_samples != Q, out->num_ants != M, a non-finite nco_step or nco_phase and an output
 * whose byte extent overlaps the input's (there is no in-place form: an output reads T inputs); GAT_ERR_RANGE for
 * num_taps or decimation outside their limits, M above 64 and (num_blocks - 1) * block_stride + N above 2^31 (theta is one
 * double rounding of a value below P/2; longer streams advance nco_phase per call); GAT_ERR_UNSUPPORTED for an integer
 * output layout or chan_stride != 0 on either side. */
#define GAT_MAX_FIR_TAPS 256
#define GAT_MAX_FIR_DECIMATION 64
typedef struct gat_fir_config {
    uint32_t struct_size; /* sizeof(gat_fir_config) */
    int32_t num_taps;     /* 1 .. GAT_MAX_FIR_TAPS */
    int32_t decimation;   /* 1 .. GAT_MAX_FIR_DECIMATION */
    double nco_step;      /* cycles per INPUT sample, finite */
    double nco_phase;     /* cycles, finite */
} gat_fir_config;
GAT_API int32_t gat_filter_samples(gat_ctx *ctx, const gat_signal_desc *signal, int32_t num_blocks, const float *taps_re_dev,
                                   const float *taps_im_dev, const gat_fir_config *cfg, const gat_signal_desc *out);
/* The same rule in a plain loop on the HOST (csrc/gat_fir.h, shared with the device): every pointer is host memory; needs
 * no context and no device.  The bit-exact reference of the device call, with the same refusals. */
GAT_API int32_t gat_filter_samples_host(const gat_signal_desc *signal, int32_t num_blocks, const float *taps_re_host,
                                        const float *taps_im_host, const gat_fir_config *cfg, const gat_signal_desc *out);

/* ---- space-time adaptive processing: the tapped covariance and the space-time sample filter --------------------------------
 * An M-antenna array nulls M - 1 interferers.  A tap delay line of T samples behind every antenna, all M*T coefficients
 * solved at once, has Q - 1 degrees of freedom, Q = M*T: narrow-band jammers are taken out in frequency as well as in space.
 * The space-time snapshot of block b at sample n, T - 1 <= n < N, is the Q-vector
 *     z[q] = x[n - t, m, b],  q = t*M + m          tap 0 is the newest sample; the antenna index runs fastest
 * and the solver is gat_array_weights with num_ants = Q, unchanged: GAT_BF_POWER_INVERSION constrains (tap 0, antenna 0);
 * GAT_BF_MVDR with a_st[t*M + m] = a[m] * (t == ref_tap) is distortionless for direction a at tap ref_tap (a = e_m: power
 * inversion referenced to (ref_tap, m)).  The filtered stream is then the input ADVANCED by d = T - 1 - ref_tap samples:
 * output n' shows the wanted signal of input sample n' + d, so a code phase found on y belongs to sample d of x. */
#define GAT_MAX_ST_TAPS 16 /* taps per antenna; num_ants * num_taps <= GAT_MAX_ARRAY_ANTS */

/* The space-time covariance, estimates grouped as in gat_spatial_covariance (E = ceil(num_blocks / blocks_per_estimate)):
 *   R_e[q][q'] = sum_{b in e} sum_{n = T-1}^{N-1} z_q[n] * conj(z_q'[n])           cov_re/cov_im: dev float [E][Q][Q] planar
 * The covariance method: every entry is summed over the same N - T + 1 snapshots, so R is positive semi-definite by
 * construction (it is not assembled from lag sums over differing ranges), and no snapshot reads outside its block.
 * The contract is gat_spatial_covariance's: every layout, any N >= T, any base alignment and strides, chan_stride 0; only
 * the upper triangle is computed, the mirror is its exact conjugate and the diagonal's imaginary part +0; two-level
 * float32 sums, per-workgroup slices added in a fixed order by the same finishing kernel, no float atomics: the same bits
 * every call; integer samples whose sums stay below 2^24 come back exact.  num_taps == 1 IS gat_spatial_covariance (the
 * call is forwarded: the same bits).  Otherwise a chunk of samples and the T - 1 samples in front of it are staged in LDS
 * once and the Q virtual antennas are shifted views of the M staged rows.  Refusals: gat_spatial_covariance's, and
 * GAT_ERR_RANGE for num_taps outside 1 .. GAT_MAX_ST_TAPS or num_ants * num_taps above GAT_MAX_ARRAY_ANTS, GAT_ERR_ARG
 * for N < num_taps. */
GAT_API int32_t gat_spacetime_covariance(gat_ctx *ctx, const gat_signal_desc *signal, int32_t num_blocks,
                                         int32_t blocks_per_estimate, int32_t num_taps, float *cov_re_dev, float *cov_im_dev);

/* The space-time filter: y[n', j, b] = sum_{q < Q} conj(w[j][q]) * z_q[n' + T - 1], 0 <= n' < N - T + 1, 0 <= j < num_beams.
 * signal: any layout, any base alignment and strides, overlapping blocks included, chan_stride 0, N >= T.
 * w: dev double [num_beams][Q] planar, exactly what gat_array_weights writes when called with num_ants = Q.
 * out: describes device memory the call WRITES: GAT_LAYOUT_PLANAR or GAT_LAYOUT_INTERLEAVED float32, num_ants ==
 *      num_beams, num_samples == N - T + 1, its own strides; nothing outside the described elements is written.  Every
 *      operator that takes a signal takes it unchanged; num_ants = 1 with chan_stride = ant_stride reads it as one signal
 *      per channel, as gat_beamform_samples documents.
 * Arithmetic: gat_beamform_samples' rule with the snapshot in place of the antenna vector: the weights are narrowed to
 * float32 once; one float32 sum from +0 in q order (all antennas of tap 0, then tap 1, ...), per element yr = fma(wr, xr,
 * yr), yr = fma(wi, xi, yr), yi = fma(wr, xi, yi), yi = fma(-wi, xr, yi):
 *     |y - y64| <= (4Q + 4) * 2^-24 * sum_q |w_q| |z_q|  per sample.
 * Integer samples convert exactly; NaN weights give NaN samples and no error.  The bits depend neither on the kernel nor
 * on the work split, the host twin gives the same ones, and num_taps == 1 IS gat_beamform_samples: after this call's own
 * refusals it is forwarded there (the same bits, kernels and launch info).
 * There is no state between calls: a continuous stream is overlapping blocks by descriptor, as for gat_filter_samples
 * (input num_samples = Qout + T - 1 and block_stride = Qout, output block_stride = Qout); every partition gives the same bits.
 * With more than one tap, every block of every antenna and of every beam on a 16-byte boundary and M <= 16, a workgroup stages a tile of
 * samples and its T - 1 sample halo of all antennas through LDS with 16-byte loads and a lane keeps the sums of up to 4
 * beams and 4 outputs in registers (a further pass per 4 more beams); everything else runs one output per lane with scalar
 * loads (8 beams a pass).  gat_last_launch_info afterwards describes this call as for the beams: vec = the samples of a
 * 16-byte load (tiled) or 1, workgroups, threads, splits (chunks of a block's outputs), ant_tile = M.  Enqueues on the
 * context's stream and does not synchronise.  Refusals, all before any launch: GAT_ERR_ARG for null pointers, num_blocks or
 * num_beams < 1, bad sizes or strides, N < T, out->num_ants != num_beams, out->num_samples != N - T + 1, a planar side
 * without im or an interleaved one with im, and an output whose byte extent overlaps the input's; GAT_ERR_RANGE for
 * num_taps outside 1 .. GAT_MAX_ST_TAPS, M * num_taps or num_beams above 64; GAT_ERR_UNSUPPORTED for an integer output
 * layout or chan_stride != 0 on either side. */
GAT_API int32_t gat_spacetime_filter(gat_ctx *ctx, const gat_signal_desc *signal, int32_t num_blocks, const double *w_re_dev,
                                     const double *w_im_dev, int32_t num_taps, int32_t num_beams, const gat_signal_desc *out);
/* The same rule in a plain loop on the HOST (csrc/gat_st.h, shared with the device): every pointer is host memory; needs
 * no context and no device.  The bit-exact reference of the device call, with the same refusals. */
GAT_API int32_t gat_spacetime_filter_host(const gat_signal_desc *signal, int32_t num_blocks, const double *w_re_host,
                                          const double *w_im_host, int32_t num_taps, int32_t num_beams,
                                          const gat_signal_desc *out);

/* ---- sample spectrum: the summed periodogram (Welch) of the raw samples, per block and antenna ----------------------------
 * How a receiver looks at the band it works in: where a tone sits before notch_taps can remove it, whether a level is
 * noise or a jammer.  F = num_bins (a power of two, 64 .. 4096), H = hop (1 .. F), w a real float32 window of F values,
 * blocks of N >= F samples, S = (N - F) / H + 1 segments a block (1 .. 4096).  For block b, antenna m, segment s:
 *     v[n]  = w[n] * x[s*H + n], 0 <= n < F        one rounded float32 product per component; integer samples convert
 *                                                  exactly; nothing outside the block is read, and the block's last
 *                                                  (N - F) mod H samples are not used
 *     tw[i] = (c, -s), 0 <= i < F/2                (c, s) the library's float polynomial of exp(j 2 pi i/F): i/F is exact
 *     X[f]  = sum_n v[n] exp(-j 2 pi f n / F)      by ONE sequence of operations: radix-2 decimation in time on the
 *                                                  bit-reversed v, stages j = 0 .. log2F - 1, h = 2^j, group g, k < h:
 *                 a = v[2hg + k], b = v[2hg + k + h], W = tw[k*F/(2h)]
 *                 t_re = fma(-W_im, b_im, W_re*b_re), t_im = fma(W_im, b_re, W_re*b_im)   (the inner product rounded)
 *                 a' = a + t, b' = a - t
 *     p     = fma(X_im, X_im, X_re*X_re)
 *     power[b][m][f] = sum_s p                     one float32 sum in segment order from +0
 * power: float32 [num_blocks][M][F], contiguous, in FFT order: bin f is f/F cycles per sample for f < F/2 and (f - F)/F
 * above.  It is the SUM over the segments, not the mean.  NaN and inf propagate by the IEEE rules: a NaN sample poisons
 * exactly the segments that hold it.  The bits depend neither on the kernel nor on the work split, and the host twin gives
 * the same ones.  With A = sum_n |w[n]| (|x_re| + |x_im|) of a segment and u = 2^-24 (DESIGN.md 4.10 derives them):
 *     |X - X64| <= E = (11 log2F + 1) u A                         per component, and in modulus
 *     |p - p64| <= (2A + E) E + 2u(1 + u) (A + E)^2               per bin of one segment
 *     |power - power64| <= sum_s [the above] + (S-1)u / (1 - (S-1)u) * sum_s (A + E)^2 (1 + 2u(1 + u)).
 * There is no state between calls: the averaging unit is the block.  A spectrogram is blocks of one segment (N = F); a
 * long stream is several blocks by descriptor (block_stride = S*H continues the segments; overlapping blocks are
 * allowed).  The sum over a block's segments is sequential by rule, so the work unit is a (block, antenna) pair and is
 * never split: parallelism comes from num_blocks * M.
 * signal: any layout, 1 <= M <= GAT_MAX_ARRAY_ANTS, any base alignment and strides, chan_stride 0.  window: F floats,
 * device memory (the host twin: host memory).  With every block of every antenna starting on a 16-byte boundary and H a
 * multiple of the samples one 16-byte load holds, the kernel loads with 16-byte loads; everything else runs scalar
 * loads.  gat_last_launch_info afterwards: vec = the samples per load (1: scalar), workgroups, threads = 256, splits = 1,
 * ant_tile = 1, lds_bytes, channels_per_wg = the (block, antenna) pairs a workgroup transforms side by side (256 lanes
 * hold one transform of F >= 1024, four of F = 256, sixteen of F = 64).  Enqueues on the context's stream, does not
 * synchronise and allocates nothing.  Refusals, all before any launch: GAT_ERR_ARG for null pointers, a wrong
 * struct_size, num_blocks < 1, bad sizes or strides, N < F, non-zero flags and an output whose byte extent overlaps the
 * input's; GAT_ERR_RANGE for num_bins not a power of two or outside its limits, hop outside 1 .. F, S above
 * GAT_MAX_SPECTRUM_SEGMENTS and M above 64; GAT_ERR_UNSUPPORTED for chan_stride != 0. */
#define GAT_MIN_SPECTRUM_BINS 64
#define GAT_MAX_SPECTRUM_BINS 4096
#define GAT_MAX_SPECTRUM_SEGMENTS 4096
typedef struct gat_spectrum_config {
    uint32_t struct_size; /* sizeof(gat_spectrum_config) */
    int32_t num_bins;     /* F: a power of two, GAT_MIN_SPECTRUM_BINS .. GAT_MAX_SPECTRUM_BINS */
    int32_t hop;          /* H: 1 .. num_bins */
    uint32_t flags;       /* 0 */
} gat_spectrum_config;
GAT_API int32_t gat_sample_spectrum(gat_ctx *ctx, const gat_signal_desc *signal, int32_t num_blocks, const float *window_dev,
                                    const gat_spectrum_config *cfg, float *power_dev);
/* The same rule in a plain loop on the HOST (csrc/gat_spec.h, shared with the device): every pointer is host memory; needs
 * no context and no device.  The bit-exact reference of the device call, with the same refusals. */
GAT_API int32_t gat_sample_spectrum_host(const gat_signal_desc *signal, int32_t num_blocks, const float *window_host,
                                         const gat_spectrum_config *cfg, float *power_host);

/* ---- tracking monitor: C/N0, phase lock, bit synchronisation and data symbols from the accumulator history ----------------
 * What a receiver asks of its tracking channels, computed from the accumulators gat_tracking_run (or the correlator) left
 * on the device: B blocks, block b at acc + b * acc_block_stride floats, element [k][l][m] at (k*L + l)*M + m.  Everything
 * is double precision, every sum is sequential from +0 in the stated order and every expression is evaluated as written
 * (csrc/gat_mon.h, shared by the kernels and the host twin: the same bits); no transcendental function and no sqrt is
 * evaluated: the call writes raw sums, and decibels are made by the caller (below).
 *   prompt   P[k][b] = the loop's prompt (gat_tracking_update): sum_m acc[b][k][prompt_index][m], or with weights
 *            sum_m conj(w[k][m]) * acc, in m order: re += wr*ar + wi*ai, im += wr*ai - wi*ar.  I = re P, Q = im P.
 *   windows  W = window_blocks, NW = ceil(B / W), the last window takes what is left.  Window v of channel k, over its
 *            blocks in order: sum_p2 = sum (I*I + Q*Q), sum_p4 = sum (I*I + Q*Q)*(I*I + Q*Q), sum_d = sum (I*I - Q*Q),
 *            sum_i = sum I, sum_q = sum Q, blocks.
 *   symbols  Pd = symbol_blocks (1 .. GAT_MAX_SYMBOL_BLOCKS) blocks make one data symbol; overlay[0 .. Pd) holds the
 *            secondary code as +1 / -1 (all +1 for GPS L1 C/A with Pd = 20; NH10 0000110101 for L5 I5, NH20
 *            00000100110101001110 for L5 Q5, a 0 bit being +1).  For a call-relative start c and symbol j
 *                S[c][j] = sum_{i < Pd} overlay[i] * P[k][c + j*Pd + i]     re and im apart, in i order
 *                wbp[c][j] = sum_i (I*I + Q*Q)                              over the same blocks
 *   bit sync J = floor((B - Pd + 1) / Pd) symbols for EVERY candidate c = 0 .. Pd-1, E[k][c] = sum_{j < J} (Sr*Sr + Si*Si)
 *            in j order, and c* = the lowest c with the largest E.  J = 0: c* = -1, no symbols, E = 0.  |S|^2 needs no
 *            phase lock and works under a secondary code, where a histogram of sign changes does not.  A forced
 *            symbol_offset = o >= 0 sets c* = (o - first_block) mod Pd and skips the choice (E is computed all the same).
 *   record   per channel: symbol_offset = (first_block + c*) mod Pd, the offset in terms of the STREAM (first_block: the
 *            stream's block number of this call's block 0), start = c*, num_symbols = floor((B - c*) / Pd), e_max = E[c*],
 *            e_second = the largest E at another c (0 if Pd = 1).  With c* = -1: -1, -1, 0, 0, 0.
 *   demod    symbol j < num_symbols of channel k is S[c*][j] (sym_re, sym_im) with wbp[c*][j] (sym_wbp); entries from
 *            num_symbols to the capacity floor(B / Pd) are written as 0.
 * What the caller makes of the sums (T = the block's seconds):
 *   phase lock   sum_d / sum_p2: an estimate of cos 2 phi that does not depend on the data bits
 *   C/N0 (moments)  M2 = sum_p2 / blocks, M4 = sum_p4 / blocks, Ps = sqrt(2 M2^2 - M4) (no estimate where the radicand
 *                is <= 0), C/N0 = 10 log10(Ps / ((M2 - Ps) T)) dB-Hz
 *   C/N0 (narrow-to-wide power ratio)  mu = mean over the symbols of |S|^2 / wbp, C/N0 = 10 log10((mu - 1) / ((Pd - mu) T))
 *                (no estimate for Pd = 1 or mu outside (1, Pd))
 *   bits         the sign of sym_re; the Costas loop's half-cycle ambiguity is left in (one sign per channel)
 * Both C/N0 estimators read low when a bit edge falls inside a block.
 * There is no state between calls: a continuing stream passes first_block and, once synchronised, the forced offset.
 * Outputs, every one optional (null: not written; at least one is given): prompt_re / prompt_im double [K][B]; windows
 * [K][NW]; energy double [K][Pd]; channels [K]; sym_re / sym_im / sym_wbp double [K][floor(B / Pd)] (nothing is written
 * where that is 0).  w_re / w_im: double [K][M] as gat_array_weights writes them, both or neither.
 * The call enqueues on the context's stream, does not synchronise and allocates nothing but the context's scratch; c* is
 * chosen on the device and read there by the kernel that writes the symbols.  No atomics: the same bits every call.
 * Refusals, all before any launch (the host twin: before any write): GAT_ERR_ARG for a null accumulator pointer or
 * config, a wrong struct_size, num_blocks, num_channels, num_ants or num_taps < 1, window_blocks < 1, an overlay entry
 * that is not +1 or -1, first_block < 0, acc_block_stride < K*L*M with more than one block, one weight pointer without
 * the other and a call with every output null; GAT_ERR_RANGE for num_ants above GAT_MAX_ARRAY_ANTS, num_blocks above 2^20,
 * num_channels above 4096, prompt_index outside [0, num_taps), symbol_blocks outside 1 .. GAT_MAX_SYMBOL_BLOCKS,
 * symbol_offset outside -1 .. Pd-1 and a call whose scratch would exceed 1 GiB (about 3 * 8 * K * B bytes). */
#define GAT_MAX_SYMBOL_BLOCKS 128
#define GAT_MAX_MONITOR_BLOCKS 1048576
#define GAT_MAX_MONITOR_CHANNELS 4096
typedef struct gat_monitor_config {
    uint32_t struct_size;  /* sizeof(gat_monitor_config) */
    int32_t num_taps;      /* L of the accumulators */
    int32_t prompt_index;  /* 0 .. L-1, the loop configuration's */
    int32_t window_blocks; /* W >= 1 */
    int32_t symbol_blocks; /* Pd: 1 .. GAT_MAX_SYMBOL_BLOCKS */
    int32_t symbol_offset; /* -1: search; 0 .. Pd-1: forced, in stream terms */
    int64_t first_block;   /* >= 0: the stream's number of this call's block 0 */
    int8_t overlay[128];   /* [0 .. Pd): +1 / -1; the rest is ignored */
} gat_monitor_config;
typedef struct gat_monitor_window {
    double sum_p2, sum_p4, sum_d, sum_i, sum_q;
    int64_t blocks;
} gat_monitor_window;
typedef struct gat_monitor_channel {
    int32_t symbol_offset; /* (first_block + start) mod Pd, or -1 */
    int32_t start;         /* c*: the call's block at which symbol 0 begins, or -1 */
    int32_t num_symbols;
    int32_t reserved;
    double e_max, e_second;
} gat_monitor_channel;
GAT_API int32_t gat_track_monitor(gat_ctx *ctx, const float *acc_re_dev, const float *acc_im_dev, int64_t acc_block_stride,
                                  int32_t num_blocks, int32_t num_channels, int32_t num_ants, const gat_monitor_config *config,
                                  const double *w_re_dev, const double *w_im_dev, double *prompt_re, double *prompt_im,
                                  gat_monitor_window *windows, double *energy, gat_monitor_channel *channels, double *sym_re,
                                  double *sym_im, double *sym_wbp);
/* The same rule in plain loops on the HOST (csrc/gat_mon.h, shared with the device): every pointer is host memory; needs
 * no context and no device.  The bit-exact reference of the device call, with the same refusals. */
GAT_API int32_t gat_track_monitor_host(const float *acc_re_host, const float *acc_im_host, int64_t acc_block_stride,
                                       int32_t num_blocks, int32_t num_channels, int32_t num_ants, const gat_monitor_config *config,
                                       const double *w_re_host, const double *w_im_host, double *prompt_re, double *prompt_im,
                                       gat_monitor_window *windows, double *energy, gat_monitor_channel *channels, double *sym_re,
                                       double *sym_im, double *sym_wbp);
/* What gat_track_monitor would do with a call (csrc/gat_mon_plan.h; no context, no device, nothing is read but config):
 * the counts, the bytes of context scratch and the workgroups of each kernel (256 threads each; the window kernel gives
 * one wave of 64 lanes to a window).  own_prompts: the caller passes no prompt buffers, the series lives in the scratch;
 * want_symbols: one of energy, channels and the symbol outputs is asked for.  The refusals are the call's. */
typedef struct gat_monitor_plan {
    uint32_t struct_size; /* sizeof(gat_monitor_plan), set by the caller */
    int32_t num_windows;      /* NW */
    int32_t search_symbols;   /* J */
    int32_t symbol_capacity;  /* floor(B / Pd) */
    int32_t prompt_workgroups, window_workgroups, term_workgroups, energy_workgroups, pick_workgroups, symbol_workgroups;
    int64_t scratch_bytes;
} gat_monitor_plan;
GAT_API int32_t gat_track_monitor_plan(int64_t acc_block_stride, int32_t num_blocks, int32_t num_channels, int32_t num_ants,
                                       const gat_monitor_config *config, int32_t own_prompts, int32_t want_symbols,
                                       gat_monitor_plan *plan);

/* ---- subspace: the accumulators' covariance, a batched Hermitian eigensolver and with them the steering estimate ---------
 * An uncalibrated array does not know its steering vectors.  The prompt accumulators of a tracking channel are
 * A * a + noise per block; their covariance over the blocks is |A|^2 a a^H + noise, without the data bits and without the
 * loop's common phase error, and its principal eigenvector is the steering vector as the receiver's own hardware sees it
 * (the eigenbeamformer).  Everything is double precision and every expression is evaluated as written (csrc/gat_eig.h,
 * shared by the kernels and the host twins: the same bits); sqrt and / are IEEE.
 *
 * gat_accumulator_covariance: the accumulators are gat_track_monitor's (B blocks, block b at acc + b * acc_block_stride
 * floats, element [k][l][m] at (k*L + l)*M + m).  blocks_per_estimate <= 0 (or >= B): one estimate of all blocks; else
 * E = ceil(B / blocks_per_estimate) estimates, the last taking what is left.  cov_re / cov_im: double [E][K][M][M].
 *   x_m = (double) acc[b][k][tap_index][m].  For i >= j the term of a block is
 *       re = xr_i*xr_j + xi_i*xi_j        im = xi_i*xr_j - xr_i*xi_j          (x_i conj(x_j); the products are exact)
 *   The sum of an estimate has two levels: chunks of GAT_ACC_COV_CHUNK consecutive blocks of the estimate (the last chunk
 *   shorter), each summed in block order from +0, and the chunk sums added in chunk order from +0.  Entry [j][i] is the
 *   conjugate (re, -im) of entry [i][j]; the diagonal's imaginary part is written as +0.
 * Whether the chunk sums pass through the context's scratch to a second kernel or one workgroup walks its chunks is the
 * plan's choice (gat_subspace_plan) and does not change a bit.  No atomics: the same bits every call.  NaN accumulators
 * give NaN entries, not an error.  Refusals, before any launch (the host twin: before any write): GAT_ERR_ARG for a null
 * pointer, num_blocks, num_channels, num_taps or num_ants < 1 and acc_block_stride < K*L*M with more than one block;
 * GAT_ERR_RANGE for num_ants above GAT_MAX_ARRAY_ANTS, num_blocks above 2^20, num_channels above 4096, tap_index outside
 * [0, num_taps), more than 2^31 - 1 workgroups and a call whose scratch would exceed 1 GiB (with fewer than 512 (estimate,
 * channel) pairs the chunk sums take 16 bytes for every chunk and lower-triangle entry of each: fewer blocks a call).
 *
 * gat_hermitian_eig: n Hermitian matrices of order Q (1 .. GAT_MAX_ARRAY_ANTS), planar [n][Q][Q], double or -- with
 * GAT_EIG_INPUT_F32 -- float (what gat_spatial_covariance and gat_spacetime_covariance write).  Only the lower triangle
 * and the diagonal's real part are read, as in gat_array_weights.  Outputs, each optional (null: not written; at least one
 * is given): eigenvalues double [n][Q], descending; vec_re / vec_im double [n][R][Q], row r the eigenvector of eigenvalue
 * r, R = num_vectors in 0 .. Q (both planes or neither; R = 0: nothing is written to them) -- with R = 1 the [K][M]
 * steering layout gat_array_weights reads --; status int32 [n]: >= 0 the sweeps used, -1 not converged within
 * GAT_EIG_MAX_SWEEPS (the outputs as they stand), -2 a non-finite input or Frobenius sum (the outputs are NaN).
 *   The method is cyclic Jacobi in the round-robin ordering.  n' = Q rounded up to even, idx = 0 .. n'-1; a round rotates
 *   the pairs (idx[i], idx[n'-1-i]), i < n'/2, p the smaller index, pairs with the dummy index Q skipped; after a round
 *   idx <- [idx[0], idx[n'-1], idx[1], .., idx[n'-2]]; n'-1 rounds make a sweep.  With b = A[p][q] a pair is rotated iff
 *   br*br + bi*bi > 2^-104 * F, F = the sum of re*re + im*im over the input matrix in row-major order from +0.  Then
 *       |b| = sqrt(br*br + bi*bi)   u = b / |b|   tau = (A[q][q] - A[p][p]) / (2 |b|)
 *       t = sign(tau) / (|tau| + sqrt(1 + tau*tau)), sign(0) = +1     c = 1 / sqrt(1 + t*t)     s = t*c     g = s*u
 *       J[p][p] = J[q][q] = c, J[p][q] = g, J[q][p] = -conj(g).
 *   All rotations of a round come from the same A; then A <- A J and V <- V J (V starts as the identity):
 *       x_p' = c x_p - conj(g) x_q:  re = c*xpr - (gr*xqr + gi*xqi)      im = c*xpi - (gr*xqi - gi*xqr)
 *       x_q' = g x_p + c x_q:        re = (gr*xpr - gi*xpi) + c*xqr      im = (gr*xpi + gi*xpr) + c*xqi
 *   then A <- J^H A:
 *       y_p' = c y_p - g y_q:        re = c*ypr - (gr*yqr - gi*yqi)      im = c*ypi - (gr*yqi + gi*yqr)
 *       y_q' = conj(g) y_p + c y_q:  re = (gr*ypr + gi*ypi) + c*yqr      im = (gr*ypi - gi*ypr) + c*yqi
 *   with A[p][q] = A[q][p] = 0 and the imaginary parts of A[p][p] and A[q][q] set to +0.  A pair that is not rotated leaves
 *   its rows and columns as they are.  A sweep that rotates nothing ends the iteration; the status counts the sweeps before
 *   it.  The eigenvalues are the diagonal, sorted descending with ties to the lower index; eigenvector r is the column of V
 *   of eigenvalue r times the unit factor conj(v_m) / |v_m| of its component of largest re*re + im*im (the lowest index of
 *   the largest), which itself is written as (|v_m|, +0).
 * Refusals, before any launch: GAT_ERR_ARG for a null input plane, every output null, n < 1, one vector plane without the
 * other and an unknown flag; GAT_ERR_RANGE for Q outside 1 .. GAT_MAX_ARRAY_ANTS and num_vectors outside 0 .. Q.
 * Both device calls enqueue on the context's stream and do not synchronise. */
#define GAT_ACC_COV_CHUNK 256
#define GAT_EIG_MAX_SWEEPS 60
#define GAT_EIG_INPUT_F32 1u
GAT_API int32_t gat_accumulator_covariance(gat_ctx *ctx, const float *acc_re_dev, const float *acc_im_dev, int64_t acc_block_stride,
                                           int32_t num_blocks, int32_t num_channels, int32_t num_taps, int32_t num_ants,
                                           int32_t tap_index, int32_t blocks_per_estimate, double *cov_re, double *cov_im);
GAT_API int32_t gat_hermitian_eig(gat_ctx *ctx, const void *a_re_dev, const void *a_im_dev, int32_t num_matrices, int32_t order,
                                  int32_t num_vectors, uint32_t flags, double *eigenvalues, double *vec_re, double *vec_im,
                                  int32_t *status);
/* The same rules in plain loops on the HOST (csrc/gat_eig.h, shared with the device): every pointer is host memory; no
 * context and no device.  The bit-exact references of the device calls, with the same refusals. */
GAT_API int32_t gat_accumulator_covariance_host(const float *acc_re_host, const float *acc_im_host, int64_t acc_block_stride,
                                                int32_t num_blocks, int32_t num_channels, int32_t num_taps, int32_t num_ants,
                                                int32_t tap_index, int32_t blocks_per_estimate, double *cov_re, double *cov_im);
GAT_API int32_t gat_hermitian_eig_host(const void *a_re_host, const void *a_im_host, int32_t num_matrices, int32_t order,
                                       int32_t num_vectors, uint32_t flags, double *eigenvalues, double *vec_re, double *vec_im,
                                       int32_t *status);
/* What the two calls would do (csrc/gat_eig_plan.h; no context, no device, nothing is read): num_blocks = 0 leaves the
 * covariance out (its fields are 0), eig_matrices = 0 the eigensolver; one of them is planned.  cov_split = 1: one workgroup
 * per (estimate, channel, chunk) writes chunk sums to the scratch and a second kernel adds them; 0: one workgroup per
 * (estimate, channel) walks its chunks.  The eigensolver runs one workgroup per matrix.  The refusals are the calls'. */
typedef struct gat_subspace_plan_info {
    uint32_t struct_size; /* sizeof(gat_subspace_plan_info), set by the caller */
    int32_t num_estimates;       /* E */
    int32_t chunks_per_estimate; /* of a full estimate */
    int32_t cov_split;
    int32_t cov_workgroups, cov_threads, cov_lds_bytes, cov_reduce_workgroups;
    int32_t eig_workgroups, eig_threads, eig_lds_bytes;
    int32_t reserved;
    int64_t scratch_bytes;
} gat_subspace_plan_info;
GAT_API int32_t gat_subspace_plan(int64_t acc_block_stride, int32_t num_blocks, int32_t num_channels, int32_t num_taps,
                                  int32_t num_ants, int32_t tap_index, int32_t blocks_per_estimate, int32_t eig_matrices,
                                  int32_t eig_order, int32_t eig_vectors, gat_subspace_plan_info *plan);

/* ---- navigation data: frame synchronisation, LNAV parity, CNAV Viterbi decoding and CRC-24Q ------------------------------
 * What a receiver makes of the monitor's data symbols: where a subframe begins, whether the Costas loop locked to the
 * carrier or to its negative, and which words passed their check.  The input is gat_track_monitor's sym_re, double
 * [K][symbol_capacity], with the monitor's channel records (null: every row is full) telling how many symbols n_k =
 * clamp(num_symbols, 0, symbol_capacity) of a row count; the records are read on the device.  A positive symbol is a 0
 * bit, a non-finite symbol counts as 0.  Everything is integer arithmetic but for the quantiser's scale, every sum is
 * sequential in the stated order and every expression is evaluated as written (csrc/gat_nav.h, shared by the kernels and
 * the host twin: the same bits).  The yardstick is IS-GPS-200 (LNAV, CNAV, CRC-24Q) and IS-GPS-705 (L5).
 *   bits     GAT_NAV_LNAV: one phase (P = 1), bit j = sym_re[j] < 0, n_k bits.  GAT_NAV_CNAV: two phases (P = 2), the
 *            symbols quantised and decoded by a Viterbi decoder from either symbol of a pair, T = floor((n_k - ph) / 2)
 *            bits of phase ph.  bit_capacity = symbol_capacity / P.
 *   quantise partial sum l < 64 adds |x[l]|, |x[l + 64]|, .. in that order from +0, S adds the 64 partials in l order from
 *            +0, unit = S / n_k; unit not finite or not > 0: every q = 0; else v = (x * 16.0) / unit, q = 127 for v >= 127,
 *            -127 for v <= -127, else (int) rint(v).
 *   decode   G1 = 171, G2 = 133 (octal; the MSB is the current input: G1 taps delays 0 1 2 3 6, G2 delays 0 2 3 5 6),
 *            G1's symbol first, neither inverted.  The state holds the six previous inputs, the newest in bit 5: s' =
 *            (u << 5) | (s >> 1), the predecessors of s' are ((s' & 31) << 1) | b.  Step t of phase ph reads q[ph + 2t] and
 *            q[ph + 2t + 1]; the metrics are int32, 0 in every state at the start, the branch metric is (1 - 2 c1) q0 +
 *            (1 - 2 c2) q1, the larger sum survives and a tie keeps b = 0; nothing is normalised (at most 254 a step).
 *            The traceback starts at the final state of the largest metric (the lowest on a tie), which is
 *            path_metric[k][ph]; the bit of step t is bit 5 of the state after step t.
 *   frames   a candidate is (ph, o, p): phase, offset o in 0 .. 299, polarity p XORed to every bit.  Frame f covers bits
 *            o + 300 f .. o + 300 f + 299; only frames wholly inside the n_k bits (LNAV) or inside bits [0, T -
 *            GAT_NAV_TAIL_BITS) (CNAV) count.  LNAV: a word is held in 32 bits, D29* in bit 31, D30* in bit 30, d1 .. d24
 *            in bits 29 .. 6, D25 .. D30 in bits 5 .. 0; with bit 30 set it is XORed with 0x3FFFFFC0; parity bit i = the
 *            parity of word & mask[i], masks 0xBB1F3480 0x5D8F9A40 0xAEC7CD00 0x5763E680 0x6BB1F340 0x8B7A89C0.  Word 1
 *            is checked with D29* = D30* = 0, word w > 1 with bits 29 and 30 of word w - 1.  A frame hits when its first
 *            eight bits are 10001011, words 1 and 2 pass, bits 29 and 30 of word 2 are 0 and the subframe ID (d20 .. d22 of
 *            word 2) is in 1 .. 5.  CNAV: a frame hits when its first eight bits are 10001011 and CRC-24Q (polynomial
 *            0x1864CFB, initial value 0, MSB first, not reflected) over its 300 bits is 0.
 *   choice   score = the hitting frames of a candidate; the largest score wins, ties to the lowest ph, then the lowest o,
 *            then p = 0; second_score = the largest score of any other candidate.  score < min_frames: no sync --
 *            frame_offset = -1, symbol_phase = inverted = num_frames = tow_steps = 0, num_bits of phase 0.
 *   record   every whole frame of the chosen candidate, up to max_frames, hit or not; rows from num_frames on are zero.
 *            status bit 0: the preamble; LNAV bits 1 .. 10: the parity of words 1 .. 10; CNAV bit 1: the CRC.  words:
 *            LNAV d1 .. d24 (D30* removed) in bits 29 .. 6 and the received parity in bits 5 .. 0; CNAV message bits
 *            30 i + 1 .. 30 i + 30 in bits 29 .. 0 of word i.  LNAV: tow = d1 .. d17 of word 2, id = the subframe ID, prn =
 *            0; CNAV: prn = bits 9 .. 14, id = bits 15 .. 20 (the message type), tow = bits 21 .. 37.  tow_steps counts the
 *            neighbouring pairs of written frames with every status bit set and tow[f + 1] = (tow[f] + 1) mod 100800.
 * Outputs, every one optional (null: not written; at least one is given): channels [K]; frames [K][max_frames]; decoded
 * uint8 [K][P][bit_capacity], the bits of every phase before the polarity, 0 from a row's count on; path_metric int32
 * [K][P] (LNAV: 0).  symbol_capacity = 0 and n_k = 0 are legal: no sync, zeros.  There is no state between calls.
 * The call enqueues on the context's stream, does not synchronise and allocates nothing but the context's scratch; the
 * choice is made on the device and read there by the kernel that writes the frames.  No atomics: the same bits every call.
 * Refusals, all before any launch (the host twin: before any write): GAT_ERR_ARG for a null sym_re or config, a wrong
 * struct_size, num_channels < 1, symbol_capacity < 0, max_frames or min_frames < 1, an unknown format and a call with
 * every output null; GAT_ERR_RANGE for num_channels above GAT_MAX_MONITOR_CHANNELS, symbol_capacity above
 * GAT_MAX_MONITOR_BLOCKS, num_channels * max_frames above 2^31 - 1 workgroups of 256 and a call whose scratch would exceed
 * 1 GiB (CNAV: about 10 bytes for every symbol of the capacity). */
#define GAT_NAV_LNAV 0        /* GPS L1 C/A legacy message: hard bits, 300-bit subframes of ten 30-bit words, (32,26) parity */
#define GAT_NAV_CNAV 1        /* GPS L5 I5 (and L2C) CNAV: rate-1/2 K=7 FEC symbols, 300-bit messages, CRC-24Q */
#define GAT_NAV_FRAME_BITS 300
#define GAT_NAV_TAIL_BITS 32  /* CNAV: decoded bits this close to the end of the traceback are not searched for frames */
typedef struct gat_nav_config {
    uint32_t struct_size;     /* sizeof(gat_nav_config) */
    int32_t format;           /* GAT_NAV_LNAV or GAT_NAV_CNAV */
    int32_t symbol_capacity;  /* row stride of sym_re: the monitor's floor(B / Pd) */
    int32_t max_frames;       /* rows of `frames` per channel, >= 1 */
    int32_t min_frames;       /* >= 1: a score below it means no sync */
} gat_nav_config;
typedef struct gat_nav_channel {
    int32_t frame_offset;     /* decoded-bit index of bit 1 of frame 0, or -1 */
    int32_t symbol_phase;     /* CNAV: 0 / 1, which symbol starts a pair; LNAV: 0 */
    int32_t inverted;         /* 1: every bit of this channel was inverted */
    int32_t score;
    int32_t second_score;     /* the best score of any other (phase, offset, polarity) */
    int32_t num_frames;
    int32_t num_bits;         /* decoded bits of the chosen phase */
    int32_t tow_steps;
} gat_nav_channel;
typedef struct gat_nav_frame {
    int32_t status;
    int32_t tow;
    int32_t id;
    int32_t prn;
    uint32_t words[10];
} gat_nav_frame;
GAT_API int32_t gat_nav_decode(gat_ctx *ctx, const double *sym_re_dev, const gat_monitor_channel *mon_channels_dev,
                               int32_t num_channels, const gat_nav_config *config, gat_nav_channel *channels,
                               gat_nav_frame *frames, uint8_t *decoded, int32_t *path_metric);
/* The same rule in plain loops on the HOST (csrc/gat_nav.h, shared with the device): every pointer is host memory; needs
 * no context and no device.  The bit-exact reference of the device call, with the same refusals. */
GAT_API int32_t gat_nav_decode_host(const double *sym_re_host, const gat_monitor_channel *mon_channels_host, int32_t num_channels,
                                    const gat_nav_config *config, gat_nav_channel *channels, gat_nav_frame *frames,
                                    uint8_t *decoded, int32_t *path_metric);
/* What gat_nav_decode would do with a call (csrc/gat_nav_plan.h; no context, no device, nothing is read but config; sized
 * by symbol_capacity): the counts, the bytes of context scratch and the workgroups of each kernel -- slice (LNAV), score
 * and frames 256 threads a workgroup, quantise (one channel) and trellis (one channel and phase) one wave of 64 lanes a
 * workgroup, the choice one wave a channel, four to a workgroup.  The plan is that of a call with every output given (a
 * call without `decoded` keeps the bits in the scratch besides: K * P * bit_capacity bytes more).  The refusals are the call's. */
typedef struct gat_nav_plan {
    uint32_t struct_size; /* sizeof(gat_nav_plan), set by the caller */
    int32_t num_phases;       /* P */
    int32_t bit_capacity;     /* symbol_capacity / P */
    int32_t num_candidates;   /* P * 300 * 2 a channel */
    int32_t slice_workgroups, quantise_workgroups, trellis_workgroups, score_workgroups, pick_workgroups, frame_workgroups;
    int64_t scratch_bytes;
} gat_nav_plan;
GAT_API int32_t gat_nav_decode_plan(int32_t num_channels, const gat_nav_config *config, gat_nav_plan *plan);

/* ---- position fix: LNAV ephemeris, satellite states and a batched least-squares solver -----------------------------------
 * What a receiver makes of the checked words and of its observables: an ephemeris from subframes 1 - 3, the satellite's
 * clock and ECEF position at the time of transmission, and per measurement epoch the receiver's position and clock bias by
 * iterated weighted least squares.  GPS LNAV, L1 single frequency (T_GD applied), no atmosphere model.  The yardstick is
 * the user algorithm of IS-GPS-200 (tables 20-I .. 20-IV).  FP64 throughout, every expression evaluated as written without
 * contraction, every sum over satellites in channel order from +0 (an unused channel adds nothing), and no libm
 * transcendental: + - * /, sqrt, rint and explicit fused multiply-adds only (csrc/gat_fix.h, shared by the kernel and the
 * host twin: the same bits).
 *   sincos   q = rint(x * 2/pi); r = x - q P1 - q P2 - q P3 by three fused multiply-adds, P1 and P2 the first and second 33
 *            bits of pi/2, P3 the rest; sin and cos of r by the Taylor polynomials of degree 17 and 18 in Horner form;
 *            the quadrant from q mod 4, taken in doubles (q - 4 floor(q / 4), exact for every finite q; 0 where q is not
 *            finite).  |error| <= 1e-15 on |x| <= 72 (Omega reaches +-69.3).  Beyond the reduction's range -- |x| above
 *            2^20, which an ephemeris that is usable below can reach: sqrt_a = 0.004 gives M = 1e18 -- the results are
 *            defined for every x and equal on the device and on the host, but are not a sine and a cosine and need not lie
 *            in [-1, 1]: such a channel counts with a meaningless finite state, or does not count where it is not finite.
 *   times    a time of the week is whole milliseconds (int32, 0 .. 604799999) and a fraction in seconds (double, [0, 1e-3)).
 *            Transmission tx_ms, tx_frac [E][K]; reception (nominal, by the receiver's clock) rx_ms, rx_frac [E].  A
 *            negative ms or a non-finite fraction: no measurement (of the channel; of the whole epoch for rx).
 *            t_sv = tx_ms * 1e-3 + tx_frac; rho = c (1e-3 wrap(rx_ms - tx_ms) + (rx_frac - tx_frac)), the wrap into
 *            [-302400000, 302400000) in integers.  Differences of seconds wrap into [-302400, 302400).
 *   clock    dt = wrap(t_sv - toc); dts = af0 + af1 dt + af2 dt dt + F e sqrt_a sin E - tgd with E solved at t_sv;
 *            t = t_sv - dts.  F = -4.442807633e-10.
 *   orbit    A = sqrt_a^2; n = sqrt(mu / A^3) + delta_n; tk = wrap(t - toe); M = m0 + n tk; E by exactly 8 Newton steps
 *            E <- E - (E - e sin E - M) / (1 - e cos E) from E = M; cos nu = (cos E - e) / (1 - e cos E), sin nu =
 *            sqrt(1 - e^2) sin E / (1 - e cos E); Phi = nu + omega and u = Phi + du by the angle-addition formulas, 2 Phi
 *            by the double-angle formulas; du, dr, di = c?s sin 2Phi + c?c cos 2Phi; r = A (1 - e cos E) + dr; i = i0 +
 *            di + idot tk; Omega = omega0 + (omega_dot - OmegaE) tk - OmegaE toe; x' = r cos u, y' = r sin u; X = x' cos
 *            Omega - y' cos i sin Omega, Y = x' sin Omega + y' cos i cos Omega, Z = y' sin i.  mu = 3.986005e14, OmegaE =
 *            7.2921151467e-5, c = 299792458.
 *   usable   a channel counts in an epoch (num_valid) when its ephemeris has valid != 0, 0 <= e < 0.5 and sqrt_a > 0, both
 *            times are given and its state and pseudorange are finite; it is used when besides its weight (1 without
 *            weights) is finite and > 0.  An unusable ephemeris is not an error.  Given means ms >= 0 and a finite
 *            fraction, nothing more: tx_ms = 604800000 or INT32_MAX counts, -0.0 is an eccentricity.  On all of e < 0.5,
 *            sqrt_a in 3000 .. 7000 and t_k in [-302400, 302400) the state is within 1e-5 m and 1e-18 s of the formulas
 *            in exact arithmetic (derived from the roundings: 4.6e-6 m at e = 0 to 7.9e-6 m at e = 0.5; measured 5e-7 to
 *            9.5e-7 m: DESIGN.md 4.15).  What passes this fence with numbers no orbit has (sqrt_a = 0.0086: a satellite
 *            76 m from the Earth's centre) counts all the same, and the fix of its epoch is wrong with status 0 or does
 *            not converge: an elevation mask takes such a satellite out, gat_position_fix_raim detects and names it.
 *   solver   unknowns (x, y, z, b), b = c * the receiver's clock error; start init_xyz, b = 0.  An iteration: per usable
 *            channel the travel time tau is 0.075 s until the channel has a range and r / c of its last range after, the
 *            satellite is turned about z by OmegaE tau, r is the range from the receiver to it, los the unit vector, v =
 *            rho - (r + b - c dts), the row a = (-los, 1); the 14 sums of w a_i a_j (i <= j) and w a_i v over the used
 *            channels; N = L L^T column by column, L L^T d = right side; the state moves by d.  A pass ends when |d_xyz| <
 *            tol_m or after max_iter iterations (GAT_FIX_NOT_CONVERGED, the outputs stand).  Fewer than 4 used channels
 *            (GAT_FIX_FEW_SATS), a sum or a step that is not finite (GAT_FIX_NONFINITE; the sums are tested first) and a
 *            pivot d_j not > 2^-40 N[j][j] -- not positive but for rounding -- (GAT_FIX_SINGULAR) end the epoch with every
 *            output of it zero but status, num_valid, num_used and iterations.
 *   mask     after a converged first pass, with mask_sin > -1 and |xyz| >= 1e6 m: sin el = (xyz / |xyz|) . los at that
 *            state; the used set keeps the channels with sin el >= mask_sin.  If that changed it and at least 4 remain, a
 *            second pass runs from the first one's state (GAT_FIX_MASKED; the iterations add, each pass has max_iter of
 *            them); with fewer than 4 the first pass stands (GAT_FIX_MASK_STARVED).
 *   record   at the final state the rows are evaluated once more: rms_residual_m = sqrt(sum v^2 / num_used) over the used
 *            channels, gdop and pdop from the diagonal of the unweighted (A^T A)^-1 through the same Cholesky (0 where it
 *            fails), clock_bias_s = b / c, last_step_m = the last |d_xyz|.
 * Optional outputs (null: not written): sat double [E][K][4], the ECEF position at transmission (in the frame of that
 * instant) and dts, zeros for a channel that does not count; resid double [E][K], v at the final state of every counting
 * channel, used or not; sin_el double [E][K] likewise (0 within 1e6 m of the centre); used uint8 [E][K].  The last three
 * are zero in an epoch that failed.  One epoch never touches another.
 * gat_position_fix enqueues one kernel on the context's stream -- a wave of 64 lanes an epoch, a lane a channel, four
 * epochs a workgroup --, does not synchronise, allocates nothing and uses no atomics: the same bits every call.
 * Refusals, all before any launch (the host twin: before any write): GAT_ERR_ARG for a null required pointer (ephemerides,
 * the four times, config, fixes), a wrong struct_size, E or K < 1, max_iter < 1, tol_m not > 0, a mask_sin or init_xyz
 * that is not finite and non-zero flags; GAT_ERR_RANGE for K above GAT_MAX_FIX_CHANNELS and E above 2^24. */
#define GAT_MAX_FIX_CHANNELS 64
#define GAT_MAX_FIX_EPOCHS 16777216
#define GAT_FIX_FEW_SATS 1
#define GAT_FIX_SINGULAR 2
#define GAT_FIX_NONFINITE 4
#define GAT_FIX_NOT_CONVERGED 8
#define GAT_FIX_MASK_STARVED 16
#define GAT_FIX_MASKED 32
/* gat_lnav_ephemeris_host's reason codes */
#define GAT_EPH_OK 0
#define GAT_EPH_MISSING 1  /* no frame with every status bit set for one of subframes 1, 2, 3 */
#define GAT_EPH_IODE 2     /* no subframe 1 has subframes 2 and 3 whose IODE is the low 8 bits of its IODC */
typedef struct gat_ephemeris {
    int32_t wn;           /* week number mod 1024 */
    int32_t iodc, iode;
    int32_t health, ura;  /* the 6-bit health and the 4-bit URA index as sent */
    int32_t fit;          /* the fit interval flag */
    double toc, toe;      /* s */
    double af0, af1, af2; /* s, s/s, s/s^2 */
    double tgd;           /* s */
    double sqrt_a;        /* m^(1/2) */
    double e;
    double m0, delta_n;   /* rad, rad/s */
    double omega0, i0, omega, omega_dot, idot; /* rad, rad/s */
    double cuc, cus, crc, crs, cic, cis;       /* rad, rad, m, m, rad, rad */
    int32_t valid;        /* 1: usable */
    int32_t reason;       /* GAT_EPH_* */
} gat_ephemeris;
typedef struct gat_fix_config {
    uint32_t struct_size; /* sizeof(gat_fix_config) */
    int32_t max_iter;     /* iterations a pass, >= 1 (10) */
    double tol_m;         /* > 0 (1e-4) */
    double mask_sin;      /* sin of the elevation mask; -1: off */
    double init_xyz[3];   /* the start, m (the Earth's centre) */
    uint32_t flags;       /* 0 */
    uint32_t reserved;
} gat_fix_config;
typedef struct gat_fix {
    int32_t status;       /* GAT_FIX_* bits; 0: a converged fix */
    int32_t num_valid;    /* channels that count in this epoch */
    int32_t num_used;     /* channels in the last pass's equations */
    int32_t iterations;
    double x, y, z;       /* ECEF at reception, m */
    double clock_bias_s;  /* the receiver's clock minus GPS time */
    double rms_residual_m;
    double last_step_m;
    double gdop, pdop;
} gat_fix;
GAT_API int32_t gat_position_fix(gat_ctx *ctx, const gat_ephemeris *eph_dev, const int32_t *tx_ms_dev, const double *tx_frac_dev,
                                 const int32_t *rx_ms_dev, const double *rx_frac_dev, const double *weights_dev, int32_t num_epochs,
                                 int32_t num_channels, const gat_fix_config *config, gat_fix *fixes_dev, double *sat_dev,
                                 double *resid_dev, double *sin_el_dev, uint8_t *used_dev);
/* The same rule in plain loops on the HOST (csrc/gat_fix.h, shared with the device): every pointer is host memory; needs
 * no context and no device.  The bit-exact reference of the device call, with the same refusals. */
GAT_API int32_t gat_position_fix_host(const gat_ephemeris *eph_host, const int32_t *tx_ms_host, const double *tx_frac_host,
                                      const int32_t *rx_ms_host, const double *rx_frac_host, const double *weights_host,
                                      int32_t num_epochs, int32_t num_channels, const gat_fix_config *config, gat_fix *fixes,
                                      double *sat, double *resid, double *sin_el, uint8_t *used);
/* What gat_position_fix would do with a call (csrc/gat_fix_plan.h; no context, no device, nothing is read but config).  The
 * refusals are the call's, but for the pointers. */
typedef struct gat_fix_plan {
    uint32_t struct_size; /* sizeof(gat_fix_plan), set by the caller */
    int32_t workgroups;
    int32_t waves_per_workgroup;  /* = epochs a workgroup: a wave an epoch */
    int32_t threads;
    int32_t lds_bytes;
    int32_t reserved;
    int64_t scratch_bytes;        /* 0: the kernel keeps an epoch in registers and LDS */
} gat_fix_plan;
GAT_API int32_t gat_position_fix_plan(int32_t num_epochs, int32_t num_channels, const gat_fix_config *config, gat_fix_plan *plan);
/* One channel's ephemeris from its gat_nav_frame records (gat_nav_decode, GAT_NAV_LNAV), on the host: the newest complete
 * set -- the frames of subframe 1 with every status bit set are tried from the newest back, each with the newest such
 * frames of subframes 2 and 3 whose IODE equals the low 8 bits of its IODC, and the first that has both is taken, so that
 * the last complete issue stands until a new one is complete.  Found: *eph filled, valid = 1, reason = GAT_EPH_OK; else
 * *eph zero but for reason.  Returns GAT_ERR_ARG for
 * a null pointer or num_frames < 0, else GAT_OK.  Data bits d1 .. d24 of words 3 .. 10, the MSB first, signed fields in
 * two's complement; semicircles become radians with pi = 3.1415926535898:
 *   subframe 1  word 3: WN(10) L2 codes(2) URA(4) health(6) IODC MSBs(2); word 7: 16 reserved, TGD(8 s, 2^-31); word 8: IODC
 *               LSBs(8) toc(16, 2^4); word 9: af2(8 s, 2^-55) af1(16 s, 2^-43); word 10: af0(22 s, 2^-31)
 *   subframe 2  word 3: IODE(8) Crs(16 s, 2^-5); word 4: delta_n(16 s, 2^-43 sc/s) M0 31..24; word 5: M0 23..0 (32 s, 2^-31 sc);
 *               word 6: Cuc(16 s, 2^-29) e 31..24; word 7: e 23..0 (32 u, 2^-33); word 8: Cus(16 s, 2^-29) sqrtA 31..24;
 *               word 9: sqrtA 23..0 (32 u, 2^-19); word 10: toe(16, 2^4) fit(1) AODO(5)
 *   subframe 3  word 3: Cic(16 s, 2^-29) Omega0 31..24; word 4: Omega0 23..0 (32 s, 2^-31 sc); word 5: Cis(16 s, 2^-29) i0
 *               31..24; word 6: i0 23..0 (32 s, 2^-31 sc); word 7: Crc(16 s, 2^-5) omega 31..24; word 8: omega 23..0 (32 s,
 *               2^-31 sc); word 9: OmegaDot(24 s, 2^-43 sc/s); word 10: IODE(8) IDOT(14 s, 2^-43 sc/s) */
GAT_API int32_t gat_lnav_ephemeris_host(const gat_nav_frame *frames, int32_t num_frames, gat_ephemeris *eph);
/* The inverse: the 190 payload bits (d1 .. d24 of words 3 .. 9, d1 .. d22 of word 10; one bit a byte) of subframes 1, 2 and
 * 3, every field rint(value / scale) kept to its width; L2 codes, reserved bits and AODO are 0.  valid is not read. */
GAT_API int32_t gat_lnav_ephemeris_words_host(const gat_ephemeris *eph, uint8_t *payload_bits);

/* ---- observables: times of transmission and carrier phase from the loop's parameter history ------------------------------
 * What lies between the loop and the fix.  gat_tracking_run_history is gat_tracking_run_weighted (w_re = w_im = NULL: the
 * unweighted run) with the ping-pong pair replaced by one array history_dev [num_blocks + 1][K]: the caller fills record 0,
 * block b is correlated with record b and its update writes record b + 1 -- the same two launches a block with cur = history
 * + b K and next = history + (b + 1) K, so accumulators, loop state and record num_blocks have the bits gat_tracking_run
 * leaves from the same start.  GAT_FLAG_GRAPH is refused (GAT_ERR_ARG), as is one weight pointer without the other. */
GAT_API int32_t gat_tracking_run_history(gat_ctx *ctx, const gat_signal_desc *sig, int32_t num_blocks, int32_t num_channels,
                                         int32_t num_taps, const int32_t *shifts_host, double sampling_freq_hz,
                                         const gat_loop_config *config_host, gat_loop_state *state_dev,
                                         gat_channel_params *history_dev, float *acc_re_dev, float *acc_im_dev,
                                         int64_t acc_block_stride, uint32_t flags, const double *w_re_dev, const double *w_im_dev);
/* gat_observables reads that history [B + 1][K] (tau = code_phase_chips, phi = carrier_phase_cycles, fcode, fcarr of record
 * b: the replica at the start of block b), the monitor's channel records [K] and the decoder's channel records [K] and frames
 * [K][max_frames] where those calls wrote them (they covered the same B blocks: monitor block = history index) and writes,
 * for E measurement epochs at the history indices b_e = epoch_first + e * epoch_stride <= B, what gat_position_fix takes.
 * Everything that accumulates is an integer, so any order of summation gives the same value; the only floating-point results
 * are single quotients, evaluated as written without contraction (csrc/gat_obs.h, shared by the kernels and the host twin:
 * the same bits).  Lc = code_length, fc = code_freq_nominal_hz (Lc * 1000 == fc: a code period is 1 ms), T = block_seconds,
 * N = block_samples, fs = sampling_freq_hz, Pd = symbol_blocks, P = 1 (LNAV) or 2 (CNAV) symbols a bit.
 *   wraps    block i < B: w_i = rint(q), q = ((tau_i + fcode_i T) - tau_{i+1}) / Lc, the whole code periods of block i; c_i =
 *            rint(d), d = (phi_i + fcarr_i T) - phi_{i+1}, its whole carrier cycles (either sign): read off the history, not
 *            recomputed from the loop's floor.  n_b = sum_{i<b} w_i, W_b = sum_{i<b} c_i (int64).  A q or d further than 1e-6
 *            from its integer or beyond 2^31, a record with a value that is not finite, or a tau outside [0, Lc) at an epoch or
 *            at the frame block: GAT_OBS_BAD_RECORD, no measurement of that channel in any epoch; other channels are untouched.
 *   frame    g = start + (symbol_phase + P * frame_offset) * Pd, the history block at which frame 0 of the decoder begins.
 *            start < 0: GAT_OBS_NO_BIT_SYNC; frame_offset < 0: GAT_OBS_NO_FRAME_SYNC; g > B: GAT_OBS_FRAME_OUTSIDE.
 *   tow      f* = the first written frame (f < min(num_frames, max_frames)) with every status bit of its format set; none, or
 *            tow_steps < min_tow_steps: GAT_OBS_NO_TOW.  The TOW count names the start of the NEXT 6 s frame: frame 0 begins
 *            at frame0_ms = 6000 * ((tow[f*] - 1 - f*) mod 100800), the mod mathematical.
 *   edge     the bit edge is the code-period boundary nearest the start of block g: x = tau_g / Lc, p* = n_g + rint(x);
 *            |x - 0.5| < edge_margin: GAT_OBS_EDGE_AMBIGUOUS -- the measurement stands, maybe a period off.
 *   tx       at the start of block b = b_e: tx_ms = (frame0_ms + (n_b - p*)) mod 604800000 (mathematical), tx_frac = tau_b /
 *            fc, a quotient >= 1e-3 written as the largest double below 1e-3.  Any status bit but EDGE_AMBIGUOUS: no
 *            measurement, tx_ms = -1 and tx_frac = 0 in every epoch.
 *   carrier  carrier_cycles = W_b, carrier_frac = phi_b, doppler_hz = fcarr_b - if_hz, code_rate_hz = fcode_b: the phase
 *            includes the IF (the caller removes if_hz t).  Written without a measurement too, zeros for a BAD_RECORD channel.
 *   rx       an anchor (ms, frac) at block a.  GAT_OBS_RX_GIVEN: (rx0_ms, rx0_frac) at a = 0.  GAT_OBS_RX_FROM_TX (the cold
 *            start): a = b_0 and the anchor is the latest transmission of epoch 0 among the measured channels plus travel_ms,
 *            with that channel's fraction -- latest by the integer ms difference to the first measured channel wrapped into
 *            [-302400000, 302400000), then by the fraction, the lowest channel on a tie; no measured channel: rx_ms = -1 and
 *            rx_frac = 0 in every epoch.  Epoch e in integers: S = (b_e - a) N, ms_add = S 1000 / fs, rem = S 1000 mod fs,
 *            frac = anchor_frac + (double) rem / (fs * 1000.0), one carry of 1e-3 into ms_add where frac >= 1e-3, rx_ms =
 *            (anchor_ms + ms_add) mod 604800000.
 * Outputs, every one optional (null: not written; at least one is given): tx_ms int32 and tx_frac double [E][K]; rx_ms int32
 * and rx_frac double [E]; carrier_cycles int64, carrier_frac, doppler_hz, code_rate_hz double [E][K]; channels [K], fields
 * zero where undefined (frame_block with both syncs; tow_frame and frame0_ms with a TOW; the edge with g <= B in a channel
 * that is not BAD_RECORD).  The four times go into gat_position_fix as they are.
 * The call enqueues on the context's stream, does not synchronise and allocates nothing but the context's scratch.  The
 * history is cut into chunks of consecutive blocks -- one contiguous span for all channels -- and the channels into groups
 * (gat_observables_plan, csrc/gat_obs_plan.h): a workgroup a (chunk, group) sums its wraps, a wave a channel scans the chunk
 * totals and resolves the channel's record, one wave picks the anchor, a workgroup a (chunk, group) walks its span again
 * and writes the epochs in it.  No atomics, no floating-point sum: the same bits every call and from the twin.
 * Refusals, all before any launch (the host twin: before any write): GAT_ERR_ARG for a null history, monitor or decoder
 * pointer or config, a wrong struct_size, an unknown format or rx_mode, B, K, E, symbol_blocks, max_frames or epoch_stride
 * < 1, epoch_first < 0, an epoch beyond record B, edge_margin outside [0, 0.5], block_seconds not > 0, block_samples < 1 and
 * a call with every output null; GAT_ERR_RANGE for travel_ms outside 0 .. 1000, a given rx0_ms outside 0 .. 604799999 or
 * rx0_frac outside [0, 1e-3), K above GAT_MAX_MONITOR_CHANNELS, B above GAT_MAX_MONITOR_BLOCKS, code_length < 1 or
 * code_length * 1000 != code_freq_nominal_hz, an fs that is not a whole number in 1 .. 2^40, B * N * 1000 >= 2^62, an if_hz
 * that is not finite and a call whose scratch would exceed 1 GiB. */
#define GAT_OBS_BAD_RECORD 1
#define GAT_OBS_NO_BIT_SYNC 2
#define GAT_OBS_NO_FRAME_SYNC 4
#define GAT_OBS_FRAME_OUTSIDE 8
#define GAT_OBS_NO_TOW 16
#define GAT_OBS_EDGE_AMBIGUOUS 32
#define GAT_OBS_RX_GIVEN 0
#define GAT_OBS_RX_FROM_TX 1
typedef struct gat_obs_config {
    uint32_t struct_size;        /* sizeof(gat_obs_config) */
    int32_t format;              /* GAT_NAV_LNAV or GAT_NAV_CNAV */
    int32_t code_length;         /* Lc */
    int32_t symbol_blocks;       /* Pd, the monitor's */
    double code_freq_nominal_hz; /* fc = Lc * 1000 */
    double block_seconds;        /* T: the loop configuration's value, bit for bit */
    double sampling_freq_hz;     /* fs, a whole number */
    double if_hz;
    int32_t block_samples;       /* N */
    int32_t max_frames;          /* rows of the decoder's frames per channel */
    int32_t min_tow_steps;       /* the decoder's tow_steps must reach this (0: any) */
    int32_t epoch_first;         /* b_0 >= 0 */
    int32_t epoch_stride;        /* >= 1 */
    int32_t rx_mode;             /* GAT_OBS_RX_GIVEN or GAT_OBS_RX_FROM_TX */
    int32_t rx0_ms;              /* given mode: reception at block 0 */
    int32_t travel_ms;           /* from-tx mode: 0 .. 1000 (68) */
    double edge_margin;          /* 0 .. 0.5 (0.1) */
    double rx0_frac;             /* given mode: [0, 1e-3) */
} gat_obs_config;
typedef struct gat_obs_channel {
    int32_t status;       /* GAT_OBS_* bits; 0 or EDGE_AMBIGUOUS alone: measured */
    int32_t frame_block;  /* g */
    int32_t tow_frame;    /* f* */
    int32_t frame0_ms;
    int64_t edge_period;  /* p* */
    double edge_fraction; /* tau_g / Lc */
} gat_obs_channel;
GAT_API int32_t gat_observables(gat_ctx *ctx, const gat_channel_params *history_dev, const gat_monitor_channel *mon_channels_dev,
                                const gat_nav_channel *nav_channels_dev, const gat_nav_frame *nav_frames_dev, int32_t num_blocks,
                                int32_t num_channels, int32_t num_epochs, const gat_obs_config *config, int32_t *tx_ms,
                                double *tx_frac, int32_t *rx_ms, double *rx_frac, int64_t *carrier_cycles, double *carrier_frac,
                                double *doppler_hz, double *code_rate_hz, gat_obs_channel *channels);
/* The same rule in plain loops on the HOST (csrc/gat_obs.h, shared with the device): every pointer is host memory; needs
 * no context and no device.  The bit-exact reference of the device call, with the same refusals. */
GAT_API int32_t gat_observables_host(const gat_channel_params *history_host, const gat_monitor_channel *mon_channels_host,
                                     const gat_nav_channel *nav_channels_host, const gat_nav_frame *nav_frames_host,
                                     int32_t num_blocks, int32_t num_channels, int32_t num_epochs, const gat_obs_config *config,
                                     int32_t *tx_ms, double *tx_frac, int32_t *rx_ms, double *rx_frac, int64_t *carrier_cycles,
                                     double *carrier_frac, double *doppler_hz, double *code_rate_hz, gat_obs_channel *channels);
/* What gat_observables would do with a call (csrc/gat_obs_plan.h; no context, no device, nothing is read but config).  A chunk
 * is chunk_blocks consecutive blocks (the last one takes what is left and record B); a channel group is channel_group
 * consecutive channels; a workgroup of `threads` is rows x lanes, lane l < lanes holds channel l of its group and row r walks
 * run_blocks consecutive blocks of the chunk.  The refusals are the call's, but for the pointers. */
typedef struct gat_obs_plan {
    uint32_t struct_size; /* sizeof(gat_obs_plan), set by the caller */
    int32_t chunk_blocks, num_chunks;
    int32_t channel_group, num_groups;
    int32_t lanes, rows, run_blocks;
    int32_t threads, lds_bytes;
    int32_t chunk_workgroups;   /* num_chunks * num_groups: the sum kernel and the epoch kernel each */
    int32_t channel_workgroups; /* four channels (waves) a workgroup */
    int64_t scratch_bytes;
} gat_obs_plan;
GAT_API int32_t gat_observables_plan(int32_t num_blocks, int32_t num_channels, int32_t num_epochs, const gat_obs_config *config,
                                     gat_obs_plan *plan);

/* ---- fix integrity: residual test and fault exclusion -------------------------------------------------------------------------
 * gat_position_fix takes every measurement with its full weight; one that is a code period off (GAT_OBS_EDGE_AMBIGUOUS: 300 km)
 * moves the fix by kilometres and the status stays 0.  gat_position_fix_raim is gat_position_fix followed per epoch by a test of
 * the weighted residuals against thresholds of the caller's and, where the test fails, by leave-one-out solves that name the
 * channel to leave out.  The arithmetic is the position fix's (FP64, no contraction, no libm transcendental, every sum in channel
 * order from +0: csrc/gat_raim.h on top of csrc/gat_fix.h, shared by the kernel and the host twin: the same bits).
 *   fix      the position fix's rule unchanged: first pass, mask, second pass -- the state, the used set U and n = num_used.  A
 *            fix that failed or carries GAT_FIX_NOT_CONVERGED: GAT_RAIM_NOT_CHECKED, every output that of gat_position_fix.
 *   test     T = sum over the used channels of w (v v) at the final rows (w = 1 without weights), d = n - 4.  d = 0:
 *            GAT_RAIM_NO_REDUNDANCY.  Else the epoch is detected (GAT_RAIM_DETECTED) when T > threshold[d]: the thresholds are
 *            the caller's, in the units of T, indexed by d = 1 .. GAT_MAX_FIX_CHANNELS - 4 (entry 0 is not read); +inf never
 *            detects.  dof = d, stat0 = T, threshold0 = threshold[d] (0 where d = 0).
 *   round    a detected epoch runs up to max_exclude rounds (0: detection only); a round needs n >= 6.  Once a round every
 *            channel is frozen where its last row put it: turned about z by OmegaE tau with tau as that row left it, (xr, yr,
 *            Z), and its range term g = rho + c dts.  A trial of the used channel j solves U \ {j} from the epoch's state
 *            with the frozen satellites: r = |(xr, yr, Z) - xyz|, los, v = g - (r + b), the same 14 sums (channel j adds +0),
 *            the same step, at most trial_iter iterations, converged when |d_xyz| < tol_m; T_j = sum of w (v v) over U \ {j}
 *            at the trial's last state.  A trial counts when it converged, no step failed (a sum or step not finite, a
 *            singular system) and T_j is finite.  The channel left out, j*, is the counting one with the smallest (T_j, j);
 *            none counts: the rounds end.
 *   final    j* leaves the used set, the state becomes j*'s trial state and the rows are evaluated there once, so that every
 *            travel time is that state's and not the one the fault had moved (68 km of state are 0.4 m of Earth rotation;
 *            the trial carries that error, a pass that began with it would take it for converged).  Then an ordinary pass of
 *            the fix's rule (live travel times, max_iter, tol_m) and the rows at its state once more as after every pass;
 *            the iterations add.  A pass that fails or does not converge ends the rounds.  Else T is tested again at d - 1: passed, the epoch is GAT_RAIM_EXCLUDED and
 *            the rounds end; failed, the next round runs from there.  There is no second elevation mask.
 *   stands   GAT_RAIM_EXCLUDED: the outputs are the last pass's -- used and num_used the final set, GAT_FIX_EXCLUDED set in
 *            fixes.status (by this call alone), the left-out channel's resid and sin_el at the final state like any unused
 *            channel's; num_excluded and excluded[] in the order of exclusion, stat and threshold those of the final set.
 *            Detected and not excluded (rounds ended or used up, n < 6, max_exclude = 0): GAT_RAIM_UNRESOLVED, every output
 *            the full set's, num_excluded = 0, excluded[] = -1, stat = stat0, threshold = threshold0.  Wherever num_excluded
 *            is 0, fixes, sat, resid, sin_el and used have the bytes gat_position_fix writes.
 *   trial    optional double [E][K]: T_j of the first round; -1 for a channel that was no candidate or whose trial did not
 *            count, and in an epoch without a round.
 * gat_position_fix_raim enqueues one kernel of gat_position_fix's geometry (a wave an epoch, a lane a channel, four epochs a
 * workgroup); in a round lane j runs trial j by itself from the wave's LDS.  No atomics, no scratch, no synchronisation.
 * Refusals: gat_position_fix's, and GAT_ERR_ARG for a null integrity pointer or raim config, a wrong struct_size, max_exclude
 * outside 0 .. GAT_RAIM_MAX_EXCLUDE, trial_iter < 1, non-zero flags and a threshold[1 ..] that is NaN or not > 0. */
#define GAT_RAIM_MAX_EXCLUDE 4
#define GAT_RAIM_NOT_CHECKED 1
#define GAT_RAIM_NO_REDUNDANCY 2
#define GAT_RAIM_DETECTED 4
#define GAT_RAIM_EXCLUDED 8
#define GAT_RAIM_UNRESOLVED 16
#define GAT_FIX_EXCLUDED 64 /* in gat_fix.status: a channel was left out by gat_position_fix_raim */
typedef struct gat_raim_config {
    uint32_t struct_size; /* sizeof(gat_raim_config) */
    int32_t max_exclude;  /* rounds, 0 .. GAT_RAIM_MAX_EXCLUDE (1); 0: detect only */
    int32_t trial_iter;   /* iterations a trial, >= 1 (8) */
    uint32_t flags;       /* 0 */
    double threshold[61]; /* [GAT_MAX_FIX_CHANNELS - 3]: by d = n - 4, in the units of T; entry 0 is not read */
} gat_raim_config;
typedef struct gat_fix_integrity {
    int32_t status;       /* GAT_RAIM_* bits; 0: tested and passed */
    int32_t dof;          /* d of the full set */
    int32_t num_excluded;
    int32_t excluded[4];  /* channels in the order of exclusion, -1 where unused */
    int32_t reserved;
    double stat0, threshold0; /* the full set */
    double stat, threshold;   /* the final set */
} gat_fix_integrity;
GAT_API int32_t gat_position_fix_raim(gat_ctx *ctx, const gat_ephemeris *eph_dev, const int32_t *tx_ms_dev, const double *tx_frac_dev,
                                      const int32_t *rx_ms_dev, const double *rx_frac_dev, const double *weights_dev,
                                      int32_t num_epochs, int32_t num_channels, const gat_fix_config *config,
                                      const gat_raim_config *raim, gat_fix *fixes_dev, gat_fix_integrity *integrity_dev,
                                      double *sat_dev, double *resid_dev, double *sin_el_dev, uint8_t *used_dev, double *trial_dev);
/* The same rule in plain loops on the HOST: every pointer is host memory; the bit-exact reference of the device call. */
GAT_API int32_t gat_position_fix_raim_host(const gat_ephemeris *eph_host, const int32_t *tx_ms_host, const double *tx_frac_host,
                                           const int32_t *rx_ms_host, const double *rx_frac_host, const double *weights_host,
                                           int32_t num_epochs, int32_t num_channels, const gat_fix_config *config,
                                           const gat_raim_config *raim, gat_fix *fixes, gat_fix_integrity *integrity, double *sat,
                                           double *resid, double *sin_el, uint8_t *used, double *trial);
/* What gat_position_fix_raim would do with a call (csrc/gat_raim_plan.h): gat_position_fix's geometry with the trial's LDS. */
GAT_API int32_t gat_position_fix_raim_plan(int32_t num_epochs, int32_t num_channels, const gat_fix_config *config,
                                           const gat_raim_config *raim, gat_fix_plan *plan);

/* ---- velocity fix: satellite velocities, a Doppler solver and the local frame ------------------------------------------------
 * From the ephemerides, the times of transmission, gat_observables' doppler_hz and the fixes of gat_position_fix or
 * gat_position_fix_raim: per epoch the receiver's ECEF velocity and clock drift by one weighted least-squares solve, the same
 * velocity as east / north / up, and the geodetic frame it was turned into.  The arithmetic is the position fix's (FP64, no
 * contraction, no libm transcendental, every sum in channel order from +0: csrc/gat_vel.h on top of csrc/gat_fix.h, shared by
 * the kernel and the host twin: the same bits).
 *   satellite the position fix's clock and orbit, the same expressions in the same order (X, Y, Z and dts have its bits), and
 *            from the sines and cosines they hold the rates: Edot = n / (1 - e cos E); nudot = Edot sqrt(1 - e^2) / (1 - e cos
 *            E); udot = nudot + 2 nudot (cus cos 2Phi - cuc sin 2Phi); rdot = A e sin E Edot + 2 nudot (crs cos 2Phi - crc sin
 *            2Phi); idot_k = idot + 2 nudot (cis cos 2Phi - cic sin 2Phi); Omegadot_k = omega_dot - OmegaE; x'dot = rdot cos u
 *            - r udot sin u, y'dot = rdot sin u + r udot cos u; Vx = x'dot cos Omega - y'dot cos i sin Omega + y' sin i sin
 *            Omega idot_k - (x' sin Omega + y' cos i cos Omega) Omegadot_k, Vy = x'dot sin Omega + y'dot cos i cos Omega - y'
 *            sin i cos Omega idot_k + (x' cos Omega - y' cos i sin Omega) Omegadot_k, Vz = y'dot sin i + y' cos i idot_k: the
 *            ECEF velocity in the frame of the instant.  ddts = af1 + 2 af2 dt + F e sqrt_a cos E Edot, E solved at t_sv.
 *   counts   a channel counts in an epoch (num_valid) when its ephemeris is usable (the position fix's fence), its transmit
 *            time is given, its doppler_hz is finite and X, Y, Z, V, dts and ddts are finite.  It is used when besides its
 *            weight (1 without weights) is finite and > 0 and its byte in `used` is non-zero (without `used`: every one).
 *   row      at the fix's state st = (x, y, z, c clock_bias_s): the position fix's row is evaluated exactly three times, with
 *            tau = 0.075 s, then r / c, then r / c.  theta = OmegaE tau of the last evaluation; (Xr, Yr) the position and Vr
 *            the velocity turned about z by theta, los the row's unit vector; q = los . (Vr - OmegaE (Yr, -Xr, 0)), the
 *            satellite's inertial velocity along the line of sight; k = 1 / (1 + q / c).  The range rate is k los . (Vr - v)
 *            -- the light-time equation differentiated: the instant of transmission advances at 1 - taudot and the angle of
 *            rotation with tau -- and the measurement -lambda doppler_hz = range rate + d - c ddts with lambda = c /
 *            carrier_hz and d = c * the receiver's clock drift: the row a = (-k los, 1), the right side y = -lambda
 *            doppler_hz - k los . Vr + c ddts.  Neglected: the second order in the receiver's own drift (doppler_hz times the
 *            drift) and the clock rate's own 1 - taudot (8e-12 m/s).
 *   solve    linear: one solve, no iteration.  The 14 sums of w a_i a_j (i <= j) and w a_i y over the used channels, the
 *            position fix's Cholesky solve with its pivot rule and its order of tests; then v_k = y_k - a_k . s of every
 *            counting channel, rms_residual_mps = sqrt(sum over the used of v^2 / num_used), clock_drift = s_3 / c.
 *   frame    p = sqrt(x^2 + y^2), R = |xyz|; from s = z / R, c = p / R exactly 8 steps N = a / sqrt(1 - e2 s^2), z' = z + e2 N s,
 *            q = sqrt(z'^2 + p^2), s = z' / q, c = p / q (a = 6378137, e2 = 6.69437999014e-3: WGS-84); sin_lat = s, cos_lat =
 *            c, height_m = p c + z s - a sqrt(1 - e2 s^2); cos_lon = x / p, sin_lon = y / p, or (1, 0) where p = 0.  east =
 *            (-sin_lon, cos_lon, 0), north = (-sin_lat cos_lon, -sin_lat sin_lon, cos_lat), up = (cos_lat cos_lon, cos_lat
 *            sin_lon, sin_lat); ve, vn, vu the velocity along them.  No arctangent: a caller turns the pairs into angles.
 *   status   GAT_VEL_NO_FIX: the fix's status has GAT_FIX_FEW_SATS, SINGULAR or NONFINITE, or its x, y, z or clock_bias_s is
 *            not finite -- every output of the epoch is zero but status.  A fix that carries only GAT_FIX_NOT_CONVERGED,
 *            MASKED, MASK_STARVED or EXCLUDED is used as it stands.  GAT_VEL_FEW_SATS: fewer than 4 used channels;
 *            GAT_VEL_SINGULAR, GAT_VEL_NONFINITE: the solve's -- the record is zero but status and the two counts, resid is
 *            zero.  GAT_VEL_NO_GEODETIC: R not >= 1e6 m -- the ECEF velocity, the drift and the rms stand, the frame, the
 *            height and ve, vn, vu are zero.
 * Optional outputs (null: not written): sat_vel double [E][K][4], Vx, Vy, Vz and ddts of every counting channel (zeros for
 * one that does not count and in a GAT_VEL_NO_FIX epoch); resid double [E][K], v of every counting channel, used or not.
 * One epoch never touches another.
 * gat_velocity_fix enqueues one kernel of gat_position_fix's geometry on the context's stream (a wave an epoch, a lane a
 * channel, four epochs a workgroup), does not synchronise, allocates nothing and uses no atomics: the same bits every call.
 * Refusals, all before any launch (the host twin: before any write): GAT_ERR_ARG for a null required pointer (ephemerides,
 * the two times, doppler_hz, fixes, config, velocities), a wrong struct_size, E or K < 1, non-zero flags and a carrier_hz
 * that is not finite or not > 0; GAT_ERR_RANGE for K above GAT_MAX_FIX_CHANNELS and E above GAT_MAX_FIX_EPOCHS. */
#define GAT_VEL_FEW_SATS 1
#define GAT_VEL_SINGULAR 2
#define GAT_VEL_NONFINITE 4
#define GAT_VEL_NO_FIX 8
#define GAT_VEL_NO_GEODETIC 16
typedef struct gat_vel_config {
    uint32_t struct_size; /* sizeof(gat_vel_config) */
    uint32_t flags;       /* 0 */
    double carrier_hz;    /* > 0, finite (1575.42e6) */
} gat_vel_config;
typedef struct gat_velocity {
    int32_t status;       /* GAT_VEL_* bits; 0: a velocity with its frame */
    int32_t num_valid;    /* channels that count in this epoch */
    int32_t num_used;     /* channels in the equations */
    int32_t reserved;
    double vx, vy, vz;    /* ECEF, m/s */
    double clock_drift;   /* s/s */
    double rms_residual_mps;
    double ve, vn, vu;    /* east, north, up, m/s */
    double sin_lat, cos_lat, sin_lon, cos_lon, height_m; /* geodetic, WGS-84 */
} gat_velocity;
GAT_API int32_t gat_velocity_fix(gat_ctx *ctx, const gat_ephemeris *eph_dev, const int32_t *tx_ms_dev, const double *tx_frac_dev,
                                 const double *doppler_hz_dev, const gat_fix *fixes_dev, const uint8_t *used_dev,
                                 const double *weights_dev, int32_t num_epochs, int32_t num_channels, const gat_vel_config *config,
                                 gat_velocity *velocities_dev, double *sat_vel_dev, double *resid_dev);
/* The same rule in plain loops on the HOST: every pointer is host memory; the bit-exact reference of the device call. */
GAT_API int32_t gat_velocity_fix_host(const gat_ephemeris *eph_host, const int32_t *tx_ms_host, const double *tx_frac_host,
                                      const double *doppler_hz_host, const gat_fix *fixes_host, const uint8_t *used_host,
                                      const double *weights_host, int32_t num_epochs, int32_t num_channels,
                                      const gat_vel_config *config, gat_velocity *velocities, double *sat_vel, double *resid);
/* What gat_velocity_fix would do with a call (csrc/gat_vel_plan.h): gat_position_fix's geometry and LDS. */
GAT_API int32_t gat_velocity_fix_plan(int32_t num_epochs, int32_t num_channels, const gat_vel_config *config, gat_fix_plan *plan);

/* ---- atmosphere: Klobuchar ionosphere, mapped troposphere, corrected transmit times -----------------------------------------
 * The fix and the velocity fix model no atmosphere.  gat_range_corrections takes a first fix (gat_position_fix or
 * gat_position_fix_raim) and gives per (epoch, channel) the ionospheric and the tropospheric delay of the IS-GPS-200
 * single-frequency user, the elevation and the azimuth as seen from the WGS-84 ellipsoid, and a transmit-time fraction
 * advanced by the delay that gat_position_fix, gat_position_fix_raim and gat_velocity_fix take as it is: fix ->
 * corrections -> fix (or RAIM) -> velocity, nothing read back.  The arithmetic is the fix's (FP64, no contraction, no libm
 * transcendental, every expression as written: csrc/gat_atm.h on top of csrc/gat_fix.h and csrc/gat_vel.h, shared by the
 * kernel and the host twin: the same bits).  c = 299792458 m/s, pi = 3.1415926535898 wherever semicircles are turned.
 *   atan2    atm_atan2(y, x): |x| and |y| are swapped so that t = min / max lies in [0, 1] (0 where max is 0: x = y = 0
 *            gives +0); k = rint(16 t), s = (t - k/16) / (1 + t k/16), |s| <= 1/32; atan t = A[k] + s + s^3 P(s^2) with A[k]
 *            = atan(k/16) (17 doubles) and P the odd Taylor polynomial to degree 11 in Horner form with explicit fused
 *            multiply-adds (truncation s^13 / 13 < 2^-68); swapped: pi/2 - a; x < 0: pi - a (pi in two parts); the sign
 *            bit of y is the result's.  |error| <= 1e-15 rad.  A quotient that is not a number (inf / inf, NaN) gives NaN.
 *   epoch    the state (x, y, z, c clock_bias_s) of the gat_fix record, accepted exactly as gat_velocity_fix accepts it
 *            (else GAT_ATM_NO_FIX); R = |xyz| not >= 1e6 m: GAT_ATM_NO_GEODETIC.  Else the velocity fix's frame (8 steps):
 *            sin / cos of the geodetic latitude phi and of the longitude lambda.  An epoch with either bit passes every
 *            tx_frac through and writes zeros to every other output of its channels.
 *   counts   a channel counts when the position fix's rule takes it: usable ephemeris, transmit and receive time given,
 *            X, Y, Z, dts and the pseudorange finite.  One that does not count: tx_frac passed through, zeros, status 0.
 *   geometry the fix's row at the state evaluated three times (tau = 0.075 s, r / c, r / c) as the velocity fix does; los
 *            its unit vector; e = -sin lambda lx + cos lambda ly, n = -sin phi cos lambda lx - sin phi sin lambda ly + cos
 *            phi lz, u = cos phi cos lambda lx + cos phi sin lambda ly + sin phi lz; e, n or u not finite:
 *            GAT_ATM_CH_NONFINITE.  sin el = u clipped to [-1, 1] -- against the ellipsoid's normal, not the fix's
 *            spherical up --; h = sqrt(e^2 + n^2), cos A = n / h, sin A = e / h, (1, 0) where h is not > 0.  A channel
 *            with sin el >= floor_sin is corrected (GAT_ATM_CH_CORRECTED), else GAT_ATM_CH_LOW: zero delays, tx_frac
 *            passed through; geom is written for both.
 *   iono     (GAT_ATM_IONO) in semicircles E = atm_atan2(u, h) / pi, phi_u = atm_atan2(sin phi, cos phi) / pi, lambda_u =
 *            atm_atan2(sin lambda, cos lambda) / pi; psi = 0.0137 / (E + 0.11) - 0.022; phi_i = phi_u + psi cos A clipped to
 *            +-0.416; lambda_i = lambda_u + psi sin A / cos(pi phi_i); phi_m = phi_i + 0.064 cos(pi (lambda_i - 1.617));
 *            t_gps = (rx_ms mod 86400000) 1e-3 + rx_frac - clock_bias_s, t = 43200 lambda_i + t_gps, less 86400 where t >=
 *            86400, then plus 86400 where t < 0; F = 1 + 16 (0.53 - E)^3; PER = beta0 + phi_m (beta1 + phi_m (beta2 + phi_m
 *            beta3)) raised to 72000, AMP the same polynomial in alpha raised to 0; xx = 2 pi (t - 50400) / PER; T = F (5e-9
 *            + AMP (1 - xx^2 / 2 + xx^4 / 24)) where |xx| < 1.57, else F 5e-9; delay = c T (1575.42e6 / carrier_hz)^2.  The
 *            two cosines are the fix's.  An AMP or PER that is not finite before it is raised, or a delay that is not
 *            finite: GAT_ATM_CH_NONFINITE for that channel alone (zero delays, tx_frac passed through).
 *   tropo    (GAT_ATM_TROPO) the zenith delays z_d (hydrostatic) and z_w (wet), metres at the receiver, are the caller's:
 *            zenith [E][2], or the config's two scalars where it is null.  Chao's mapping with s = sin el, tan = s / sqrt(1
 *            - s^2): m_d = 1 / (s + 0.00143 / (tan + 0.0445)), m_w = 1 / (s + 0.00035 / (tan + 0.017)), delay = z_d m_d +
 *            z_w m_w (s = 1: tan infinite, m = 1).  Not finite: GAT_ATM_CH_NONFINITE.
 *   output   d = iono + tropo (a switched-off term is 0); tx_frac_out = tx_frac + d / c, tx_frac itself where d = 0.  No
 *            carry into tx_ms: the fix takes any finite fraction.  Advancing the transmit time by d / c also moves the
 *            satellite by v d / c: along the line of sight at most 930 m/s d / c, 0.3 mm for d = 100 m.  The exact
 *            alternative, a range-correction input to the fix and RAIM kernels, would need new variants of both.
 * tx_frac_out double [E][K] is required.  Optional (null: not written): delay double [E][K][2] (iono, tropo, m), geom double
 * [E][K][3] (sin el, cos A, sin A), channel_status uint8 [E][K], epoch_status int32 [E].
 * gat_range_corrections enqueues one kernel on the context's stream: one thread an (epoch, channel), t = e K + k, 256
 * threads a workgroup, every thread forming its epoch's frame itself; no LDS, no barrier, no atomics, no scratch, no
 * allocation, no synchronisation.
 * Refusals, all before any launch (the host twin: before any write): GAT_ERR_ARG for a null required pointer (ephemerides,
 * the four times, fixes, config, tx_frac_out), a wrong struct_size, E or K < 1, a flag other than GAT_ATM_IONO and
 * GAT_ATM_TROPO, a floor_sin that is not finite and a carrier_hz that is not finite or not > 0; GAT_ERR_RANGE for K above
 * GAT_MAX_FIX_CHANNELS and E above GAT_MAX_FIX_EPOCHS. */
#define GAT_ATM_IONO 1
#define GAT_ATM_TROPO 2
#define GAT_ATM_NO_FIX 1          /* epoch_status */
#define GAT_ATM_NO_GEODETIC 2
#define GAT_ATM_CH_CORRECTED 1    /* channel_status; 0: the channel does not count, or its epoch has no frame */
#define GAT_ATM_CH_LOW 2
#define GAT_ATM_CH_NONFINITE 4
typedef struct gat_atm_config {
    uint32_t struct_size; /* sizeof(gat_atm_config) */
    uint32_t flags;       /* GAT_ATM_IONO | GAT_ATM_TROPO */
    double carrier_hz;    /* > 0, finite (1575.42e6) */
    double floor_sin;     /* finite (0): a channel below it is not corrected */
    double alpha[4];      /* Klobuchar: s, s/sc, s/sc^2, s/sc^3 */
    double beta[4];       /* s, s/sc, s/sc^2, s/sc^3 */
    double zenith_dry_m;  /* where zenith is null */
    double zenith_wet_m;
} gat_atm_config;
GAT_API int32_t gat_range_corrections(gat_ctx *ctx, const gat_ephemeris *eph_dev, const int32_t *tx_ms_dev, const double *tx_frac_dev,
                                      const int32_t *rx_ms_dev, const double *rx_frac_dev, const gat_fix *fixes_dev,
                                      const double *zenith_dev, int32_t num_epochs, int32_t num_channels,
                                      const gat_atm_config *config, double *tx_frac_out_dev, double *delay_dev, double *geom_dev,
                                      uint8_t *channel_status_dev, int32_t *epoch_status_dev);
/* The same rule in plain loops on the HOST: every pointer is host memory; the bit-exact reference of the device call. */
GAT_API int32_t gat_range_corrections_host(const gat_ephemeris *eph_host, const int32_t *tx_ms_host, const double *tx_frac_host,
                                           const int32_t *rx_ms_host, const double *rx_frac_host, const gat_fix *fixes_host,
                                           const double *zenith_host, int32_t num_epochs, int32_t num_channels,
                                           const gat_atm_config *config, double *tx_frac_out, double *delay, double *geom,
                                           uint8_t *channel_status, int32_t *epoch_status);
/* What gat_range_corrections would do with a call (csrc/gat_atm_plan.h): workgroups of `threads`, waves_per_workgroup waves
 * each, no LDS and no scratch. */
GAT_API int32_t gat_range_corrections_plan(int32_t num_epochs, int32_t num_channels, const gat_atm_config *config, gat_fix_plan *plan);
/* atm_atan2 (above) of count pairs, on the host: what the rule's angles are made of.  GAT_ERR_ARG for a null pointer or
 * count < 0. */
GAT_API int32_t gat_atm_atan2_host(const double *y, const double *x, int64_t count, double *angle);
/* Subframe 4, page 18 (ionospheric and UTC data) from one channel's gat_nav_frame records, on the host: the newest frame
 * with every status bit set, id 4 and SV ID 56.  Found: *page filled, valid = 1; else *page zero.  Returns GAT_ERR_ARG for a
 * null pointer or num_frames < 0, else GAT_OK.  Data bits d1 .. d24 of words 3 .. 10, the MSB first, signed fields in two's
 * complement:
 *   word 3: data ID(2) SV ID(6) alpha0(8 s, 2^-30) alpha1(8 s, 2^-27); word 4: alpha2(8 s, 2^-24) alpha3(8 s, 2^-24) beta0(8 s,
 *   2^11); word 5: beta1(8 s, 2^14) beta2(8 s, 2^16) beta3(8 s, 2^16); word 6: A1(24 s, 2^-50); word 7: A0 31..8; word 8: A0
 *   7..0 (32 s, 2^-30) tot(8, 2^12) WNt(8); word 9: dtLS(8 s) WNLSF(8) DN(8); word 10: dtLSF(8 s).
 * The UTC fields are extracted because they share the page; nothing converts times with them. */
typedef struct gat_lnav_page18 {
    int32_t valid;
    int32_t data_id;
    int32_t sv_id;    /* 56 */
    int32_t wnt;
    int32_t dt_ls;    /* s */
    int32_t wnlsf;
    int32_t dn;
    int32_t dt_lsf;   /* s */
    double alpha[4];  /* as gat_atm_config */
    double beta[4];
    double a0;        /* s */
    double a1;        /* s/s */
    double tot;       /* s */
} gat_lnav_page18;
GAT_API int32_t gat_lnav_page18_host(const gat_nav_frame *frames, int32_t num_frames, gat_lnav_page18 *page);
/* The inverse: the 190 payload bits of the page (one bit a byte), every field rint(value / scale) kept to its width; the
 * reserved bits of word 10 are 0.  valid is not read. */
GAT_API int32_t gat_lnav_page18_words_host(const gat_lnav_page18 *page, uint8_t *payload_bits);

/* ---- carrier smoothing: cycle-slip arcs and Hatch-filtered transmit times ---------------------------------------------------
 * Raw code phase carries metres of noise; the carrier phase of the same channel is good to millimetres but ambiguous by whole
 * cycles and broken at a slip.  gat_smooth_observables reads what gat_observables wrote (tx_ms int32 and tx_frac double [E][K],
 * the fraction raw or corrected by gat_range_corrections; rx_ms int32 and rx_frac double [E]; carrier_cycles int64 and
 * carrier_frac double [E][K]; optionally doppler_hz double [E][K] and a lock mask valid uint8 [E][K], 0 = not measured, the
 * hook for a lock detector of the caller's), cuts every channel into arcs at gaps and cycle slips and writes a transmit-time
 * fraction smoothed by the carrier over the last W epochs of the arc, which gat_position_fix, gat_position_fix_raim,
 * gat_range_corrections and gat_velocity_fix take as it is.  FP64, no contraction, every expression as written, no libm
 * beyond rint and fabs (csrc/gat_smooth.h, shared by the kernels and the host twin: the same bits).  u = 2^-48 s (c u = 1.07
 * um); W = window, g = cmc_gate_s, fL = carrier_hz, Te = epoch_seconds.
 *   measured  epoch e of channel k is measured when tx_ms >= 0 and rx_ms[e] >= 0; tx_frac, rx_frac[e] and carrier_frac are
 *             finite; doppler_hz is finite (with GAT_SMOOTH_RATE_TEST; not read without); valid is null or nonzero.  Not
 *             measured: tx_frac passed through, count 0, cmc_s 0, status 0.
 *   increment for e > 0 with e - 1 and e measured: dms = wrap(rx_ms[e] - rx_ms[e-1]) - wrap(tx_ms[e] - tx_ms[e-1]), each
 *             difference in int64 and wrapped once (one week's 604800000 added or taken) into [-302400000, 302400000);
 *             dPhi = (double)(cycles[e] - cycles[e-1]) + (frac[e] - frac[e-1]), the integer difference in int64 (modulo
 *             2^64); dPhin = dPhi - if_hz * Te; delta = (double) dms * 1e-3 + ((rx_frac[e] - rx_frac[e-1]) - (tx_frac[e] -
 *             tx_frac[e-1])) + dPhin / fL: the growth of pseudorange minus carrier range between the two epochs in seconds
 *             (the replica's phase grows by IF plus Doppler, and a falling range is a positive Doppler).
 *   resets    epoch e begins an arc for any of: GAT_SMOOTH_GAP, e = 0 or e - 1 not measured; GAT_SMOOTH_CMC, |dms| > 1000 or
 *             !(fabs(delta) <= g), which catches NaN; GAT_SMOOTH_RATE (with GAT_SMOOTH_RATE_TEST), !(fabs(dPhin - 0.5 *
 *             (doppler[e] + doppler[e-1]) * Te) <= rate_gate_cycles).  status = GAT_SMOOTH_MEASURED | the reasons.  At an arc
 *             start q_e = 0, else q_e = (int64) rint(delta / u): |q| <= 2^30 by the bound on g.
 *   scans     per channel over all epochs: C_e = sum_{i<=e} q_i and SS_e = sum_{i<=e} C_i, uint64 modulo 2^64; a(e) the
 *             latest arc start at or before e (a max-scan).  An epoch that is not measured adds q = 0, starts no arc and
 *             gets no smoothed output.
 *   output    for a measured e: n = min(e - a(e) + 1, W); S = (int64)(SS_e - SS_{e-n} - n C_e), SS_{-1} = 0; m = ((double) S *
 *             0x1p-48) / (double) n; tx_frac_out = tx_frac - m (n = 1: tx_frac itself); count = n; cmc_s = (double)(int64)(C_e -
 *             C_{a(e)}) * 0x1p-48, code minus carrier since the arc began (the multipath and divergence monitor).  S is the
 *             sum over the window of (P_j - L_j) - (P_e - L_e): tx_frac_out is the transmit time of the pseudorange L_e +
 *             mean(P_j - L_j) over the last n epochs of the arc, the Hatch filter in sliding-window form, identical to the
 *             recursive form while n < W; white code noise of sigma leaves sigma / sqrt(n).  |S| <= 2^30 W (W - 1) / 2 <
 *             2^62, so the modular differences are exact whatever the global sums wrapped to.  The ionosphere delays the
 *             code and advances the carrier: code minus carrier diverges at twice the ionosphere's rate of change, and the
 *             mean over the window lags by half the window's share of it -- W bounds that bias.  No carry into tx_ms: the
 *             fix takes any finite fraction.
 * tx_frac_out double [E][K] is required.  Optional (null: not written): count int32 [E][K], cmc_s double [E][K], status
 * uint8 [E][K], channels [K].
 * The call enqueues four kernels on the context's stream, does not synchronise and allocates nothing but the context's
 * scratch (gat_smooth_observables_plan, csrc/gat_smooth_plan.h).  The epochs are cut into chunks of consecutive epochs, one
 * contiguous [chunk][K] span each; a workgroup a chunk reduces every thread's run to (len, Q, S, last reset, counts) --
 * segments combine as Q = Q_A + Q_B, S = S_A + S_B + len_B Q_A, the later reset -- and the chunk through LDS; a wave a
 * channel scans the chunks' segments and writes the channel's record; a workgroup a chunk walks its span again and writes C,
 * SS and a(e) to the scratch, and the status; one thread an (epoch, channel) gathers SS_{e-n} and C_{a(e)} and writes the
 * rest.  No atomics, no floating-point sum, plain vector stores: the same bits every call and from the twin.
 * Refusals, all before any launch (the host twin: before any write): GAT_ERR_ARG for a null required pointer (the four
 * times, carrier_cycles, carrier_frac, config, tx_frac_out), a wrong struct_size, E or K < 1, a flag other than
 * GAT_SMOOTH_RATE_TEST, reserved != 0, the rate test without doppler_hz, a carrier_hz or epoch_seconds that is not finite
 * or not > 0 and an if_hz that is not finite; GAT_ERR_RANGE for a window outside 1 .. 65536, a cmc_gate_s outside (0,
 * 2^-18], a rate_gate_cycles that is not finite and > 0 with the rate test, K above GAT_MAX_FIX_CHANNELS, E above
 * GAT_MAX_SMOOTH_EPOCHS and a call whose scratch would exceed 1 GiB. */
#define GAT_MAX_SMOOTH_EPOCHS 1048576
#define GAT_SMOOTH_RATE_TEST 1  /* flags */
#define GAT_SMOOTH_MEASURED 1   /* status */
#define GAT_SMOOTH_GAP 2
#define GAT_SMOOTH_CMC 4
#define GAT_SMOOTH_RATE 8
typedef struct gat_smooth_config {
    uint32_t struct_size;    /* sizeof(gat_smooth_config) */
    uint32_t flags;          /* GAT_SMOOTH_RATE_TEST */
    int32_t window;          /* W, 1 .. 65536 epochs */
    int32_t reserved;        /* 0 */
    double carrier_hz;       /* > 0, finite (1575.42e6) */
    double if_hz;            /* finite: the observables' */
    double epoch_seconds;    /* > 0, finite: epoch_stride * block_seconds */
    double cmc_gate_s;       /* 0 < g <= 2^-18 s */
    double rate_gate_cycles; /* > 0 with GAT_SMOOTH_RATE_TEST */
} gat_smooth_config;
typedef struct gat_smooth_channel {
    int32_t measured;    /* measured epochs */
    int32_t arcs;        /* arc starts */
    int32_t cmc_resets;  /* epochs with GAT_SMOOTH_CMC */
    int32_t rate_resets; /* epochs with GAT_SMOOTH_RATE */
} gat_smooth_channel;
GAT_API int32_t gat_smooth_observables(gat_ctx *ctx, const int32_t *tx_ms_dev, const double *tx_frac_dev, const int32_t *rx_ms_dev,
                                       const double *rx_frac_dev, const int64_t *carrier_cycles_dev, const double *carrier_frac_dev,
                                       const double *doppler_hz_dev, const uint8_t *valid_dev, int32_t num_epochs, int32_t num_channels,
                                       const gat_smooth_config *config, double *tx_frac_out_dev, int32_t *count_dev, double *cmc_s_dev,
                                       uint8_t *status_dev, gat_smooth_channel *channels_dev);
/* The same rule in plain loops on the HOST: every pointer is host memory; the bit-exact reference of the device call. */
GAT_API int32_t gat_smooth_observables_host(const int32_t *tx_ms_host, const double *tx_frac_host, const int32_t *rx_ms_host,
                                            const double *rx_frac_host, const int64_t *carrier_cycles_host,
                                            const double *carrier_frac_host, const double *doppler_hz_host, const uint8_t *valid_host,
                                            int32_t num_epochs, int32_t num_channels, const gat_smooth_config *config,
                                            double *tx_frac_out, int32_t *count, double *cmc_s, uint8_t *status,
                                            gat_smooth_channel *channels);
/* What gat_smooth_observables would do with a call (csrc/gat_smooth_plan.h; no context, no device, nothing is read but
 * config).  A chunk is chunk_epochs consecutive epochs (the last one takes what is left); a workgroup of `threads` is rows x
 * lanes, lane l < num_channels holds channel l and row r walks run_epochs consecutive epochs of the chunk.  The emit and the
 * output stage are separate kernels for every call: a look-back of up to W epochs leaves the workgroup's chunk.  The refusals
 * are the call's, but for the pointers. */
typedef struct gat_smooth_plan {
    uint32_t struct_size; /* sizeof(gat_smooth_plan), set by the caller */
    int32_t chunk_epochs, num_chunks;
    int32_t lanes, rows, run_epochs;
    int32_t threads, lds_bytes;
    int32_t chunk_workgroups;   /* num_chunks: the sum kernel and the emit kernel each */
    int32_t channel_workgroups; /* four channels (waves) a workgroup */
    int32_t output_workgroups;  /* `threads` (epoch, channel) pairs a workgroup */
    int32_t reserved;
    int64_t scratch_bytes;
} gat_smooth_plan;
GAT_API int32_t gat_smooth_observables_plan(int32_t num_epochs, int32_t num_channels, const gat_smooth_config *config,
                                            gat_smooth_plan *plan);

/* ---- snapshot fix: a coarse-time position from code phases alone -------------------------------------------------------------
 * Every stage behind the loop takes transmit times as whole milliseconds and a fraction, and only gat_observables makes the
 * whole milliseconds: it needs bit sync, frame sync and a decoded TOW.  gat_snapshot_fix needs the fraction alone -- what
 * gat_observables writes as tx_frac, or an acquisition's code phase over the chipping rate --, the ephemerides, a position
 * known to tens of kilometres and a clock known to tens of seconds: the whole milliseconds are resolved against the
 * predicted ranges, and a solve of five unknowns finds position, clock bias and the error of the coarse time together
 * (coarse-time navigation).  The rule is csrc/gat_snap.h on top of gat_fix.h and gat_vel.h: FP64, no contraction, no libm
 * transcendental, every sum in channel order from +0, the same text in the kernel and in the host twin, the same bits.
 * Per epoch (K <= 64 channels; Lambda = c 1e-3):
 *   fraction code_frac [E][K], the transmit time modulo 1 ms in seconds; not finite or outside [0, 1e-3): no measurement.
 *            phi = rx_frac - code_frac, plus 1e-3 with the borrow beta = 1 where it is negative; z = c phi.
 *   predict  at a state (x, y, z, b, t_c) -- first (prior, 0, 0), the prior prior_xyz [E][3] or config.init_xyz -- the
 *            transmit time is R - t_c - tau, R = rx_ms 1e-3 + rx_frac, tau = 0.075 s, then r / c of the last range, three
 *            evaluations as the velocity fix does; clock, orbit and their rates by the fix's and the velocity fix's
 *            expressions; p = r + b - c dts with the fix's Earth-rotation turn; sin el as the fix's.
 *   usable   a channel counts (num_valid) when its ephemeris is usable as in gat_position_fix, its fraction and the
 *            reception are given and its first predicted state is finite; it is used when besides its weight is finite and
 *            > 0.  Fewer than 5 used channels: GAT_SNAP_FEW_SATS.
 *   integers the reference k0 is the used channel with the largest predicted sin el, the lowest index on a tie (within 1e6 m
 *            of the centre every sin el is 0: the lowest used channel).  n_k0 = rint((p_k0 - z_k0) / Lambda); n_k = rint(q_k),
 *            q_k = (p_k - p_k0 + n_k0 Lambda + z_k0 - z_k) / Lambda, for every usable channel.  GAT_SNAP_AMBIGUOUS: a used
 *            channel has |q_k - n_k| > 0.5 - ambiguity_margin; the fix stands.  A |q| above 1e6: GAT_SNAP_NONFINITE.  A wrong
 *            n_k0 shifts every n_k alike and is absorbed by b and one millisecond of t_c: no error.  The margin guards a prior
 *            within (0.5 - margin) Lambda / 2 of the truth in every relative range (30 km and 20 s with the default); far
 *            beyond it a relative error near a whole Lambda clears the margin with a wrong integer: with more than five
 *            used channels rms_residual_m then shows hundreds of metres, and gat_position_fix_raim finds it in the times.
 *   solver   rho_k = n_k Lambda + z_k stays fixed.  An iteration: per usable channel the satellite at its own time (rx_ms -
 *            n_k - beta_k) 1e-3 + code_frac_k - t_c, the fix's row with v = rho - (r + b - c dts), the row a = (-los, 1,
 *            -(los . v_sat - c ddts)), the satellite's velocity turned as its position; the 20 sums of w a_i a_j (i <= j)
 *            and w a_i v over the used channels; a 5 x 5 Cholesky with the fix's pivot rule; the state moves by the step.
 *            A pass ends when |d_xyz| < tol_m or after max_iter iterations (GAT_SNAP_NOT_CONVERGED, the outputs stand).
 *            GAT_SNAP_SINGULAR and GAT_SNAP_NONFINITE as the fix's; FEW_SATS, SINGULAR and NONFINITE end the epoch with every
 *            output zero (tx_ms and rx_ms_out -1) but status, num_valid, num_used and iterations.
 *   again    after a converged pass the integers are resolved once more at the solved state; if a used channel's changed, one
 *            more pass runs from that state (GAT_SNAP_RERESOLVED).
 *   mask     then the fix's mask at the solved state, with at least 5 channels kept (GAT_SNAP_MASKED, GAT_SNAP_MASK_STARVED).
 *   record   the rows once more at the final state: rms_residual_m over the used channels; pdop, gdop (x, y, z, b) and tdop
 *            (t_c, s / m) from the diagonal of the unweighted 5 x 5 (A^T A)^-1; clock_bias_s = b / c; coarse_time_s = t_c.
 * Optional outputs (null: not written): tx_ms int32 [E][K] = (rx_ms - n_k - beta_k - m) mod 604800000 with m = rint(1000 t_c),
 * -1 for a channel that does not count; rx_ms_out int32 [E] = (rx_ms - m) mod 604800000; n_ms int32 [E][K]; resid, sin_el
 * double [E][K] and used uint8 [E][K] with the fix's conventions.  tx_ms, the caller's code_frac, rx_ms_out and rx_frac go
 * into gat_position_fix, gat_position_fix_raim, gat_range_corrections and gat_velocity_fix as they are.  The true t_c is a
 * whole number of milliseconds (the fraction of the clock's error is b); an m off by one moves every satellite by a
 * millisecond of its flight, every range by less than 1 m, and is not flagged.  One epoch never touches another.
 * gat_snapshot_fix enqueues one kernel of the fix's geometry on the context's stream (a wave an epoch, a lane a channel, four
 * epochs a workgroup; the satellite is evaluated again every iteration), does not synchronise, allocates nothing and uses no
 * atomics.  Refusals, all before any launch or write: GAT_ERR_ARG for a null required pointer (ephemerides, code_frac, rx_ms,
 * rx_frac, config, fixes), a wrong struct_size, E or K < 1, max_iter < 1, tol_m not > 0, a mask_sin or init_xyz that is not
 * finite, an ambiguity_margin outside [0, 0.5] and non-zero flags; GAT_ERR_RANGE for K above GAT_MAX_FIX_CHANNELS and E above
 * GAT_MAX_FIX_EPOCHS. */
#define GAT_SNAP_FEW_SATS 1
#define GAT_SNAP_SINGULAR 2
#define GAT_SNAP_NONFINITE 4
#define GAT_SNAP_NOT_CONVERGED 8
#define GAT_SNAP_MASK_STARVED 16
#define GAT_SNAP_MASKED 32
#define GAT_SNAP_AMBIGUOUS 64
#define GAT_SNAP_RERESOLVED 128
typedef struct gat_snap_config {
    uint32_t struct_size;    /* sizeof(gat_snap_config) */
    int32_t max_iter;        /* iterations a pass, >= 1 (10) */
    double tol_m;            /* > 0 (1e-4) */
    double mask_sin;         /* sin of the elevation mask; -1: off */
    double init_xyz[3];      /* the prior of every epoch without prior_xyz, m */
    double ambiguity_margin; /* 0 .. 0.5 (0.1) */
    uint32_t flags;          /* 0 */
    uint32_t reserved;
} gat_snap_config;
typedef struct gat_snap_fix {
    int32_t status;       /* GAT_SNAP_* bits; 0: a converged fix with every integer clear of the margin */
    int32_t num_valid;    /* channels that count in this epoch */
    int32_t num_used;     /* channels in the last pass's equations */
    int32_t iterations;
    double x, y, z;       /* ECEF at reception, m */
    double clock_bias_s;  /* b / c */
    double coarse_time_s; /* t_c: the receiver's coarse clock minus the time the satellites were evaluated at */
    double rms_residual_m;
    double last_step_m;
    double gdop, pdop;
    double tdop;          /* s / m */
} gat_snap_fix;
GAT_API int32_t gat_snapshot_fix(gat_ctx *ctx, const gat_ephemeris *eph_dev, const double *code_frac_dev, const int32_t *rx_ms_dev,
                                 const double *rx_frac_dev, const double *prior_xyz_dev, const double *weights_dev, int32_t num_epochs,
                                 int32_t num_channels, const gat_snap_config *config, gat_snap_fix *fixes_dev, int32_t *tx_ms_dev,
                                 int32_t *rx_ms_out_dev, int32_t *n_ms_dev, double *resid_dev, double *sin_el_dev, uint8_t *used_dev);
/* The same rule in plain loops on the HOST: every pointer is host memory; the bit-exact reference of the device call. */
GAT_API int32_t gat_snapshot_fix_host(const gat_ephemeris *eph_host, const double *code_frac_host, const int32_t *rx_ms_host,
                                      const double *rx_frac_host, const double *prior_xyz_host, const double *weights_host,
                                      int32_t num_epochs, int32_t num_channels, const gat_snap_config *config, gat_snap_fix *fixes,
                                      int32_t *tx_ms, int32_t *rx_ms_out, int32_t *n_ms, double *resid, double *sin_el, uint8_t *used);
/* What gat_snapshot_fix would do with a call (csrc/gat_snap_plan.h): gat_position_fix's geometry, its own LDS (20 terms). */
GAT_API int32_t gat_snapshot_fix_plan(int32_t num_epochs, int32_t num_channels, const gat_snap_config *config, gat_fix_plan *plan);

#ifdef __cplusplus
}
#endif
#endif /* GAT_H_ */
