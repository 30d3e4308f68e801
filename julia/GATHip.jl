# GATHip.jl -- reference-side binding of libgat (include/gat.h) for GPUAcceleratedTracking.jl.
#
# NOT EXECUTED ANYWHERE IN THIS PROJECT: neither this container nor the GPU box has a `julia`
# binary.  It is the thin `ccall` shim a maintainer of the reference would add (INTEGRATION.md);
# every entry point it binds is exercised through the same C ABI by the Python host layer, by
# examples/gat_known_answer.c (the same call sequence as `downconvert_and_correlate!` below, in C) and
# by the tests.  Keep it mechanical: one ccall per exported symbol, no logic of its own.  Since it cannot run, it is
# linted instead: tests/test_julia_shim_lint.py parses every `ccall` below and checks symbol, argument count and
# argument type classes against include/gat.h, the struct mirrors field by field, and that every export is bound.
#
# Usage inside the reference (src/GPUAcceleratedTracking.jl), no other edits:
#     include("GATHip.jl"); using .GATHip
#     include("GATHipHarness.jl")         # methods of _run_kernel_benchmark / kernel_algorithm for id 9000
#     ALGODICT["hip_fused"] = 9000; ALGODICTINV[9000] = "hip_fused"
# and in scripts/run_benchmarks_gpsl1.jl:  "processor" => ["GPU"], "algorithm" => ["hip_fused"].
module GATHip

using StaticArrays
import Tracking
import Tracking: NumAnts, NumAccumulators, EarlyPromptLateCorrelator
import GNSSSignals: get_code_frequency, get_code_length
import Unitful: Hz, ustrip

const libgat = get(ENV, "LIBGAT", "libgat.so")

const GAT_OK = Int32(0)
const GAT_FLAG_ATOMIC = UInt32(1)
const GAT_FLAG_GRAPH = UInt32(2)
const GAT_OWN_STREAM = Ptr{Cvoid}(typemax(UInt))   # (void *)-1: the library creates and owns a non-blocking stream
const GAT_LAYOUT_PLANAR = Int32(0)
const GAT_LAYOUT_INTERLEAVED = Int32(1)
const GAT_LAYOUT_INTERLEAVED_I16 = Int32(2)
const GAT_LAYOUT_INTERLEAVED_I8 = Int32(3)
# kernel selection (gat_set_matrix_core): vector kernel / automatic / f32 MFMA / split-bf16 MFMA
const GAT_MC_VECTOR, GAT_MC_AUTO, GAT_MC_F32, GAT_MC_BF16_SPLIT = Int32(0), Int32(1), Int32(2), Int32(3)

# struct gat_channel_params (40 bytes)
struct ChannelParams
    prn::Int32            # 0-based
    reserved::Int32
    code_freq_hz::Float64
    carrier_freq_hz::Float64
    code_phase_chips::Float64
    carrier_phase_cycles::Float64
end

# struct gat_signal_desc (56 bytes)
struct SignalDesc
    re::Ptr{Cvoid}
    im::Ptr{Cvoid}
    layout::Int32
    num_ants::Int32
    num_samples::Int64
    ant_stride::Int64
    block_stride::Int64
    chan_stride::Int64
end

# struct gat_loop_config (80 bytes: 7 doubles, 5 int32, 4 bytes of tail padding)
struct LoopConfig
    block_seconds::Float64
    pll_bandwidth_hz::Float64
    dll_bandwidth_hz::Float64
    code_freq_nominal_hz::Float64
    carrier_center_hz::Float64
    if_hz::Float64
    early_late_spacing_chips::Float64
    code_length::Int32
    num_taps::Int32
    early_index::Int32
    prompt_index::Int32
    late_index::Int32
end

# struct gat_loop_state (72 bytes), one per channel, device-resident
struct LoopState
    init_carrier_doppler_hz::Float64
    carrier_doppler_hz::Float64
    code_doppler_hz::Float64
    pll_acc1::Float64
    pll_acc2::Float64
    dll_acc::Float64
    last_pll_error_cycles::Float64
    last_dll_error_chips::Float64
    prompt_power::Float64
end

# struct gat_launch_info (48 bytes): geometry of the last correlate call
struct LaunchInfo
    workgroups::Int32
    threads::Int32
    splits::Int32
    ant_tile::Int32
    vec::Int32
    lds_bytes::Int32
    finalize_launched::Int32
    matrix_core::Int32
    channels_per_wg::Int32
    blocks_per_wg::Int32
    prefetch_depth::Int32
    bf16_terms::Int32
end

# struct gat_resident_config (28 bytes) / gat_resident_info (32 bytes): the resident correlator (single-block calls
# without a kernel launch, include/gat.h)
struct ResidentConfig
    struct_size::UInt32
    idle_us::UInt32
    life_ms::UInt32
    max_calls::UInt32
    max_workgroups::UInt32
    host_pollers::UInt32
    doorbell::UInt32
end
struct ResidentInfo
    workgroups::Int32
    splits::Int32
    running::Int32
    last_exit::Int32
    launches::UInt64
    calls::UInt64
end

# struct gat_acq_config (72 bytes) / gat_acq_result (80 bytes): the acquisition search (include/gat.h gat_acquire)
struct AcqConfig
    struct_size::UInt32
    num_doppler_bins::Int32
    if_hz::Float64
    code_freq_hz::Float64
    doppler_first_hz::Float64
    doppler_step_hz::Float64
    first_shift::Int64
    code_step_samples::Int32
    num_code_bins::Int32
    min_peak_ratio::Float64
    code_length::Int32
    reserved::Int32
end
# struct gat_acq_fft_plan (40 bytes): what gat_acquire_fft would do with a call (include/gat.h gat_acquire_fft_plan)
struct AcqFftPlan
    struct_size::UInt32
    fft_log2::Int32
    num_segments::Int32
    segment_lags::Int32
    passes::Int32
    doppler_batch::Int32
    unit_batch::Int32
    unit_groups::Int32
    scratch_bytes::Int64
end
struct AcqResult
    prn::Int32
    detected::Int32
    doppler_bin::Int32
    code_bin::Int32
    peak_power::Float64
    noise_power::Float64
    second_power::Float64
    peak_to_second::Float64
    cn0_dbhz::Float64
    carrier_doppler_hz::Float64
    code_phase_chips::Float64
    num_noise_bins::Int64
end

struct GatError <: Exception
    status::Int32
    msg::String
end

# One libgat context plus the buffers the operator re-uses on every call: device outputs and their host copies are
# allocated once (grown on demand), so that a timed `downconvert_and_correlate!` does no allocation at all.
mutable struct Context
    handle::Ptr{Cvoid}
    out_re::Ptr{Cfloat}      # device, out_cap floats each
    out_im::Ptr{Cfloat}
    out_cap::Int
    host_re::Vector{Float32}
    host_im::Vector{Float32}
    # argument buffers of the single-channel call, written in place: the harness method times nothing but the ccall
    prm1::Vector{ChannelParams}
    shifts::Vector{Int32}
    desc::Base.RefValue{SignalDesc}
    # a library-owned stream by default: single-block calls then end with the completion flag gat_sync spins on
    # (include/gat.h; ~4 us less per call + sync than hipStreamSynchronize on this platform)
    function Context(device::Integer = 0, stream::Ptr{Cvoid} = GAT_OWN_STREAM)
        h = Ref{Ptr{Cvoid}}(C_NULL)
        rc = ccall((:gat_create, libgat), Int32, (Int32, Ptr{Cvoid}, Ref{Ptr{Cvoid}}), device, stream, h)
        rc == GAT_OK || throw(GatError(rc, "gat_create"))
        ctx = new(h[], C_NULL, C_NULL, 0, Float32[], Float32[], [ChannelParams(0, 0, 0.0, 0.0, 0.0, 0.0)], Int32[],
                  Ref(SignalDesc(C_NULL, C_NULL, GAT_LAYOUT_PLANAR, 0, 0, 0, 0, 0)))
        finalizer(ctx) do c
            c.out_re == C_NULL || ccall((:gat_free, libgat), Int32, (Ptr{Cvoid}, Ptr{Cvoid}), c.handle, c.out_re)
            c.out_im == C_NULL || ccall((:gat_free, libgat), Int32, (Ptr{Cvoid}, Ptr{Cvoid}), c.handle, c.out_im)
            ccall((:gat_destroy, libgat), Int32, (Ptr{Cvoid},), c.handle)
        end
        ctx
    end
end

function check(ctx::Context, rc::Int32)
    rc == GAT_OK && return nothing
    msg = unsafe_string(ccall((:gat_last_error, libgat), Cstring, (Ptr{Cvoid},), ctx.handle))
    throw(GatError(rc, msg))
end

sync(ctx::Context) = check(ctx, ccall((:gat_sync, libgat), Int32, (Ptr{Cvoid},), ctx.handle))
set_matrix_core(ctx::Context, mode::Integer) =
    check(ctx, ccall((:gat_set_matrix_core, libgat), Int32, (Ptr{Cvoid}, Int32), ctx.handle, Int32(mode)))

set_stream(ctx::Context, stream::Ptr{Cvoid}) =
    check(ctx, ccall((:gat_set_stream, libgat), Int32, (Ptr{Cvoid}, Ptr{Cvoid}), ctx.handle, stream))
set_vector_tiling(ctx::Context, max_antenna_tiles::Integer, max_channels::Integer, max_blocks::Integer) =
    check(ctx, ccall((:gat_set_vector_tiling, libgat), Int32, (Ptr{Cvoid}, Int32, Int32, Int32), ctx.handle,
                     Int32(max_antenna_tiles), Int32(max_channels), Int32(max_blocks)))
# launch-geometry option by name ("dc_one_wave_min", "dc_depth", "sync_flag_wgs", ...: include/gat.h gat_set_option)
set_option(ctx::Context, name::AbstractString, value::Integer) =
    check(ctx, ccall((:gat_set_option, libgat), Int32, (Ptr{Cvoid}, Cstring, Int64), ctx.handle, name, Int64(value)))
function last_launch_info(ctx::Context)
    info = Ref(LaunchInfo(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0))
    check(ctx, ccall((:gat_last_launch_info, libgat), Int32, (Ptr{Cvoid}, Ref{LaunchInfo}, Csize_t), ctx.handle, info,
                     sizeof(LaunchInfo)))
    info[]
end

# library build identity: "libgat <version> (gfx950) git:<sha> flags:<-D list | none>"
version() = unsafe_string(ccall((:gat_version, libgat), Cstring, ()))

# ---- what add_metadata! needs (src/benchmarks.jl:11-32: GPU_model = name(CUDA.CuDevice(0)), CUDA = CUDA.version()):
#      (device name, HIP runtime version as "major.minor.patch", compute units)
function device_info(ctx::Context)
    name = Vector{UInt8}(undef, 256)
    ver, cus = Ref{Int32}(0), Ref{Int32}(0)
    check(ctx, ccall((:gat_device_info, libgat), Int32, (Ptr{Cvoid}, Ptr{UInt8}, Csize_t, Ref{Int32}, Ref{Int32}),
                     ctx.handle, name, length(name), ver, cus))
    v = Int(ver[])                                   # HIP_VERSION = major * 10^7 + minor * 10^5 + patch
    unsafe_string(pointer(name)), string(v ÷ 10_000_000, ".", (v ÷ 100_000) % 100, ".", v % 100_000), Int(cus[])
end
function device_info(device::Integer = 0)
    ctx = Context(device, Ptr{Cvoid}(C_NULL))        # default stream: nothing is launched
    info = device_info(ctx)
    finalize(ctx)
    info
end

# ---- get_correlator_sample_shifts(system, correlator, fs, preferred_code_shift) (src/benchmarks.jl:105-107) as the
#      library computes it: s = max(1, round(spacing * fs / fc)), shifts[l] = (l - L ÷ 2) * s
function sample_shifts(num_taps::Integer, sampling_frequency_hz::Float64, code_frequency_hz::Float64, spacing_chips::Float64 = 0.5)
    shifts = Vector{Int32}(undef, num_taps)
    rc = ccall((:gat_sample_shifts, libgat), Int32, (Int32, Float64, Float64, Float64, Ptr{Int32}),
               Int32(num_taps), sampling_frequency_hz, code_frequency_hz, spacing_chips, shifts)
    rc == GAT_OK || throw(GatError(rc, "gat_sample_shifts"))
    shifts
end

# ---- the library's own PRN generators ("GPSL1" / "GPSL5"; IS-GPS-200 / -705) for hosts without GNSSSignals.jl:
#      (codes Int8 [code_length x num_prns], code frequency in Hz)
function gen_codes(system::AbstractString, num_prns::Integer)
    lc, fc = Ref{Int32}(0), Ref{Float64}(0.0)
    rc = ccall((:gat_gen_codes, libgat), Int32, (Cstring, Int32, Ptr{Int8}, Ref{Int32}, Ref{Float64}),
               system, Int32(num_prns), Ptr{Int8}(C_NULL), lc, fc)               # size query
    rc == GAT_OK || throw(GatError(rc, "gat_gen_codes"))
    codes = Matrix{Int8}(undef, lc[], num_prns)
    rc = ccall((:gat_gen_codes, libgat), Int32, (Cstring, Int32, Ptr{Int8}, Ref{Int32}, Ref{Float64}),
               system, Int32(num_prns), codes, lc, fc)
    rc == GAT_OK || throw(GatError(rc, "gat_gen_codes"))
    codes, fc[]
end

# ---- hipEvent pair on the context's stream (CUDA.@elapsed of test/algorithms.jl:1242): device time of what is enqueued between
timer_start(ctx::Context) = check(ctx, ccall((:gat_timer_start, libgat), Int32, (Ptr{Cvoid},), ctx.handle))
function timer_stop(ctx::Context)                   # synchronises; milliseconds
    ms = Ref{Cfloat}(0)
    check(ctx, ccall((:gat_timer_stop, libgat), Int32, (Ptr{Cvoid}, Ref{Cfloat}), ctx.handle, ms))
    Float64(ms[])
end

# per-call statistics (BenchmarkTools keeps every sample's time, src/benchmarks.jl:1-9): one lap before the first timed launch and
# one after every launch; `timer_laps` waits for the newest and returns the intervals in milliseconds
timer_lap(ctx::Context) = check(ctx, ccall((:gat_timer_lap, libgat), Int32, (Ptr{Cvoid},), ctx.handle))
function timer_laps(ctx::Context, capacity::Integer = 65536)
    ms = Vector{Cfloat}(undef, capacity)
    n = Ref{Int32}(0)
    check(ctx, ccall((:gat_timer_laps, libgat), Int32, (Ptr{Cvoid}, Ptr{Cfloat}, Int32, Ref{Int32}), ctx.handle, ms, Int32(capacity), n))
    Float64.(ms[1:n[]])
end
# a kernel that only reads `bytes` of device memory, `launches` times: milliseconds per launch (the in-run read ceiling)
function debug_read_stream(ctx::Context, dev::Ptr{Cvoid}, bytes::Integer, variant::Integer = 0, launches::Integer = 8)
    ms = Vector{Cfloat}(undef, launches)
    check(ctx, ccall((:gat_debug_read_stream, libgat), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Csize_t, Int32, Int32, Ptr{Cfloat}),
                     ctx.handle, dev, Csize_t(bytes), Int32(variant), Int32(launches), ms))
    Float64.(ms)
end

# ---- device memory (for hosts without AMDGPU.jl; with AMDGPU.jl pass ROCArray pointers instead)
function dmalloc(ctx::Context, bytes::Integer)
    p = Ref{Ptr{Cvoid}}(C_NULL)
    check(ctx, ccall((:gat_malloc, libgat), Int32, (Ptr{Cvoid}, Csize_t, Ref{Ptr{Cvoid}}), ctx.handle, bytes, p))
    p[]
end
dfree(ctx::Context, p) = check(ctx, ccall((:gat_free, libgat), Int32, (Ptr{Cvoid}, Ptr{Cvoid}), ctx.handle, p))
h2d(ctx::Context, dst, src::Array) = check(ctx, ccall((:gat_memcpy_h2d, libgat), Int32,
    (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Csize_t), ctx.handle, dst, src, sizeof(src)))
d2h(ctx::Context, dst::Array, src, bytes::Integer = sizeof(dst)) = check(ctx, ccall((:gat_memcpy_d2h, libgat), Int32,
    (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Csize_t), ctx.handle, dst, src, bytes))

dmemset(ctx::Context, dst, value::Integer, bytes::Integer) = check(ctx, ccall((:gat_memset, libgat), Int32,
    (Ptr{Cvoid}, Ptr{Cvoid}, Int32, Csize_t), ctx.handle, dst, Int32(value), bytes))

# make room for `n` output floats per plane (device + host); a no-op once the buffers are large enough
function reserve_outputs!(ctx::Context, n::Integer)
    n <= ctx.out_cap && return nothing
    ctx.out_re == C_NULL || dfree(ctx, ctx.out_re)
    ctx.out_im == C_NULL || dfree(ctx, ctx.out_im)
    ctx.out_re = convert(Ptr{Cfloat}, dmalloc(ctx, 4n))
    ctx.out_im = convert(Ptr{Cfloat}, dmalloc(ctx, 4n))
    ctx.out_cap = n
    resize!(ctx.host_re, n); resize!(ctx.host_im, n)
    nothing
end

# ---- system wrapper: `system.codes` stays whatever GNSSSignals provides; we upload it once.
struct HipSystem{S}
    system::S              # GPSL1() / GPSL5() from GNSSSignals (CPU codes)
    ctx::Context
end
function HipSystem(system; device = 0)
    ctx = Context(device)
    codes = Int8.(system.codes)                     # [code_length x num_prns], column-major
    check(ctx, ccall((:gat_set_codes, libgat), Int32, (Ptr{Cvoid}, Ptr{Int8}, Int32, Int32),
                     ctx.handle, codes, size(codes, 1), size(codes, 2)))
    HipSystem(system, ctx)
end
get_code_frequency(s::HipSystem) = get_code_frequency(s.system)
get_code_length(s::HipSystem) = get_code_length(s.system)

# ---- device-resident signal [N x M] in any of libgat's four sample layouts
struct HipSignal
    re::Ptr{Cvoid}          # planar: Float32 real plane; interleaved layouts: base pointer
    im::Ptr{Cvoid}          # planar: Float32 imaginary plane; interleaved layouts: C_NULL
    layout::Int32
    sample_bytes::Int       # bytes of one sample in `re` (planar: 4; ComplexF32: 8; int16 pairs: 4; int8 pairs: 2)
    num_samples::Int
    num_ants::Int
end
# planar re / im planes: the reference's StructArray{ComplexF32} (src/gen_signal.jl:179)
function HipSignal(ctx::Context, re::Matrix{Float32}, im::Matrix{Float32})
    dre = dmalloc(ctx, sizeof(re)); h2d(ctx, dre, re)
    dim = dmalloc(ctx, sizeof(im)); h2d(ctx, dim, im)
    HipSignal(dre, dim, GAT_LAYOUT_PLANAR, 4, size(re, 1), size(re, 2))
end
# interleaved ComplexF32 [N x M]
function HipSignal(ctx::Context, x::Matrix{ComplexF32})
    d = dmalloc(ctx, sizeof(x)); h2d(ctx, d, x)
    HipSignal(d, C_NULL, GAT_LAYOUT_INTERLEAVED, 8, size(x, 1), size(x, 2))
end
# interleaved {Int16 re, Int16 im} pairs as a front-end delivers them ("sc16"): Complex{Int16} [N x M]
function HipSignal(ctx::Context, x::Matrix{Complex{Int16}})
    d = dmalloc(ctx, sizeof(x)); h2d(ctx, d, x)
    HipSignal(d, C_NULL, GAT_LAYOUT_INTERLEAVED_I16, 4, size(x, 1), size(x, 2))
end
function HipSignal(ctx::Context, x::Matrix{Complex{Int8}})
    d = dmalloc(ctx, sizeof(x)); h2d(ctx, d, x)
    HipSignal(d, C_NULL, GAT_LAYOUT_INTERLEAVED_I8, 2, size(x, 1), size(x, 2))
end
function free!(ctx::Context, s::HipSignal)
    dfree(ctx, s.re); s.im == C_NULL || dfree(ctx, s.im)
end

function signal_desc(signal::HipSignal, start_sample::Integer, num_samples::Integer)
    off = (start_sample - 1) * signal.sample_bytes
    SignalDesc(signal.re + off, signal.im == C_NULL ? C_NULL : signal.im + off, signal.layout, signal.num_ants,
               num_samples, signal.num_samples, num_samples, 0)
end

# ---- the hot call, nothing but the ccall: K channels of one block into the context's cached output buffers
#      [M x L x K] (asynchronous on the context's stream)
function correlate_async!(ctx::Context, desc::SignalDesc, prm::Vector{ChannelParams}, shifts::Vector{Int32},
                          sampling_frequency_hz::Float64, M::Integer, flags::UInt32 = UInt32(0))
    K, L = length(prm), length(shifts)
    reserve_outputs!(ctx, M * L * K)
    check(ctx, ccall((:gat_downconvert_and_correlate, libgat), Int32,
                     (Ptr{Cvoid}, Ref{SignalDesc}, Ptr{ChannelParams}, Int32, Int32, Int32, Ptr{Int32}, Float64,
                      Ptr{Cfloat}, Ptr{Cfloat}, UInt32),
                     ctx.handle, Ref(desc), prm, 1, K, L, shifts, sampling_frequency_hz, ctx.out_re, ctx.out_im, flags))
end
# blocking read-back of the last result into the cached host buffers: (re, im) views of length M*L*K
function fetch_result!(ctx::Context, n::Integer)
    d2h(ctx, ctx.host_re, ctx.out_re, 4n); d2h(ctx, ctx.host_im, ctx.out_im, 4n)   # gat_memcpy_d2h synchronises
    view(ctx.host_re, 1:n), view(ctx.host_im, 1:n)
end

# ---- the same launch with the [K x B] parameter records already on the device (a tracking loop that produces them
#      there; flags may carry GAT_FLAG_GRAPH: the call's launches replayed as one hipGraph when it repeats)
function correlate_dev_async!(ctx::Context, desc::SignalDesc, params_dev::Ptr{Cvoid}, B::Integer, K::Integer,
                              shifts::Vector{Int32}, sampling_frequency_hz::Float64, out_re::Ptr{Cfloat}, out_im::Ptr{Cfloat},
                              flags::UInt32 = UInt32(0))
    check(ctx, ccall((:gat_downconvert_and_correlate_dev, libgat), Int32,
                     (Ptr{Cvoid}, Ref{SignalDesc}, Ptr{Cvoid}, Int32, Int32, Int32, Ptr{Int32}, Float64,
                      Ptr{Cfloat}, Ptr{Cfloat}, UInt32),
                     ctx.handle, Ref(desc), params_dev, Int32(B), Int32(K), Int32(length(shifts)), shifts,
                     sampling_frequency_hz, out_re, out_im, flags))
end

# ---- closed tracking loop around the correlator (what Tracking.track does around downconvert_and_correlate!; the
#      reference only borrows TrackingState buffers, src/benchmarks.jl:54-61).  All arrays device-resident:
#      acc [M x L x K] of one block, state LoopState[K], cur / next ChannelParams[K] (may alias)
function tracking_update!(ctx::Context, acc_re::Ptr{Cfloat}, acc_im::Ptr{Cfloat}, K::Integer, M::Integer, cfg::LoopConfig,
                          state_dev::Ptr{Cvoid}, cur_dev::Ptr{Cvoid}, next_dev::Ptr{Cvoid})
    check(ctx, ccall((:gat_tracking_update, libgat), Int32,
                     (Ptr{Cvoid}, Ptr{Cfloat}, Ptr{Cfloat}, Int32, Int32, Ref{LoopConfig}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                     ctx.handle, acc_re, acc_im, Int32(K), Int32(M), Ref(cfg), state_dev, cur_dev, next_dev))
end
# num_blocks x {correlate, update} enqueued from native code, parameters ping-ponging between params_a (current at
# entry) and params_b; returns true when params_b holds the parameters of the block after the last one
function tracking_run!(ctx::Context, desc::SignalDesc, num_blocks::Integer, K::Integer, shifts::Vector{Int32},
                       sampling_frequency_hz::Float64, cfg::LoopConfig, state_dev::Ptr{Cvoid}, params_a_dev::Ptr{Cvoid},
                       params_b_dev::Ptr{Cvoid}, acc_re::Ptr{Cfloat}, acc_im::Ptr{Cfloat}, acc_block_stride::Integer = 0,
                       flags::UInt32 = UInt32(0))
    cur_is_b = Ref{Int32}(0)
    check(ctx, ccall((:gat_tracking_run, libgat), Int32,
                     (Ptr{Cvoid}, Ref{SignalDesc}, Int32, Int32, Int32, Ptr{Int32}, Float64, Ref{LoopConfig}, Ptr{Cvoid}, Ptr{Cvoid},
                      Ptr{Cvoid}, Ptr{Cfloat}, Ptr{Cfloat}, Int64, UInt32, Ref{Int32}),
                     ctx.handle, Ref(desc), Int32(num_blocks), Int32(K), Int32(length(shifts)), shifts, sampling_frequency_hz,
                     Ref(cfg), state_dev, params_a_dev, params_b_dev, acc_re, acc_im, Int64(acc_block_stride), flags, cur_is_b))
    cur_is_b[] != 0
end

# ---- the operator: same argument list as Tracking.downconvert_and_correlate!
#      (call site src/benchmarks.jl:63-79).  Scratch arguments are ignored.  No allocation on the device or of
#      result arrays: outputs live in the context (first call sizes them).
function Tracking.downconvert_and_correlate!(
    system::HipSystem, signal::HipSignal, correlator::EarlyPromptLateCorrelator,
    code_replica, code_phase, carrier_replica, carrier_phase, downconverted_signal,
    code_frequency, correlator_sample_shifts::SVector{L,<:Integer}, carrier_frequency,
    sampling_frequency, signal_start_sample, num_samples, prn
) where {L}
    ctx = system.ctx
    M = signal.num_ants
    reserve_outputs!(ctx, M * L)                         # a no-op after the first call
    correlate_single!(ctx, signal_desc(signal, signal_start_sample, num_samples), prn - 1,
                      Float64(ustrip(Hz, code_frequency)), Float64(ustrip(Hz, carrier_frequency)), Float64(code_phase),
                      Float64(carrier_phase), correlator_sample_shifts, Float64(ustrip(Hz, sampling_frequency)),
                      ctx.out_re, ctx.out_im)
    re, im = fetch_result!(ctx, M * L)
    accumulators = SVector{L}(ntuple(l -> SVector{M}(ntuple(m -> complex(re[(l - 1) * M + m], im[(l - 1) * M + m]), M)), L))
    return EarlyPromptLateCorrelator(accumulators)       # functional update, as Tracking.jl does
end

# ---- K satellite channels of one block in ONE launch (the reference's experimental _3d_4431! kernel,
#      src/algorithms.jl:637, correlates several satellites per launch too).  Returns ComplexF32 [M x L x K].
function downconvert_and_correlate_channels!(
    system::HipSystem, signal::HipSignal, code_phases, carrier_phases, code_frequencies,
    correlator_sample_shifts::SVector{L,<:Integer}, carrier_frequencies, sampling_frequency,
    signal_start_sample, num_samples, prns
) where {L}
    ctx = system.ctx
    M, K = signal.num_ants, length(prns)
    prm = [ChannelParams(prns[k] - 1, 0, ustrip(Hz, code_frequencies[k]), ustrip(Hz, carrier_frequencies[k]),
                         Float64(code_phases[k]), Float64(carrier_phases[k])) for k in 1:K]
    correlate_async!(ctx, signal_desc(signal, signal_start_sample, num_samples), prm,
                     Int32[correlator_sample_shifts...], Float64(ustrip(Hz, sampling_frequency)), M)
    re, im = fetch_result!(ctx, M * L * K)
    reshape(complex.(re, im), M, L, K)
end

# ---- the same call with every argument buffer cached in the context (no allocation at all per call): what
#      kernel_algorithm(..., ::KernelAlgorithm{9000}) in GATHipHarness.jl runs
function correlate_single!(ctx::Context, desc::SignalDesc, prn0::Integer,
                           code_freq_hz::Float64, carrier_freq_hz::Float64, code_phase::Float64, carrier_phase::Float64,
                           shifts, sampling_frequency_hz::Float64, out_re::Ptr{Cfloat}, out_im::Ptr{Cfloat})
    L = length(shifts)
    length(ctx.shifts) == L || resize!(ctx.shifts, L)          # first call / another tap count only
    @inbounds for l in 1:L
        ctx.shifts[l] = shifts[l]
    end
    @inbounds ctx.prm1[1] = ChannelParams(prn0, 0, code_freq_hz, carrier_freq_hz, code_phase, carrier_phase)
    ctx.desc[] = desc
    check(ctx, ccall((:gat_downconvert_and_correlate, libgat), Int32,
                     (Ptr{Cvoid}, Ref{SignalDesc}, Ptr{ChannelParams}, Int32, Int32, Int32, Ptr{Int32}, Float64,
                      Ptr{Cfloat}, Ptr{Cfloat}, UInt32),
                     ctx.handle, ctx.desc, ctx.prm1, 1, 1, L, ctx.shifts, sampling_frequency_hz, out_re, out_im, UInt32(0)))
end

# ---- reduce_cplx_multi_3/4/5 two-pass column sums (src/reduction.jl:93, :331, :548; launch sequence
#      src/algorithms.jl:914-922; test/reduction.jl:13-52): planar complex [n x cols] on the device -> [cols]
function reduce_cplx_multi!(ctx::Context, out_re::Ptr{Cfloat}, out_im::Ptr{Cfloat}, in_re::Ptr{Cfloat}, in_im::Ptr{Cfloat},
                            n::Integer, cols::Integer)
    check(ctx, ccall((:gat_reduce_cplx_multi, libgat), Int32,
                     (Ptr{Cvoid}, Ptr{Cfloat}, Ptr{Cfloat}, Int64, Int32, Ptr{Cfloat}, Ptr{Cfloat}),
                     ctx.handle, in_re, in_im, n, cols, out_re, out_im))
end

# ---- gen_code_replica_texture_mem_strided_nsat_kernel! (src/algorithms.jl:78-98; test/algorithms.jl:1199): the
#      replicas of K satellite channels in one launch, row k of `replica_dev` (row_stride floats apart) = channel k.
#      params_dev: device array of K ChannelParams (prn, code_freq_hz, code_phase_chips used)
function gen_code_replica_nsat!(ctx::Context, replica_dev::Ptr{Cfloat}, count::Integer, row_stride::Integer, K::Integer,
                                params_dev::Ptr{Cvoid}, sampling_frequency_hz::Float64, first_shift::Integer)
    check(ctx, ccall((:gat_gen_code_replica_multi, libgat), Int32,
                     (Ptr{Cvoid}, Ptr{Cfloat}, Int64, Int64, Int32, Ptr{Cvoid}, Float64, Int64),
                     ctx.handle, replica_dev, count, row_stride, K, params_dev, sampling_frequency_hz, first_shift))
end

# ---- downconvert_and_accumulate_strided_kernel! (src/algorithms.jl:828-866; test/algorithms.jl:1438-1514): the
#      materialising middle stage of the reference's algorithm 2 as a debug export -- carrier [N], downconverted
#      signal [N x M], per-sample products [N x M x L]; any output pointer may be C_NULL
function downconvert_and_accumulate!(ctx::Context, signal::HipSignal, prm::ChannelParams, shifts::Vector{Int32},
                                     sampling_frequency_hz::Float64; carrier_re = C_NULL, carrier_im = C_NULL, dw_re = C_NULL,
                                     dw_im = C_NULL, accum_re = C_NULL, accum_im = C_NULL)
    desc = signal_desc(signal, 1, signal.num_samples)
    check(ctx, ccall((:gat_downconvert_and_accumulate, libgat), Int32,
                     (Ptr{Cvoid}, Ref{SignalDesc}, Ref{ChannelParams}, Int32, Ptr{Int32}, Float64, Ptr{Cfloat}, Ptr{Cfloat},
                      Ptr{Cfloat}, Ptr{Cfloat}, Ptr{Cfloat}, Ptr{Cfloat}),
                     ctx.handle, Ref(desc), Ref(prm), length(shifts), shifts, sampling_frequency_hz, carrier_re, carrier_im,
                     dw_re, dw_im, accum_re, accum_im))
end

# ---- synthetic input on the device: gen_signal! (src/gen_signal.jl:53-175) and its noisy, steered form (AWGN sigma per
#      component, per-antenna steering phases in cycles; the reference's generator is noise-free, paper/paper.tex:116)
function gen_signal!(ctx::Context, signal::HipSignal, params_dev::Ptr{Cvoid}, K::Integer, sampling_frequency_hz::Float64;
                     amplitude = 1.0, steering_cycles_dev::Ptr{Cfloat} = Ptr{Cfloat}(C_NULL), noise_sigma = 0.0, seed = UInt64(0))
    check(ctx, ccall((:gat_gen_signal_noisy, libgat), Int32,
                     (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int32, Int64, Int32, Int64, Int64, Int32, Int32, Ptr{Cvoid}, Float64, Float64,
                      Ptr{Cfloat}, Float64, UInt64),
                     ctx.handle, signal.re, signal.im, signal.layout, signal.num_samples, signal.num_ants, signal.num_samples,
                     signal.num_samples, 1, K, params_dev, sampling_frequency_hz, Float64(amplitude), steering_cycles_dev,
                     Float64(noise_sigma), UInt64(seed)))
end

# the reference's noise-free generator itself (src/gen_signal.jl:53-175), B blocks of K satellites summed
function gen_signal_plain!(ctx::Context, signal::HipSignal, params_dev::Ptr{Cvoid}, B::Integer, K::Integer,
                           sampling_frequency_hz::Float64, block_samples::Integer = signal.num_samples; amplitude = 1.0)
    check(ctx, ccall((:gat_gen_signal, libgat), Int32,
                     (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int32, Int64, Int32, Int64, Int64, Int32, Int32, Ptr{Cvoid}, Float64, Float64),
                     ctx.handle, signal.re, signal.im, signal.layout, Int64(block_samples), Int32(signal.num_ants),
                     Int64(signal.num_samples), Int64(block_samples), Int32(B), Int32(K), params_dev, sampling_frequency_hz,
                     Float64(amplitude)))
end

# ---- several GPUs from one Julia task: one context per device, channels sharded contiguously, no collective
#      (include/gat.h gat_group_*; the C form of this sequence is examples/gat_multi_gpu.c)
mutable struct DeviceGroup
    handle::Ptr{Cvoid}
    n::Int
    function DeviceGroup(devices::Vector{Int32})
        h = Ref{Ptr{Cvoid}}(C_NULL)
        rc = ccall((:gat_group_create, libgat), Int32, (Int32, Ptr{Int32}, Ref{Ptr{Cvoid}}), length(devices), devices, h)
        rc == GAT_OK || throw(GatError(rc, "gat_group_create"))
        g = new(h[], length(devices))
        finalizer(x -> ccall((:gat_group_destroy, libgat), Int32, (Ptr{Cvoid},), x.handle), g)
        g
    end
end
function device_count()
    n = Ref{Int32}(0)
    ccall((:gat_device_count, libgat), Int32, (Ref{Int32},), n) == GAT_OK || throw(GatError(1, "gat_device_count"))
    Int(n[])
end
DeviceGroup() = DeviceGroup(Int32.(0:device_count() - 1))
function gcheck(g::DeviceGroup, rc::Int32)
    rc == GAT_OK && return nothing
    throw(GatError(rc, unsafe_string(ccall((:gat_group_last_error, libgat), Cstring, (Ptr{Cvoid},), g.handle))))
end
set_codes!(g::DeviceGroup, codes::Matrix{Int8}) = gcheck(g, ccall((:gat_group_set_codes, libgat), Int32,
    (Ptr{Cvoid}, Ptr{Int8}, Int32, Int32), g.handle, codes, size(codes, 1), size(codes, 2)))
function shard(g::DeviceGroup, K::Integer, rank::Integer)       # rank 0-based -> (first channel 0-based, count)
    lo, cnt = Ref{Int32}(0), Ref{Int32}(0)
    gcheck(g, ccall((:gat_group_shard, libgat), Int32, (Ptr{Cvoid}, Int32, Int32, Ref{Int32}, Ref{Int32}), g.handle, K, rank, lo, cnt))
    Int(lo[]), Int(cnt[])
end
# bufs[r + 1] (r != src_rank) <- bufs[src_rank + 1]: the ingest device's signal to its peers (hipMemcpyPeerAsync)
replicate!(g::DeviceGroup, src_rank::Integer, bufs::Vector{Ptr{Cvoid}}, bytes::Integer) = gcheck(g, ccall(
    (:gat_group_replicate, libgat), Int32, (Ptr{Cvoid}, Int32, Ptr{Ptr{Cvoid}}, Csize_t), g.handle, src_rank, bufs, bytes))
# member r correlates its channel slice of prm ([K x B], channel fastest) on descs[r + 1] into its own device outputs
correlate!(g::DeviceGroup, descs::Vector{SignalDesc}, prm::Matrix{ChannelParams}, shifts::Vector{Int32}, fs_hz::Float64,
           out_re::Vector{Ptr{Cfloat}}, out_im::Vector{Ptr{Cfloat}}, flags::UInt32 = UInt32(0)) = gcheck(g, ccall(
    (:gat_group_correlate, libgat), Int32,
    (Ptr{Cvoid}, Ptr{SignalDesc}, Ptr{ChannelParams}, Int32, Int32, Int32, Ptr{Int32}, Float64, Ptr{Ptr{Cfloat}}, Ptr{Ptr{Cfloat}}, UInt32),
    g.handle, descs, prm, size(prm, 2), size(prm, 1), length(shifts), shifts, fs_hz, out_re, out_im, flags))
# the members' outputs concatenated along the channel axis: ComplexF32 [M x L x K x B] (synchronises)
function gather(g::DeviceGroup, out_re::Vector{Ptr{Cfloat}}, out_im::Vector{Ptr{Cfloat}}, B, K, L, M)
    re, im = Array{Float32}(undef, M, L, K, B), Array{Float32}(undef, M, L, K, B)
    gcheck(g, ccall((:gat_group_gather, libgat), Int32,
        (Ptr{Cvoid}, Ptr{Ptr{Cfloat}}, Ptr{Ptr{Cfloat}}, Int32, Int32, Int32, Int32, Ptr{Cfloat}, Ptr{Cfloat}),
        g.handle, out_re, out_im, B, K, L, M, re, im))
    complex.(re, im)
end
sync(g::DeviceGroup) = gcheck(g, ccall((:gat_group_sync, libgat), Int32, (Ptr{Cvoid},), g.handle))
function group_size(g::DeviceGroup)
    n = Ref{Int32}(0)
    gcheck(g, ccall((:gat_group_size, libgat), Int32, (Ptr{Cvoid}, Ref{Int32}), g.handle, n))
    Int(n[])
end
# member `rank`'s context handle (borrowed: destroyed with the group) for the single-device entry points
function member_handle(g::DeviceGroup, rank::Integer)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    gcheck(g, ccall((:gat_group_ctx, libgat), Int32, (Ptr{Cvoid}, Int32, Ref{Ptr{Cvoid}}), g.handle, Int32(rank), h))
    h[]
end
# dst (on member dst_rank's device) <- src (on member src_rank's device), asynchronous on the destination's stream,
# ordered behind the source's stream and ahead of the source's later work
function memcpy_peer!(g::DeviceGroup, dst_rank::Integer, dst::Ptr{Cvoid}, src_rank::Integer, src::Ptr{Cvoid}, bytes::Integer)
    gcheck(g, ccall((:gat_memcpy_peer, libgat), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Csize_t),
                    member_handle(g, dst_rank), dst, member_handle(g, src_rank), src, bytes))
end

# the closed loop's update on the host (same arithmetic as gat_tracking_update on the device): `acc_re` / `acc_im` are HOST arrays
# [M x L x K] of one block -- e.g. a `Resident`'s `re` / `im` --, `state` / `cur` / `next` host vectors of length K
tracking_update_host!(acc_re::Array{Float32}, acc_im::Array{Float32}, num_channels::Integer, num_ants::Integer, cfg::LoopConfig,
                      state::Vector{LoopState}, cur::Vector{ChannelParams}, next::Vector{ChannelParams}) =
    ccall((:gat_tracking_update_host, libgat), Int32,
          (Ptr{Cfloat}, Ptr{Cfloat}, Int32, Int32, Ref{LoopConfig}, Ptr{LoopState}, Ptr{ChannelParams}, Ptr{ChannelParams}),
          acc_re, acc_im, Int32(num_channels), Int32(num_ants), Ref(cfg), state, cur, next) == GAT_OK || throw(GatError(Int32(1), "gat_tracking_update_host"))

# ---- resident correlator: what `@benchmark CUDA.@sync kernel_algorithm(...)` (src/benchmarks.jl:120-146) times, without
#      the launch -- one kernel stays on the device for a fixed call geometry (signal buffer, channels, taps), a call rings
#      it through pinned host memory and returns the outputs on the host, ComplexF32 [M x L x K].  The kernel ends by itself
#      (idle / lifetime / call budget, ResidentConfig; zeros = library defaults) and is started again by the next call.
mutable struct Resident
    handle::Ptr{Cvoid}
    ctx::Context
    re::Array{Float32,3}
    im::Array{Float32,3}
    prm::Vector{ChannelParams}
end
function Resident(ctx::Context, desc::SignalDesc, num_channels::Integer, shifts::Vector{Int32}, sampling_frequency_hz::Float64;
                  idle_us = 0, life_ms = 0, max_calls = 0, max_workgroups = 0, host_pollers = 0, doorbell = 0)
    cfg = Ref(ResidentConfig(sizeof(ResidentConfig), idle_us, life_ms, max_calls, max_workgroups, host_pollers, doorbell))
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ctx, ccall((:gat_resident_open, libgat), Int32,
                     (Ptr{Cvoid}, Ref{SignalDesc}, Int32, Int32, Ptr{Int32}, Float64, Ref{ResidentConfig}, Ref{Ptr{Cvoid}}),
                     ctx.handle, Ref(desc), Int32(num_channels), Int32(length(shifts)), shifts, sampling_frequency_hz, cfg, h))
    r = Resident(h[], ctx, Array{Float32}(undef, desc.num_ants, length(shifts), num_channels),
                 Array{Float32}(undef, desc.num_ants, length(shifts), num_channels),
                 [ChannelParams(0, 0, 0.0, 0.0, 0.0, 0.0) for _ in 1:num_channels])
    finalizer(x -> x.handle == C_NULL || ccall((:gat_resident_close, libgat), Int32, (Ptr{Cvoid},), x.handle), r)
    r
end
# one call: r.prm holds the channels' records (written in place by the caller), block_offset in samples from the buffer's
# start; the outputs are in r.re / r.im when it returns
function correlate!(r::Resident, block_offset::Integer = 0)
    check(r.ctx, ccall((:gat_resident_correlate, libgat), Int32, (Ptr{Cvoid}, Ptr{ChannelParams}, Int64, Ptr{Cfloat}, Ptr{Cfloat}),
                       r.handle, r.prm, Int64(block_offset), r.re, r.im))
    r
end
function info(r::Resident)
    i = Ref(ResidentInfo(0, 0, 0, 0, 0, 0))
    check(r.ctx, ccall((:gat_resident_info_get, libgat), Int32, (Ptr{Cvoid}, Ref{ResidentInfo}, Csize_t), r.handle, i, sizeof(ResidentInfo)))
    i[]
end
park!(r::Resident) = check(r.ctx, ccall((:gat_resident_park, libgat), Int32, (Ptr{Cvoid},), r.handle))
# every resident correlator of the context: before anything that waits for the whole device (AMDGPU.synchronize(), hipFree)
park_residents!(ctx::Context) = check(ctx, ccall((:gat_resident_park_all, libgat), Int32, (Ptr{Cvoid},), ctx.handle))
# the receiver loop with the host in it, from native code: num_blocks blocks (block b at first_block_offset + b * block_stride
# samples of the buffer) through {resident call, gat_tracking_update_host}; r.prm: in the first block's records, out the next
# ones; acc_re / acc_im: host arrays of at least max(1, acc_block_stride > 0 ? num_blocks : 1) * M * L * K floats
function tracking_run!(r::Resident, num_blocks::Integer, first_block_offset::Integer, block_stride::Integer, cfg::LoopConfig,
                       state::Vector{LoopState}, acc_re::Array{Float32}, acc_im::Array{Float32}, acc_block_stride::Integer = 0)
    check(r.ctx, ccall((:gat_resident_tracking_run, libgat), Int32,
                       (Ptr{Cvoid}, Int32, Int64, Int64, Ref{LoopConfig}, Ptr{LoopState}, Ptr{ChannelParams}, Ptr{Cfloat}, Ptr{Cfloat}, Int64),
                       r.handle, Int32(num_blocks), Int64(first_block_offset), Int64(block_stride), Ref(cfg), state, r.prm, acc_re, acc_im,
                       Int64(acc_block_stride)))
    r
end
function Base.close(r::Resident)
    r.handle == C_NULL && return nothing
    rc = ccall((:gat_resident_close, libgat), Int32, (Ptr{Cvoid},), r.handle)
    r.handle = C_NULL
    check(r.ctx, rc)
end

# ---- Tracking.gen_code_replica! (scripts/code_replica_experiment.jl:70)
function gen_code_replica!(ctx::Context, code_replica_dev::Ptr{Cfloat}, code_frequency, sampling_frequency,
                           start_code_phase, start_sample, num_samples, shifts, prn)
    count = num_samples + shifts[end] - shifts[1]
    check(ctx, ccall((:gat_gen_code_replica, libgat), Int32,
                     (Ptr{Cvoid}, Ptr{Cfloat}, Int64, Int32, Float64, Float64, Float64, Int64),
                     ctx.handle, code_replica_dev + (start_sample - 1) * sizeof(Cfloat), count, prn - 1,
                     ustrip(Hz, code_frequency), ustrip(Hz, sampling_frequency), Float64(start_code_phase), shifts[1]))
end


# ---- gen_code_replica_texture_mem_kernel! (src/algorithms.jl:121-140): the replica addressed through a Float32 normalised
#      coordinate -- emulation for the code-phase-error study (scripts/code_replica_experiment.jl:81-82); study use only
function gen_code_replica_f32coord!(ctx::Context, code_replica_dev::Ptr{Cfloat}, count::Integer, prn::Integer,
                                    code_frequency_hz::Float64, sampling_frequency_hz::Float64, start_code_phase::Float64,
                                    first_shift::Integer)
    check(ctx, ccall((:gat_gen_code_replica_f32coord, libgat), Int32,
                     (Ptr{Cvoid}, Ptr{Cfloat}, Int64, Int32, Float64, Float64, Float64, Int64),
                     ctx.handle, code_replica_dev, Int64(count), Int32(prn - 1), code_frequency_hz, sampling_frequency_hz,
                     start_code_phase, Int64(first_shift)))
end

# the same study with the texture unit's fixed-point addressing modelled (include/gat.h gat_gen_code_replica_texaddr):
# coord_frac_bits > 0 truncates the wrapped normalised coordinate, texel_frac_bits >= 0 rounds the texel address
function gen_code_replica_texaddr!(ctx::Context, code_replica_dev::Ptr{Cfloat}, count::Integer, prn::Integer,
                                   code_frequency_hz::Float64, sampling_frequency_hz::Float64, start_code_phase::Float64,
                                   first_shift::Integer, coord_frac_bits::Integer, texel_frac_bits::Integer)
    check(ctx, ccall((:gat_gen_code_replica_texaddr, libgat), Int32,
                     (Ptr{Cvoid}, Ptr{Cfloat}, Int64, Int32, Float64, Float64, Float64, Int64, Int32, Int32),
                     ctx.handle, code_replica_dev, Int64(count), Int32(prn - 1), code_frequency_hz, sampling_frequency_hz,
                     start_code_phase, Int64(first_shift), Int32(coord_frac_bits), Int32(texel_frac_bits)))
end

# ---- acquisition (Acquisition.jl's acquire): power over PRN x Doppler x code phase on the device, per-PRN statistics
#      (peak, noise, C/N0, detection) on the host.  `prns` are 1-based as in the reference; power_dev: a device buffer of
#      length(prns) * D * J Float32 (code bin fastest) or C_NULL.  Synchronises.
function acquire!(ctx::Context, desc::SignalDesc, num_blocks::Integer, prns::AbstractVector{<:Integer}, sampling_frequency_hz::Float64,
                  cfg::AcqConfig, power_dev::Ptr{Cvoid} = C_NULL)
    cols = Int32[p - 1 for p in prns]
    res = Vector{AcqResult}(undef, length(cols))
    check(ctx, ccall((:gat_acquire, libgat), Int32,
                     (Ptr{Cvoid}, Ref{SignalDesc}, Int32, Ptr{Int32}, Int32, Float64, Ref{AcqConfig}, Ptr{Cvoid}, Ptr{AcqResult}),
                     ctx.handle, Ref(desc), Int32(num_blocks), cols, Int32(length(cols)), sampling_frequency_hz, Ref(cfg),
                     power_dev, res))
    res
end
# the same search by fast correlation (include/gat.h gat_acquire_fft): the same arguments, results and errors as acquire!; zero-padded
# transforms of F > N points give every lag of a block, so it is the method for sample-spaced grids (code_step_samples = 1) and long codes
function acquire_fft!(ctx::Context, desc::SignalDesc, num_blocks::Integer, prns::AbstractVector{<:Integer}, sampling_frequency_hz::Float64,
                      cfg::AcqConfig, power_dev::Ptr{Cvoid} = C_NULL)
    cols = Int32[p - 1 for p in prns]
    res = Vector{AcqResult}(undef, length(cols))
    check(ctx, ccall((:gat_acquire_fft, libgat), Int32,
                     (Ptr{Cvoid}, Ref{SignalDesc}, Int32, Ptr{Int32}, Int32, Float64, Ref{AcqConfig}, Ptr{Cvoid}, Ptr{AcqResult}),
                     ctx.handle, Ref(desc), Int32(num_blocks), cols, Int32(length(cols)), sampling_frequency_hz, Ref(cfg),
                     power_dev, res))
    res
end
# what acquire_fft! would do with the call, without a device: cfg.code_length must be set; fft_log2, doppler_batch, unit_batch as the
# options acq_fft_log2 / acq_fft_doppler_batch / acq_fft_unit_batch would set them (0: the plan's choice); num_cus from device_info
function acquire_fft_plan(desc::SignalDesc, num_blocks::Integer, num_prns::Integer, sampling_frequency_hz::Float64, cfg::AcqConfig;
                          fft_log2::Integer = 0, doppler_batch::Integer = 0, unit_batch::Integer = 0, num_cus::Integer = 256, own_power::Bool = false)
    plan = Ref(AcqFftPlan(UInt32(sizeof(AcqFftPlan)), 0, 0, 0, 0, 0, 0, 0, 0))
    rc = ccall((:gat_acquire_fft_plan, libgat), Int32,
               (Ref{SignalDesc}, Int32, Int32, Float64, Ref{AcqConfig}, Int32, Int32, Int32, Int32, Int32, Ref{AcqFftPlan}),
               Ref(desc), Int32(num_blocks), Int32(num_prns), sampling_frequency_hz, Ref(cfg), Int32(fft_log2), Int32(doppler_batch),
               Int32(unit_batch), Int32(num_cus), Int32(own_power), plan)
    rc == GAT_OK || throw(GatError(rc, "gat_acquire_fft_plan"))
    plan[]
end
# the twin on the host: desc over host memory, codes[Lc, rows] (Julia's view of the library's [rows x Lc]), prns 1-based rows; the grid
# power[J, D, P], bit for bit the device's for the same fft_log2 and unit_groups
function acquire_fft_host(desc::SignalDesc, num_blocks::Integer, codes::Matrix{Int8}, prns::AbstractVector{<:Integer}, sampling_frequency_hz::Float64,
                          cfg::AcqConfig, fft_log2::Integer, unit_groups::Integer = 1)
    rows = Int32[p - 1 for p in prns]
    power = Array{Float32,3}(undef, Int(cfg.num_code_bins), Int(cfg.num_doppler_bins), length(rows))
    rc = ccall((:gat_acquire_fft_host, libgat), Int32,
               (Ref{SignalDesc}, Int32, Ptr{Int8}, Int32, Int32, Ptr{Int32}, Int32, Float64, Ref{AcqConfig}, Int32, Int32, Ptr{Cfloat}),
               Ref(desc), Int32(num_blocks), codes, Int32(size(codes, 1)), Int32(size(codes, 1)), rows, Int32(length(rows)), sampling_frequency_hz,
               Ref(cfg), Int32(fft_log2), Int32(unit_groups), power)
    rc == GAT_OK || throw(GatError(rc, "gat_acquire_fft_host"))
    power
end
# the same statistics over a host grid power[J, D, P] (Julia's column-major view of the library's [P x D x J])
function acq_stats_host(power::Array{Float32,3}, cfg::AcqConfig, sampling_frequency_hz::Float64, num_samples::Integer)
    J, D, P = size(power)
    res = Vector{AcqResult}(undef, P)
    rc = ccall((:gat_acq_stats_host, libgat), Int32, (Ptr{Cfloat}, Int32, Int32, Int32, Ref{AcqConfig}, Float64, Int64, Ptr{AcqResult}),
               power, Int32(P), Int32(D), Int32(J), Ref(cfg), sampling_frequency_hz, Int64(num_samples), res)
    rc == GAT_OK || throw(GatError(rc, "gat_acq_stats_host"))
    res
end

# ---- antenna-array processing (include/gat.h): spatial covariance of the raw samples, beamformer weights from it, the
#      weights applied to accumulators and inside the loop's update.  Device pointers unless a name says host.
const GAT_BF_CONVENTIONAL, GAT_BF_MVDR, GAT_BF_POWER_INVERSION = Int32(0), Int32(1), Int32(2)
# cov_re / cov_im: device Float32 [M x M x E] (Julia's view of [E][M][M]), E = cld(num_blocks, blocks_per_estimate)
function spatial_covariance!(ctx::Context, desc::SignalDesc, num_blocks::Integer, blocks_per_estimate::Integer, cov_re::Ptr{Cfloat},
                             cov_im::Ptr{Cfloat})
    check(ctx, ccall((:gat_spatial_covariance, libgat), Int32, (Ptr{Cvoid}, Ref{SignalDesc}, Int32, Int32, Ptr{Cfloat}, Ptr{Cfloat}),
                     ctx.handle, Ref(desc), Int32(num_blocks), Int32(blocks_per_estimate), cov_re, cov_im))
end
# w [M x K] Float64 planes from one covariance and K steering vectors [M x K]
function array_weights!(ctx::Context, cov_re::Ptr{Cfloat}, cov_im::Ptr{Cfloat}, num_ants::Integer, steer_re::Ptr{Float64},
                        steer_im::Ptr{Float64}, num_channels::Integer, mode::Int32, loading::Float64, w_re::Ptr{Float64},
                        w_im::Ptr{Float64})
    check(ctx, ccall((:gat_array_weights, libgat), Int32,
                     (Ptr{Cvoid}, Ptr{Cfloat}, Ptr{Cfloat}, Int32, Ptr{Float64}, Ptr{Float64}, Int32, Int32, Float64, Ptr{Float64}, Ptr{Float64}),
                     ctx.handle, cov_re, cov_im, Int32(num_ants), steer_re, steer_im, Int32(num_channels), mode, loading, w_re, w_im))
end
# the same on the host: cov [M x M] planes, steering [M x K] planes (ignored for power inversion); returns ComplexF64 [M x K]
function array_weights_host(cov_re::Matrix{Float32}, cov_im::Matrix{Float32}, steer_re::Matrix{Float64}, steer_im::Matrix{Float64},
                            mode::Int32, loading::Float64 = 0.0)
    M, K = size(cov_re, 1), size(steer_re, 2)
    w_re, w_im = Matrix{Float64}(undef, M, K), Matrix{Float64}(undef, M, K)
    rc = ccall((:gat_array_weights_host, libgat), Int32,
               (Ptr{Cfloat}, Ptr{Cfloat}, Int32, Ptr{Float64}, Ptr{Float64}, Int32, Int32, Float64, Ptr{Float64}, Ptr{Float64}),
               cov_re, cov_im, Int32(M), steer_re, steer_im, Int32(K), mode, loading, w_re, w_im)
    rc == GAT_OK || throw(GatError(rc, "gat_array_weights_host"))
    complex.(w_re, w_im)
end
# y [L x K x B] = sum_m conj(w[m, k]) acc[m, l, k, b]
function beamform!(ctx::Context, acc_re::Ptr{Cfloat}, acc_im::Ptr{Cfloat}, num_blocks::Integer, K::Integer, L::Integer, M::Integer,
                   w_re::Ptr{Float64}, w_im::Ptr{Float64}, out_re::Ptr{Cfloat}, out_im::Ptr{Cfloat})
    check(ctx, ccall((:gat_beamform, libgat), Int32,
                     (Ptr{Cvoid}, Ptr{Cfloat}, Ptr{Cfloat}, Int32, Int32, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Cfloat}, Ptr{Cfloat}),
                     ctx.handle, acc_re, acc_im, Int32(num_blocks), Int32(K), Int32(L), Int32(M), w_re, w_im, out_re, out_im))
end
# beams of the raw samples, y[n, j, b] = sum_m conj(w[m, j]) x[n, m, b]: `out` describes the device memory the call writes
# (GAT_LAYOUT_PLANAR or GAT_LAYOUT_INTERLEAVED, num_ants = num_beams, num_samples = desc.num_samples, chan_stride 0) and is
# afterwards a signal for acquire!, spatial_covariance! and the correlators.  w [M x num_beams] Float64 planes on the device.
function beamform_samples!(ctx::Context, desc::SignalDesc, num_blocks::Integer, w_re::Ptr{Float64}, w_im::Ptr{Float64}, num_beams::Integer,
                           out::SignalDesc)
    check(ctx, ccall((:gat_beamform_samples, libgat), Int32,
                     (Ptr{Cvoid}, Ref{SignalDesc}, Int32, Ptr{Float64}, Ptr{Float64}, Int32, Ref{SignalDesc}),
                     ctx.handle, Ref(desc), Int32(num_blocks), w_re, w_im, Int32(num_beams), Ref(out)))
    out
end
# the same with the planar output described here: out_re / out_im device Float32, beam j at j * out_ant_stride, block b at
# b * out_block_stride (default: blocks back to back)
function beamform_samples(ctx::Context, desc::SignalDesc, num_blocks::Integer, w_re::Ptr{Float64}, w_im::Ptr{Float64}, num_beams::Integer,
                          out_re::Ptr{Cvoid}, out_im::Ptr{Cvoid}, out_ant_stride::Integer, out_block_stride::Integer = desc.num_samples)
    out = SignalDesc(out_re, out_im, Int32(0), Int32(num_beams), desc.num_samples, Int64(out_ant_stride), Int64(out_block_stride), Int64(0))
    beamform_samples!(ctx, desc, num_blocks, w_re, w_im, num_beams, out)
end
# ---- sample conditioning: level statistics, pulse blanking, AGC, requantisation (include/gat.h) --------------------------------
const GAT_COND_BLANK_ALL_ANTS = UInt32(1)
struct CondParams    # gat_cond_params: y = (x - dc) * scale; blanked unless |re| <= threshold and |im| <= threshold
    scale::Float32
    dc_re::Float32
    dc_im::Float32
    threshold::Float32
end
struct SampleStats   # gat_sample_stats_t, one per (estimate, antenna)
    kept::Int64
    blanked::Int64
    sum_re::Float64
    sum_im::Float64
    sum_pow::Float64
    max_abs::Float32
    pad_::Float32
end
struct AgcConfig     # gat_agc_config
    struct_size::UInt32
    target_rms::Float64
    blank_factor::Float64
    remove_dc::Int32
end
AgcConfig(target_rms::Real, blank_factor::Real = 0.0, remove_dc::Bool = false) =
    AgcConfig(UInt32(sizeof(AgcConfig)), Float64(target_rms), Float64(blank_factor), Int32(remove_dc))
# the conditioned stream: `out` describes the device memory the call writes (any layout, the signal's num_ants and num_samples) and
# is afterwards a signal for acquire!, spatial_covariance! and the correlators; params_dev: M CondParams; counts_dev: UInt64
# [2 x M] = (blanked samples, clipped components), added to, or C_NULL
function condition_samples!(ctx::Context, desc::SignalDesc, num_blocks::Integer, params_dev::Ptr{Cvoid}, out::SignalDesc;
                            blank_all::Bool = false, counts_dev::Ptr{Cvoid} = C_NULL)
    check(ctx, ccall((:gat_condition_samples, libgat), Int32,
                     (Ptr{Cvoid}, Ref{SignalDesc}, Int32, Ptr{Cvoid}, UInt32, Ref{SignalDesc}, Ptr{Cvoid}),
                     ctx.handle, Ref(desc), Int32(num_blocks), params_dev, blank_all ? GAT_COND_BLANK_ALL_ANTS : UInt32(0), Ref(out), counts_dev))
    out
end
# the same rule on host memory (both descriptors point into host arrays): the bit-exact reference of the device call
function condition_samples_host!(desc::SignalDesc, num_blocks::Integer, params::Vector{CondParams}, out::SignalDesc;
                                 blank_all::Bool = false, counts::Union{Nothing,Matrix{UInt64}} = nothing)
    rc = ccall((:gat_condition_samples_host, libgat), Int32,
               (Ref{SignalDesc}, Int32, Ptr{CondParams}, UInt32, Ref{SignalDesc}, Ptr{UInt64}),
               Ref(desc), Int32(num_blocks), params, blank_all ? GAT_COND_BLANK_ALL_ANTS : UInt32(0), Ref(out),
               counts === nothing ? Ptr{UInt64}(C_NULL) : pointer(counts))
    rc == GAT_OK || error("gat_condition_samples_host: status $rc")
    out
end
# level statistics [M x E] SampleStats on the device, E = cld(num_blocks, blocks_per_estimate); params_dev: C_NULL keeps every sample
function sample_stats!(ctx::Context, desc::SignalDesc, num_blocks::Integer, blocks_per_estimate::Integer, stats_dev::Ptr{Cvoid};
                       params_dev::Ptr{Cvoid} = C_NULL, blank_all::Bool = false)
    check(ctx, ccall((:gat_sample_stats, libgat), Int32,
                     (Ptr{Cvoid}, Ref{SignalDesc}, Int32, Int32, Ptr{Cvoid}, UInt32, Ptr{Cvoid}),
                     ctx.handle, Ref(desc), Int32(num_blocks), Int32(blocks_per_estimate), params_dev,
                     blank_all ? GAT_COND_BLANK_ALL_ANTS : UInt32(0), stats_dev))
end
# one estimate's statistics into the next records, on the device
function agc_update!(ctx::Context, stats_dev::Ptr{Cvoid}, num_ants::Integer, cfg::AgcConfig, params_dev::Ptr{Cvoid})
    check(ctx, ccall((:gat_agc_update, libgat), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Int32, Ref{AgcConfig}, Ptr{Cvoid}),
                     ctx.handle, stats_dev, Int32(num_ants), Ref(cfg), params_dev))
end
function agc_update_host(stats::Vector{SampleStats}, cfg::AgcConfig)
    params = Vector{CondParams}(undef, length(stats))
    rc = ccall((:gat_agc_update_host, libgat), Int32, (Ptr{SampleStats}, Int32, Ref{AgcConfig}, Ptr{CondParams}),
               stats, Int32(length(stats)), Ref(cfg), params)
    rc == GAT_OK || error("gat_agc_update_host: status $rc")
    params
end
# ---- sample filtering: complex FIR, decimation and an oscillator over the raw samples (include/gat.h) --------------------------
const GAT_MAX_FIR_TAPS = 256
const GAT_MAX_FIR_DECIMATION = 64
struct FirConfig     # gat_fir_config
    struct_size::UInt32
    num_taps::Int32
    decimation::Int32
    nco_step::Float64    # cycles per INPUT sample
    nco_phase::Float64   # cycles
end
FirConfig(num_taps::Integer, decimation::Integer = 1, nco_step::Real = 0.0, nco_phase::Real = 0.0) =
    FirConfig(UInt32(sizeof(FirConfig)), Int32(num_taps), Int32(decimation), Float64(nco_step), Float64(nco_phase))
# outputs of a block of N samples: the "valid" convolution, decimated
fir_outputs(N::Integer, cfg::FirConfig) = (N - cfg.num_taps) ÷ cfg.decimation + 1
# the filtered stream: y[q] = exp(-2 pi j (P step + phase)) sum_t g[t] x[q D + T - 1 - t]; `out` describes the device memory the call
# writes (GAT_LAYOUT_PLANAR or GAT_LAYOUT_INTERLEAVED, the signal's num_ants, num_samples = fir_outputs(desc.num_samples, cfg)) and is
# afterwards a signal for acquire!, spatial_covariance!, condition_samples! and the correlators; taps: num_taps Float32 each, on the device
function filter_samples!(ctx::Context, desc::SignalDesc, num_blocks::Integer, taps_re::Ptr{Cfloat}, taps_im::Ptr{Cfloat}, cfg::FirConfig,
                         out::SignalDesc)
    check(ctx, ccall((:gat_filter_samples, libgat), Int32,
                     (Ptr{Cvoid}, Ref{SignalDesc}, Int32, Ptr{Cfloat}, Ptr{Cfloat}, Ref{FirConfig}, Ref{SignalDesc}),
                     ctx.handle, Ref(desc), Int32(num_blocks), taps_re, taps_im, Ref(cfg), Ref(out)))
    out
end
# the same rule on host memory (both descriptors and the taps are host arrays): the bit-exact reference of the device call
function filter_samples_host!(desc::SignalDesc, num_blocks::Integer, taps_re::Vector{Float32}, taps_im::Vector{Float32}, cfg::FirConfig,
                              out::SignalDesc)
    rc = ccall((:gat_filter_samples_host, libgat), Int32,
               (Ref{SignalDesc}, Int32, Ptr{Cfloat}, Ptr{Cfloat}, Ref{FirConfig}, Ref{SignalDesc}),
               Ref(desc), Int32(num_blocks), taps_re, taps_im, Ref(cfg), Ref(out))
    rc == GAT_OK || error("gat_filter_samples_host: status $rc")
    out
end
# ---- space-time adaptive processing: the tapped covariance and the space-time sample filter (include/gat.h) ---------------------
#      The snapshot at sample n is z[t * M + m] = x[n - t, m] (tap 0 the newest sample), Q = M * num_taps elements; the weights
#      come from array_weights! with num_ants = Q.  Weights referenced to tap r advance the stream by num_taps - 1 - r samples.
const GAT_MAX_ST_TAPS = 16
spacetime_delay(num_taps::Integer, ref_tap::Integer) = num_taps - 1 - ref_tap
# cov_re / cov_im: device Float32 [Q x Q x E]; every entry over the same N - num_taps + 1 snapshots of a block
function spacetime_covariance!(ctx::Context, desc::SignalDesc, num_blocks::Integer, blocks_per_estimate::Integer, num_taps::Integer,
                               cov_re::Ptr{Cfloat}, cov_im::Ptr{Cfloat})
    check(ctx, ccall((:gat_spacetime_covariance, libgat), Int32, (Ptr{Cvoid}, Ref{SignalDesc}, Int32, Int32, Int32, Ptr{Cfloat}, Ptr{Cfloat}),
                     ctx.handle, Ref(desc), Int32(num_blocks), Int32(blocks_per_estimate), Int32(num_taps), cov_re, cov_im))
end
# y[n', j, b] = sum_q conj(w[q, j]) z_q[n' + T - 1]: `out` describes the device memory the call writes (GAT_LAYOUT_PLANAR or
# GAT_LAYOUT_INTERLEAVED, num_ants = num_beams, num_samples = desc.num_samples - num_taps + 1) and is afterwards a signal for
# acquire!, spatial_covariance! and the correlators.  w [Q x num_beams] Float64 planes on the device.
function spacetime_filter!(ctx::Context, desc::SignalDesc, num_blocks::Integer, w_re::Ptr{Float64}, w_im::Ptr{Float64}, num_taps::Integer,
                           num_beams::Integer, out::SignalDesc)
    check(ctx, ccall((:gat_spacetime_filter, libgat), Int32,
                     (Ptr{Cvoid}, Ref{SignalDesc}, Int32, Ptr{Float64}, Ptr{Float64}, Int32, Int32, Ref{SignalDesc}),
                     ctx.handle, Ref(desc), Int32(num_blocks), w_re, w_im, Int32(num_taps), Int32(num_beams), Ref(out)))
    out
end
# the same rule on host memory (both descriptors and the weights are host arrays): the bit-exact reference of the device call
function spacetime_filter_host!(desc::SignalDesc, num_blocks::Integer, w_re::Matrix{Float64}, w_im::Matrix{Float64}, num_taps::Integer,
                                out::SignalDesc)
    rc = ccall((:gat_spacetime_filter_host, libgat), Int32,
               (Ref{SignalDesc}, Int32, Ptr{Float64}, Ptr{Float64}, Int32, Int32, Ref{SignalDesc}),
               Ref(desc), Int32(num_blocks), w_re, w_im, Int32(num_taps), Int32(size(w_re, 2)), Ref(out))
    rc == GAT_OK || error("gat_spacetime_filter_host: status $rc")
    out
end
# ---- sample spectrum: the summed periodogram of the raw samples per block and antenna (include/gat.h) ---------------------------
const GAT_MIN_SPECTRUM_BINS = 64
const GAT_MAX_SPECTRUM_BINS = 4096
const GAT_MAX_SPECTRUM_SEGMENTS = 4096
struct SpectrumConfig     # gat_spectrum_config
    struct_size::UInt32
    num_bins::Int32      # F: a power of two, 64 .. 4096
    hop::Int32           # H: 1 .. F
    flags::UInt32        # 0
end
SpectrumConfig(num_bins::Integer, hop::Integer = num_bins ÷ 2) =
    SpectrumConfig(UInt32(sizeof(SpectrumConfig)), Int32(num_bins), Int32(hop), UInt32(0))
# segments of a block of N samples
spectrum_segments(N::Integer, cfg::SpectrumConfig) = (N - cfg.num_bins) ÷ cfg.hop + 1
# power[f, m, b] (Float32, num_bins x num_ants x num_blocks in Julia's order, on the device) = sum over the block's segments of
# |FFT(window .* x[s H .+ (1:F)])|^2 in FFT order: the sum, not the mean; window: num_bins Float32 on the device
function sample_spectrum!(ctx::Context, desc::SignalDesc, num_blocks::Integer, window::Ptr{Cfloat}, cfg::SpectrumConfig, power::Ptr{Cfloat})
    check(ctx, ccall((:gat_sample_spectrum, libgat), Int32,
                     (Ptr{Cvoid}, Ref{SignalDesc}, Int32, Ptr{Cfloat}, Ref{SpectrumConfig}, Ptr{Cfloat}),
                     ctx.handle, Ref(desc), Int32(num_blocks), window, Ref(cfg), power))
    power
end
# the same rule on host memory: the bit-exact reference of the device call
function sample_spectrum_host!(desc::SignalDesc, num_blocks::Integer, window::Vector{Float32}, cfg::SpectrumConfig, power::Array{Float32})
    rc = ccall((:gat_sample_spectrum_host, libgat), Int32,
               (Ref{SignalDesc}, Int32, Ptr{Cfloat}, Ref{SpectrumConfig}, Ptr{Cfloat}),
               Ref(desc), Int32(num_blocks), window, Ref(cfg), power)
    rc == GAT_OK || error("gat_sample_spectrum_host: status $rc")
    power
end
# tracking_update! / tracking_update_host! / tracking_run! with weights [M x K] (C_NULL planes: the unweighted calls)
function tracking_update_weighted!(ctx::Context, acc_re::Ptr{Cfloat}, acc_im::Ptr{Cfloat}, K::Integer, M::Integer, cfg::LoopConfig,
                                   state_dev::Ptr{Cvoid}, cur_dev::Ptr{Cvoid}, next_dev::Ptr{Cvoid}, w_re::Ptr{Float64}, w_im::Ptr{Float64})
    check(ctx, ccall((:gat_tracking_update_weighted, libgat), Int32,
                     (Ptr{Cvoid}, Ptr{Cfloat}, Ptr{Cfloat}, Int32, Int32, Ref{LoopConfig}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64},
                      Ptr{Float64}),
                     ctx.handle, acc_re, acc_im, Int32(K), Int32(M), Ref(cfg), state_dev, cur_dev, next_dev, w_re, w_im))
end
tracking_update_host_weighted!(acc_re::Array{Float32}, acc_im::Array{Float32}, num_channels::Integer, num_ants::Integer, cfg::LoopConfig,
                               state::Vector{LoopState}, cur::Vector{ChannelParams}, next::Vector{ChannelParams}, w_re::Matrix{Float64},
                               w_im::Matrix{Float64}) =
    ccall((:gat_tracking_update_host_weighted, libgat), Int32,
          (Ptr{Cfloat}, Ptr{Cfloat}, Int32, Int32, Ref{LoopConfig}, Ptr{LoopState}, Ptr{ChannelParams}, Ptr{ChannelParams}, Ptr{Float64}, Ptr{Float64}),
          acc_re, acc_im, Int32(num_channels), Int32(num_ants), Ref(cfg), state, cur, next, w_re, w_im) == GAT_OK ||
    throw(GatError(Int32(1), "gat_tracking_update_host_weighted"))
function tracking_run_weighted!(ctx::Context, desc::SignalDesc, num_blocks::Integer, K::Integer, shifts::Vector{Int32},
                                sampling_frequency_hz::Float64, cfg::LoopConfig, state_dev::Ptr{Cvoid}, params_a_dev::Ptr{Cvoid},
                                params_b_dev::Ptr{Cvoid}, acc_re::Ptr{Cfloat}, acc_im::Ptr{Cfloat}, w_re::Ptr{Float64}, w_im::Ptr{Float64},
                                acc_block_stride::Integer = 0, flags::UInt32 = UInt32(0))
    cur_is_b = Ref{Int32}(0)
    check(ctx, ccall((:gat_tracking_run_weighted, libgat), Int32,
                     (Ptr{Cvoid}, Ref{SignalDesc}, Int32, Int32, Int32, Ptr{Int32}, Float64, Ref{LoopConfig}, Ptr{Cvoid}, Ptr{Cvoid},
                      Ptr{Cvoid}, Ptr{Cfloat}, Ptr{Cfloat}, Int64, UInt32, Ref{Int32}, Ptr{Float64}, Ptr{Float64}),
                     ctx.handle, Ref(desc), Int32(num_blocks), Int32(K), Int32(length(shifts)), shifts, sampling_frequency_hz,
                     Ref(cfg), state_dev, params_a_dev, params_b_dev, acc_re, acc_im, Int64(acc_block_stride), flags, cur_is_b, w_re, w_im))
    cur_is_b[] != 0
end

# ---- tracking monitor: C/N0, phase lock, bit synchronisation and data symbols from the accumulator history (include/gat.h) ----
# struct gat_monitor_config (160 bytes)
struct MonitorConfig
    struct_size::UInt32
    num_taps::Int32
    prompt_index::Int32       # 0-based, the loop configuration's
    window_blocks::Int32
    symbol_blocks::Int32      # Pd: 1 .. 128
    symbol_offset::Int32      # -1: search; 0 .. Pd-1: forced, in stream blocks
    first_block::Int64        # the stream's number of this call's block 0
    overlay::NTuple{128,Int8} # +1 / -1 for the Pd blocks of a symbol
end
function MonitorConfig(num_taps::Integer, prompt_index::Integer, overlay::AbstractVector{<:Integer}; window_blocks::Integer = 20,
                       symbol_offset::Integer = -1, first_block::Integer = 0)
    ov = ntuple(i -> i <= length(overlay) ? Int8(overlay[i]) : Int8(0), 128)
    MonitorConfig(UInt32(sizeof(MonitorConfig)), Int32(num_taps), Int32(prompt_index), Int32(window_blocks), Int32(length(overlay)),
                  Int32(symbol_offset), Int64(first_block), ov)
end
# the secondary codes as +-1 (a 0 bit is +1): GPS L5 I5 and Q5; GPS L1 C/A has none: ones(Int8, 20)
const NH10 = Int8[1 - 2 * (c - '0') for c in "0000110101"]
const NH20 = Int8[1 - 2 * (c - '0') for c in "00000100110101001110"]
struct MonitorWindow
    sum_p2::Float64
    sum_p4::Float64
    sum_d::Float64
    sum_i::Float64
    sum_q::Float64
    blocks::Int64
end
struct MonitorChannel
    symbol_offset::Int32
    start::Int32
    num_symbols::Int32
    reserved::Int32
    e_max::Float64
    e_second::Float64
end
struct MonitorPlan
    struct_size::UInt32
    num_windows::Int32
    search_symbols::Int32
    symbol_capacity::Int32
    prompt_workgroups::Int32
    window_workgroups::Int32
    term_workgroups::Int32
    energy_workgroups::Int32
    pick_workgroups::Int32
    symbol_workgroups::Int32
    scratch_bytes::Int64
end
# what the caller makes of the raw sums (T: seconds of a block): decibels are not made on the device
phase_lock(w::MonitorWindow) = w.sum_d / w.sum_p2
function cn0_m2m4(w::MonitorWindow, T::Float64)
    m2, m4 = w.sum_p2 / w.blocks, w.sum_p4 / w.blocks
    rad = 2 * m2 * m2 - m4
    rad > 0 || return NaN
    ps = sqrt(rad)
    10 * log10(ps / ((m2 - ps) * T))
end
function cn0_nwpr(sym_re::AbstractVector{Float64}, sym_im::AbstractVector{Float64}, sym_wbp::AbstractVector{Float64}, Pd::Integer, T::Float64)
    (Pd == 1 || isempty(sym_re)) && return NaN
    mu = sum((sym_re .^ 2 .+ sym_im .^ 2) ./ sym_wbp) / length(sym_re)
    1 < mu < Pd || return NaN
    10 * log10((mu - 1) / ((Pd - mu) * T))
end
# Every output is a device pointer or C_NULL (not written); acc: [M x L x K] floats a block, blocks acc_block_stride floats apart;
# prompts [B x K], windows [NW x K], energy [Pd x K], channels [K], symbols [floor(B / Pd) x K] in Julia's order.  Enqueues only.
function track_monitor!(ctx::Context, acc_re::Ptr{Cfloat}, acc_im::Ptr{Cfloat}, acc_block_stride::Integer, num_blocks::Integer,
                        num_channels::Integer, num_ants::Integer, cfg::MonitorConfig; w_re::Ptr{Float64} = Ptr{Float64}(C_NULL),
                        w_im::Ptr{Float64} = Ptr{Float64}(C_NULL), prompt_re::Ptr{Float64} = Ptr{Float64}(C_NULL),
                        prompt_im::Ptr{Float64} = Ptr{Float64}(C_NULL), windows::Ptr{MonitorWindow} = Ptr{MonitorWindow}(C_NULL),
                        energy::Ptr{Float64} = Ptr{Float64}(C_NULL), channels::Ptr{MonitorChannel} = Ptr{MonitorChannel}(C_NULL),
                        sym_re::Ptr{Float64} = Ptr{Float64}(C_NULL), sym_im::Ptr{Float64} = Ptr{Float64}(C_NULL),
                        sym_wbp::Ptr{Float64} = Ptr{Float64}(C_NULL))
    check(ctx, ccall((:gat_track_monitor, libgat), Int32,
                     (Ptr{Cvoid}, Ptr{Cfloat}, Ptr{Cfloat}, Int64, Int32, Int32, Int32, Ref{MonitorConfig}, Ptr{Float64}, Ptr{Float64},
                      Ptr{Float64}, Ptr{Float64}, Ptr{MonitorWindow}, Ptr{Float64}, Ptr{MonitorChannel}, Ptr{Float64}, Ptr{Float64},
                      Ptr{Float64}),
                     ctx.handle, acc_re, acc_im, Int64(acc_block_stride), Int32(num_blocks), Int32(num_channels), Int32(num_ants), Ref(cfg),
                     w_re, w_im, prompt_re, prompt_im, windows, energy, channels, sym_re, sym_im, sym_wbp))
end
# the same rule on host memory, the bit-exact reference of the device call: acc [M, L, K, B] contiguous; returns
# (windows [NW, K], energy [Pd, K], channels [K], sym_re, sym_im, sym_wbp [floor(B / Pd), K])
function track_monitor_host(acc_re::Array{Float32,4}, acc_im::Array{Float32,4}, cfg::MonitorConfig)
    M, L, K, B = size(acc_re)
    Pd, W = Int(cfg.symbol_blocks), Int(cfg.window_blocks)
    windows = Matrix{MonitorWindow}(undef, cld(B, W), K)
    energy = Matrix{Float64}(undef, Pd, K)
    channels = Vector{MonitorChannel}(undef, K)
    sym_re, sym_im, sym_wbp = zeros(Float64, B ÷ Pd, K), zeros(Float64, B ÷ Pd, K), zeros(Float64, B ÷ Pd, K)
    rc = ccall((:gat_track_monitor_host, libgat), Int32,
               (Ptr{Cfloat}, Ptr{Cfloat}, Int64, Int32, Int32, Int32, Ref{MonitorConfig}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                Ptr{Float64}, Ptr{MonitorWindow}, Ptr{Float64}, Ptr{MonitorChannel}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
               acc_re, acc_im, Int64(M * L * K), Int32(B), Int32(K), Int32(M), Ref(cfg), C_NULL, C_NULL, C_NULL, C_NULL, windows, energy,
               channels, sym_re, sym_im, sym_wbp)
    rc == GAT_OK || throw(GatError(rc, "gat_track_monitor_host"))
    windows, energy, channels, sym_re, sym_im, sym_wbp
end
# what track_monitor! would do with the call, without a device
function track_monitor_plan(acc_block_stride::Integer, num_blocks::Integer, num_channels::Integer, num_ants::Integer, cfg::MonitorConfig;
                            own_prompts::Bool = true, want_symbols::Bool = true)
    plan = Ref(MonitorPlan(UInt32(sizeof(MonitorPlan)), 0, 0, 0, 0, 0, 0, 0, 0, 0, 0))
    rc = ccall((:gat_track_monitor_plan, libgat), Int32,
               (Int64, Int32, Int32, Int32, Ref{MonitorConfig}, Int32, Int32, Ref{MonitorPlan}),
               Int64(acc_block_stride), Int32(num_blocks), Int32(num_channels), Int32(num_ants), Ref(cfg), Int32(own_prompts),
               Int32(want_symbols), plan)
    rc == GAT_OK || throw(GatError(rc, "gat_track_monitor_plan"))
    plan[]
end

# ---- subspace: the accumulators' covariance, a batched Hermitian eigensolver, the steering estimate (include/gat.h) ----
const GAT_ACC_COV_CHUNK = 256
const GAT_EIG_MAX_SWEEPS = 60
const GAT_EIG_INPUT_F32 = UInt32(1)
# struct gat_subspace_plan_info (56 bytes)
struct SubspacePlan
    struct_size::UInt32
    num_estimates::Int32
    chunks_per_estimate::Int32
    cov_split::Int32
    cov_workgroups::Int32
    cov_threads::Int32
    cov_lds_bytes::Int32
    cov_reduce_workgroups::Int32
    eig_workgroups::Int32
    eig_threads::Int32
    eig_lds_bytes::Int32
    reserved::Int32
    scratch_bytes::Int64
end
# cov_re / cov_im: device pointers to [M x M x K x E] doubles in Julia's order, E = cld(B, blocks_per_estimate) (<= 0: one estimate);
# tap_index is 0-based as in the loop configuration.  Enqueues only.
function accumulator_covariance!(ctx::Context, acc_re::Ptr{Cfloat}, acc_im::Ptr{Cfloat}, acc_block_stride::Integer, num_blocks::Integer,
                                 num_channels::Integer, num_taps::Integer, num_ants::Integer, tap_index::Integer, cov_re::Ptr{Float64},
                                 cov_im::Ptr{Float64}; blocks_per_estimate::Integer = 0)
    check(ctx, ccall((:gat_accumulator_covariance, libgat), Int32,
                     (Ptr{Cvoid}, Ptr{Cfloat}, Ptr{Cfloat}, Int64, Int32, Int32, Int32, Int32, Int32, Int32, Ptr{Float64}, Ptr{Float64}),
                     ctx.handle, acc_re, acc_im, Int64(acc_block_stride), Int32(num_blocks), Int32(num_channels), Int32(num_taps),
                     Int32(num_ants), Int32(tap_index), Int32(blocks_per_estimate), cov_re, cov_im))
end
# the same rule on host memory, the bit-exact reference: acc [M, L, K, B] contiguous; returns (cov_re, cov_im) [M, M, K, E]
# (Julia's order: element [j, i] of the C matrix [i][j] -- the transpose, i.e. the conjugate of a Hermitian matrix)
function accumulator_covariance_host(acc_re::Array{Float32,4}, acc_im::Array{Float32,4}, tap_index::Integer; blocks_per_estimate::Integer = 0)
    M, L, K, B = size(acc_re)
    bpe = blocks_per_estimate <= 0 || blocks_per_estimate > B ? B : Int(blocks_per_estimate)
    E = cld(B, bpe)
    cov_re, cov_im = zeros(Float64, M, M, K, E), zeros(Float64, M, M, K, E)
    rc = ccall((:gat_accumulator_covariance_host, libgat), Int32,
               (Ptr{Cfloat}, Ptr{Cfloat}, Int64, Int32, Int32, Int32, Int32, Int32, Int32, Ptr{Float64}, Ptr{Float64}),
               acc_re, acc_im, Int64(M * L * K), Int32(B), Int32(K), Int32(L), Int32(M), Int32(tap_index), Int32(blocks_per_estimate), cov_re,
               cov_im)
    rc == GAT_OK || throw(GatError(rc, "gat_accumulator_covariance_host"))
    cov_re, cov_im
end
# a_re / a_im: device pointers to n matrices [Q x Q] of doubles, or of floats with flags = GAT_EIG_INPUT_F32 (the lower triangle of the
# C matrix is read); every output is a device pointer or C_NULL: eigenvalues [Q x n], vectors [Q x R x n], status [n].  Enqueues only.
function hermitian_eig!(ctx::Context, a_re::Ptr{Cvoid}, a_im::Ptr{Cvoid}, num_matrices::Integer, order::Integer, num_vectors::Integer;
                        flags::UInt32 = UInt32(0), eigenvalues::Ptr{Float64} = Ptr{Float64}(C_NULL), vec_re::Ptr{Float64} = Ptr{Float64}(C_NULL),
                        vec_im::Ptr{Float64} = Ptr{Float64}(C_NULL), status::Ptr{Int32} = Ptr{Int32}(C_NULL))
    check(ctx, ccall((:gat_hermitian_eig, libgat), Int32,
                     (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int32, Int32, Int32, UInt32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}),
                     ctx.handle, a_re, a_im, Int32(num_matrices), Int32(order), Int32(num_vectors), flags, eigenvalues, vec_re, vec_im, status))
end
# the same rule on host memory: a_re / a_im [Q, Q, n] as C wrote them (accumulator_covariance_host's planes go in as they are); returns
# (eigenvalues [Q, n] descending, vec_re, vec_im [Q, R, n], status [n])
function hermitian_eig_host(a_re::Array{Float64,3}, a_im::Array{Float64,3}; num_vectors::Integer = size(a_re, 1))
    Q, _, n = size(a_re)
    R = Int(num_vectors)
    eigenvalues = zeros(Float64, Q, n)
    vec_re, vec_im = zeros(Float64, Q, R, n), zeros(Float64, Q, R, n)
    status = zeros(Int32, n)
    rc = ccall((:gat_hermitian_eig_host, libgat), Int32,
               (Ptr{Cvoid}, Ptr{Cvoid}, Int32, Int32, Int32, UInt32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}),
               a_re, a_im, Int32(n), Int32(Q), Int32(R), UInt32(0), eigenvalues, vec_re, vec_im, status)
    rc == GAT_OK || throw(GatError(rc, "gat_hermitian_eig_host"))
    eigenvalues, vec_re, vec_im, status
end
# what the two calls would do, without a device: num_blocks = 0 leaves the covariance out, eig_matrices = 0 the eigensolver
function subspace_plan(; acc_block_stride::Integer = 0, num_blocks::Integer = 0, num_channels::Integer = 1, num_taps::Integer = 1,
                       num_ants::Integer = 1, tap_index::Integer = 0, blocks_per_estimate::Integer = 0, eig_matrices::Integer = 0,
                       eig_order::Integer = 1, eig_vectors::Integer = 0)
    plan = Ref(SubspacePlan(UInt32(sizeof(SubspacePlan)), 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0))
    rc = ccall((:gat_subspace_plan, libgat), Int32,
               (Int64, Int32, Int32, Int32, Int32, Int32, Int32, Int32, Int32, Int32, Ref{SubspacePlan}),
               Int64(acc_block_stride), Int32(num_blocks), Int32(num_channels), Int32(num_taps), Int32(num_ants), Int32(tap_index),
               Int32(blocks_per_estimate), Int32(eig_matrices), Int32(eig_order), Int32(eig_vectors), plan)
    rc == GAT_OK || throw(GatError(rc, "gat_subspace_plan"))
    plan[]
end

# ---- navigation data: frame synchronisation, LNAV parity, CNAV Viterbi decoding and CRC-24Q (include/gat.h) ----
const GAT_NAV_LNAV = Int32(0)   # GPS L1 C/A: hard bits, ten words of (32,26) parity to a 300-bit subframe
const GAT_NAV_CNAV = Int32(1)   # GPS L5 I5: rate-1/2 K = 7 symbols, 300-bit messages with CRC-24Q
const GAT_NAV_FRAME_BITS = 300
const GAT_NAV_TAIL_BITS = 32
# struct gat_nav_config (20 bytes)
struct NavConfig
    struct_size::UInt32
    format::Int32
    symbol_capacity::Int32    # row stride of sym_re: the monitor's floor(B / Pd)
    max_frames::Int32
    min_frames::Int32
end
NavConfig(format::Integer, symbol_capacity::Integer; max_frames::Integer = max(1, symbol_capacity ÷ (format == GAT_NAV_CNAV ? 600 : 300)),
          min_frames::Integer = 1) = NavConfig(UInt32(sizeof(NavConfig)), Int32(format), Int32(symbol_capacity), Int32(max_frames), Int32(min_frames))
struct NavChannel
    frame_offset::Int32       # decoded-bit index of bit 1 of frame 0, or -1
    symbol_phase::Int32
    inverted::Int32
    score::Int32
    second_score::Int32
    num_frames::Int32
    num_bits::Int32
    tow_steps::Int32
end
struct NavFrame
    status::Int32
    tow::Int32
    id::Int32
    prn::Int32
    words::NTuple{10,UInt32}
end
struct NavPlan
    struct_size::UInt32
    num_phases::Int32
    bit_capacity::Int32
    num_candidates::Int32
    slice_workgroups::Int32
    quantise_workgroups::Int32
    trellis_workgroups::Int32
    score_workgroups::Int32
    pick_workgroups::Int32
    frame_workgroups::Int32
    scratch_bytes::Int64
end
nav_phases(cfg::NavConfig) = cfg.format == GAT_NAV_CNAV ? 2 : 1
# Every pointer is a device pointer; an output may be C_NULL (not written); sym_re: [capacity x K] in Julia's order, mon_channels:
# the monitor's records (C_NULL: every row is full); frames [max_frames x K], decoded [bit_capacity x P x K], path_metric [P x K].
# Enqueues only.
function nav_decode!(ctx::Context, sym_re::Ptr{Float64}, num_channels::Integer, cfg::NavConfig;
                     mon_channels::Ptr{MonitorChannel} = Ptr{MonitorChannel}(C_NULL), channels::Ptr{NavChannel} = Ptr{NavChannel}(C_NULL),
                     frames::Ptr{NavFrame} = Ptr{NavFrame}(C_NULL), decoded::Ptr{UInt8} = Ptr{UInt8}(C_NULL),
                     path_metric::Ptr{Int32} = Ptr{Int32}(C_NULL))
    check(ctx, ccall((:gat_nav_decode, libgat), Int32,
                     (Ptr{Cvoid}, Ptr{Float64}, Ptr{MonitorChannel}, Int32, Ref{NavConfig}, Ptr{NavChannel}, Ptr{NavFrame}, Ptr{UInt8}, Ptr{Int32}),
                     ctx.handle, sym_re, mon_channels, Int32(num_channels), Ref(cfg), channels, frames, decoded, path_metric))
end
# the same rule on host memory, the bit-exact reference of the device call: sym_re [capacity, K]; returns
# (channels [K], frames [max_frames, K], decoded [bit_capacity, P, K], path_metric [P, K])
function nav_decode_host(sym_re::Matrix{Float64}, format::Integer; mon_channels::Union{Nothing,Vector{MonitorChannel}} = nothing,
                         max_frames::Integer = max(1, size(sym_re, 1) ÷ (format == GAT_NAV_CNAV ? 600 : 300)), min_frames::Integer = 1)
    cap, K = size(sym_re)
    cfg = NavConfig(format, cap; max_frames = max_frames, min_frames = min_frames)
    P = nav_phases(cfg)
    channels = Vector{NavChannel}(undef, K)
    frames = Matrix{NavFrame}(undef, Int(max_frames), K)
    decoded = zeros(UInt8, cap ÷ P, P, K)
    path_metric = zeros(Int32, P, K)
    rc = ccall((:gat_nav_decode_host, libgat), Int32,
               (Ptr{Float64}, Ptr{MonitorChannel}, Int32, Ref{NavConfig}, Ptr{NavChannel}, Ptr{NavFrame}, Ptr{UInt8}, Ptr{Int32}),
               sym_re, mon_channels === nothing ? Ptr{MonitorChannel}(C_NULL) : pointer(mon_channels), Int32(K), Ref(cfg), channels, frames,
               decoded, path_metric)
    rc == GAT_OK || throw(GatError(rc, "gat_nav_decode_host"))
    channels, frames, decoded, path_metric
end
# what nav_decode! would do with a call that asks for every output, without a device
function nav_decode_plan(num_channels::Integer, cfg::NavConfig)
    plan = Ref(NavPlan(UInt32(sizeof(NavPlan)), 0, 0, 0, 0, 0, 0, 0, 0, 0, 0))
    rc = ccall((:gat_nav_decode_plan, libgat), Int32, (Int32, Ref{NavConfig}, Ref{NavPlan}), Int32(num_channels), Ref(cfg), plan)
    rc == GAT_OK || throw(GatError(rc, "gat_nav_decode_plan"))
    plan[]
end

# ---- position fix: LNAV ephemeris, satellite states and the batched least-squares solver (include/gat.h) ----
const GAT_MAX_FIX_CHANNELS = 64
const GAT_MAX_FIX_EPOCHS = 16777216
const GAT_FIX_FEW_SATS = Int32(1)
const GAT_FIX_SINGULAR = Int32(2)
const GAT_FIX_NONFINITE = Int32(4)
const GAT_FIX_NOT_CONVERGED = Int32(8)
const GAT_FIX_MASK_STARVED = Int32(16)
const GAT_FIX_MASKED = Int32(32)
const GAT_EPH_OK = Int32(0)
const GAT_EPH_MISSING = Int32(1)
const GAT_EPH_IODE = Int32(2)
# struct gat_ephemeris (200 bytes): SI units and radians
struct Ephemeris
    wn::Int32
    iodc::Int32
    iode::Int32
    health::Int32
    ura::Int32
    fit::Int32
    toc::Float64
    toe::Float64
    af0::Float64
    af1::Float64
    af2::Float64
    tgd::Float64
    sqrt_a::Float64
    e::Float64
    m0::Float64
    delta_n::Float64
    omega0::Float64
    i0::Float64
    omega::Float64
    omega_dot::Float64
    idot::Float64
    cuc::Float64
    cus::Float64
    crc::Float64
    crs::Float64
    cic::Float64
    cis::Float64
    valid::Int32
    reason::Int32
end
# struct gat_fix_config (56 bytes)
struct FixConfig
    struct_size::UInt32
    max_iter::Int32
    tol_m::Float64
    mask_sin::Float64             # sin of the elevation mask; -1: off
    init_xyz::NTuple{3,Float64}
    flags::UInt32
    reserved::UInt32
end
FixConfig(; max_iter::Integer = 10, tol_m::Real = 1e-4, mask_sin::Real = -1.0, init_xyz = (0.0, 0.0, 0.0)) =
    FixConfig(UInt32(sizeof(FixConfig)), Int32(max_iter), Float64(tol_m), Float64(mask_sin), Float64.(Tuple(init_xyz)), UInt32(0), UInt32(0))
# struct gat_fix (80 bytes)
struct Fix
    status::Int32
    num_valid::Int32
    num_used::Int32
    iterations::Int32
    x::Float64
    y::Float64
    z::Float64
    clock_bias_s::Float64
    rms_residual_m::Float64
    last_step_m::Float64
    gdop::Float64
    pdop::Float64
end
struct FixPlan
    struct_size::UInt32
    workgroups::Int32
    waves_per_workgroup::Int32
    threads::Int32
    lds_bytes::Int32
    reserved::Int32
    scratch_bytes::Int64
end
# Every pointer is a device pointer; weights and the four last outputs may be C_NULL.  In Julia's order tx_ms, tx_frac, weights,
# resid, sin_el, used are [K x E], sat [4 x K x E], rx_ms, rx_frac, fixes [E].  Enqueues only.
function position_fix!(ctx::Context, eph::Ptr{Ephemeris}, tx_ms::Ptr{Int32}, tx_frac::Ptr{Float64}, rx_ms::Ptr{Int32}, rx_frac::Ptr{Float64},
                       num_epochs::Integer, num_channels::Integer, cfg::FixConfig, fixes::Ptr{Fix};
                       weights::Ptr{Float64} = Ptr{Float64}(C_NULL), sat::Ptr{Float64} = Ptr{Float64}(C_NULL),
                       resid::Ptr{Float64} = Ptr{Float64}(C_NULL), sin_el::Ptr{Float64} = Ptr{Float64}(C_NULL),
                       used::Ptr{UInt8} = Ptr{UInt8}(C_NULL))
    check(ctx, ccall((:gat_position_fix, libgat), Int32,
                     (Ptr{Cvoid}, Ptr{Ephemeris}, Ptr{Int32}, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Int32, Int32, Ref{FixConfig},
                      Ptr{Fix}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{UInt8}),
                     ctx.handle, eph, tx_ms, tx_frac, rx_ms, rx_frac, weights, Int32(num_epochs), Int32(num_channels), Ref(cfg), fixes, sat,
                     resid, sin_el, used))
end
# the same rule on host memory, the bit-exact reference of the device call: tx_ms, tx_frac [K, E]; returns
# (fixes [E], sat [4, K, E], resid [K, E], sin_el [K, E], used [K, E])
function position_fix_host(eph::Vector{Ephemeris}, tx_ms::Matrix{Int32}, tx_frac::Matrix{Float64}, rx_ms::Vector{Int32}, rx_frac::Vector{Float64};
                           weights::Union{Nothing,Matrix{Float64}} = nothing, cfg::FixConfig = FixConfig())
    K, E = size(tx_ms)
    fixes = Vector{Fix}(undef, E)
    sat = zeros(Float64, 4, K, E)
    resid = zeros(Float64, K, E)
    sin_el = zeros(Float64, K, E)
    used = zeros(UInt8, K, E)
    rc = ccall((:gat_position_fix_host, libgat), Int32,
               (Ptr{Ephemeris}, Ptr{Int32}, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Int32, Int32, Ref{FixConfig}, Ptr{Fix},
                Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{UInt8}),
               eph, tx_ms, tx_frac, rx_ms, rx_frac, weights === nothing ? Ptr{Float64}(C_NULL) : pointer(weights), Int32(E), Int32(K), Ref(cfg),
               fixes, sat, resid, sin_el, used)
    rc == GAT_OK || throw(GatError(rc, "gat_position_fix_host"))
    fixes, sat, resid, sin_el, used
end
# what position_fix! would do with a call, without a device
function position_fix_plan(num_epochs::Integer, num_channels::Integer, cfg::FixConfig = FixConfig())
    plan = Ref(FixPlan(UInt32(sizeof(FixPlan)), 0, 0, 0, 0, 0, 0))
    rc = ccall((:gat_position_fix_plan, libgat), Int32, (Int32, Int32, Ref{FixConfig}, Ref{FixPlan}), Int32(num_epochs), Int32(num_channels),
               Ref(cfg), plan)
    rc == GAT_OK || throw(GatError(rc, "gat_position_fix_plan"))
    plan[]
end
# one channel's ephemeris from its frame records (nav_decode_host's frames[:, k]); valid = 0 and a reason where there is none
function lnav_ephemeris(frames::Vector{NavFrame})
    eph = Ref{Ephemeris}()
    rc = ccall((:gat_lnav_ephemeris_host, libgat), Int32, (Ptr{NavFrame}, Int32, Ref{Ephemeris}), frames, Int32(length(frames)), eph)
    rc == GAT_OK || throw(GatError(rc, "gat_lnav_ephemeris_host"))
    eph[]
end
# the inverse: the 190 payload bits of subframes 1, 2 and 3, [190, 3]
function lnav_ephemeris_words(eph::Ephemeris)
    bits = zeros(UInt8, 190, 3)
    rc = ccall((:gat_lnav_ephemeris_words_host, libgat), Int32, (Ref{Ephemeris}, Ptr{UInt8}), Ref(eph), bits)
    rc == GAT_OK || throw(GatError(rc, "gat_lnav_ephemeris_words_host"))
    bits
end

# ---- observables: the loop's parameter history, transmit times and carrier phase from it (include/gat.h) ----
const GAT_OBS_BAD_RECORD = Int32(1)
const GAT_OBS_NO_BIT_SYNC = Int32(2)
const GAT_OBS_NO_FRAME_SYNC = Int32(4)
const GAT_OBS_FRAME_OUTSIDE = Int32(8)
const GAT_OBS_NO_TOW = Int32(16)
const GAT_OBS_EDGE_AMBIGUOUS = Int32(32)
const GAT_OBS_RX_GIVEN = Int32(0)
const GAT_OBS_RX_FROM_TX = Int32(1)
# tracking_run_weighted! with the ping-pong pair replaced by history_dev [K x (num_blocks + 1)] records: the caller fills record
# 1 (Julia's order), block b is correlated with record b and its update writes the next one.  C_NULL weight planes: the unweighted run.
function tracking_run_history!(ctx::Context, desc::SignalDesc, num_blocks::Integer, K::Integer, shifts::Vector{Int32},
                               sampling_frequency_hz::Float64, cfg::LoopConfig, state_dev::Ptr{Cvoid}, history_dev::Ptr{Cvoid},
                               acc_re::Ptr{Cfloat}, acc_im::Ptr{Cfloat}, acc_block_stride::Integer = 0;
                               w_re::Ptr{Float64} = Ptr{Float64}(C_NULL), w_im::Ptr{Float64} = Ptr{Float64}(C_NULL), flags::UInt32 = UInt32(0))
    check(ctx, ccall((:gat_tracking_run_history, libgat), Int32,
                     (Ptr{Cvoid}, Ref{SignalDesc}, Int32, Int32, Int32, Ptr{Int32}, Float64, Ref{LoopConfig}, Ptr{Cvoid}, Ptr{Cvoid},
                      Ptr{Cfloat}, Ptr{Cfloat}, Int64, UInt32, Ptr{Float64}, Ptr{Float64}),
                     ctx.handle, Ref(desc), Int32(num_blocks), Int32(K), Int32(length(shifts)), shifts, sampling_frequency_hz,
                     Ref(cfg), state_dev, history_dev, acc_re, acc_im, Int64(acc_block_stride), flags, w_re, w_im))
end
# struct gat_obs_config (96 bytes)
struct ObsConfig
    struct_size::UInt32
    format::Int32                 # GAT_NAV_LNAV or GAT_NAV_CNAV
    code_length::Int32
    symbol_blocks::Int32          # the monitor's
    code_freq_nominal_hz::Float64 # code_length * 1000
    block_seconds::Float64        # the loop configuration's value
    sampling_freq_hz::Float64     # a whole number
    if_hz::Float64
    block_samples::Int32
    max_frames::Int32             # rows of the decoder's frames per channel
    min_tow_steps::Int32
    epoch_first::Int32            # 0-based history index of epoch 0
    epoch_stride::Int32
    rx_mode::Int32                # GAT_OBS_RX_GIVEN or GAT_OBS_RX_FROM_TX
    rx0_ms::Int32
    travel_ms::Int32
    edge_margin::Float64
    rx0_frac::Float64
end
ObsConfig(format::Integer, code_length::Integer, symbol_blocks::Integer, block_seconds::Real, block_samples::Integer, sampling_freq_hz::Real,
          max_frames::Integer; if_hz::Real = 0.0, min_tow_steps::Integer = 0, epoch_first::Integer = 0, epoch_stride::Integer = 1,
          rx_mode::Integer = GAT_OBS_RX_FROM_TX, rx0_ms::Integer = 0, rx0_frac::Real = 0.0, travel_ms::Integer = 68, edge_margin::Real = 0.1) =
    ObsConfig(UInt32(sizeof(ObsConfig)), Int32(format), Int32(code_length), Int32(symbol_blocks), Float64(code_length) * 1000.0,
              Float64(block_seconds), Float64(sampling_freq_hz), Float64(if_hz), Int32(block_samples), Int32(max_frames), Int32(min_tow_steps),
              Int32(epoch_first), Int32(epoch_stride), Int32(rx_mode), Int32(rx0_ms), Int32(travel_ms), Float64(edge_margin), Float64(rx0_frac))
# struct gat_obs_channel (32 bytes)
struct ObsChannel
    status::Int32
    frame_block::Int32
    tow_frame::Int32
    frame0_ms::Int32
    edge_period::Int64
    edge_fraction::Float64
end
struct ObsPlan
    struct_size::UInt32
    chunk_blocks::Int32
    num_chunks::Int32
    channel_group::Int32
    num_groups::Int32
    lanes::Int32
    rows::Int32
    run_blocks::Int32
    threads::Int32
    lds_bytes::Int32
    chunk_workgroups::Int32
    channel_workgroups::Int32
    scratch_bytes::Int64
end
# Every pointer is a device pointer; every output may be C_NULL but one.  In Julia's order history is [K x (B + 1)], frames
# [max_frames x K], tx_ms .. code_rate_hz [K x E], rx_ms, rx_frac [E], channels [K].  Enqueues only.
function observables!(ctx::Context, history::Ptr{ChannelParams}, mon_channels::Ptr{MonitorChannel}, nav_channels::Ptr{NavChannel},
                      nav_frames::Ptr{NavFrame}, num_blocks::Integer, num_channels::Integer, num_epochs::Integer, cfg::ObsConfig;
                      tx_ms::Ptr{Int32} = Ptr{Int32}(C_NULL), tx_frac::Ptr{Float64} = Ptr{Float64}(C_NULL),
                      rx_ms::Ptr{Int32} = Ptr{Int32}(C_NULL), rx_frac::Ptr{Float64} = Ptr{Float64}(C_NULL),
                      carrier_cycles::Ptr{Int64} = Ptr{Int64}(C_NULL), carrier_frac::Ptr{Float64} = Ptr{Float64}(C_NULL),
                      doppler_hz::Ptr{Float64} = Ptr{Float64}(C_NULL), code_rate_hz::Ptr{Float64} = Ptr{Float64}(C_NULL),
                      channels::Ptr{ObsChannel} = Ptr{ObsChannel}(C_NULL))
    check(ctx, ccall((:gat_observables, libgat), Int32,
                     (Ptr{Cvoid}, Ptr{ChannelParams}, Ptr{MonitorChannel}, Ptr{NavChannel}, Ptr{NavFrame}, Int32, Int32, Int32, Ref{ObsConfig},
                      Ptr{Int32}, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{ObsChannel}),
                     ctx.handle, history, mon_channels, nav_channels, nav_frames, Int32(num_blocks), Int32(num_channels), Int32(num_epochs),
                     Ref(cfg), tx_ms, tx_frac, rx_ms, rx_frac, carrier_cycles, carrier_frac, doppler_hz, code_rate_hz, channels))
end
# the same rule on host memory, the bit-exact reference of the device call: history [K, B + 1], frames [max_frames, K]; returns
# (tx_ms, tx_frac, rx_ms, rx_frac, carrier_cycles, carrier_frac, doppler_hz, code_rate_hz, channels)
function observables_host(history::Matrix{ChannelParams}, mon_channels::Vector{MonitorChannel}, nav_channels::Vector{NavChannel},
                          nav_frames::Matrix{NavFrame}, num_epochs::Integer, cfg::ObsConfig)
    K, B1 = size(history)
    E = Int(num_epochs)
    tx_ms = zeros(Int32, K, E)
    tx_frac = zeros(Float64, K, E)
    rx_ms = zeros(Int32, E)
    rx_frac = zeros(Float64, E)
    cycles = zeros(Int64, K, E)
    carrier_frac = zeros(Float64, K, E)
    doppler = zeros(Float64, K, E)
    code_rate = zeros(Float64, K, E)
    channels = Vector{ObsChannel}(undef, K)
    rc = ccall((:gat_observables_host, libgat), Int32,
               (Ptr{ChannelParams}, Ptr{MonitorChannel}, Ptr{NavChannel}, Ptr{NavFrame}, Int32, Int32, Int32, Ref{ObsConfig},
                Ptr{Int32}, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{ObsChannel}),
               history, mon_channels, nav_channels, nav_frames, Int32(B1 - 1), Int32(K), Int32(E), Ref(cfg), tx_ms, tx_frac, rx_ms, rx_frac,
               cycles, carrier_frac, doppler, code_rate, channels)
    rc == GAT_OK || throw(GatError(rc, "gat_observables_host"))
    tx_ms, tx_frac, rx_ms, rx_frac, cycles, carrier_frac, doppler, code_rate, channels
end
# what observables! would do with a call, without a device
function observables_plan(num_blocks::Integer, num_channels::Integer, num_epochs::Integer, cfg::ObsConfig)
    plan = Ref(ObsPlan(UInt32(sizeof(ObsPlan)), 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0))
    rc = ccall((:gat_observables_plan, libgat), Int32, (Int32, Int32, Int32, Ref{ObsConfig}, Ref{ObsPlan}), Int32(num_blocks),
               Int32(num_channels), Int32(num_epochs), Ref(cfg), plan)
    rc == GAT_OK || throw(GatError(rc, "gat_observables_plan"))
    plan[]
end

# ---- fix integrity: the residual test and fault exclusion on top of the position fix (include/gat.h) ----
const GAT_RAIM_MAX_EXCLUDE = 4
const GAT_RAIM_NOT_CHECKED = Int32(1)
const GAT_RAIM_NO_REDUNDANCY = Int32(2)
const GAT_RAIM_DETECTED = Int32(4)
const GAT_RAIM_EXCLUDED = Int32(8)
const GAT_RAIM_UNRESOLVED = Int32(16)
const GAT_FIX_EXCLUDED = Int32(64)
# struct gat_raim_config (504 bytes): threshold by d = n - 4 in the units of T = sum w v^2; entry 1 (d = 0) is not read
struct RaimConfig
    struct_size::UInt32
    max_exclude::Int32            # rounds, 0 .. 4; 0: detect only
    trial_iter::Int32
    flags::UInt32
    threshold::NTuple{61,Float64}
end
RaimConfig(threshold; max_exclude::Integer = 1, trial_iter::Integer = 8) =
    RaimConfig(UInt32(sizeof(RaimConfig)), Int32(max_exclude), Int32(trial_iter), UInt32(0), NTuple{61,Float64}(Float64.(threshold)))
# struct gat_fix_integrity (64 bytes)
struct FixIntegrity
    status::Int32                 # GAT_RAIM_* bits
    dof::Int32
    num_excluded::Int32
    excluded::NTuple{4,Int32}     # 0-based channels in the order of exclusion, -1 where unused
    reserved::Int32
    stat0::Float64
    threshold0::Float64
    stat::Float64
    threshold::Float64
end
# position_fix! with the residual test and fault exclusion; integrity [E], trial [K x E] (may be C_NULL).  Enqueues only.
function position_fix_raim!(ctx::Context, eph::Ptr{Ephemeris}, tx_ms::Ptr{Int32}, tx_frac::Ptr{Float64}, rx_ms::Ptr{Int32}, rx_frac::Ptr{Float64},
                            num_epochs::Integer, num_channels::Integer, cfg::FixConfig, raim::RaimConfig, fixes::Ptr{Fix},
                            integrity::Ptr{FixIntegrity}; weights::Ptr{Float64} = Ptr{Float64}(C_NULL), sat::Ptr{Float64} = Ptr{Float64}(C_NULL),
                            resid::Ptr{Float64} = Ptr{Float64}(C_NULL), sin_el::Ptr{Float64} = Ptr{Float64}(C_NULL),
                            used::Ptr{UInt8} = Ptr{UInt8}(C_NULL), trial::Ptr{Float64} = Ptr{Float64}(C_NULL))
    check(ctx, ccall((:gat_position_fix_raim, libgat), Int32,
                     (Ptr{Cvoid}, Ptr{Ephemeris}, Ptr{Int32}, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Int32, Int32, Ref{FixConfig},
                      Ref{RaimConfig}, Ptr{Fix}, Ptr{FixIntegrity}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{UInt8}, Ptr{Float64}),
                     ctx.handle, eph, tx_ms, tx_frac, rx_ms, rx_frac, weights, Int32(num_epochs), Int32(num_channels), Ref(cfg), Ref(raim), fixes,
                     integrity, sat, resid, sin_el, used, trial))
end
# the same rule on host memory, the bit-exact reference of the device call: tx_ms, tx_frac [K, E]; returns
# (fixes [E], integrity [E], sat [4, K, E], resid [K, E], sin_el [K, E], used [K, E], trial [K, E])
function position_fix_raim_host(eph::Vector{Ephemeris}, tx_ms::Matrix{Int32}, tx_frac::Matrix{Float64}, rx_ms::Vector{Int32},
                                rx_frac::Vector{Float64}, raim::RaimConfig; weights::Union{Nothing,Matrix{Float64}} = nothing,
                                cfg::FixConfig = FixConfig())
    K, E = size(tx_ms)
    fixes = Vector{Fix}(undef, E)
    integrity = Vector{FixIntegrity}(undef, E)
    sat = zeros(Float64, 4, K, E)
    resid = zeros(Float64, K, E)
    sin_el = zeros(Float64, K, E)
    used = zeros(UInt8, K, E)
    trial = zeros(Float64, K, E)
    rc = ccall((:gat_position_fix_raim_host, libgat), Int32,
               (Ptr{Ephemeris}, Ptr{Int32}, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Int32, Int32, Ref{FixConfig}, Ref{RaimConfig},
                Ptr{Fix}, Ptr{FixIntegrity}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{UInt8}, Ptr{Float64}),
               eph, tx_ms, tx_frac, rx_ms, rx_frac, weights === nothing ? Ptr{Float64}(C_NULL) : pointer(weights), Int32(E), Int32(K), Ref(cfg),
               Ref(raim), fixes, integrity, sat, resid, sin_el, used, trial)
    rc == GAT_OK || throw(GatError(rc, "gat_position_fix_raim_host"))
    fixes, integrity, sat, resid, sin_el, used, trial
end
# what position_fix_raim! would do with a call, without a device
function position_fix_raim_plan(num_epochs::Integer, num_channels::Integer, raim::RaimConfig, cfg::FixConfig = FixConfig())
    plan = Ref(FixPlan(UInt32(sizeof(FixPlan)), 0, 0, 0, 0, 0, 0))
    rc = ccall((:gat_position_fix_raim_plan, libgat), Int32, (Int32, Int32, Ref{FixConfig}, Ref{RaimConfig}, Ref{FixPlan}), Int32(num_epochs),
               Int32(num_channels), Ref(cfg), Ref(raim), plan)
    rc == GAT_OK || throw(GatError(rc, "gat_position_fix_raim_plan"))
    plan[]
end

# ---- velocity fix: satellite velocities, the Doppler solver and the local frame (include/gat.h) ----
const GAT_VEL_FEW_SATS = Int32(1)
const GAT_VEL_SINGULAR = Int32(2)
const GAT_VEL_NONFINITE = Int32(4)
const GAT_VEL_NO_FIX = Int32(8)
const GAT_VEL_NO_GEODETIC = Int32(16)
# struct gat_vel_config (16 bytes)
struct VelConfig
    struct_size::UInt32
    flags::UInt32
    carrier_hz::Float64
end
VelConfig(; carrier_hz::Real = 1575.42e6) = VelConfig(UInt32(sizeof(VelConfig)), UInt32(0), Float64(carrier_hz))
# struct gat_velocity (120 bytes)
struct Velocity
    status::Int32                 # GAT_VEL_* bits
    num_valid::Int32
    num_used::Int32
    reserved::Int32
    vx::Float64                   # ECEF, m/s
    vy::Float64
    vz::Float64
    clock_drift::Float64          # s/s
    rms_residual_mps::Float64
    ve::Float64                   # east, north, up, m/s
    vn::Float64
    vu::Float64
    sin_lat::Float64              # geodetic, WGS-84
    cos_lat::Float64
    sin_lon::Float64
    cos_lon::Float64
    height_m::Float64
end
# the velocity of every epoch from its Doppler and its fix; doppler_hz [K x E], fixes and velocities [E]; used, weights, sat_vel
# [4 x K x E] and resid [K x E] may be C_NULL.  Enqueues only.
function velocity_fix!(ctx::Context, eph::Ptr{Ephemeris}, tx_ms::Ptr{Int32}, tx_frac::Ptr{Float64}, doppler_hz::Ptr{Float64}, fixes::Ptr{Fix},
                       num_epochs::Integer, num_channels::Integer, velocities::Ptr{Velocity}; cfg::VelConfig = VelConfig(),
                       used::Ptr{UInt8} = Ptr{UInt8}(C_NULL), weights::Ptr{Float64} = Ptr{Float64}(C_NULL),
                       sat_vel::Ptr{Float64} = Ptr{Float64}(C_NULL), resid::Ptr{Float64} = Ptr{Float64}(C_NULL))
    check(ctx, ccall((:gat_velocity_fix, libgat), Int32,
                     (Ptr{Cvoid}, Ptr{Ephemeris}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Fix}, Ptr{UInt8}, Ptr{Float64}, Int32, Int32,
                      Ref{VelConfig}, Ptr{Velocity}, Ptr{Float64}, Ptr{Float64}),
                     ctx.handle, eph, tx_ms, tx_frac, doppler_hz, fixes, used, weights, Int32(num_epochs), Int32(num_channels), Ref(cfg),
                     velocities, sat_vel, resid))
end
# the same rule on host memory, the bit-exact reference of the device call: tx_ms, tx_frac, doppler_hz [K, E]; returns
# (velocities [E], sat_vel [4, K, E], resid [K, E])
function velocity_fix_host(eph::Vector{Ephemeris}, tx_ms::Matrix{Int32}, tx_frac::Matrix{Float64}, doppler_hz::Matrix{Float64},
                           fixes::Vector{Fix}; used::Union{Nothing,Matrix{UInt8}} = nothing,
                           weights::Union{Nothing,Matrix{Float64}} = nothing, cfg::VelConfig = VelConfig())
    K, E = size(tx_ms)
    velocities = Vector{Velocity}(undef, E)
    sat_vel = zeros(Float64, 4, K, E)
    resid = zeros(Float64, K, E)
    rc = ccall((:gat_velocity_fix_host, libgat), Int32,
               (Ptr{Ephemeris}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Fix}, Ptr{UInt8}, Ptr{Float64}, Int32, Int32, Ref{VelConfig},
                Ptr{Velocity}, Ptr{Float64}, Ptr{Float64}),
               eph, tx_ms, tx_frac, doppler_hz, fixes, used === nothing ? Ptr{UInt8}(C_NULL) : pointer(used),
               weights === nothing ? Ptr{Float64}(C_NULL) : pointer(weights), Int32(E), Int32(K), Ref(cfg), velocities, sat_vel, resid)
    rc == GAT_OK || throw(GatError(rc, "gat_velocity_fix_host"))
    velocities, sat_vel, resid
end
# what velocity_fix! would do with a call, without a device
function velocity_fix_plan(num_epochs::Integer, num_channels::Integer, cfg::VelConfig = VelConfig())
    plan = Ref(FixPlan(UInt32(sizeof(FixPlan)), 0, 0, 0, 0, 0, 0))
    rc = ccall((:gat_velocity_fix_plan, libgat), Int32, (Int32, Int32, Ref{VelConfig}, Ref{FixPlan}), Int32(num_epochs), Int32(num_channels),
               Ref(cfg), plan)
    rc == GAT_OK || throw(GatError(rc, "gat_velocity_fix_plan"))
    plan[]
end

# ---- atmosphere: Klobuchar and troposphere delays, corrected transmit times, subframe 4 page 18 (include/gat.h) ----
const GAT_ATM_IONO = UInt32(1)
const GAT_ATM_TROPO = UInt32(2)
const GAT_ATM_NO_FIX = Int32(1)
const GAT_ATM_NO_GEODETIC = Int32(2)
const GAT_ATM_CH_CORRECTED = UInt8(1)
const GAT_ATM_CH_LOW = UInt8(2)
const GAT_ATM_CH_NONFINITE = UInt8(4)
# struct gat_atm_config (104 bytes)
struct AtmConfig
    struct_size::UInt32
    flags::UInt32                 # GAT_ATM_IONO | GAT_ATM_TROPO
    carrier_hz::Float64
    floor_sin::Float64
    alpha::NTuple{4,Float64}      # Klobuchar: s, s/sc, s/sc^2, s/sc^3
    beta::NTuple{4,Float64}
    zenith_dry_m::Float64         # where zenith is C_NULL / nothing
    zenith_wet_m::Float64
end
AtmConfig(; flags::Integer = GAT_ATM_IONO | GAT_ATM_TROPO, carrier_hz::Real = 1575.42e6, floor_sin::Real = 0.0, alpha = (0.0, 0.0, 0.0, 0.0),
          beta = (0.0, 0.0, 0.0, 0.0), zenith_dry_m::Real = 0.0, zenith_wet_m::Real = 0.0) =
    AtmConfig(UInt32(sizeof(AtmConfig)), UInt32(flags), Float64(carrier_hz), Float64(floor_sin), NTuple{4,Float64}(Float64.(alpha)),
              NTuple{4,Float64}(Float64.(beta)), Float64(zenith_dry_m), Float64(zenith_wet_m))
# struct gat_lnav_page18 (120 bytes)
struct Page18
    valid::Int32
    data_id::Int32
    sv_id::Int32
    wnt::Int32
    dt_ls::Int32
    wnlsf::Int32
    dn::Int32
    dt_lsf::Int32
    alpha::NTuple{4,Float64}
    beta::NTuple{4,Float64}
    a0::Float64
    a1::Float64
    tot::Float64
end
# the delays of every (epoch, channel) at the fixes and the corrected transmit-time fractions; tx_frac_out [K x E]; zenith [2 x E],
# delay [2 x K x E], geom [3 x K x E], channel_status [K x E] and epoch_status [E] may be C_NULL.  Enqueues only.
function range_corrections!(ctx::Context, eph::Ptr{Ephemeris}, tx_ms::Ptr{Int32}, tx_frac::Ptr{Float64}, rx_ms::Ptr{Int32}, rx_frac::Ptr{Float64},
                            fixes::Ptr{Fix}, num_epochs::Integer, num_channels::Integer, tx_frac_out::Ptr{Float64}; cfg::AtmConfig = AtmConfig(),
                            zenith::Ptr{Float64} = Ptr{Float64}(C_NULL), delay::Ptr{Float64} = Ptr{Float64}(C_NULL),
                            geom::Ptr{Float64} = Ptr{Float64}(C_NULL), channel_status::Ptr{UInt8} = Ptr{UInt8}(C_NULL),
                            epoch_status::Ptr{Int32} = Ptr{Int32}(C_NULL))
    check(ctx, ccall((:gat_range_corrections, libgat), Int32,
                     (Ptr{Cvoid}, Ptr{Ephemeris}, Ptr{Int32}, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}, Ptr{Fix}, Ptr{Float64}, Int32, Int32,
                      Ref{AtmConfig}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{UInt8}, Ptr{Int32}),
                     ctx.handle, eph, tx_ms, tx_frac, rx_ms, rx_frac, fixes, zenith, Int32(num_epochs), Int32(num_channels), Ref(cfg),
                     tx_frac_out, delay, geom, channel_status, epoch_status))
end
# the same rule on host memory, the bit-exact reference of the device call: tx_ms, tx_frac [K, E]; returns (tx_frac_out [K, E],
# delay [2, K, E], geom [3, K, E], channel_status [K, E], epoch_status [E])
function range_corrections_host(eph::Vector{Ephemeris}, tx_ms::Matrix{Int32}, tx_frac::Matrix{Float64}, rx_ms::Vector{Int32},
                                rx_frac::Vector{Float64}, fixes::Vector{Fix}; zenith::Union{Nothing,Matrix{Float64}} = nothing,
                                cfg::AtmConfig = AtmConfig())
    K, E = size(tx_ms)
    tx_frac_out = zeros(Float64, K, E)
    delay = zeros(Float64, 2, K, E)
    geom = zeros(Float64, 3, K, E)
    channel_status = zeros(UInt8, K, E)
    epoch_status = zeros(Int32, E)
    rc = ccall((:gat_range_corrections_host, libgat), Int32,
               (Ptr{Ephemeris}, Ptr{Int32}, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}, Ptr{Fix}, Ptr{Float64}, Int32, Int32, Ref{AtmConfig},
                Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{UInt8}, Ptr{Int32}),
               eph, tx_ms, tx_frac, rx_ms, rx_frac, fixes, zenith === nothing ? Ptr{Float64}(C_NULL) : pointer(zenith), Int32(E), Int32(K),
               Ref(cfg), tx_frac_out, delay, geom, channel_status, epoch_status)
    rc == GAT_OK || throw(GatError(rc, "gat_range_corrections_host"))
    tx_frac_out, delay, geom, channel_status, epoch_status
end
# what range_corrections! would do with a call, without a device
function range_corrections_plan(num_epochs::Integer, num_channels::Integer, cfg::AtmConfig = AtmConfig())
    plan = Ref(FixPlan(UInt32(sizeof(FixPlan)), 0, 0, 0, 0, 0, 0))
    rc = ccall((:gat_range_corrections_plan, libgat), Int32, (Int32, Int32, Ref{AtmConfig}, Ref{FixPlan}), Int32(num_epochs),
               Int32(num_channels), Ref(cfg), plan)
    rc == GAT_OK || throw(GatError(rc, "gat_range_corrections_plan"))
    plan[]
end
# the rule's arctangent of every pair
function atm_atan2(y::Vector{Float64}, x::Vector{Float64})
    angle = zeros(Float64, length(y))
    rc = ccall((:gat_atm_atan2_host, libgat), Int32, (Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Float64}), y, x, Int64(length(y)), angle)
    rc == GAT_OK || throw(GatError(rc, "gat_atm_atan2_host"))
    angle
end
# subframe 4, page 18 from one channel's frame records (nav_decode_host's frames[:, k]); valid = 0 where there is none
function lnav_page18(frames::Vector{NavFrame})
    page = Ref{Page18}()
    rc = ccall((:gat_lnav_page18_host, libgat), Int32, (Ptr{NavFrame}, Int32, Ref{Page18}), frames, Int32(length(frames)), page)
    rc == GAT_OK || throw(GatError(rc, "gat_lnav_page18_host"))
    page[]
end
# the inverse: the page's 190 payload bits
function lnav_page18_words(page::Page18)
    bits = zeros(UInt8, 190)
    rc = ccall((:gat_lnav_page18_words_host, libgat), Int32, (Ref{Page18}, Ptr{UInt8}), Ref(page), bits)
    rc == GAT_OK || throw(GatError(rc, "gat_lnav_page18_words_host"))
    bits
end

# ---- carrier smoothing: cycle-slip arcs and Hatch-filtered transmit times (include/gat.h) ----
const GAT_MAX_SMOOTH_EPOCHS = 1048576
const GAT_SMOOTH_RATE_TEST = UInt32(1)
const GAT_SMOOTH_MEASURED = UInt8(1)
const GAT_SMOOTH_GAP = UInt8(2)
const GAT_SMOOTH_CMC = UInt8(4)
const GAT_SMOOTH_RATE = UInt8(8)
# struct gat_smooth_config (56 bytes)
struct SmoothConfig
    struct_size::UInt32
    flags::UInt32                 # GAT_SMOOTH_RATE_TEST
    window::Int32                 # W, 1 .. 65536 epochs
    reserved::Int32
    carrier_hz::Float64
    if_hz::Float64                # the observables'
    epoch_seconds::Float64        # epoch_stride * block_seconds
    cmc_gate_s::Float64           # 0 < g <= 2^-18 s
    rate_gate_cycles::Float64     # > 0 with GAT_SMOOTH_RATE_TEST
end
SmoothConfig(; window::Integer, epoch_seconds::Real, if_hz::Real = 0.0, cmc_gate_s::Real = 15.0 / 299792458.0,
             rate_gate_cycles::Union{Nothing,Real} = nothing, carrier_hz::Real = 1575.42e6,
             flags::Integer = rate_gate_cycles === nothing ? 0 : GAT_SMOOTH_RATE_TEST) =
    SmoothConfig(UInt32(sizeof(SmoothConfig)), UInt32(flags), Int32(window), Int32(0), Float64(carrier_hz), Float64(if_hz), Float64(epoch_seconds),
                 Float64(cmc_gate_s), rate_gate_cycles === nothing ? 0.0 : Float64(rate_gate_cycles))
# struct gat_smooth_channel (16 bytes)
struct SmoothChannel
    measured::Int32
    arcs::Int32
    cmc_resets::Int32
    rate_resets::Int32
end
# struct gat_smooth_plan (56 bytes)
struct SmoothPlan
    struct_size::UInt32
    chunk_epochs::Int32
    num_chunks::Int32
    lanes::Int32
    rows::Int32
    run_epochs::Int32
    threads::Int32
    lds_bytes::Int32
    chunk_workgroups::Int32
    channel_workgroups::Int32
    output_workgroups::Int32
    reserved::Int32
    scratch_bytes::Int64
end
# the observables' transmit-time fractions smoothed by their carrier phase; tx_ms, tx_frac, carrier_cycles, carrier_frac, tx_frac_out
# [K x E], rx_ms, rx_frac [E]; doppler_hz and valid [K x E], count, cmc_s, status [K x E] and channels [K] may be C_NULL.  Enqueues only.
function smooth_observables!(ctx::Context, tx_ms::Ptr{Int32}, tx_frac::Ptr{Float64}, rx_ms::Ptr{Int32}, rx_frac::Ptr{Float64},
                             carrier_cycles::Ptr{Int64}, carrier_frac::Ptr{Float64}, num_epochs::Integer, num_channels::Integer,
                             cfg::SmoothConfig, tx_frac_out::Ptr{Float64}; doppler_hz::Ptr{Float64} = Ptr{Float64}(C_NULL),
                             valid::Ptr{UInt8} = Ptr{UInt8}(C_NULL), count::Ptr{Int32} = Ptr{Int32}(C_NULL),
                             cmc_s::Ptr{Float64} = Ptr{Float64}(C_NULL), status::Ptr{UInt8} = Ptr{UInt8}(C_NULL),
                             channels::Ptr{SmoothChannel} = Ptr{SmoothChannel}(C_NULL))
    check(ctx, ccall((:gat_smooth_observables, libgat), Int32,
                     (Ptr{Cvoid}, Ptr{Int32}, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{UInt8}, Int32, Int32,
                      Ref{SmoothConfig}, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}, Ptr{UInt8}, Ptr{SmoothChannel}),
                     ctx.handle, tx_ms, tx_frac, rx_ms, rx_frac, carrier_cycles, carrier_frac, doppler_hz, valid, Int32(num_epochs),
                     Int32(num_channels), Ref(cfg), tx_frac_out, count, cmc_s, status, channels))
end
# the same rule on host memory, the bit-exact reference of the device call: returns (tx_frac_out, count, cmc_s, status [K, E], channels [K])
function smooth_observables_host(tx_ms::Matrix{Int32}, tx_frac::Matrix{Float64}, rx_ms::Vector{Int32}, rx_frac::Vector{Float64},
                                 carrier_cycles::Matrix{Int64}, carrier_frac::Matrix{Float64}, cfg::SmoothConfig;
                                 doppler_hz::Union{Nothing,Matrix{Float64}} = nothing, valid::Union{Nothing,Matrix{UInt8}} = nothing)
    K, E = size(tx_ms)
    tx_frac_out = zeros(Float64, K, E)
    count = zeros(Int32, K, E)
    cmc_s = zeros(Float64, K, E)
    status = zeros(UInt8, K, E)
    channels = Vector{SmoothChannel}(undef, K)
    rc = ccall((:gat_smooth_observables_host, libgat), Int32,
               (Ptr{Int32}, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{UInt8}, Int32, Int32,
                Ref{SmoothConfig}, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}, Ptr{UInt8}, Ptr{SmoothChannel}),
               tx_ms, tx_frac, rx_ms, rx_frac, carrier_cycles, carrier_frac, doppler_hz === nothing ? Ptr{Float64}(C_NULL) : pointer(doppler_hz),
               valid === nothing ? Ptr{UInt8}(C_NULL) : pointer(valid), Int32(E), Int32(K), Ref(cfg), tx_frac_out, count, cmc_s, status, channels)
    rc == GAT_OK || throw(GatError(rc, "gat_smooth_observables_host"))
    tx_frac_out, count, cmc_s, status, channels
end
# what smooth_observables! would do with a call, without a device
function smooth_observables_plan(num_epochs::Integer, num_channels::Integer, cfg::SmoothConfig)
    plan = Ref(SmoothPlan(UInt32(sizeof(SmoothPlan)), 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0))
    rc = ccall((:gat_smooth_observables_plan, libgat), Int32, (Int32, Int32, Ref{SmoothConfig}, Ref{SmoothPlan}), Int32(num_epochs),
               Int32(num_channels), Ref(cfg), plan)
    rc == GAT_OK || throw(GatError(rc, "gat_smooth_observables_plan"))
    plan[]
end

# ---- snapshot fix: a coarse-time position from code phases alone (include/gat.h) ----
const GAT_SNAP_FEW_SATS = Int32(1)
const GAT_SNAP_SINGULAR = Int32(2)
const GAT_SNAP_NONFINITE = Int32(4)
const GAT_SNAP_NOT_CONVERGED = Int32(8)
const GAT_SNAP_MASK_STARVED = Int32(16)
const GAT_SNAP_MASKED = Int32(32)
const GAT_SNAP_AMBIGUOUS = Int32(64)
const GAT_SNAP_RERESOLVED = Int32(128)
# struct gat_snap_config (64 bytes)
struct SnapConfig
    struct_size::UInt32
    max_iter::Int32
    tol_m::Float64
    mask_sin::Float64
    init_xyz::NTuple{3,Float64}
    ambiguity_margin::Float64
    flags::UInt32
    reserved::UInt32
end
SnapConfig(; max_iter::Integer = 10, tol_m::Real = 1e-4, mask_sin::Real = -1.0, init_xyz = (0.0, 0.0, 0.0), ambiguity_margin::Real = 0.1) =
    SnapConfig(UInt32(sizeof(SnapConfig)), Int32(max_iter), Float64(tol_m), Float64(mask_sin), Float64.(Tuple(init_xyz)), Float64(ambiguity_margin),
               UInt32(0), UInt32(0))
# struct gat_snap_fix (96 bytes)
struct SnapFix
    status::Int32                 # GAT_SNAP_* bits
    num_valid::Int32
    num_used::Int32
    iterations::Int32
    x::Float64                    # ECEF at reception, m
    y::Float64
    z::Float64
    clock_bias_s::Float64
    coarse_time_s::Float64
    rms_residual_m::Float64
    last_step_m::Float64
    gdop::Float64
    pdop::Float64
    tdop::Float64                 # s / m
end
# the position, clock bias and coarse-time error of every epoch from the fractions of its transmit times; code_frac [K x E], rx_ms,
# rx_frac, fixes [E]; prior_xyz [3 x E], weights, tx_ms, n_ms, resid, sin_el, used [K x E] and rx_ms_out [E] may be C_NULL.  Enqueues only.
function snapshot_fix!(ctx::Context, eph::Ptr{Ephemeris}, code_frac::Ptr{Float64}, rx_ms::Ptr{Int32}, rx_frac::Ptr{Float64},
                       num_epochs::Integer, num_channels::Integer, cfg::SnapConfig, fixes::Ptr{SnapFix};
                       prior_xyz::Ptr{Float64} = Ptr{Float64}(C_NULL), weights::Ptr{Float64} = Ptr{Float64}(C_NULL),
                       tx_ms::Ptr{Int32} = Ptr{Int32}(C_NULL), rx_ms_out::Ptr{Int32} = Ptr{Int32}(C_NULL), n_ms::Ptr{Int32} = Ptr{Int32}(C_NULL),
                       resid::Ptr{Float64} = Ptr{Float64}(C_NULL), sin_el::Ptr{Float64} = Ptr{Float64}(C_NULL),
                       used::Ptr{UInt8} = Ptr{UInt8}(C_NULL))
    check(ctx, ccall((:gat_snapshot_fix, libgat), Int32,
                     (Ptr{Cvoid}, Ptr{Ephemeris}, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int32, Int32, Ref{SnapConfig},
                      Ptr{SnapFix}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{UInt8}),
                     ctx.handle, eph, code_frac, rx_ms, rx_frac, prior_xyz, weights, Int32(num_epochs), Int32(num_channels), Ref(cfg), fixes, tx_ms,
                     rx_ms_out, n_ms, resid, sin_el, used))
end
# the same rule on host memory, the bit-exact reference of the device call: code_frac [K, E]; returns
# (fixes [E], tx_ms [K, E], rx_ms_out [E], n_ms [K, E], resid [K, E], sin_el [K, E], used [K, E])
function snapshot_fix_host(eph::Vector{Ephemeris}, code_frac::Matrix{Float64}, rx_ms::Vector{Int32}, rx_frac::Vector{Float64};
                           prior_xyz::Union{Nothing,Matrix{Float64}} = nothing, weights::Union{Nothing,Matrix{Float64}} = nothing,
                           cfg::SnapConfig = SnapConfig())
    K, E = size(code_frac)
    fixes = Vector{SnapFix}(undef, E)
    tx_ms = zeros(Int32, K, E)
    rx_ms_out = zeros(Int32, E)
    n_ms = zeros(Int32, K, E)
    resid = zeros(Float64, K, E)
    sin_el = zeros(Float64, K, E)
    used = zeros(UInt8, K, E)
    rc = ccall((:gat_snapshot_fix_host, libgat), Int32,
               (Ptr{Ephemeris}, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int32, Int32, Ref{SnapConfig}, Ptr{SnapFix},
                Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{UInt8}),
               eph, code_frac, rx_ms, rx_frac, prior_xyz === nothing ? Ptr{Float64}(C_NULL) : pointer(prior_xyz),
               weights === nothing ? Ptr{Float64}(C_NULL) : pointer(weights), Int32(E), Int32(K), Ref(cfg), fixes, tx_ms, rx_ms_out, n_ms, resid,
               sin_el, used)
    rc == GAT_OK || throw(GatError(rc, "gat_snapshot_fix_host"))
    fixes, tx_ms, rx_ms_out, n_ms, resid, sin_el, used
end
# what snapshot_fix! would do with a call, without a device
function snapshot_fix_plan(num_epochs::Integer, num_channels::Integer, cfg::SnapConfig = SnapConfig())
    plan = Ref(FixPlan(UInt32(sizeof(FixPlan)), 0, 0, 0, 0, 0, 0))
    rc = ccall((:gat_snapshot_fix_plan, libgat), Int32, (Int32, Int32, Ref{SnapConfig}, Ref{FixPlan}), Int32(num_epochs), Int32(num_channels),
               Ref(cfg), plan)
    rc == GAT_OK || throw(GatError(rc, "gat_snapshot_fix_plan"))
    plan[]
end

end # module
