// hostsim.h -- shared between the fake HIP runtime, the fake launchers and the driver (tests/hostsim/).
#pragma once
#include <hip/hip_runtime_api.h>

#include <atomic>
#include <thread>
#include <utility>
#include <vector>

namespace hostsim {
struct Counters {
    std::atomic<long> mallocs{0}, frees{0}, graphs{0}, graph_launches{0};
    std::atomic<long> dc_launches{0}, finalize_launches{0}, tail_launches{0}, mfma_launches{0}, other_launches{0}, resident_starts{0}, resident_calls{0};
    std::atomic<long> acq_grid_launches{0}, acq_split_launches{0};
    std::atomic<long> cov_small_launches{0}, cov_tiled_launches{0}, cov_finish_launches{0}; // the array path (gat_array_api.cpp)
    std::atomic<long> cov_split_launches{0}, cov_multi_unit_launches{0}; // ... with splits > 1; with a workgroup that takes several units
    std::atomic<long> array_weight_launches{0}, beamform_launches{0}, weighted_update_launches{0};
    std::atomic<long> violations{0}; // planner invariants broken (each one is printed)
};
extern Counters counters;
// What the covariance launches of one gat_spatial_covariance call read (main.cpp sets the call's signal and clears the table
// before a call and checks it after): seen[b * N + n] counts how often sample n of block b (of the CALL, whatever batch of
// estimates the launch belongs to) was part of a work unit.
struct CovCover {
    const void *re = nullptr;    // the call's sig->re: a launch's block 0 is (its re - this) / (block_stride * sample bytes)
    long long N = 0, block_stride = 0;
    int B = 0;
    std::vector<unsigned char> seen;
    void reset(const void *re_, int B_, long long N_, long long block_stride_)
    {
        re = re_, B = B_, N = N_, block_stride = block_stride_;
        seen.assign((size_t)B_ * (size_t)N_, 0);
    }
};
extern CovCover cov_cover;
// What the correlator's launches of one call did with the caller's tap list (main.cpp clears it before a call and checks it
// after): (tap_index, shift) of the first cfg.taps / L entries of every vector-kernel and matrix-core launch, and the shift
// lists of the tail launches (in the caller's order).
struct TapCover {
    std::vector<std::pair<int, int>> main;
    std::vector<std::vector<int>> tail;
    void clear() { main.clear(); tail.clear(); }
};
extern TapCover tap_cover;
void attach_worker(hipStream_t s, std::thread &&t); // the emulated resident kernel of a launch on stream s
float resident_value(unsigned seq_independent_slot, int o); // what the emulated workgroup `slot` posts as its sum o
} // namespace hostsim
