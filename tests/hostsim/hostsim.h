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
    std::atomic<long> violations{0}; // planner invariants broken (each one is printed)
};
extern Counters counters;
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
