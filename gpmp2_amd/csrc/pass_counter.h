// pass_counter.h -- the word through which the workgroups of a pass-closing kernel count themselves in: arrivals in the
// high half, the trajectories that keep iterating in the low half.  Every workgroup adds pass_arrival(continues) with
// ONE atomic add; the value the add returns tells the workgroup whether it arrived last, and the same value carries
// what the others contributed, so the last arriver forms the pass's count without a second location and without
// ordering anything against anything (plan_device.h: publish_pass_count).  Pure functions, no pointer, no thread
// index: a plain host compiler builds the same text for the CPU test (tests/cpp/pass_counter_shim.cpp).
#pragma once
#include <cstdint>

#ifndef G2_PURE
#ifdef __HIPCC__
#define G2_PURE __host__ __device__ __forceinline__
#else
#define G2_PURE inline
#endif
#endif

namespace g2 {

// what a workgroup adds: one arrival and its `continues` (0 or 1; any count below 2^31 a grid can reach)
G2_PURE uint64_t pass_arrival(int continues) { return (uint64_t(1) << 32) + (uint64_t)(uint32_t)continues; }
// `before`: the word as the workgroup's add found it.  The low half never carries into the high one: it is bounded by
// the grid size, an int.
G2_PURE int pass_arrivals_before(uint64_t before) { return (int)(uint32_t)(before >> 32); }
G2_PURE bool pass_arrived_last(uint64_t before, int grid) { return pass_arrivals_before(before) == grid - 1; }
// the pass's count as the last arriver sees it: what the others left plus its own share
G2_PURE int pass_count(uint64_t before, int continues) { return (int)(uint32_t)before + continues; }

}  // namespace g2
