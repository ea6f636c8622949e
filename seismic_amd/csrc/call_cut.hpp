// call_cut.hpp — how an entry-point call (sgpu_batch_search) is cut into launches, as pure functions: the knobs, the rule
// that picks how many chunks and how small, the bounds of every chunk, the segments of a call too large for one round of
// lanes, the offsets of a part rebased to 0. No HIP call, no lane, no allocation, no state beyond the knobs read once;
// call_cut.cpp is host code, abi.cpp (search_segment, batch_search) is its one user in the product, and the test hooks
// sgpu_debug_cut_rule / sgpu_debug_chunk_bounds / sgpu_debug_call_bounds drive it without a device
// (tests/test_entry_chunks_cpu.py, tools/call_cut_check.cpp).
#pragma once
#include <cstdint>

#include "common.hpp"

namespace sgpu {

// SGPU_CHUNK_MIN / SGPU_CHUNK_MAX / SGPU_CHUNK_FIRST, read ONCE per process (cut_knobs: a test starts a child per setting).
constexpr uint32_t kCutByRule = 0xffffffffu;
struct CutKnobs {
  uint32_t chunk_min = kCutByRule;   // SGPU_CHUNK_MIN (0: never cut a call; unset: by the rule)
  uint32_t chunk_max = 0;            // SGPU_CHUNK_MAX, at most 8 (0 or unset: by the rule)
  uint32_t first_pm = 0;             // SGPU_CHUNK_FIRST, a test hook: the first chunk's share of a call in per mille (0: equal chunks)
};
const CutKnobs& cut_knobs();

// The smallest chunk worth a launch of its own and the most chunks of a call (a segment of it).
// shared: other calls are - or were a moment ago - in flight on the replica (call_enter); device_plans: chunks of this call
// would be planned on the device (device_plan_dots).
struct CutRule {
  uint32_t chunk_min, chunk_max;
};
CutRule cut_rule(const CutKnobs& knobs, bool shared, bool device_plans);

// i-th of the `parts` boundaries that cut n queries evenly: part i is [split_at(n, parts, i), split_at(n, parts, i + 1)).
// The shards of a batch, the segments of a call and the equal chunks of a segment are all cut like this.
inline uint32_t split_at(uint32_t n, uint32_t parts, uint32_t i) { return (uint32_t)((uint64_t)n * i / parts); }

// The launches wanted for nq queries before lanes are taken (chunk_max is taken as 1 ... 8) - never fewer than it takes to
// keep every chunk within kChunkQueriesMax (what a lane's arena and a launch plan are sized for), up to the eight lanes of
// a replica.
uint32_t cut_jobs(uint32_t nq, uint32_t chunk_min, uint32_t chunk_max);

// The cut of one segment of nq queries: cut_jobs, at most lanes_free of them (0: as many as wanted), and the queries
// [bounds[j][0], bounds[j][1]) of launch j (first_pm: the first chunk's share in per mille, 0 or >= 1000 = equal chunks; the
// others share the rest equally). Returns the number of launches, 1 ... 8.
uint32_t cut_segment(uint32_t nq, uint32_t chunk_min, uint32_t chunk_max, uint32_t lanes_free, uint32_t first_pm, uint32_t bounds[8][2]);

// A call of more than 8 x kChunkQueriesMax queries is served in SEGMENTS of at most that many, one after the other
// (segment s of n is [split_at(nq, n, s), split_at(nq, n, s + 1))), each cut by cut_segment: the bound on a chunk then holds
// whatever nq is.
uint32_t call_segments(uint32_t nq);

// Every launch of a call in order, its segments one after the other: bounds[2 * i], bounds[2 * i + 1] = the queries of
// launch i in the call's numbering, at most `cap` launches written. Returns the number there are.
uint32_t cut_call(uint32_t nq, uint32_t chunk_min, uint32_t chunk_max, uint32_t lanes_free, uint32_t first_pm, uint32_t* bounds, uint32_t cap);

// The offsets of queries [q0, q1) of a batch as a batch of their own: out[0 .. q1 - q0], out[0] = 0 (q0 <= q1).
void rebase_offsets(const uint64_t* q_off, uint32_t q0, uint32_t q1, uint64_t* out);

}  // namespace sgpu
