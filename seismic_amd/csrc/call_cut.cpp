// call_cut.cpp — the cut of an entry-point call into launches (call_cut.hpp). Host code: no HIP, no lanes, no allocation.
#include "call_cut.hpp"

#include <algorithm>
#include <cstdlib>

namespace sgpu {

static uint32_t env_number(const char* name, uint32_t unset) {
  const char* v = std::getenv(name);
  return v && *v ? (uint32_t)std::strtoul(v, nullptr, 10) : unset;
}

const CutKnobs& cut_knobs() {
  static const CutKnobs knobs = [] {
    CutKnobs k;
    k.chunk_min = env_number("SGPU_CHUNK_MIN", kCutByRule);
    k.chunk_max = std::min(env_number("SGPU_CHUNK_MAX", 0u), 8u);
    k.first_pm = test_hooks_on() ? env_number("SGPU_CHUNK_FIRST", 0u) : 0u;
    return k;
  }();
  return knobs;
}

CutRule cut_rule(const CutKnobs& knobs, bool shared, bool device_plans) {
  CutRule r;
  // The smallest chunk.
  // (600 since r03: a 1250-query call - one rank's shard of a 10 000-query batch on eight GPUs - takes 1115 us in two
  // chunks against 1260 in one, a 2500-query call 1.94 against 2.35 ms: the host side of a chunk, ~0.3 us per query,
  // hides behind the previous chunk's kernel; chunks of ~300 lose to their launch tails. profiles/r03_chunk_probe.txt)
  // (r06: 1300 where the chunks are planned on the device - a 1250- or 2500-query call is then ONE launch: from two request
  // threads 864 -> 781 us and 1551 -> 1475 us per call, from one thread no difference; profiles/r06_shard_probe_chunk_min.txt)
  r.chunk_min = knobs.chunk_min != kCutByRule ? knobs.chunk_min : (device_plans ? 1300u : 600u);
  // Chunks per call: FOUR when this call is alone on the replica (its host side - validation, plan, staging: ~0.2 us per
  // query - hides behind its own earlier chunks' kernels: 1.44 M queries/s from one request thread against 1.31 / 1.11 M
  // with two / one chunk), TWO when other calls are - or were a moment ago - in flight on it (their kernels hide it, and every extra chunk is a launch
  // tail: 10 000-query calls from two / three request threads 1.670 / 1.683 M queries/s with two chunks against 1.636 /
  // 1.596 M with four - the device-resident rate is 1.685 M; r05, gpurun_out r05y). SGPU_CHUNK_MAX fixes the number.
  // (r06: with the launch plan computed on the device - plan_kernel.hip - a chunk's host side is validation and a copy,
  // ~20 us per 1000 queries: two chunks whoever else is calling - one request thread 1.61 M queries/s against 1.59 / 1.54 M
  // with four / one, two threads 1.71 against 1.69 / 1.68; profiles/r06_entry_point_chunks.txt)
  r.chunk_max = knobs.chunk_max ? knobs.chunk_max : ((shared || device_plans) ? 2u : 4u);
  return r;
}

uint32_t cut_jobs(uint32_t nq, uint32_t chunk_min, uint32_t chunk_max) {
  if (!chunk_min) return 1u;
  chunk_max = std::min(std::max(chunk_max, 1u), 8u);
  const uint32_t by_rule = nq >= 2 * (uint64_t)chunk_min ? std::min<uint32_t>(chunk_max, nq / chunk_min) : 1u;
  const uint32_t by_size = (uint32_t)std::min<uint64_t>(((uint64_t)nq + kChunkQueriesMax - 1) / kChunkQueriesMax, 8u);
  return std::max(by_rule, by_size);
}

uint32_t cut_segment(uint32_t nq, uint32_t chunk_min, uint32_t chunk_max, uint32_t lanes_free, uint32_t first_pm, uint32_t bounds[8][2]) {
  uint32_t n_jobs = cut_jobs(nq, chunk_min, chunk_max);
  if (lanes_free >= 1 && n_jobs > lanes_free) n_jobs = lanes_free;
  if (first_pm == 0 || first_pm >= 1000 || n_jobs < 2) {
    for (uint32_t j = 0; j < n_jobs; ++j) bounds[j][0] = split_at(nq, n_jobs, j), bounds[j][1] = split_at(nq, n_jobs, j + 1);
    return n_jobs;
  }
  const uint32_t first = std::min<uint32_t>(std::max<uint32_t>((uint32_t)((uint64_t)nq * first_pm / 1000), 1u), nq - (n_jobs - 1));
  bounds[0][0] = 0, bounds[0][1] = first;
  for (uint32_t j = 1; j < n_jobs; ++j)
    bounds[j][0] = first + split_at(nq - first, n_jobs - 1, j - 1), bounds[j][1] = first + split_at(nq - first, n_jobs - 1, j);
  return n_jobs;
}

uint32_t call_segments(uint32_t nq) {
  return (uint32_t)std::max<uint64_t>(((uint64_t)nq + 8ull * kChunkQueriesMax - 1) / (8ull * kChunkQueriesMax), 1u);
}

uint32_t cut_call(uint32_t nq, uint32_t chunk_min, uint32_t chunk_max, uint32_t lanes_free, uint32_t first_pm, uint32_t* bounds, uint32_t cap) {
  const uint32_t n_seg = call_segments(nq);
  uint32_t n = 0;
  for (uint32_t s = 0; s < n_seg; ++s) {
    const uint32_t s0 = split_at(nq, n_seg, s), s1 = split_at(nq, n_seg, s + 1);
    uint32_t b[8][2];
    const uint32_t n_jobs = cut_segment(s1 - s0, chunk_min, chunk_max, lanes_free, first_pm, b);
    for (uint32_t j = 0; j < n_jobs; ++j, ++n)
      if (n < cap) bounds[2 * n] = s0 + b[j][0], bounds[2 * n + 1] = s0 + b[j][1];
  }
  return n;
}

void rebase_offsets(const uint64_t* q_off, uint32_t q0, uint32_t q1, uint64_t* out) {
  for (uint32_t q = q0; q <= q1; ++q) out[q - q0] = q_off[q] - q_off[q0];
}

}  // namespace sgpu
