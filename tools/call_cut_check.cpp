// call_cut_check.cpp - the cut of an entry-point call (seismic_amd/csrc/call_cut.cpp) at its edges, as a stand-alone host
// program for the sanitizers: no HIP, no library, call_cut.cpp alone. From the repository root:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -c seismic_amd/csrc/call_cut.cpp -o /tmp/call_cut.o
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all tools/call_cut_check.cpp /tmp/call_cut.o -o /tmp/call_cut_check
//   /tmp/call_cut_check
// Every buffer is a heap allocation of exactly the size the functions may touch, so a write or read past it is reported.
#include <cstdio>
#include <cstdlib>
#include <memory>

#include "../seismic_amd/csrc/call_cut.hpp"

using namespace sgpu;

bool sgpu::test_hooks_on() { return true; }   // (the one symbol call_cut.cpp takes from the rest of the library)

#define CHECK(c)                                                      \
  do {                                                                \
    if (!(c)) {                                                       \
      std::fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #c); \
      std::exit(1);                                                   \
    }                                                                 \
  } while (0)

// cut_segment into a buffer of exactly 8 x 2 words: a contiguous cover of [0, nq) by non-empty chunks (nq > 0)
static uint32_t segment(uint32_t nq, uint32_t chunk_min, uint32_t chunk_max, uint32_t lanes_free, uint32_t first_pm) {
  std::unique_ptr<uint32_t[][2]> b(new uint32_t[8][2]);
  const uint32_t n = cut_segment(nq, chunk_min, chunk_max, lanes_free, first_pm, b.get());
  CHECK(n >= 1 && n <= 8 && b[0][0] == 0 && b[n - 1][1] == nq);
  CHECK(n == cut_jobs(nq, chunk_min, chunk_max) || (lanes_free >= 1 && n == lanes_free));
  for (uint32_t j = 0; j < n; ++j) {
    CHECK(b[j][0] < b[j][1] || nq == 0);   // no chunk is empty: rebase_offsets is never asked for an empty part
    if (j) CHECK(b[j][0] == b[j - 1][1]);
  }
  return n;
}

int main() {
  // ---- cut_segment
  CHECK(segment(0, 600, 4, 8, 0) == 1);
  CHECK(segment(1, 600, 4, 8, 0) == 1);
  CHECK(segment(1, 1, 8, 8, 999) == 1);
  CHECK(segment(8, 1, 8, 8, 0) == 8);          // eight chunks of one query each
  CHECK(segment(8, 1, 8, 8, 999) == 8);        // a first share of 99.9 % still leaves every other chunk a query
  CHECK(segment(8, 1, 99, 0, 1) == 8);         // chunk_max is taken as at most 8, lanes_free 0 caps nothing
  CHECK(segment(8, 1, 0, 8, 0) == 1);          // ... and as at least 1
  CHECK(segment(9, 1, 8, 1, 999) == 1);        // one lane: one launch
  CHECK(segment(10000, 600, 4, 3, 300) == 3);
  CHECK(segment(10000, 0, 4, 8, 300) == 1);    // chunk_min 0: never cut
  CHECK(segment(10000, 1300, 2, 8, 1000) == 2);
  CHECK(segment(8u * kChunkQueriesMax, 1300, 2, 8, 999) == 8);
  CHECK(segment(0xffffffffu, 1, 8, 8, 999) == 8);   // (more than a segment ever holds: the arithmetic is 64-bit)
  CHECK(segment(0xffffffffu, 0xffffffffu, 8, 8, 0) == 8);
  for (uint32_t nq = 1; nq <= 40; ++nq)
    for (uint32_t chunk_min = 1; chunk_min <= 5; ++chunk_min)
      for (uint32_t lanes = 0; lanes <= 9; ++lanes)
        for (uint32_t pm : {0u, 1u, 300u, 999u, 1000u, 5000u}) segment(nq, chunk_min, 8, lanes, pm);

  // ---- call_segments, cut_call
  const uint32_t seg = 8u * kChunkQueriesMax;
  CHECK(call_segments(0) == 1 && call_segments(1) == 1 && call_segments(seg) == 1 && call_segments(seg + 1) == 2);
  CHECK(call_segments(0xffffffffu) == (uint32_t)((0xffffffffull + seg - 1) / seg));
  for (uint32_t nq : {1u, 8u, seg, seg + 1, 2 * seg + 7, 1000003u}) {
    for (uint32_t cap : {0u, 1u, 5u, 64u}) {
      std::unique_ptr<uint32_t[]> b(new uint32_t[2 * cap + (cap ? 0 : 1)]);   // exactly cap launches fit
      const uint32_t n = cut_call(nq, 1300, 2, 8, 0, b.get(), cap);
      CHECK(n >= call_segments(nq) && n <= 8 * call_segments(nq));
      const uint32_t w = n < cap ? n : cap;
      for (uint32_t i = 0; i < w; ++i) {
        CHECK(b[2 * i] < b[2 * i + 1] && b[2 * i + 1] - b[2 * i] <= kChunkQueriesMax);
        CHECK(b[2 * i] == (i ? b[2 * i - 1] : 0u));
      }
      if (w == n) CHECK(b[2 * n - 1] == nq);
    }
  }

  // ---- cut_rule (the knobs given, not read)
  CutKnobs k;
  CHECK(cut_rule(k, false, false).chunk_min == 600 && cut_rule(k, false, false).chunk_max == 4);
  CHECK(cut_rule(k, true, true).chunk_min == 1300 && cut_rule(k, true, false).chunk_max == 2);
  k.chunk_min = 0, k.chunk_max = 8;
  CHECK(cut_rule(k, false, true).chunk_min == 0 && cut_rule(k, false, true).chunk_max == 8);
  CHECK(cut_knobs().chunk_max <= 8);

  // ---- rebase_offsets: exactly q1 - q0 + 1 words written, q_off read in [q0, q1] only
  {
    const uint32_t nq = 8;
    std::unique_ptr<uint64_t[]> q_off(new uint64_t[nq + 1]);
    for (uint32_t q = 0; q <= nq; ++q) q_off[q] = 3ull * q * q;
    for (uint32_t q0 = 0; q0 <= nq; ++q0)
      for (uint32_t q1 = q0; q1 <= nq; ++q1) {   // (q0 == q1: a single zero - the cut itself never asks for it, see segment())
        std::unique_ptr<uint64_t[]> out(new uint64_t[q1 - q0 + 1]);
        rebase_offsets(q_off.get(), q0, q1, out.get());
        CHECK(out[0] == 0);
        for (uint32_t q = q0; q <= q1; ++q) CHECK(out[q - q0] == q_off[q] - q_off[q0]);
      }
  }
  std::puts("call_cut_check ok");
  return 0;
}
