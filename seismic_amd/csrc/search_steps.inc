// search_steps.inc - part of search_kernel.inc (included there, inside namespace sgpu; needs search_lds.inc,
// search_replay.inc).
// Holds: named steps of the kernel body - the phase clocks (PhaseClocks, TICK), the serial role's wave priority
// (serial_prio_on / _off) and write_stats.
// Called by: the kernel body only - the clocks and write_stats once per query by the whole workgroup, the priority pair
// by wavefront 0 around its replay or its control role.

// Phase clocks (s_memtime): TICK(i), inside the kernel's query loop, charges the time since the previous TICK to bucket
// i. Only the profiling build (make prof) counts: the clocks cost ~2% and 14 registers. The plain build writes the
// twelve zeros of `prof` with the stats and keeps its one clock read per query (without it every symbol's code changes).
struct PhaseClocks {
  uint32_t prof[12];
  uint64_t tprev;
  SGPU_DEV void start() {
#pragma unroll
    for (int i = 0; i < 12; ++i) prof[i] = 0;
    tprev = clock64();
  }
  SGPU_DEV void tick(int i) {
#ifdef SGPU_PROF
    const uint64_t t_ = clock64();
    prof[i] += (uint32_t)((t_ - tprev) >> 4);
    tprev = t_;
#endif
  }
};
#define TICK(i) clk.tick(i)

// The serial stretch of a workgroup - wavefront 0's replay while the others wait at the barrier, or its control role in
// the stream - issues ahead of the scoring wavefronts on its SIMD.
SGPU_DEV void serial_prio_on() {
#if SGPU_REPLAY_PRIO
  __builtin_amdgcn_s_setprio(SGPU_REPLAY_PRIO);
#endif
}
SGPU_DEV void serial_prio_off() {
#if SGPU_REPLAY_PRIO
  __builtin_amdgcn_s_setprio(0);
#endif
}

// Work counters of the query (see DESIGN.md "Algorithmic bytes"): [0] blocks of the chosen lists, [1] matched rows,
// [2] summary entries, [3..6] what the replay counted (wavefront 0's lane-local partial sums, folded here), [7] documents
// scored speculatively (every wavefront adds its own).
SGPU_DEV void write_stats(const Lds& s, const BatchView& qb, uint32_t q, uint32_t nl, uint32_t spec_docs, WorkCount& wc) {
  uint32_t sd = spec_docs;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    sd += __shfl_xor(sd, d);
    wc.blocks += __shfl_xor(wc.blocks, d);
    wc.posts += __shfl_xor(wc.posts, d);
    wc.docs += __shfl_xor(wc.docs, d);
    wc.len += __shfl_xor(wc.len, d);
  }
  uint32_t* os = qb.out_stats + (size_t)q * STATS_WORDS;
  if ((threadIdx.x & 63) == 0) atomicAdd(&os[7], sd);
  if (threadIdx.x == 0) {
    uint32_t nbt = 0;
    for (uint32_t l = 0; l < nl; ++l) nbt += s.sel_nb[l];
    os[0] = nbt;
    os[1] = s.st[ST_ROWS];
    os[2] = s.st[ST_ENTRIES];
    os[3] = wc.blocks;
    os[4] = wc.posts;
    os[5] = wc.docs;
    os[6] = wc.len;
  }
}
