// search_stream.inc - part of search_kernel.inc (included there, inside namespace sgpu; needs search_lds.inc,
// search_score.inc, search_replay.inc).
// Holds: the streamed stage 2 - the ST_S_* state words, the ring (Ring, carve_ring), the scorers (score_stream_class,
// stream_scorer), the replay over the ring (replay_span), the control wavefront (stream_control) and the
// SGPU_STREAM_NCH default.
// Called by: the STREAM variants of the kernel (plain launches), once per list group: wavefront 0 runs stream_control,
// wavefronts 1 .. run stream_scorer; no workgroup barrier inside.

// ---------------------------------------------------------------------------
// stage 2 as a STREAM (r06): one control wavefront (feeder + replayer) and the scoring wavefronts
// ---------------------------------------------------------------------------
// The round loop of stage 2 (the kernel's `while (pos < nb)`, search_kernel.inc; still what the counted and the cooperative
// variants run) is a chain of dependent steps - filter, posting ranges (one trip to HBM), posting refs (a second),
// records (a third), replay - with a workgroup barrier between any two: ~8 barriers and 3 trips per round, 7 - 11
// rounds per query, and while one step runs the wavefronts of the others wait. On the headline collection the
// co-resident workgroup's scoring fills those gaps (the chip sits at the memory system's ceiling either way); on
// MS-MARCO-like work per query (the clustered collection: 1750 documents, 7 rounds of ~300) 60 % of a query's time
// is spent in the chain, not in scoring (profiles/r05_phase_profile_clustered.txt), and the chip at 0.40 of peak.
//
// The streamed variants (template parameter STREAM; plain launches) run the same steps as ROLES that never meet at a
// barrier inside a list group:
//   control   (wavefront 0; stream_control) FEEDS: it walks the group's positions in traversal order, 128 at a time -
//             skip test against the live threshold, posting ranges of the survivors (the loads of the NEXT step in
//             flight while this step's items are produced), posting refs + document ids of up to 384 items at a time -
//             and files every item, in traversal order, into a RING of item slots in LDS and its slot number into the
//             queue of its length class; it runs ahead of the replay by at most `budget` items (the speculation budget
//             of the round loop: doubled while >= 3/4 of the replayed items were live, halved below 1/2). And it
//             REPLAYS - while its posting loads are in flight, and whenever it waits for room: the items IN ORDER, a
//             64-slot window at a time as soon as every item of the window is scored, with the reference's sequential
//             decisions and the live threshold (replay_span = replay_chunk over the ring). The top-k stays in its
//             registers for the whole group.
//   scorers   (wavefronts 1 ..) claim slot numbers from the two queues (a compare-and-swap on the queue's tail),
//             score the documents exactly as phase B does - 16 lanes per document, rotating register slots - store
//             the score into the item's slot and count the item in its 64-slot window.
// Exactness is the round loop's argument unchanged: a block is tested against the threshold after a PREFIX of the
// items that precede it (no item of a block is produced before the block's last test), the threshold only rises, so
// every block the reference evaluates is produced; the replay applies the reference's own test with the live
// threshold and ignores the rest. Scores do not depend on who computes them. A window of the stream can straddle two
// lists, i.e. hold the same document twice: the not-full path dedups inside the window (replay_chunk's `dups` rule),
// the full path by heap membership as always.
// Synchronisation is through LDS words only (queue heads and tails, the windows' counters, DONE): a wavefront's DS
// operations execute in order, so "write the data, then the word that publishes it" needs a compiler barrier, not a
// fence; every wait is bounded and flags the launch (status word; host: SGPU_EDEVICE). Waits sleep (s_sleep), so a
// waiting wavefront leaves its SIMD to the others.
typedef __attribute__((address_space(3))) uint32_t lds_u32_t;
typedef __attribute__((address_space(3))) uint64_t lds_u64_t;
SGPU_DEV uint32_t lds_ld(const uint32_t* p) { return __hip_atomic_load((lds_u32_t*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
SGPU_DEV uint64_t lds_ld64(const uint32_t* p) { return __hip_atomic_load((lds_u64_t*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
SGPU_DEV void lds_st(uint32_t* p, uint32_t v) { __hip_atomic_store((lds_u32_t*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
SGPU_DEV void lds_order() { asm volatile("" ::: "memory"); }   // (compiler barrier: the LDS pipeline itself is in order per wavefront)
// state words of the stream: they live where the round loop keeps its candidate lists (ST_CAND ..), which the
// streamed variants do not use. {tail, head} of a queue are one aligned 64-bit word.
enum { ST_S_THR = 9 /* the threshold the control wavefront last published: -inf while the heap is not full */,
       ST_S_DONE = 10, ST_S_BUDGET = 11, ST_S_QS_TAIL = 12, ST_S_QS_HEAD = 13,
       ST_S_QL_TAIL = 14, ST_S_QL_HEAD = 15, ST_S_ABORT = 16,
       // (profiling build) polls of starved scorers, polls of the blocked feeder, replayed spans, sum of the budget over them
       ST_S_STARVED = 18, ST_S_BLOCKED = 19, ST_S_SPANS = 20, ST_S_BUDGET_SUM = 21, ST_S_SKIPPED = 22 };
constexpr uint32_t kStreamSpinLimit = 1u << 21;   // polls (>= ~0.1 us each) before a wait gives up and flags the launch

struct Ring {
  uint64_t* it_ref;     // [ring] packed record ref; once scored, the high word holds the score
  uint32_t* it_doc;     // [ring] document id
  uint16_t* it_blk;     // [ring] index of the item's block in Lds::dots (group-wide)
  uint16_t* q_short;    // [ring] slot numbers of the items of <= 128 elements, in arrival order
  uint16_t* q_long;     // [ring] ... of the longer ones
  uint32_t* win_done;   // [ring / 64] per 64-slot window: items that have their score | (those of them that beat the published threshold) << 16
  uint32_t* f_incl;     // feeder: [kStreamFeedPos] inclusive item count of the step's blocks
  uint32_t* f_p0;       //         [kStreamFeedPos] first posting
  uint16_t* f_dix;      //         [kStreamFeedPos] dot index
  uint32_t mask;        // ring - 1
};
SGPU_DEV Ring carve_ring(uint8_t* uni, uint32_t ring) {   // (device_types.hpp: stream_ring_bytes)
  Ring r;
  uint8_t* p = uni;
  r.it_ref = (uint64_t*)p;   p += (size_t)ring * 8;
  r.it_doc = (uint32_t*)p;   p += (size_t)ring * 4;
  r.it_blk = (uint16_t*)p;   p += (size_t)ring * 2;
  r.q_short = (uint16_t*)p;  p += (size_t)ring * 2;
  r.q_long = (uint16_t*)p;   p += (size_t)ring * 2;
  r.win_done = (uint32_t*)p; p += (size_t)(ring / 64) * 4;
  r.f_incl = (uint32_t*)p;
  r.f_p0 = r.f_incl + kStreamFeedPos;
  r.f_dix = (uint16_t*)(r.f_p0 + kStreamFeedPos);
  r.mask = ring - 1u;
  return r;
}

// A bounded wait gave up (16: the final replay, 17: the feeder's wait for room, 18: a scorer): every role leaves its loops, the launch's status word
// says so and the host fails the call (device_index.hip: kernel_report).
SGPU_DEV void stream_abort(const Lds& s, const BatchView& qb, uint32_t code) {
  lds_st(&s.st[ST_S_ABORT], code);
  if (qb.status) __hip_atomic_store(qb.status, code, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// ---- scorers ----
// score_class over a queue of the ring: the same slots, loads and arithmetic; items come from claims of at most 4 * ND
// queue positions (compare-and-swap on the tail, by the wavefront's first lane) instead of a counter over a fixed list,
// and every scored item is counted in its window. Returns once a pass of the slots found nothing to claim and every
// slot is empty (the caller looks at both queues again).
template <typename CT, int LK, int ND, int NS, int VT, bool SC>
SGPU_DEV void score_stream_class(const Lds& s, const DevView& ix, const Ring& rg, const uint16_t* queue, uint32_t* tail_head,
                                 uint32_t& spec_docs) {
  constexpr uint32_t len_mask = LenMask<VT>::v;
  const uint32_t sub = threadIdx.x & 15, grp = (threadIdx.x & 63) >> 4;
  const bool first_lane = (threadIdx.x & 63) == 0;
  float* it_score = (float*)rg.it_ref;
  const uint32_t e0 = sub * 8u;
  uint32_t len[ND], item[ND];
  const uint8_t* rec[ND];
  bool rawf[ND];
  DocChunk<CT, VT> d[ND][NS];
  float thr_pub = -__builtin_inff();
  auto issue = [&](int u, uint32_t qpos, bool has) {
    const uint32_t it = has ? (uint32_t)queue[qpos & rg.mask] : 0u;
    const uint64_t ref = rg.it_ref[it];
    item[u] = has ? it : 0xffffffffu;
    len[u] = has ? ((uint32_t)ref & len_mask) : 0u;
    rec[u] = ix.fwd + (has ? (ref >> 16) : 0ull) * 16ull;
    rawf[u] = Vt<VT>::sliced && has && ((uint32_t)ref & kRawBit) != 0;
#pragma unroll
    for (int h = 0; h < NS; ++h) {
      const uint32_t e = e0 + 128u * h;
      const bool act = e < len[u];
      const uint8_t *pc, *pv;
      slice_ptrs<CT, VT>(rec[u], len[u], e >> 3, pc, pv);
      if (Vt<VT>::sliced) {
        const uint8_t *rc, *rv;
        slice_ptrs<CT, Vt<VT>::raw>(rec[u], len[u], e >> 3, rc, rv);
        pc = rawf[u] ? rc : pc;
        pv = rawf[u] ? rv : pv;
        d[u][h].c0 = *(const uint4*)(act ? pc : rec[u]);
        load_values<Vt<VT>::raw>(d[u][h].v, act ? pv : rec[u]);
      } else {
        load_slice<CT, VT>(d[u][h], act ? pc : rec[u], act ? pv : rec[u]);
      }
    }
  };
  auto consume = [&](int u) {
    float a = 0.0f;
#pragma unroll
    for (int h = 0; h < NS; ++h) {
      if (Vt<VT>::sliced) {
        a = score_pass<CT, LK, VT, SC>(s, d[u][h], rawf[u], e0 + 128u * h, len[u], a);
        continue;
      }
      uint32_t c[8];
      slice_components<CT, VT>(d[u][h], c, dvb_bias<LK, VT>(s));
      if (e0 + 128u * h < len[u]) a = accumulate_chunk<CT, LK, VT, SC>(s, d[u][h], c, e0 + 128u * h, len[u], a);
    }
    if (NS > 1) {
      for (uint32_t eb = 128u * NS; eb < len[u]; eb += 128u) {
        const uint32_t e = eb + e0;
        DocChunk<CT, VT> t;
        if (Vt<VT>::sliced) {
          load_pass<CT, VT>(t, rec[u], len[u], rawf[u], e);
          a = score_pass<CT, LK, VT, SC>(s, t, rawf[u], e, len[u], a);
          continue;
        }
        load_chunk<CT, VT>(t, rec[u], len[u], e < len[u] ? e : 0u);
        uint32_t c[8];
        slice_components<CT, VT>(t, c, dvb_bias<LK, VT>(s));
        if (e < len[u]) a = accumulate_chunk<CT, LK, VT, SC>(s, t, c, e, len[u], a);
      }
    }
    a = reduce16(a);
    spec_docs += (sub == 0 && len[u] != 0);
    if (sub == 0 && item[u] != 0xffffffffu) {
      it_score[2 * item[u] + 1] = a;
      lds_order();   // (the score, then the count that lets the control wavefront read it)
      // + 1 item scored; + 1 << 16 if it beats the published threshold (-inf while the heap is not full), which is never
      // above the live one: a window without such an item cannot change a full heap and is not even looked at
      __hip_atomic_fetch_add((lds_u32_t*)&rg.win_done[item[u] >> 6], a > thr_pub ? 0x10001u : 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
  };
  // up to 4 * ND queue positions for this wavefront: {first position, count}; count 0 = nothing there, or the
  // compare-and-swap lost against another wavefront's claim (the caller simply comes back)
  auto claim = [&](uint32_t& base, uint32_t& cnt) {
    uint32_t t = 0, n = 0;
    if (first_lane) {
      const uint64_t w = lds_ld64(tail_head);
      t = (uint32_t)w;
      n = (uint32_t)(w >> 32) - t;
      n = n < 4u * (uint32_t)ND ? n : 4u * (uint32_t)ND;
      if (n) {
        uint32_t expect = t;
        if (!__hip_atomic_compare_exchange_strong((lds_u32_t*)tail_head, &expect, t + n, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                  __HIP_MEMORY_SCOPE_WORKGROUP))
          n = 0;
      }
    }
    base = uniform_u(t);
    cnt = uniform_u(n);
    lds_order();   // (the queue entries and item slots are read after the claim)
  };
  uint32_t base, cnt;
  claim(base, cnt);
  if (cnt == 0) return;
#pragma unroll
  for (int u = 0; u < ND; ++u) issue(u, base + 4u * (uint32_t)u + grp, 4u * (uint32_t)u + grp < cnt);
  for (;;) {
    thr_pub = __uint_as_float(lds_ld(&s.st[ST_S_THR]));   // (a stale value is a lower one: it only flags more)
    claim(base, cnt);   // the batch that refills the slots
    consume(0);
    issue(0, base + grp, grp < cnt);
#pragma unroll
    for (int u = 1; u < ND; ++u) {
      consume(u);
      issue(u, base + 4u * (uint32_t)u + grp, 4u * (uint32_t)u + grp < cnt);
    }
    if (cnt == 0) break;   // every slot was refilled with nothing
  }
}

template <typename CT, int NT, int LK, int VT, bool SC>
SGPU_DEV void stream_scorer_sc(const Lds& s, const DevView& ix, const BatchView& qb, const Ring& rg, uint32_t& spec_docs) {
  constexpr int kShort = sizeof(CT) == 2 ? (Vt<VT>::half ? SGPU_ND_SHORT : SGPU_ND_SHORT_U8) : SGPU_ND_SHORT_U32;
  constexpr int kLong = sizeof(CT) == 2 ? (Vt<VT>::half ? SGPU_ND_LONG : SGPU_ND_LONG_U8) : SGPU_ND_LONG_U32;
  // odd wavefronts prefer the long class, even ones the short one (as in the round loop: score_items_sc); each takes
  // whatever there is when its own class has nothing
  const bool long_first = ((threadIdx.x >> 6) & 1u) != 0;
  uint32_t spins = 0;
#pragma nounroll
  for (;;) {
    const uint32_t dn = uniform_u(lds_ld(&s.st[ST_S_DONE]));   // (before the heads: DONE is stored after the last of them)
    lds_order();
    const uint64_t ws = lds_ld64(&s.st[ST_S_QS_TAIL]), wl = lds_ld64(&s.st[ST_S_QL_TAIL]);
    const bool as = uniform_u((uint32_t)((uint32_t)(ws >> 32) != (uint32_t)ws)) != 0u;
    const bool al = uniform_u((uint32_t)((uint32_t)(wl >> 32) != (uint32_t)wl)) != 0u;
    if (al && (long_first || !as)) {
      score_stream_class<CT, LK, kLong, 2, VT, SC>(s, ix, rg, rg.q_long, &s.st[ST_S_QL_TAIL], spec_docs);
      spins = 0;
      continue;
    }
    if (as) {
      score_stream_class<CT, LK, kShort, 1, VT, SC>(s, ix, rg, rg.q_short, &s.st[ST_S_QS_TAIL], spec_docs);
      spins = 0;
      continue;
    }
    if (dn) break;   // the feeder is through and both queues are drained
    if (uniform_u(lds_ld(&s.st[ST_S_ABORT]))) break;
    if (++spins > kStreamSpinLimit) {
      stream_abort(s, qb, 18u);
      break;
    }
#ifdef SGPU_PROF
    if ((threadIdx.x & 63) == 0) atomicAdd(&s.st[ST_S_STARVED], 1u);
#endif
    __builtin_amdgcn_s_sleep(2);
  }
}
template <typename CT, int NT, int LK, int VT>
SGPU_DEV void stream_scorer(const Lds& s, const DevView& ix, const BatchView& qb, const Ring& rg, uint32_t& spec_docs) {
  if (LK == LK_DENSE && uniform_u(s.st[ST_SCALED]) != 0u) stream_scorer_sc<CT, NT, LK, VT, true>(s, ix, qb, rg, spec_docs);
  else stream_scorer_sc<CT, NT, LK, VT, false>(s, ix, qb, rg, spec_docs);
}

// ---- replayer ----
// replay_chunk (no visited bitmap) over `n` <= 64 consecutive items of the ring, the first at stream position
// `first`: same windows, same rules. `decided_blk` names a block by its dot index (unique across the group's lists).
template <int KR>
SGPU_DEV void replay_span(RegHeap<KR>& heap, const Ring& rg, const float* dots, uint32_t first, uint32_t n, uint32_t k,
                          float heap_factor, uint32_t& decided_blk, uint32_t& live_items) {
  const uint32_t lane = lane_id();
  const uint32_t* it_words = (const uint32_t*)rg.it_ref;   // [2 slot] = low ref word, [2 slot + 1] = score
  uint32_t i = 0;
  while (i < n) {
    const uint32_t idx = i + lane;
    const bool valid = idx < n;
    const uint32_t slot = (first + idx) & rg.mask;
    float sc = 0.0f, bdot = 0.0f;
    uint32_t blk = 0;
    if (valid) {
      sc = __uint_as_float(it_words[2 * slot + 1]);
      blk = rg.it_blk[slot];
      bdot = dots[blk];
    }
    if (heap.len == k && __ballot(valid && sc > heap.thr) == 0ull) {
      // no score of the window exceeds the k-th best, which only rises: nothing here can change the heap
      live_items += (uint32_t)__popcll(__ballot(valid && !(bdot < __fmul_rn(heap_factor, heap.thr))));
      return;
    }
    const uint32_t doc = valid ? rg.it_doc[slot] : 0u;
#ifdef SGPU_STREAM_PRINTF
    if (valid) printf("R seq %u doc %u score %.7g blk %u bdot %.7g hlen %u thr %.7g\n", first + idx, doc, sc, blk, bdot, heap.len, heap.thr);
#endif
    if (heap.len < k) {
      // heap not full: every block that starts now is evaluated, every new document is pushed; visited == in the
      // heap already, or an earlier copy inside this window (a window of the stream can straddle two lists)
      bool vis = !valid;
#pragma unroll
      for (int r = 0; r < KR; ++r) {
        const uint32_t lim = heap.len > (uint32_t)r * 64u ? heap.len - (uint32_t)r * 64u : 0u;
        for (uint32_t l = 0; l < (lim < 64u ? lim : 64u); ++l) vis |= doc == readlane_u(heap.doc[r], l);
      }
      {
        const uint64_t nv0 = __ballot(valid && !vis);
        for (uint32_t l = 0; l < 63; ++l)
          if (((nv0 >> l) & 1ull) && lane > l && doc == readlane_u(doc, l)) vis = true;
      }
      const uint64_t nvm = __ballot(valid && !vis);
      const uint32_t need = k - heap.len;
      const uint32_t before = (uint32_t)__popcll(nvm & ((1ull << lane) - 1ull));
      const bool take = valid && !vis && before < need;
      const uint64_t tm = __ballot(take);
      uint32_t last;   // window position of the last item consumed in this step
      if ((uint32_t)__popcll(nvm) >= need) last = 63u - (uint32_t)__clzll(tm);
      else last = (n - i < 64u ? n - i : 64u) - 1u;
      live_items += last + 1;
      uint64_t m = tm;
      while (m) {
        const int l = __ffsll((long long)m) - 1;
        m &= m - 1;
        heap.insert(readlane_f(sc, (uint32_t)l), readlane_u(doc, (uint32_t)l), k);
      }
      decided_blk = readlane_u(blk, last);
      i += last + 1;
      continue;
    }
    // heap full: the window stays in registers; every heap change re-evaluates the remaining lanes
    uint32_t start = 0;
    for (;;) {
      const float thr = heap.thr;
      const float cut = __fmul_rn(heap_factor, thr);
      const bool live = valid && lane >= start && ((blk == decided_blk) || !(bdot < cut));
      const bool changing = live && (sc > thr);
      uint64_t cm = __ballot(changing);
      while (cm) {   // drop recurring documents: they are in the heap already (proof at replay_chunk)
        const uint32_t c0 = (uint32_t)(__ffsll((long long)cm) - 1);
        if (!heap_contains<KR>(heap, readlane_u(doc, c0))) break;
        cm &= cm - 1;
      }
      const uint32_t f = cm ? (uint32_t)(__ffsll((long long)cm) - 1) : 63u;
      live_items += (uint32_t)__popcll(__ballot(live && lane <= f));
      if (cm == 0) break;
      heap.insert(readlane_f(sc, f), readlane_u(doc, f), k);
      decided_blk = readlane_u(blk, f);
      start = f + 1;
      if (start >= 64) break;
    }
    i += 64;
  }
}

// ---- control wavefront: feeder + replayer ----
// (r06, second form. The first form gave the feeder and the replayer a wavefront each and let them talk through LDS
// words - REPLAYED, BUDGET, THR: bit-identical and 3 - 4 % faster than the round loop, with SIX scoring wavefronts of
// eight. Scoring is what a query's time is made of, so the two serial roles now share ONE wavefront: the replay of
// whatever is scored runs while the feeder's posting loads are in flight, the heap stays in this wavefront's registers
// for the whole group and the skip test reads the live threshold from a register, not a published copy.)
//   * walks the group's positions in traversal order, 128 per step: skip test against the live threshold, posting
//     ranges of the survivors - the loads of the NEXT step are in flight while this step's items are produced;
//   * per batch of at most 384 items: waits for room under the speculation budget (replaying meanwhile), tests the
//     blocks not yet started once more, loads posting refs + document ids, REPLAYS what is scored while they fly,
//     files the items into the ring and their slot numbers into the class queues, publishes the queue heads;
//   * replays the rest once the last item is out.
// (profiling build) where the control wavefront's time goes: busy_ticks[0] replay, [1] skip test + tables + block lookup
// of a batch, [2] posting loads + filing the items, [3] waiting for room, [4] the final replay, [5] skipped windows.
// CTICK(i), inside stream_control: the time since the previous CTICK goes to busy_ticks[i].
#ifdef SGPU_PROF
#define CTICK(i) { const uint64_t t_ = clock64(); busy_ticks[i] += (uint32_t)((t_ - tq) >> 4); tq = t_; }
#else
#define CTICK(i) {}
#endif
template <int KR, int VT>
SGPU_DEV void stream_control(const Lds& s, const DevView& ix, const BatchView& qb, const Ring& rg, const KParams& p,
                             uint32_t l0, uint32_t l1, uint32_t& budget_io, uint32_t* busy_ticks) {
#ifdef SGPU_PROF
  uint64_t tq = clock64();
#endif
  constexpr int R = kStreamFeedPos / 64;   // positions per lane and step
#ifndef SGPU_STREAM_NCH
#define SGPU_STREAM_NCH 6
#endif
  constexpr int NCH = SGPU_STREAM_NCH;     // 64-item chunks whose posting loads are in flight together
  const uint32_t lane = lane_id();
  RegHeap<KR> heap;
  heap.load(s.heap, s.st[ST_HLEN], __uint_as_float(s.st[ST_THR]));
  // The lead never reaches into a window of the ring whose previous items are not all replayed: at most ring - 64 items
  // (a window's counter is shared by its 64 slots, and the replay can stand in the middle of a window).
  const uint32_t ring = rg.mask + 1u, bud_max = ring - 64u;
  uint32_t budget = budget_io < bud_max ? budget_io : bud_max;
  uint32_t next = 0, decided = 0xffffffffu, since_items = 0, since_live = 0;   // replay: items replayed, ...
  uint32_t produced = 0, qs = 0, ql = 0;                                       // feed: items produced, queue heads
  float thr_pub = __uint_as_float(s.st[ST_S_THR]);                             // what the scorers compare with
  bool failed = false;

  // Replays every window whose items - as far as they are produced - all have their score; a window that is not yet
  // full only when `flush` (the feeder needs the room, or is through). A window none of whose items beat the threshold
  // that was published when it was scored cannot change a full heap: it is counted, not read.
  auto replay_ready = [&](bool flush) {
    for (;;) {
      if (next == produced) return;
      const uint32_t w0 = next & ~63u;
      uint32_t* wd = &rg.win_done[(w0 & rg.mask) >> 6];
      const uint32_t cw = uniform_u(lds_ld(wd));
      lds_order();   // (the scores are read after the count that covers them)
      const uint32_t end = produced - w0 < 64u ? produced : w0 + 64u;
      if ((cw & 0xffffu) != end - w0) return;    // an item of the window is still being scored
      if (end != w0 + 64u && !flush) return;
#ifdef SGPU_PROF
      const uint64_t t0 = clock64();
      if (heap.len == p.k && (cw >> 16) == 0u) busy_ticks[5] += 1;
#endif
      uint32_t live = end - next;   // (an unread window counts as live, as the round loop's candidate path does)
      if (!(heap.len == p.k && (cw >> 16) == 0u)) {
        live = 0;
        replay_span<KR>(heap, rg, s.dots, next, end - next, p.k, p.heap_factor, decided, live);
        const float tp = heap.len == p.k ? heap.thr : -__builtin_inff();
        if (__float_as_uint(tp) != __float_as_uint(thr_pub)) {
          thr_pub = tp;
          if (lane == 0) lds_st(&s.st[ST_S_THR], __float_as_uint(tp));
        }
      }
      since_items += end - next;
      since_live += live;
      next = end;
      if ((next & 63u) == 0 && lane == 0) lds_st(wd, 0u);   // the window is through: its counter starts over
      if (since_items >= budget) {   // the round loop's budget rule over a span of `budget` replayed items
        if (since_live * 4 >= since_items * 3) budget = budget * 2 < bud_max ? budget * 2 : bud_max;
        else if (since_live * 2 < since_items) budget = budget / 2 > p.items_min ? budget / 2 : p.items_min;
        budget = budget < bud_max ? budget : bud_max;
        since_items = 0;
        since_live = 0;
      }
#ifdef SGPU_PROF
      {
        const uint64_t t1 = clock64();
        busy_ticks[0] += (uint32_t)((t1 - t0) >> 4);
        tq += t1 - t0;   // (not charged to the bucket the call sits in)
      }
      if (lane == 0) {
        s.st[ST_S_SPANS] += 1;
        s.st[ST_S_BUDGET_SUM] += budget;
      }
#endif
    }
  };

  const uint32_t ng = l1 - l0;
  const uint32_t total_pos = uniform_u(s.sel_doff[l1]);   // the group's dots start at 0 (plan_list_group)
  const bool sorted0 = l0 == 0 && p.first_sorted && s.sel_nb[0] > 1;
  const uint32_t my_doff = lane < ng ? s.sel_doff[l0 + lane] : 0xffffffffu;   // lane j: first position of list l0 + j
  const uint64_t below = (1ull << lane) - 1ull;
  struct Step {
    uint32_t p0[R], p1[R], dix[R];
    float dot[R];
    bool live[R];
  };
  // skip test + posting range of positions [g0, g0 + kStreamFeedPos) (lane i: g0 + i, g0 + 64 + i, ...)
  auto stage_a = [&](uint32_t g0, Step& f) {
    // (heap_factor * threshold only rises for heap_factor >= 0; a negative factor prunes nothing here, see the round loop)
    const bool full = heap.len == p.k && p.heap_factor >= 0.0f;
    const float cut = __fmul_rn(p.heap_factor, heap.thr);
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const uint32_t g = g0 + (uint32_t)r * 64u + lane;
      const bool valid = g < total_pos;
      uint32_t li = 0, d0 = 0;
      for (uint32_t j = 1; j < ng; ++j) {
        const uint32_t dj = readlane_u(my_doff, j);
        if (g >= dj) {
          li = j;
          d0 = dj;
        }
      }
      const uint32_t l = l0 + li;
      uint32_t bl = valid ? g - d0 : 0u;
      if (sorted0 && l == 0) bl = (uint32_t)s.order[bl];
      f.dix[r] = d0 + bl;
      f.dot[r] = s.dots[f.dix[r]];
      f.live[r] = valid && !(full && f.dot[r] < cut);
      f.p0[r] = 0;
      f.p1[r] = 0;
      if (f.live[r]) {
        const uint32_t gb = s.sel_b0[l] + bl;
        f.p0[r] = ix.block_post_start[gb];
        f.p1[r] = ix.block_post_start[gb + 1];
      }
    }
  };
  Step cur, nxt;
  if (total_pos) stage_a(0, nxt);
  for (uint32_t g0 = 0; g0 < total_pos && !failed; g0 += kStreamFeedPos) {
    cur = nxt;
    if (g0 + kStreamFeedPos < total_pos) stage_a(g0 + kStreamFeedPos, nxt);   // (its loads fly while this step's items are produced)
    replay_ready(false);
    // the skip test once more, against the threshold of NOW: no item of these blocks has been produced yet, so the
    // threshold stems from a prefix of what precedes them
    uint32_t incl[R], carry = 0;
    {
      const bool full = heap.len == p.k && p.heap_factor >= 0.0f;
      const float cut = __fmul_rn(p.heap_factor, heap.thr);
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const uint32_t cnt = (cur.live[r] && !(full && cur.dot[r] < cut)) ? cur.p1[r] - cur.p0[r] : 0u;
        incl[r] = wave_inclusive_scan(cnt) + carry;
        carry = readlane_u(incl[r], 63);
      }
    }
    uint32_t total = carry;
    if (total == 0) continue;
    // the step's block tables (this wavefront only: its DS operations execute in order)
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const uint32_t e = (uint32_t)r * 64u + lane;
      rg.f_incl[e] = incl[r];
      rg.f_p0[e] = cur.p0[r];
      rg.f_dix[e] = (uint16_t)cur.dix[r];
    }
    uint32_t done_items = 0;
    CTICK(1);
    while (done_items < total) {
      // room under the speculation budget (<= the ring: a slot is rewritten only after its item was replayed); while
      // there is none, whatever is scored is replayed, window full or not - the stream cannot go on before it is
      uint32_t spins = 0;
      while (produced - next >= budget) {
        replay_ready(true);
        if (produced - next < budget) break;
        if (uniform_u(lds_ld(&s.st[ST_S_ABORT])) || ++spins > kStreamSpinLimit) {
          if (spins > kStreamSpinLimit) stream_abort(s, qb, 17u);
          failed = true;
          break;
        }
#ifdef SGPU_PROF
        if (lane == 0) s.st[ST_S_BLOCKED] += 1;
#endif
        __builtin_amdgcn_s_sleep(1);
      }
      if (failed) break;
      CTICK(3);
      const uint32_t room = budget - (produced - next);
      // the blocks' exclusive item counts and sizes, from the inclusive counts in registers
      uint32_t before[R], cnt[R];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const uint32_t prev = r ? readlane_u(incl[r - 1], 63) : 0u;
        // (the lane shift is its own statement: inside `lane ? shift : prev` it would run with lane 0 switched off, and a
        // DPP read of a disabled lane returns nothing - lane 1 then lost its predecessor's count)
        const uint32_t up = shift_up1_u(incl[r]);
        before[r] = lane ? up : prev;   // (lane 0 takes the previous register's total)
        cnt[r] = incl[r] - before[r];
      }
      if (done_items) {
        // The threshold has moved on while the step's first items were produced: the blocks NOT YET STARTED are tested once
        // more (none of their items is out, so the threshold still stems from a prefix of what precedes them) and the
        // dead ones leave the tables; items already numbered keep their numbers.
        const bool full = heap.len == p.k && p.heap_factor >= 0.0f;
        const float cut = __fmul_rn(p.heap_factor, heap.thr);
        bool any = false;
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const bool drop = cnt[r] != 0u && before[r] >= done_items && full && cur.dot[r] < cut;
          any |= __ballot(drop) != 0ull;
          if (drop) cnt[r] = 0;
        }
        if (any) {
          uint32_t c2 = 0;
#pragma unroll
          for (int r = 0; r < R; ++r) {
            incl[r] = wave_inclusive_scan(cnt[r]) + c2;
            before[r] = incl[r] - cnt[r];
            c2 = readlane_u(incl[r], 63);
            rg.f_incl[(uint32_t)r * 64u + lane] = incl[r];
          }
          total = c2;
          if (done_items >= total) break;
        }
      }
      uint32_t n = total - done_items;
      n = n < room ? n : room;
      n = n < 64u * NCH ? n : 64u * NCH;
      // Which block does item done_items + j belong to? The n target slots' it_blk entries serve as scratch (they are
      // free, and written for good below): zeroed, then every block that STARTS inside the batch stores 1 + its table
      // index at its first item, and a running maximum over the items - seeded with the block that holds the batch's
      // first item - hands every item its block: two trips to LDS (this read-back, then the tables) where a binary
      // search of the inclusive counts took eight. (A wavefront's DS operations execute in order.)
#pragma unroll
      for (int c = 0; c < NCH; ++c)
        if ((uint32_t)c * 64u + lane < n) rg.it_blk[(produced + (uint32_t)c * 64u + lane) & rg.mask] = 0;
      uint32_t e_carry = 0;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        if (cnt[r] != 0u && before[r] >= done_items && before[r] - done_items < n)
          rg.it_blk[(produced + (before[r] - done_items)) & rg.mask] = (uint16_t)((uint32_t)r * 64u + lane + 1u);
        const uint64_t m = __ballot(cnt[r] != 0u && before[r] <= done_items);
        if (m) e_carry = (uint32_t)r * 64u + (63u - (uint32_t)__clzll(m)) + 1u;
      }
      uint64_t ref[NCH];
      uint32_t doc[NCH], dixc[NCH];
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        ref[c] = 0ull;
        doc[c] = 0u;
        dixc[c] = 0u;
        if ((uint32_t)c * 64u < n) {   // (uniform)
          const bool has = (uint32_t)c * 64u + lane < n;
          const uint32_t v = has ? (uint32_t)rg.it_blk[(produced + (uint32_t)c * 64u + lane) & rg.mask] : 0u;
          uint32_t e1 = wave_inclusive_max(v);
          e1 = e1 > e_carry ? e1 : e_carry;
          e_carry = readlane_u(e1, 63);
          const uint32_t e = e1 - 1u;   // (e1 >= 1: the batch's first item lies in a block that started at or before it)
          const uint32_t i = done_items + (has ? (uint32_t)c * 64u + lane : 0u);
          const uint32_t excl = e ? rg.f_incl[e - 1u] : 0u;
          const uint32_t pidx = rg.f_p0[e] + (i - excl);
          dixc[c] = (uint32_t)rg.f_dix[e];
          if (has) {
            ref[c] = ix.post_ref[pidx];
            doc[c] = ix.post_doc[pidx];
          }
        }
      }
      lds_order();
      CTICK(1);
      replay_ready(false);   // (while the posting loads are in flight)
      lds_order();
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        if ((uint32_t)c * 64u < n) {
          const bool has = (uint32_t)c * 64u + lane < n;
          const uint32_t slot = (produced + (uint32_t)c * 64u + lane) & rg.mask;
          const uint32_t len = (uint32_t)ref[c] & LenMask<VT>::v;
          const bool sh = has && len <= 128u, lg = has && len > 128u;
          if (has) {
            rg.it_ref[slot] = ref[c];
            rg.it_doc[slot] = doc[c];
            rg.it_blk[slot] = (uint16_t)dixc[c];
          }
          const uint64_t ms = __ballot(sh), ml = __ballot(lg);
          if (sh) rg.q_short[(qs + (uint32_t)__popcll(ms & below)) & rg.mask] = (uint16_t)slot;
          if (lg) rg.q_long[(ql + (uint32_t)__popcll(ml & below)) & rg.mask] = (uint16_t)slot;
          qs += (uint32_t)__popcll(ms);
          ql += (uint32_t)__popcll(ml);
        }
      }
      produced += n;
      done_items += n;
      lds_order();
      if (lane == 0) {
        lds_st(&s.st[ST_S_QS_HEAD], qs);
        lds_st(&s.st[ST_S_QL_HEAD], ql);
      }
      CTICK(2);
    }
  }
  lds_order();
  if (lane == 0) lds_st(&s.st[ST_S_DONE], 1u);   // (after the last heads: a scorer looks at DONE first)
  CTICK(1);
  // the rest of the replay
  for (uint32_t spins = 0; next != produced && !failed;) {
    replay_ready(true);
    if (next == produced) break;
    if (uniform_u(lds_ld(&s.st[ST_S_ABORT])) || ++spins > kStreamSpinLimit) {
      if (spins > kStreamSpinLimit) stream_abort(s, qb, 16u);
      break;
    }
    __builtin_amdgcn_s_sleep(1);
  }
  CTICK(4);
  heap.store(s.heap);
  if (lane == 0) {
    s.st[ST_HLEN] = heap.len;
    s.st[ST_THR] = __float_as_uint(heap.len == p.k ? heap.thr : 0.0f);
  }
  budget_io = budget;
}
