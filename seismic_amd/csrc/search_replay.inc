// search_replay.inc - part of search_kernel.inc (included there, inside namespace sgpu; needs search_lds.inc).
// Holds: the top-k heap in registers (RegHeap, heap_contains), the counted pass's visited bitmap (visited_test,
// visited_mark), the work counters (WorkCount) and the round loop's exact replay (replay_chunk, replay_candidates,
// replay_round).
// Called by: wavefront 0 only - of a round-loop workgroup (replay_round, from the kernel body), of a streamed one
// (search_stream.inc: the control wavefront keeps a RegHeap; replay_span restates replay_chunk over the ring) and of a
// wide round's owner (search_coop.inc: wide_round). visited_test is also read by phase A of the counted pass.

// ---------------------------------------------------------------------------
// top-k heap in the registers of wavefront 0 (KHeap, src/utils.rs:12-66)
// ---------------------------------------------------------------------------
template <int KR>
struct RegHeap {
  float sc[KR];
  uint32_t doc[KR];
  uint32_t len;   // wave-uniform
  float thr;      // wave-uniform: score of entry k-1 once len == k
  // Between replays the heap rests in LDS (entry e at word e: scores, then documents), so that its
  // 2*KR registers are not live - and not spilled - while the other phases run; wavefront 0 loads it
  // at the start of a replay and stores it back at the end (2*KR DS operations each way).
  SGPU_DEV void load(const uint32_t* hl, uint32_t len_, float thr_) {
    const uint32_t lane = lane_id();
#pragma unroll
    for (int r = 0; r < KR; ++r) {
      sc[r] = __uint_as_float(hl[r * 64 + lane]);
      doc[r] = hl[KR * 64 + r * 64 + lane];
    }
    len = len_;
    thr = thr_;
  }
  SGPU_DEV void store(uint32_t* hl) const {
    const uint32_t lane = lane_id();
#pragma unroll
    for (int r = 0; r < KR; ++r) {
      hl[r * 64 + lane] = __float_as_uint(sc[r]);
      hl[KR * 64 + r * 64 + lane] = doc[r];
    }
  }
  // x (wave-uniform) is inserted at its rank; entries at index >= k are dropped.
  SGPU_DEV void insert(float xs, uint32_t xd, uint32_t k) {
    const uint32_t lane = lane_id();
    uint32_t pos = 0;
#pragma unroll
    for (int r = 0; r < KR; ++r) {
      const bool better = (sc[r] > xs) || (sc[r] == xs && doc[r] < xd);
      pos += (uint32_t)__popcll(__ballot(better));
    }
#pragma unroll
    for (int r = KR - 1; r >= 0; --r) {
      float ps = shift_up1_f(sc[r]);
      uint32_t pd = shift_up1_u(doc[r]);
      if (r > 0) {
        const float cs = readlane_f(sc[r - 1], 63);
        const uint32_t cd = readlane_u(doc[r - 1], 63);
        if (lane == 0) {
          ps = cs;
          pd = cd;
        }
      }
      const uint32_t e = (uint32_t)r * 64u + lane;
      if (e == pos) {
        sc[r] = xs;
        doc[r] = xd;
      } else if (e > pos) {
        sc[r] = ps;
        doc[r] = pd;
      }
      if (e >= k) {
        sc[r] = -__builtin_inff();
        doc[r] = 0xffffffffu;
      }
    }
    if (len < k) ++len;
    if (len == k) thr = kth(k);
  }
  SGPU_DEV float kth(uint32_t k) const {   // score of entry k-1 (valid when len == k)
    float v = 0.0f;
#pragma unroll
    for (int r = 0; r < KR; ++r) {
      const float x = readlane_f(sc[r], (k - 1) & 63);
      if ((uint32_t)r == ((k - 1) >> 6)) v = x;
    }
    return v;
  }
};

// ---------------------------------------------------------------------------
// stage 2: the exact replay of the reference's sequential decisions (wavefront 0)
// ---------------------------------------------------------------------------
SGPU_DEV bool visited_test(const uint32_t* bitmap, uint32_t doc) {
  // written by other waves of this workgroup through L2 atomics: read past the (per-CU,
  // not atomically updated) L1 with an agent-scope load
  const uint32_t w = __hip_atomic_load(bitmap + (doc >> 5), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return (w >> (doc & 31)) & 1u;
}
SGPU_DEV void visited_mark(uint32_t* bitmap, uint32_t doc) {
  __hip_atomic_fetch_or(bitmap + (doc >> 5), 1u << (doc & 31), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Work the reference algorithm performs for this query (lane-local partial counts, wave 0).
struct WorkCount {
  uint32_t blocks, posts, docs, len;
};

// Is document `d` (wave-uniform) currently in the heap?
template <int KR>
SGPU_DEV bool heap_contains(const RegHeap<KR>& heap, uint32_t d) {
  bool m = false;
#pragma unroll
  for (int r = 0; r < KR; ++r) m |= __ballot(heap.doc[r] == d) != 0ull;
  return m;
}

// Sequential replay of the reference's decisions over the chunk's items (wavefront 0 only).
//
// Visited set (reference: FxHashSet keyed by the document's forward-index offset,
// src/inverted_index.rs:181-184, src/posting_list.rs:200,209). A document can recur only in a
// LATER list of the same query (a list holds a document once). USE_BITMAP = true keeps a
// per-workgroup bitmap in HBM (exact work counters; ~0.8 MB of extra traffic per query).
// USE_BITMAP = false needs no visited set at all and is exactly equivalent: a recurring document
// d has the same score s as the first time, and
//   * while the heap is not full every visited document is in the heap, so membership == visited;
//   * once full, a push is attempted only if s > kth. The first visit pushed d (then-kth <= kth < s)
//     and d cannot have been evicted while s > kth, so d is still in the heap: membership == visited
//     for exactly the items whose push would change anything. Recurring documents with s <= kth
//     are rejected by the reference's visited test and by the push rule alike.
// The price is re-scoring the recurring documents (1-2% of the postings).
template <int KR, bool USE_BITMAP>
SGPU_DEV void replay_chunk(RegHeap<KR>& heap, const ChunkBufs& cb, uint32_t n_items, uint32_t k,
                           float heap_factor, uint32_t* bitmap, uint32_t& decided_blk,
                           bool block_starts_at_0, WorkCount& wc, uint32_t& live_items, bool dups,
                           const float* dots, uint32_t len_mask) {
  // dots: summary dots of the current list (LDS); nullptr = no block test (kNN refinement)
  // dups: the round may hold the same document more than once (kNN refinement: two results can
  // share a neighbour; a posting list never repeats a document). The reference inserts into its
  // visited set item by item, so a later copy must see the earlier one.
  const uint32_t lane = lane_id();
  const uint32_t* it_words = (const uint32_t*)cb.it_ref;   // [2i] = low ref word (len), [2i+1] = score
  uint32_t i = 0;
  while (i < n_items) {
    const uint32_t idx = i + lane;
    const bool valid = idx < n_items;
    if (!USE_BITMAP && heap.len == k) {
      // Fast skip: the k-th best score only rises, so a window in which no score exceeds it
      // cannot change the heap; without a visited set to maintain there is nothing else to do.
      // (Work counters are exact only in the counted pass, which never takes this shortcut.)
      const float sc0 = valid ? __uint_as_float(it_words[2 * idx + 1]) : 0.0f;
      const float bd0 = valid ? (dots ? dots[cb.it_blk[idx]] : __builtin_inff()) : 0.0f;
      if (__ballot(valid && sc0 > heap.thr) == 0ull) {
        live_items += (uint32_t)__popcll(__ballot(valid && !(bd0 < __fmul_rn(heap_factor, heap.thr))));
        i += 64;
        continue;
      }
    }
    float sc = 0.0f;
    uint32_t doc = 0, blk = 0, len = 0;
    float bdot = 0.0f;
    bool vis = true, first = false;
    if (valid) {
      sc = __uint_as_float(it_words[2 * idx + 1]);
      len = it_words[2 * idx] & len_mask;
      const uint32_t d = cb.it_doc[idx];
      doc = d & 0x7fffffffu;
      vis = (d >> 31) != 0;
      blk = cb.it_blk[idx];
      bdot = dots ? dots[blk] : __builtin_inff();
      first = idx == 0 ? block_starts_at_0 : (cb.it_blk[idx - 1] != blk);
    }
    if (dups && USE_BITMAP) {   // marks made earlier in this round (by this wavefront) must be seen
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");
      if (valid && !vis) vis = visited_test(bitmap, doc);
    }
    if (heap.len < k) {
      // heap not full: every block that starts now is evaluated, every new doc is pushed
      if (!USE_BITMAP) {   // visited == already in the heap
#pragma unroll
        for (int r = 0; r < KR; ++r) {
          const uint32_t lim = heap.len > (uint32_t)r * 64u ? heap.len - (uint32_t)r * 64u : 0u;
          for (uint32_t l = 0; l < (lim < 64u ? lim : 64u); ++l) vis |= doc == readlane_u(heap.doc[r], l);
        }
      }
      if (dups) {   // a later copy of a document inside this window is "visited" by the earlier one
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
      else last = (n_items - i < 64u ? n_items - i : 64u) - 1u;
      if (take) {
        if (USE_BITMAP) visited_mark(bitmap, doc);
        wc.docs += 1;
        wc.len += len;
      }
      if ((!USE_BITMAP || dots) && valid && lane <= last) {   // (counted pass: the refinement's neighbours are no postings of a block)
        wc.posts += 1;
        wc.blocks += first;
      }
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
    // Heap full: the window's 64 items stay in registers; every heap change re-evaluates the
    // remaining lanes against the new threshold (the reference's per-item test, 64 at a time).
    uint32_t start = 0, advance = 64;
    if (dups && USE_BITMAP) {   // exact work counters: a later copy of a document inside this window is visited by the
      // earlier one, as above (it cannot change the heap either way: the window is reloaded after every insertion)
      const uint64_t nv0 = __ballot(valid && !vis);
      for (uint32_t l = 0; l < 63; ++l)
        if (((nv0 >> l) & 1ull) && lane > l && doc == readlane_u(doc, l)) vis = true;
    }
    for (;;) {
      const float thr = heap.thr;
      const float cut = __fmul_rn(heap_factor, thr);
      const bool live = valid && lane >= start && ((blk == decided_blk) || !(bdot < cut));
      const bool changing = live && !vis && (sc > thr);
      uint64_t cm = __ballot(changing);
      if (!USE_BITMAP) {   // drop recurring documents: they are in the heap already
        while (cm) {
          const uint32_t c0 = (uint32_t)(__ffsll((long long)cm) - 1);
          if (!heap_contains<KR>(heap, readlane_u(doc, c0))) break;
          cm &= cm - 1;
        }
      }
      const uint32_t f = cm ? (uint32_t)(__ffsll((long long)cm) - 1) : 63u;
      live_items += (uint32_t)__popcll(__ballot(live && lane <= f));
      if (USE_BITMAP && live && lane <= f) {   // exact work counters: the counted pass only
        if (dots) {
          wc.posts += 1;
          wc.blocks += first;
        }
        if (!vis) {
          visited_mark(bitmap, doc);
          wc.docs += 1;
          wc.len += len;
        }
      }
      if (cm == 0) break;
      heap.insert(readlane_f(sc, f), readlane_u(doc, f), k);
      decided_blk = readlane_u(blk, f);
      if (dups) {   // later copies of a document must see this step's visited marks: reload the window
        advance = f + 1;
        break;
      }
      start = f + 1;
      if (start >= 64) break;
    }
    i += advance;
  }
}

// Replay when the heap was already full at the start of the round and no visited bitmap is kept:
// only items whose score exceeds the round's starting threshold can change the heap (the
// threshold never decreases). Phase B collected their indices (<= kMaxCand, unordered); they are
// ranked by item index and walked in order with the same liveness / membership / push rules as
// replay_chunk, everything in registers.
template <int KR>
SGPU_DEV void replay_candidates(RegHeap<KR>& heap, const ChunkBufs& cb, const uint32_t* st, uint32_t nc,
                                uint32_t k, float heap_factor, uint32_t& decided_blk, const float* dots) {
  const uint32_t lane = lane_id();
  const uint32_t* it_words = (const uint32_t*)cb.it_ref;
  uint32_t idx = lane < nc ? st[ST_CAND + lane] : 0xffffffffu;
  uint32_t rank = 0;
  for (uint32_t l = 0; l < nc; ++l) rank += readlane_u(idx, l) < idx;
  uint32_t* sorted = (uint32_t*)st + ST_CAND_SORTED;
  if (lane < nc) sorted[rank] = idx;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  idx = lane < nc ? sorted[lane] : 0u;
  float sc = 0.0f, bdot = 0.0f;
  uint32_t doc = 0, blk = 0;
  if (lane < nc) {
    sc = __uint_as_float(it_words[2 * idx + 1]);
    doc = cb.it_doc[idx] & 0x7fffffffu;
    blk = cb.it_blk[idx];
    bdot = dots ? dots[blk] : __builtin_inff();
  }
  // lane c holds the c-th candidate in item order; each step jumps to the next one that still beats
  // the (rising) threshold, so the loop runs once per heap change rather than once per candidate
  uint64_t todo = nc >= 64 ? ~0ull : ((1ull << nc) - 1ull);
  for (;;) {
    const float thr = heap.thr;
    todo &= __ballot(sc > thr);
    if (todo == 0) break;
    const uint32_t c = (uint32_t)(__ffsll((long long)todo) - 1);
    todo &= todo - 1;
    const uint32_t blk_c = readlane_u(blk, c);
    const bool live = (blk_c == decided_blk) || !(readlane_f(bdot, c) < __fmul_rn(heap_factor, thr));
    if (!live) continue;
    const uint32_t doc_c = readlane_u(doc, c);
    if (heap_contains<KR>(heap, doc_c)) continue;   // re-encountered document: already in the heap
    heap.insert(readlane_f(sc, c), doc_c, k);
    decided_blk = blk_c;
  }
}

// Replay of one round on wavefront 0 + publication of the new heap state for the next filter.
template <int KR, bool COUNTED>
SGPU_DEV void replay_round(const ChunkBufs& cb, const Lds& s, const KParams& p,
                           uint32_t n_items, uint32_t* bitmap, uint32_t& decided_blk, bool block_starts_at_0,
                           WorkCount& wc, const float* dots, uint32_t len_mask, bool dups = false, uint32_t idle_now = 0xffffffffu) {
  // (idle_now: cooperative variant, the number of idle workgroups thread 0 fetched earlier in the round -
  // the next round's decision to go wide reads it from LDS; 0xffffffff = not fetched)
  RegHeap<KR> heap;
  heap.load(s.heap, s.st[ST_HLEN], __uint_as_float(s.st[ST_THR]));
  uint32_t live_items = 0;
  const uint32_t nc = s.st[ST_NCAND];
  if (!COUNTED && heap.len == p.k && nc <= kMaxCand) {
    // (the heap was full when the round started: phase B collected every item that can matter)
    replay_candidates<KR>(heap, cb, s.st, nc, p.k, p.heap_factor, decided_blk, dots);
    live_items = n_items;
  } else {
    replay_chunk<KR, COUNTED>(heap, cb, n_items, p.k, p.heap_factor, bitmap, decided_blk, block_starts_at_0, wc,
                              live_items, dups, dots, len_mask);
  }
  heap.store(s.heap);
  if (lane_id() == 0) {
    s.st[ST_HLEN] = heap.len;
    s.st[ST_THR] = __float_as_uint(heap.len == p.k ? heap.thr : 0.0f);
    s.st[ST_TMP1] = live_items;
    s.st[ST_ITEMS_DONE] += n_items;
    if (idle_now != 0xffffffffu) s.st[ST_CO_IDLE] = idle_now;
    s.st[ST_NSHORT] = 0;   // the next round's class lists start empty
  }
}
