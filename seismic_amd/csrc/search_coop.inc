// search_coop.inc - part of search_kernel.inc (included there, inside namespace sgpu; needs search_lds.inc,
// search_stage01.inc, search_score.inc, search_replay.inc).
// Holds: the cooperative protocol over the board in device memory - SGPU_RLX and the co_* accessors, CO_TRACE, the
// claim word, coop_work (a round's chunks: owner and helpers alike), wide_round (the owner's side) and coop_help
// (a workgroup without a query).
// Called by: the COOP variants of the kernel, by the whole workgroup: wide_round from the round loop once the heap is
// full, coop_help after the query queue is empty.

// ---------------------------------------------------------------------------
// cooperative mode (device_types.hpp: CoopView)
// ---------------------------------------------------------------------------
// Every word of the board is accessed with relaxed agent-scope atomics (sc1: L1 is bypassed, the L2s of
// the eight XCDs stay coherent for these lines); a publisher drains its stores (s_waitcnt vmcnt(0) in
// every storing wave, then a workgroup barrier) before ONE lane stores the word that makes them
// reachable (the claim word of a round, the done count of a chunk). No plain load ever touches the board.
#define SGPU_RLX __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT
// Timeline of a cooperative launch (tools/coop_trace.py; library built with -DSGPU_COOP_TRACE): event e of
// workgroup w = the first (or, for e >= 12, the last) time it passed the point, in 10 ns ticks of the
// constant 100 MHz counter, at trace[w * 16 + e].
#ifdef SGPU_COOP_TRACE
#define CO_TRACE(co, e)                                                                         \
  if (threadIdx.x == 0 && (co).trace) {                                                         \
    uint64_t* t_ = (co).trace + (size_t)blockIdx.x * 16 + (e);                                  \
    if ((e) >= 12 || *t_ == 0) *t_ = wall_clock64();                                            \
  }
#else
#define CO_TRACE(co, e) {}
#endif
SGPU_DEV uint64_t co_ld64(const uint64_t* p) { return __hip_atomic_load(p, SGPU_RLX); }
SGPU_DEV uint32_t co_ld32(const uint32_t* p) { return __hip_atomic_load(p, SGPU_RLX); }
SGPU_DEV void co_st64(uint64_t* p, uint64_t v) { __hip_atomic_store(p, v, SGPU_RLX); }
SGPU_DEV void co_drain() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
// A protocol error (a bounded wait that gave up, control words of the wrong round): the code goes to the board's
// sticky word AND to the launch's status word, which travels back to the host with the result rows - every
// cooperative launch is checked, at no cost (device_index.hip: staged_finish / batch_fetch).
SGPU_DEV void co_flag(const CoopView& co, const BatchView& qb, uint32_t code) {
  __hip_atomic_store(co.counters + 3, code, SGPU_RLX);
  if (qb.status) __hip_atomic_store(qb.status, code, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
constexpr uint32_t kCoopSpinLimit = 1u << 22;   // polls (of ~0.3 us or more each) before a wait gives up and flags the launch
// Claim word of a slot: next CHUNK : 20 | positions of the round : 22 | positions per chunk : 10 | round number : 10.
// A claim is ALWAYS fetch_add(word, 1): the amount does not depend on the round, so a claimer that looked at the
// word of round r and whose add lands on the word of round r + 1 (the owner finished r and published r + 1 in
// between) has simply claimed chunk `next` of round r + 1 - it decodes chunk size, extent and round number from the
// word the add RETURNED, never from the one it looked at. (Until r04 `next` counted positions and the claimer added
// the chunk size it had looked at: a stale look could add round r's size to round r + 1's counter.)
constexpr uint32_t kClaimNextBits = 20, kClaimPosBits = 22;
SGPU_DEV uint64_t co_claim_word(uint32_t seq, uint32_t chunk, uint32_t n_pos, uint32_t next) {
  return ((uint64_t)(seq & 1023u) << 52) | ((uint64_t)(chunk & 1023u) << 42) | ((uint64_t)n_pos << kClaimNextBits) | (uint64_t)next;
}
SGPU_DEV uint32_t co_claim_next(uint64_t w) { return (uint32_t)w & ((1u << kClaimNextBits) - 1u); }
SGPU_DEV uint32_t co_claim_npos(uint64_t w) { return (uint32_t)(w >> kClaimNextBits) & ((1u << kClaimPosBits) - 1u); }
SGPU_DEV uint32_t co_claim_chunk(uint64_t w) { return (uint32_t)(w >> 42) & 1023u; }
SGPU_DEV uint32_t co_claim_seq(uint64_t w) { return (uint32_t)(w >> 52) & 1023u; }
// first position of the chunk a word names; >= n_pos: nothing (left) to claim. (64-bit: an exhausted word keeps
// being incremented by claimers that looked a moment too early - at most one each)
SGPU_DEV uint64_t co_claim_first(uint64_t w) { return (uint64_t)co_claim_next(w) * co_claim_chunk(w); }

// Works on the open round of slot `slot` until its positions are all claimed: claim a chunk of positions,
// apply the skip test to its blocks (against the round's starting threshold: a staler threshold only
// admits more), expand the surviving blocks to their postings and score them - one document per 16-lane
// group at a time, four in flight - and append every item that beats the round's starting threshold to
// the owner's candidate list. A helper first brings the round's query into its own LDS (weights + lookup
// table). Returns with the workgroup in step. `own`: the caller is the round's owner (it then clears the
// round's open bit once everything is claimed).
template <typename CT, int NT, int LK, int VT>
SGPU_DEV bool coop_work(const Lds& s, const DevView& ix, const BatchView& qb, const CoopView& co, const KParams& p,
                        uint32_t slot, bool own, uint32_t& cur_q) {
  uint64_t* sw = co.slots + (size_t)slot * kCoopSlotWords;
  const uint64_t* pos_pub = co.pos_pub + (size_t)slot * co.max_pos;
  uint64_t* cands = co.cands + (size_t)slot * co.max_cand * 2;
  // chunk tables in the union region: per surviving block [co.chunk]: first posting, inclusive item count, dot bits, position
  uint32_t* hu_p0 = (uint32_t*)s.uni;
  uint32_t* hu_incl = hu_p0 + co.chunk;
  uint32_t* hu_dot = hu_incl + co.chunk;
  uint32_t* hu_pos = hu_dot + co.chunk;
  const uint32_t lane = threadIdx.x & 63, sub = threadIdx.x & 15;
  bool worked = false;
  uint32_t pending = 0;   // positions of the chunk just finished, reported by thread 0 with its next claim
  // (Every thread-0 section of this loop sits at the HEAD of an iteration, in front of a barrier. A second
  // one at the tail - "report the chunk, then loop" - gets merged with the head's across the back edge by
  // the compiler, which then parks thread 0 outside a loop the other lanes of its wavefront keep running:
  // barriers no longer pair up. Seen on ROCm 7.2 / gfx950; the report therefore rides on the next claim.)
  for (;;) {
    uint32_t spec = 0;
    if (threadIdx.x == 0) {
      if (pending) __hip_atomic_fetch_add((uint32_t*)(sw + 1), pending, SGPU_RLX);   // the previous chunk is done
      // look before claiming: an exhausted round is not worth an atomic (and its word is not polluted)
      uint64_t w = co_ld64(sw);
      if (co_claim_first(w) < (uint64_t)co_claim_npos(w)) w = __hip_atomic_fetch_add(sw, 1ull, SGPU_RLX);
      s.st[ST_CO_CLAIM_LO] = (uint32_t)w;
      s.st[ST_CO_CLAIM_HI] = (uint32_t)(w >> 32);
    }
    __syncthreads();
    const uint64_t w = ((uint64_t)s.st[ST_CO_CLAIM_HI] << 32) | s.st[ST_CO_CLAIM_LO];
    const uint32_t end = co_claim_npos(w), chunk = co_claim_chunk(w);
    if (co_claim_first(w) >= (uint64_t)end) break;   // nothing (left) to claim
    const uint32_t c0 = (uint32_t)co_claim_first(w);
    // A valid claim pins the round: its control words cannot change before this chunk is reported done.
    // (the word the add returned IS the round's: the owner publishes the next round only after every chunk of
    // this one has been reported done)
    if (threadIdx.x == 0) {
      const uint64_t a = co_ld64(sw + 3), b = co_ld64(sw + 4);
      s.st[ST_CO_QUERY] = (uint32_t)(a >> 32);
      s.st[ST_CO_THR0] = (uint32_t)a;
      s.st[ST_CO_CUT] = (uint32_t)(b >> 32);
      // the control words belong to the claimed round; anything else is a protocol error: flag the launch
      if (((uint32_t)b & 1023u) != co_claim_seq(w)) co_flag(co, qb, 3u);
    }
    const uint32_t n = end - c0 < chunk ? end - c0 : chunk;
    if (!own) CO_TRACE(co, 9);
    __syncthreads();
    // a helper brings the round's query into its own LDS: weights + lookup table (kept while it helps
    // rounds of the same query; the owner's are in place)
    const uint32_t rq = s.st[ST_CO_QUERY];
    if (!own && rq != cur_q) {
      if (LK == LK_HASH && threadIdx.x == 0) s.st[ST_HMULT] = qb.q_seed ? hash_mult(qb.q_seed[rq]) : 1u;
      uint32_t nnz;
      load_query<NT>(s, qb, rq, &nnz);
      if (!Vt<VT>::half)
        for (uint32_t j = threadIdx.x; j < nnz; j += NT) s.q_sc[j] = __fmul_rn(qb.q_val[qb.q_off[rq] + j], p.val_scale);
      lookup_clear<LK>(s, ix.dim, threadIdx.x, NT);
      __syncthreads();
      build_lookup<NT, LK>(s, ix.dim, nnz);
      cur_q = rq;
      __syncthreads();
    }
    if (!own) CO_TRACE(co, 10);
    // ---- the chunk's blocks (n <= chunk <= co.chunk <= 64 x waves): skip test, posting range, item prefix ----
    const float thr0 = __uint_as_float(s.st[ST_CO_THR0]), cut = __uint_as_float(s.st[ST_CO_CUT]);
    uint32_t n_live, n_items;
    {
      const uint32_t t = threadIdx.x;
      bool live = false;
      uint32_t p0 = 0, cnt = 0, dotb = 0;
      if (t < n) {
        const uint64_t r = co_ld64(pos_pub + c0 + t);
        dotb = (uint32_t)(r >> 32);
        const uint32_t gb = (uint32_t)r;
        live = !(__uint_as_float(dotb) < cut);
        if (live) {
          p0 = ix.block_post_start[gb];
          cnt = ix.block_post_start[gb + 1] - p0;
          live = cnt != 0;
        }
      }
      // blocks in position order, items prefixed: slot = live blocks before this one, incl = items up to and with it
      uint32_t tot_live, tot_items;
      const uint32_t live_incl = wg_inclusive_scan<NT>(live ? 1u : 0u, s.part, &tot_live);
      const uint32_t item_incl = wg_inclusive_scan<NT>(cnt, s.part + (NT / 64 + 1), &tot_items);
      if (live) {
        const uint32_t x = live_incl - 1u;
        hu_p0[x] = p0;
        hu_incl[x] = item_incl;
        hu_dot[x] = dotb;
        hu_pos[x] = c0 + t;
      }
      n_live = tot_live;
      n_items = tot_items;
    }
    __syncthreads();
    if (!own) CO_TRACE(co, 11);
    // ---- score: lane group g takes items g, g + NT/16, ...; four in flight (three in a 1024-thread workgroup, whose
    // waves have 128 registers: with four the single-query symbol spilled 62 VGPRs, 100 scratch instructions in its round
    // loops - with three 50, and a single query takes 107.5 instead of 113.6 us, a 64-query launch 209 instead of 218;
    // two in flight: the same again, profiles/r05_coop_in_flight.txt) ----
    {
      constexpr int ND = NT == 1024 ? 3 : 4;
      constexpr uint32_t NG = NT / 16;
      const bool sc = LK == LK_DENSE && uniform_u(s.st[ST_SCALED]) != 0u;   // the form of the lookup table in THIS workgroup's LDS
      for (uint32_t ib = threadIdx.x >> 4; ib < n_items; ib += NG * ND) {
        uint32_t len[ND], doc[ND], key[ND], dotb[ND];
        uint64_t ref[ND];
        // the postings of this lane group's items (all 16 lanes read the same words)
#pragma unroll
        for (int u = 0; u < ND; ++u) {
          const uint32_t i = ib + (uint32_t)u * NG;
          const bool has = i < n_items;
          const uint32_t ii = has ? i : ib;
          uint32_t lo = 0, hi = n_live;   // first block with incl > ii
          while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (hu_incl[mid] <= ii) lo = mid + 1; else hi = mid;
          }
          const uint32_t excl = lo ? hu_incl[lo - 1] : 0u, j = ii - excl;
          const uint32_t pidx = hu_p0[lo] + j;
          ref[u] = ix.post_ref[pidx];
          doc[u] = ix.post_doc[pidx];
          dotb[u] = hu_dot[lo];
          key[u] = j > 0xffffu ? 0xffffffffu : ((hu_pos[lo] << 16) | j);   // (a block of > 65536 postings cannot be keyed)
          len[u] = has ? 1u : 0u;
        }
        const uint8_t* rec[ND];
        DocChunk<CT, VT> d[ND];
        bool raw[ND];   // (VT_DVB) the record is in the raw VT_U8 form
        const uint32_t e0 = sub * 8u;
#pragma unroll
        for (int u = 0; u < ND; ++u) {
          raw[u] = Vt<VT>::sliced && ((uint32_t)ref[u] & kRawBit) != 0;
          len[u] = len[u] ? ((uint32_t)ref[u] & LenMask<VT>::v) : 0u;
          rec[u] = ix.fwd + (ref[u] >> 16) * 16ull;
          load_pass<CT, VT>(d[u], rec[u], len[u], raw[u], e0);
        }
#pragma unroll
        for (int u = 0; u < ND; ++u) {
          float a = 0.0f;
          a = sc ? score_pass<CT, LK, VT, true>(s, d[u], raw[u], e0, len[u], a)
                 : score_pass<CT, LK, VT, false>(s, d[u], raw[u], e0, len[u], a);
          for (uint32_t eb = 128u; eb < len[u]; eb += 128u) {   // documents longer than 128 elements (trip count per group)
            DocChunk<CT, VT> t;
            load_pass<CT, VT>(t, rec[u], len[u], raw[u], eb + e0);
            a = sc ? score_pass<CT, LK, VT, true>(s, t, raw[u], eb + e0, len[u], a)
                   : score_pass<CT, LK, VT, false>(s, t, raw[u], eb + e0, len[u], a);
          }
          a = reduce16(a);
          spec += (sub == 0 && len[u] != 0);
          if (sub == 0 && len[u] != 0 && a > thr0) {
            const uint32_t ci = __hip_atomic_fetch_add((uint32_t*)(sw + 2), key[u] == 0xffffffffu ? 0x40000000u : 1u, SGPU_RLX);
            if (ci < co.max_cand && key[u] != 0xffffffffu) {
              co_st64(cands + 2 * (size_t)ci, ((uint64_t)__float_as_uint(a) << 32) | (uint64_t)key[u]);
              co_st64(cands + 2 * (size_t)ci + 1, ((uint64_t)dotb[u] << 32) | (uint64_t)doc[u]);
            }
          }
        }
      }
    }
    if (qb.out_stats) {   // documents scored speculatively: work counter [7] of the round's query
#pragma unroll
      for (int dd = 32; dd >= 1; dd >>= 1) spec += __shfl_xor(spec, dd);
      if (lane == 0 && spec) atomicAdd(&qb.out_stats[(size_t)rq * STATS_WORDS + 7], spec);
    }
    co_drain();   // every wave: its candidate stores have landed
    __syncthreads();
    if (!own) CO_TRACE(co, 12);
    pending = n;    // reported at the head of the next iteration
    worked = true;
  }
  if (own && threadIdx.x == 0)   // all positions are claimed: helpers need not look at this slot any more
    __hip_atomic_fetch_and(co.open + (slot >> 6), ~(1ull << (slot & 63)), SGPU_RLX);
  __syncthreads();
  return worked;
}

// The owner's side of a wide round over the lists [l, l1) of the current group, list l from traversal
// position `pos`. Returns false (nothing changed) when the round cannot be keyed or held, or produced
// more candidates than the owner can sort - the caller then carries on with local rounds.
// (Out-of-line versions of the two cooperative functions were tried - so that their registers and spills
// stay out of the hot loops - and run the whole kernel 2.5-3x slower: the calls' register conventions spill
// the kernel's own live state.)
template <typename CT, int NT, int KR, int LK, int VT>
SGPU_DEV bool wide_round(const Lds& s, const DevView& ix, const BatchView& qb, const CoopView& co, const KParams& p,
                         uint32_t q, uint32_t& l_io, uint32_t& pos_io, uint32_t l1, bool sorted0, uint32_t limit, uint32_t& seq) {
  // the round covers at most `limit` positions from (l, pos); on success (l_io, pos_io) is where it ended
  const uint32_t l = l_io, pos = pos_io;
  const uint32_t slot = blockIdx.x;
  uint64_t* sw = co.slots + (size_t)slot * kCoopSlotWords;
  uint32_t n_pos = 0;
  for (uint32_t li = l; li < l1; ++li) n_pos += s.sel_nb[li] - (li == l ? pos : 0u);
  if (n_pos > limit) n_pos = limit;
  if (n_pos == 0 || n_pos > co.max_pos) return false;
  CO_TRACE(co, 1);
  // ---- publish the positions: {summary dot, global block id}, traversal order ----
  {
    uint64_t* pub = co.pos_pub + (size_t)slot * co.max_pos;
    uint32_t base = 0;
    for (uint32_t li = l; li < l1 && base < n_pos; ++li) {
      const uint32_t first = li == l ? pos : 0u, b0 = s.sel_b0[li];
      const uint32_t nb = s.sel_nb[li] - first <= n_pos - base ? s.sel_nb[li] : first + (n_pos - base);   // (end of this list's share)
      const float* dots = s.dots + s.sel_doff[li];
      const bool sorted = sorted0 && li == 0;
      for (uint32_t i = first + threadIdx.x; i < nb; i += NT) {
        const uint32_t b = sorted ? (uint32_t)s.order[i] : i;
        co_st64(pub + base + (i - first), ((uint64_t)__float_as_uint(dots[b]) << 32) | (uint64_t)(b0 + b));
      }
      base += nb - first;
      // where the round ends
      if (nb == s.sel_nb[li]) {
        l_io = li + 1;
        pos_io = 0;
      } else {
        l_io = li;
        pos_io = nb;
      }
    }
  }
  CO_TRACE(co, 2);
  const uint32_t thr0b = s.st[ST_THR];
  // the skip test of the filter: heap_factor * threshold only rises for heap_factor >= 0; a negative
  // factor prunes nothing ahead of the replay (see the local filter)
  const float cut = p.heap_factor >= 0.0f ? __fmul_rn(p.heap_factor, __uint_as_float(thr0b)) : -__builtin_inff();
  seq += 1;
  if (threadIdx.x == 0) {
    co_st64(sw + 1, 0ull);   // done
    co_st64(sw + 2, 0ull);   // candidates
    co_st64(sw + 3, ((uint64_t)q << 32) | (uint64_t)thr0b);
    co_st64(sw + 4, ((uint64_t)__float_as_uint(cut) << 32) | (uint64_t)(seq & 1023u));
    // positions per claim: about one claim per workgroup that can take part (a claim costs two atomics on
    // this slot's words, and a workgroup scores a chunk's documents one per 16-lane group)
    const uint32_t idle = co_ld32(co.counters + 0);
    const uint32_t owners = gridDim.x > idle ? gridDim.x - idle : 1u;   // (they may all have a round open at once)
    const uint32_t takers = idle / owners + 1u;
    uint32_t chunk = (n_pos + takers - 1u) / takers;
    chunk = chunk < co.chunk_min ? co.chunk_min : chunk;
    s.st[ST_CO_FLAG] = chunk < co.chunk ? chunk : co.chunk;
  }
  co_drain();
  __syncthreads();
  if (threadIdx.x == 0) {
    co_st64(sw, co_claim_word(seq, s.st[ST_CO_FLAG], n_pos, 0));
    __hip_atomic_fetch_or(co.open + (slot >> 6), 1ull << (slot & 63), SGPU_RLX);
  }
  // (A barrier keeps this thread-0 section apart from the one at the head of coop_work's claim loop: left
  // adjacent, the compiler fuses them and restructures the loop around the fused section - the barrier
  // mismatch described at coop_work, seen again when a uniform branch that used to sit here was removed.)
  __syncthreads();
  // ---- work on the round like any helper, then wait for the chunks others took ----
  {
    uint32_t mine = q;
    coop_work<CT, NT, LK, VT>(s, ix, qb, co, p, slot, true, mine);
  }
  CO_TRACE(co, 3);
  if (threadIdx.x == 0) {
    // (bounded: a protocol error must surface as a flagged, failing launch, never as a hung device)
    uint32_t spins = 0;
    const uint32_t spin_limit = kCoopSpinLimit;
    while (co_ld32((const uint32_t*)(sw + 1)) < n_pos && ++spins < spin_limit) __builtin_amdgcn_s_sleep(8);
    if (spins >= spin_limit) co_flag(co, qb, 1u);
    s.st[ST_CO_NCAND] = spins >= spin_limit ? 0xffffffffu : co_ld32((const uint32_t*)(sw + 2));
  }
  __syncthreads();
  CO_TRACE(co, 4);
  const uint32_t nc = s.st[ST_CO_NCAND];
  if (nc > co.max_cand) {   // too many to sort here: the heap is untouched, local rounds take over from where
    l_io = l;               // the round began
    pos_io = pos;
    return false;
  }
  // ---- candidates into LDS, ranked by (position, posting) ----
  uint32_t* ck = (uint32_t*)s.uni;           // [max_cand] keys as they came
  uint32_t* c_key = ck + co.max_cand;        // sorted: key, score bits, doc, block dot bits
  uint32_t* c_sc = c_key + co.max_cand;
  uint32_t* c_doc = c_sc + co.max_cand;
  uint32_t* c_dot = c_doc + co.max_cand;
  const uint64_t* cands = co.cands + (size_t)slot * co.max_cand * 2;
  // (max_cand <= NT: one candidate per thread, one trip to the board)
  uint64_t r0 = 0, r1 = 0;
  if (threadIdx.x < nc) {
    r0 = co_ld64(cands + 2 * (size_t)threadIdx.x);
    r1 = co_ld64(cands + 2 * (size_t)threadIdx.x + 1);
    ck[threadIdx.x] = (uint32_t)r0;
  }
  __syncthreads();
  if (threadIdx.x < nc) {
    const uint32_t key = (uint32_t)r0;
    uint32_t rank = 0;
    for (uint32_t j = 0; j < nc; ++j) rank += ck[j] < key;   // keys are distinct (one per posting)
    c_key[rank] = key;
    c_sc[rank] = (uint32_t)(r0 >> 32);
    c_doc[rank] = (uint32_t)r1;
    c_dot[rank] = (uint32_t)(r1 >> 32);
  }
  __syncthreads();
  // ---- exact replay on wavefront 0: the rules of replay_candidates, window by window ----
  if ((threadIdx.x >> 6) == 0) {
    RegHeap<KR> heap;
    heap.load(s.heap, s.st[ST_HLEN], __uint_as_float(s.st[ST_THR]));
    const uint32_t lane = lane_id();
    uint32_t decided = 0xffffffffu;
    for (uint32_t w0 = 0; w0 < nc; w0 += 64) {
      const uint32_t c = w0 + lane;
      const bool valid = c < nc;
      const float sc = valid ? __uint_as_float(c_sc[c]) : 0.0f;
      const float bdot = valid ? __uint_as_float(c_dot[c]) : 0.0f;
      const uint32_t doc = valid ? c_doc[c] : 0u, upos = valid ? (c_key[c] >> 16) : 0u;
      uint64_t todo = __ballot(valid);
      for (;;) {
        const float thr = heap.thr;
        todo &= __ballot(sc > thr);
        if (todo == 0) break;
        const uint32_t f = (uint32_t)(__ffsll((long long)todo) - 1);
        todo &= todo - 1;
        const uint32_t pos_f = readlane_u(upos, f);
        const bool live = (pos_f == decided) || !(readlane_f(bdot, f) < __fmul_rn(p.heap_factor, thr));
        if (!live) continue;
        const uint32_t doc_f = readlane_u(doc, f);
        if (heap_contains<KR>(heap, doc_f)) continue;   // re-encountered document: already in the heap
        heap.insert(readlane_f(sc, f), doc_f, p.k);
        decided = pos_f;
      }
    }
    heap.store(s.heap);
    if (lane == 0) {
      s.st[ST_HLEN] = heap.len;
      s.st[ST_THR] = __float_as_uint(heap.len == p.k ? heap.thr : 0.0f);
    }
  }
  __syncthreads();
  CO_TRACE(co, 5);
  return true;
}

// What a workgroup does once the query queue is empty: it helps the owners of open rounds until every
// query of the launch is finished.
template <typename CT, int NT, int LK, int VT>
SGPU_DEV void coop_help(const Lds& s, const DevView& ix, const BatchView& qb, const CoopView& co, const KParams& p) {
  if (threadIdx.x == 0) __hip_atomic_fetch_add(co.counters + 0, 1u, SGPU_RLX);
  uint32_t cur_q = 0xffffffffu;
  const uint32_t lane = threadIdx.x & 63;
  for (;;) {
    if ((threadIdx.x >> 6) == 0) {
      uint32_t found, spins = 0;
      for (;;) {
        const uint64_t w = lane < 8 ? co_ld64(co.open + lane) : 0ull;
        const uint32_t pc = (uint32_t)__popcll(w);
        const uint32_t incl = wave_inclusive_scan(pc);
        const uint32_t total = readlane_u(incl, 63);
        if (total) {   // the (blockIdx mod total)-th open slot: helpers spread over the open rounds
          const uint32_t r = blockIdx.x % total;
          const bool mine = r >= incl - pc && r < incl;
          uint32_t which = 0;
          if (mine) {
            uint64_t ww = w;
            for (uint32_t i = incl - pc; i < r; ++i) ww &= ww - 1;
            which = lane * 64u + (uint32_t)(__ffsll((long long)ww) - 1);
          }
          const uint64_t mm = __ballot(mine);
          found = readlane_u(which, (uint32_t)(__ffsll((long long)mm) - 1));
          break;
        }
        const uint32_t dq = co_ld32(co.counters + 1);
        if (dq >= qb.nq) {
          found = 0xffffffffu;
          break;
        }
        if (++spins >= kCoopSpinLimit) {   // (bounded, as the owner's wait is)
          if (lane == 0) co_flag(co, qb, 2u);
          found = 0xffffffffu;
          break;
        }
        for (uint32_t z = 0; z < co.poll_sleep; ++z) __builtin_amdgcn_s_sleep(16);   // ~0.45 us each
      }
      if (lane == 0) s.st[ST_CO_SLOT] = found;
    }
    __syncthreads();
    const uint32_t slot = s.st[ST_CO_SLOT];
    if (slot == 0xffffffffu) break;
    CO_TRACE(co, 8);
    if (!coop_work<CT, NT, LK, VT>(s, ix, qb, co, p, slot, false, cur_q))
      __builtin_amdgcn_s_sleep(16);   // an open bit whose positions were all taken: its owner is about to clear it
  }
}
