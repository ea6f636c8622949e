// search_kernel.inc — the Seismic search hot path as one persistent gfx950 kernel (included by the
// sk_*.hip translation units, which instantiate it per component type and lookup layout).
//
// One query per workgroup (persistent workgroups pull queries from an atomic
// queue, longest-expected first). Per query, following InvertedIndexBase::search
// (reference src/inverted_index.rs:153-234):
//
//   stage 0  query -> LDS: sorted (component, value) pairs; the query_cut heaviest
//            components are ranked (k_largest_by, src/inverted_index.rs:187-190)
//            -> the posting lists to walk, in order.
//   stage 1  hot loop A, QuantizedSummary::distances (src/quantized_summary.rs:64-160)
//            for ALL selected lists at once (a pure function of the query) - or, when the block
//            dots of all lists do not fit the LDS area, for one GROUP of lists after the other
//            (stage 1 of the group, stage 2 of its lists, next group; plan_list_group):
//            matching summary rows are located by binary search; one wavefront per
//            list then streams the list's matched rows in ascending query component
//            order, 64 (block id, dequantised value) entries per step, the loads of
//            the next 16 steps in flight, and adds value * weight to f32
//            accumulators in LDS. A wavefront issues its DS operations in order and
//            block ids are distinct within a row, so every accumulator receives its
//            additions in ascending query component order with the reference's
//            roundings ((code*quant + min) * qv, then +=; no FMA; code*quant + min
//            is precomputed once at upload): BIT-EXACT.
//   lookup   the query lookup table (cleared during stage 1 by the wavefronts that
//            have no list): one byte per vocabulary id (1 + rank in the query,
//            0 = absent) when it fits, else {32 bits, rank} per 32 ids.
//   stage 2  hot loop B, PostingList::search / sort_and_search /
//            evaluate_posting_block (src/posting_list.rs:115-215), list by list.
//            The reference's skip test reads the LIVE k-th best score, so the set of
//            scored documents depends on the traversal order. The threshold only
//            rises, hence testing a block against an OLDER threshold can only admit
//            more blocks. Each round therefore
//              (a) filters the remaining blocks against the current threshold and
//                  compacts the survivors in traversal order, under an item budget;
//              (b) fetches their postings and scores every document SPECULATIVELY:
//                  16 lanes per document, 16-byte loads of the record (components |
//                  f16 values, or fixed-u8 codes); per lane group four documents of <= 128
//                  elements (or two longer ones) in flight in rotating register slots; a
//                  wavefront pulls 4*ND consecutive items at once and interleaves them over its
//                  lane groups, so one load instruction covers four consecutive items - adjacent
//                  records in the block-major forward store;
//              (c) REPLAYS the reference's sequential decisions on one wavefront over
//                  the (block dot, doc score) table in LDS: same skip tests with the
//                  live threshold, same heap pushes in the same order. Once the heap
//                  is full only items scoring above the round's starting threshold
//                  can matter; phase (b) collects them and the replay walks just
//                  those, in order, in registers.
//            The result is the reference's exact candidate set and top-k.
//            (r06: for plain launches steps (a) - (c) no longer alternate round by round with a workgroup barrier between any
//            two: they run as a STREAM - one control wavefront filters, fetches postings and replays, the others score items
//            out of a ring in LDS - see "stage 2 as a stream", search_stream.inc. The counted pass and the cooperative variant keep the rounds.)
//   visited  the reference's FxHashSet (src/inverted_index.rs:181-184) is replaced by
//            an exactly equivalent heap-membership test at push time (proof at
//            replay_chunk); a bitmap in HBM is kept only for the "counted" pass that
//            reports exact work counters.
//   top-k    KHeap (src/utils.rs:12-66) is a sorted array in the VGPRs of wavefront 0 during a
//            replay (entry e in lane e%64, register e/64): insertion is a ballot + one DPP lane
//            shift, the threshold is a readlane. Between replays it rests in LDS, so its
//            registers are not live (and not spilled) in the other phases.
//
// No MFMA: this is gather / scatter-add / reduce work bounded by HBM latency and
// bandwidth. Floating point follows the reference (Rust never contracts): compiled
// with -ffp-contract=off and written with __fmul_rn/__fadd_rn.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>

#include "device_types.hpp"
#include "record.hpp"

namespace sgpu {

#ifndef SGPU_REPLAY_PRIO
#define SGPU_REPLAY_PRIO 2
#endif
#ifndef SGPU_WAVES_PER_EU
#define SGPU_WAVES_PER_EU 4   // 2 workgroups of 512 threads per CU (<= 128 VGPRs)
#endif

// The kernel's parts, one subject each, all inside namespace sgpu (this file keeps the kernel body and the launcher):
#include "search_lds.inc"       // lane and workgroup primitives, the LDS carve, the ST_* state words, the round loop's buffers
#include "search_stage01.inc"   // stage 0 and stage 1: query, list choice, row tables, summary dots, lookup table, first-list sort
#include "search_score.inc"     // a document's score by its 16-lane group; the round loop's phase B (score_items, classify_item)
#include "search_replay.inc"    // the register heap and the exact replay of a round (replay_round)
#include "search_stream.inc"    // stage 2 as a stream: the ring, the scorers, the control wavefront
#include "search_coop.inc"      // the cooperative protocol: coop_work, wide_round, coop_help

// ---------------------------------------------------------------------------
// the kernel
// ---------------------------------------------------------------------------
// COOP: the cooperative variant (CoopView; small launches and launch tails). The plain variant carries
// none of its code, registers or kernel arguments (its board argument is an empty struct).
template <bool COOP> struct CoopArg { using type = CoopView; };
template <> struct CoopArg<false> { struct type {}; };
template <bool COOP> SGPU_DEV CoopView coop_view(const typename CoopArg<COOP>::type& a);
template <> SGPU_DEV CoopView coop_view<true>(const CoopView& a) { return a; }
template <> SGPU_DEV CoopView coop_view<false>(const CoopArg<false>::type&) { return CoopView{}; }

#include "search_steps.inc"   // what frames a query in the body: the phase clocks (TICK), the serial role's priority, write_stats

// STREAM: stage 2 as a stream of items between a feeder, the scorers and a replayer wavefront ("stage 2 as a stream",
// search_stream.inc) instead of the round loop; plain launches only (the counted and the cooperative variants keep the rounds).
template <typename CT, int NT, int KR, int LK, bool COUNTED, int VT, bool COOP, bool STREAM = false>
__global__ __launch_bounds__(NT, SGPU_WAVES_PER_EU) void seismic_search_kernel(DevView ix, BatchView qb, KParams p,
                                                           LdsLayout L, uint32_t* queue,
                                                           uint32_t* bitmaps, typename CoopArg<COOP>::type co_arg) {
  static_assert(!STREAM || (!COUNTED && !COOP), "the streamed stage 2 serves plain launches");
  const CoopView co = coop_view<COOP>(co_arg);
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const Lds s = carve(smem, L);
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t* bitmap = bitmaps + (size_t)blockIdx.x * ix.n_bitmap_words;
  const ChunkBufs cb = carve_chunk<NT>(s.uni, p.items_max);
  WorkCount wc;       // lane-local partial counts, wavefront 0

  // one-time LDS init
  if (threadIdx.x == 0) {   // the weight every non-matching component resolves to
    s.q_val[-1] = 0.0f;
    s.q_sc[-1] = 0.0f;
  }
  __syncthreads();
  uint32_t co_seq = 0;      // rounds this workgroup has opened on its slot
  bool wide_ok = false;     // enough idle workgroups were seen (they never go back to owning a query)

  for (;;) {
    if (threadIdx.x == 0) {
      const uint32_t ticket = atomicAdd(queue, 1u) - p.queue_base;   // (every workgroup ends on exactly one ticket >= nq: nq + gridDim.x in all)
      // longest-expected-first order prepared by the host (tail balance); identity if absent
      s.st[ST_Q] = ticket < qb.nq ? (qb.q_order ? qb.q_order[ticket] : ticket) : 0xffffffffu;
      // workgroups can only run out of queries while one of the last `gridDim` tickets is being served
      if (COOP) s.st[ST_CO_TAIL] = (uint64_t)ticket + gridDim.x >= qb.nq ? 1u : 0u;
    }
    __syncthreads();
    const uint32_t q = s.st[ST_Q];
    if (q == 0xffffffffu) break;
    if (COOP) CO_TRACE(co, 0);
    // LK_HASH: the multiplier under which this query's components hash without collision (host-chosen)
    if (LK == LK_HASH && threadIdx.x == 0) s.st[ST_HMULT] = qb.q_seed ? hash_mult(qb.q_seed[q]) : 1u;

    PhaseClocks clk;   // (TICK)
    clk.start();
    // ---- stage 0 ----
    uint32_t nnz;
    load_query<NT>(s, qb, q, &nnz);
    if (!Vt<VT>::half)   // the scoring loop's weights carry the (power of two) value scale
      for (uint32_t j = threadIdx.x; j < nnz; j += NT) s.q_sc[j] = __fmul_rn(qb.q_val[qb.q_off[q] + j], p.val_scale);
    for (uint32_t e = threadIdx.x; e < (uint32_t)KR * 64u; e += NT) {   // empty heap (KHeap::new)
      s.heap[e] = 0xff800000u;                    // -inf
      s.heap[KR * 64 + e] = 0xffffffffu;
    }
    wc = WorkCount{0, 0, 0, 0};
    uint32_t spec_docs = 0;
    if (threadIdx.x == 0) {
      s.st[ST_HLEN] = 0;
      s.st[ST_THR] = 0;
      s.st[ST_NSHORT] = 0;
      s.st[ST_ENTRIES] = 0;
      s.st[ST_ROWS] = 0;
      s.st[ST_ITEMS_DONE] = 0;
      s.st[ST_CO_IDLE] = 0;
#ifdef SGPU_PROF
      if (STREAM) {
        s.st[ST_S_STARVED] = 0;
        s.st[ST_S_BLOCKED] = 0;
        s.st[ST_S_SPANS] = 0;
        s.st[ST_S_BUDGET_SUM] = 0;
        s.st[ST_S_SKIPPED] = 0;
      }
#endif
    }
    bool wide_off = false;   // this query's round did not fit the board: local rounds only
    __syncthreads();
    if (p.mode == MODE_DOTS) {   // sgpu_summary_distances: aim stage 1 at one given list
      if (threadIdx.x == 0) {
        const uint32_t c = p.target_list;
        s.sel_comp[0] = c;
        s.sel_b0[0] = ix.list_block_start[c];
        s.sel_nb[0] = ix.list_block_start[c + 1] - ix.list_block_start[c];
        if constexpr (sizeof(CT) != 2) {   // (u16: the row directory, no row range)
          s.sel_r0[0] = ix.list_row_start[c];
          s.sel_nr[0] = ix.list_row_start[c + 1] - ix.list_row_start[c];
        }
        s.st[ST_NLISTS] = nnz ? 1u : 0u;
      }
    } else {
      select_lists<CT, NT>(s, ix, nnz, p.query_cut);
    }
    __syncthreads();
    const uint32_t nl = s.st[ST_NLISTS];
    TICK(0);

    if (nl > 0) {
      // ---- stage 1 (per list group: row tables, then the summary dots) ----
      uint32_t budget = p.items_init;
      for (uint32_t l0 = 0; l0 < nl;) {
      // the group of lists [l0, l1) whose block dots share the LDS area (normally all of them)
      const uint32_t l1 = plan_list_group<NT>(s, l0, nl, L.dots_cap, L.qg);
      build_row_table<CT, NT>(s, ix, nnz, l0, l1, L.qn);
      TICK(1);
      summary_dots<NT, LK>(s, ix, nnz, l0, l1, L.qn, ix.dim, l0 == 0 && p.mode != MODE_DOTS);
      TICK(2);
      if (COOP) CO_TRACE(co, 7);

      if (p.mode == MODE_DOTS) {   // sgpu_summary_distances: dump the dots of list 0
        for (uint32_t i = threadIdx.x; i < s.sel_nb[0]; i += NT) qb.out_scores[i] = s.dots[i];
        if (threadIdx.x == 0) qb.out_n[q] = s.sel_nb[0];
        break;
      }

      // ---- stage 2 ----
      if (l0 == 0) build_lookup<NT, LK>(s, ix.dim, nnz);
      if constexpr (STREAM) {
        // the group's lists as ONE stream of items: control wavefront 0 (feeder + replayer), scorers 1 ..; no barrier
        // until the group is through. The speculation budget carries over from group to group.
        if (l0 == 0 && p.first_sorted && s.sel_nb[0] > 1) sort_first_list<NT>(s, s.sel_nb[0]);
        TICK(3);
        const Ring rg = carve_ring(s.uni, p.ring);
        for (uint32_t i = threadIdx.x; i < p.ring / 64u; i += NT) rg.win_done[i] = 0;
        if (threadIdx.x == 0) {
          s.st[ST_S_DONE] = 0;
          s.st[ST_S_THR] = s.st[ST_HLEN] == p.k ? s.st[ST_THR] : 0xff800000u;   // (-inf: while the heap is not full every item matters)
          s.st[ST_S_QS_TAIL] = 0;
          s.st[ST_S_QS_HEAD] = 0;
          s.st[ST_S_QL_TAIL] = 0;
          s.st[ST_S_QL_HEAD] = 0;
          s.st[ST_S_ABORT] = 0;
        }
        __syncthreads();
        uint32_t busy[6] = {0, 0, 0, 0, 0, 0};
        if (wave == 0) {
          // (the control wavefront is the serial role: it issues ahead of the scoring wavefronts on its SIMD)
          serial_prio_on();
          stream_control<KR, VT>(s, ix, qb, rg, p, l0, l1, budget, busy);
          if (lane == 0) s.st[ST_S_BUDGET] = budget;
          serial_prio_off();
        } else {
          stream_scorer<CT, NT, LK, VT>(s, ix, qb, rg, spec_docs);
        }
        __syncthreads();
        budget = s.st[ST_S_BUDGET];
        TICK(7);
#ifdef SGPU_PROF
        // (thread 0 is the control wavefront's first lane: the stream's time by what that wavefront was doing - the clocks
        // of the round loop's phases stand in: [4] skip test + tables + block lookup, [5] posting loads + filing, [6] waiting
        // for room, [7] the final replay, [8] replay of scored windows; tools/phase_profile.py names them)
        clk.prof[7] = clk.prof[7] - (clk.prof[7] < busy[0] + busy[1] + busy[2] + busy[3] ? clk.prof[7] : busy[0] + busy[1] + busy[2] + busy[3]);
        clk.prof[8] += busy[0];
        clk.prof[4] += busy[1];
        clk.prof[5] += busy[2];
        clk.prof[6] += busy[3];
        clk.prof[10] += 1;
        if (threadIdx.x == 0) s.st[ST_S_SKIPPED] += busy[5];
#endif
        l0 = l1;
        continue;
      }
      bool group_done = false;   // wide rounds took everything that was left of the group
      uint32_t resume_pos = 0;   // (cooperative variant) where local rounds pick a list up after wide rounds
      for (uint32_t l = l0; l < l1 && !group_done; ++l) {
        const uint32_t nb = s.sel_nb[l];
        const uint32_t b0 = s.sel_b0[l];
        const float* dots = s.dots + s.sel_doff[l];
        const bool sorted = (l == 0) && p.first_sorted && nb > 1;
        if (sorted && resume_pos == 0) sort_first_list<NT>(s, nb);
        TICK(3);
        uint32_t decided_blk = 0xffffffffu;   // wavefront 0 state
        uint32_t pos = resume_pos;
        resume_pos = 0;
        while (pos < nb) {
          if (COOP && !COUNTED && co.enabled && !wide_off && s.st[ST_HLEN] == p.k && s.st[ST_ITEMS_DONE] >= co.min_items) {
            // Cooperative mode: once the heap is full and a first threshold stands, everything that is left
            // of the list group goes out as ONE wide round if idle workgroups are there to take it: enough
            // of them in absolute terms and per workgroup still owning a query (the count the last replay fetched).
            if (!wide_ok) {
              const uint32_t idle = s.st[ST_CO_IDLE];
              wide_ok = idle >= co.idle_min && idle >= co.idle_ratio * (gridDim.x - idle);
            }
            if (wide_ok) {
              // a first round of limited reach (its threshold is young: every document above it comes back
              // as a candidate), then one over all that is left
              uint32_t wl = l, wpos = pos, limit = co.first_reach;
              bool ok = true;
              while (ok && wl < l1) {
                ok = wide_round<CT, NT, KR, LK, VT>(s, ix, qb, co, p, q, wl, wpos, l1, p.first_sorted && s.sel_nb[0] > 1, limit, co_seq);
                limit = 0xffffffffu;
              }
              if (ok) {
                group_done = true;
                break;
              }
              wide_off = true;   // a round came back with more candidates than fit: local rounds from where it began
              if (wl != l) {     // ... in a later list: the list loop re-enters there
                resume_pos = wpos;
                l = wl - 1;
                break;
              }
              pos = wpos;
              decided_blk = 0xffffffffu;
              if (pos >= nb) break;
            }
          }
          // (a) filter the remaining blocks against the current threshold
          const uint32_t hlen = s.st[ST_HLEN];
          // A block may be dropped here against a threshold that is older than the one the replay
          // will use only because heap_factor * threshold never decreases - true for
          // heap_factor >= 0. A negative factor prunes nothing here; the replay decides alone.
          const bool full = hlen == p.k && p.heap_factor >= 0.0f;
          const float cut = __fmul_rn(p.heap_factor, __uint_as_float(s.st[ST_THR]));
          const uint32_t remaining = nb - pos;
          uint32_t R = (remaining + NT - 1) / NT;
          if (R > p.rblocks_max) R = p.rblocks_max;
          const uint32_t scan_end = (pos + R * NT < nb) ? pos + R * NT : nb;
          uint32_t live_mask = 0;   // bit r: block my0 + r passes the skip test (R <= 32)
          const uint32_t my0 = pos + threadIdx.x * R;
          for (uint32_t r = 0; r < R; ++r) {
            const uint32_t idx = my0 + r;
            if (idx < scan_end) {
              const uint32_t b = sorted ? (uint32_t)s.order[idx] : idx;
              live_mask |= (uint32_t)!(full && dots[b] < cut) << r;
            }
          }
          const uint32_t my_live = (uint32_t)__popc(live_mask);
          uint32_t n_live_total;
          const uint32_t live_incl = wg_inclusive_scan<NT>(my_live, s.part, &n_live_total);
          if (n_live_total == 0) {
            pos = scan_end;
            __syncthreads();   // everyone is done with s.part before the next scan writes it
            TICK(4);
            continue;
          }
          {
            uint32_t o = live_incl - my_live;
            for (uint32_t m = live_mask; m && o < NT; m &= m - 1)
              cb.live_pos[o++] = (uint16_t)(my0 + (uint32_t)__ffs((int)m) - 1u);
          }
          const uint32_t n_live = n_live_total < NT ? n_live_total : NT;
          __syncthreads();
          TICK(4);
          // (cooperative variant, launch tail) thread 0 asks for the number of idle workgroups now; the
          // answer is in by the time the replay files it for the next round's decision to go wide
          uint32_t idle_fetch = 0xffffffffu;
          if (COOP && !COUNTED && co.enabled && !wide_ok && threadIdx.x == 0 && s.st[ST_CO_TAIL]) idle_fetch = co_ld32(co.counters + 0);
          // (b) postings of the live blocks, budget cut
          uint32_t cnt = 0, p0 = 0, myb = 0;
          if (threadIdx.x < n_live) {
            const uint32_t idx = cb.live_pos[threadIdx.x];
            myb = sorted ? (uint32_t)s.order[idx] : idx;
            p0 = ix.block_post_start[b0 + myb];
            cnt = ix.block_post_start[b0 + myb + 1] - p0;
          }
          uint32_t items_total;
          if (threadIdx.x == 0) {
            s.st[ST_TMP0] = cnt;   // size of the first live block
            s.st[ST_NBLK] = 0;
          }
          const uint32_t incl = wg_inclusive_scan<NT>(cnt, s.part + (NT / 64 + 1), &items_total);
          const uint32_t first_cnt = s.st[ST_TMP0];
          uint32_t B = budget;
          if (first_cnt > B) B = first_cnt;             // always make progress
          const bool oversize = first_cnt > p.items_max;
          if (B > p.items_max) B = p.items_max;
          {   // blocks taken this round: the live blocks whose inclusive item count fits the budget
            const uint64_t tk = __ballot(threadIdx.x < n_live && incl <= B);
            if (lane == 0 && tk) atomicAdd(&s.st[ST_NBLK], (uint32_t)__popcll(tk));
          }
          if (threadIdx.x < n_live) {
            cb.cb_incl[threadIdx.x] = incl;
            cb.cb_p0[threadIdx.x] = p0;
            cb.cb_blk[threadIdx.x] = (uint16_t)myb;
          }
          __syncthreads();
          uint32_t nblk = s.st[ST_NBLK];
          uint32_t next_pos;
          uint32_t n_pieces = 1, piece_items = 0;
          if (oversize) {   // one block larger than the item buffer: evaluate it in pieces
            nblk = 1;
            n_pieces = (first_cnt + p.items_max - 1) / p.items_max;
          }
          if (nblk == n_live && n_live == n_live_total) next_pos = scan_end;
          else next_pos = (uint32_t)cb.live_pos[nblk - 1] + 1;
          TICK(5);
#ifdef SGPU_PROF
          clk.prof[10] += 1;
#endif

          for (uint32_t piece = 0; piece < n_pieces; ++piece) {
            uint32_t n_items, item0 = 0;
            if (oversize) {
              item0 = piece * p.items_max;
              n_items = first_cnt - item0 < p.items_max ? first_cnt - item0 : p.items_max;
            } else {
              n_items = cb.cb_incl[nblk - 1];
            }
            piece_items = n_items;
            // (c) phase A: posting refs (thread per item; + visited bits in the counted pass)
            if (threadIdx.x == 0) {
              s.st[ST_TMP2] = 0;    // phase B's item counters
              s.st[ST_PULL_L] = 0;
              s.st[ST_NCAND] = 0;   // phase B's candidate counter
            }
            for (uint32_t ib = 0; ib < n_items; ib += NT) {
              const uint32_t i = ib + threadIdx.x;
              if (i >= n_items) {
                classify_item<VT>(s.st, cb, p.items_max, 0, 0, false);
                continue;
              }
              const uint32_t gi = i + item0;
              uint32_t lo = 0, hi = nblk;   // first block with cb_incl > gi
              while (lo < hi) {
                const uint32_t mid = (lo + hi) >> 1;
                if (cb.cb_incl[mid] <= gi) lo = mid + 1; else hi = mid;
              }
              const uint32_t excl = lo ? cb.cb_incl[lo - 1] : 0;
              const uint32_t pidx = cb.cb_p0[lo] + (gi - excl);
              const uint32_t doc = ix.post_doc[pidx];
              const uint64_t ref = ix.post_ref[pidx];
              const uint32_t vis = (COUNTED && visited_test(bitmap, doc)) ? 0x80000000u : 0u;
              cb.it_ref[i] = ref;
              cb.it_doc[i] = doc | vis;
              cb.it_blk[i] = (uint16_t)cb.cb_blk[lo];
              classify_item<VT>(s.st, cb, p.items_max, i, (uint32_t)ref, vis == 0);
            }
            __syncthreads();
            TICK(6);
            // (d) phase B: speculative scoring (score_items)
            score_items<CT, NT, LK, COUNTED, VT>(s, ix, cb, p, spec_docs);
            __syncthreads();
            TICK(7);
            // (e) exact replay on wavefront 0
            if (wave == 0) {
              // the replay is this workgroup's serial stretch (its other wavefronts wait at the barrier): it
              // issues ahead of the co-resident workgroup's scoring wavefronts on the same SIMD
              serial_prio_on();
              replay_round<KR, COUNTED>(cb, s, p, n_items, bitmap, decided_blk, piece == 0, wc, dots, LenMask<VT>::v, false, idle_fetch);
              serial_prio_off();
            }
            __syncthreads();
            TICK(8);
          }
          pos = next_pos;
          // adapt the speculation budget to how much of the last round the replay kept
          {
            const uint32_t kept = s.st[ST_TMP1];
            if (kept * 4 >= piece_items * 3) budget = budget * 2 < p.items_max ? budget * 2 : p.items_max;
            else if (kept * 2 < piece_items) budget = budget / 2 > p.items_min ? budget / 2 : p.items_min;
          }
        }
      }
      l0 = l1;
      }   // list groups
      if (p.mode == MODE_DOTS) {
        __syncthreads();
        continue;
      }

      // ---- kNN refinement (Knn::refine, reference src/inverted_index.rs:551-593): for every document
      // of the current top-k (snapshot, best first) its first n_knn graph neighbours are scored and
      // pushed unless already visited. One more round through the same scoring + replay machinery;
      // "visited" is again heap membership (or the bitmap in the counted pass).
      if (p.n_knn && ix.knn) {
        uint32_t* snap = cb.cb_incl;   // cb_incl + cb_p0 are contiguous: 2*NT words >= k
        const uint32_t hl = s.st[ST_HLEN];
        for (uint32_t e = threadIdx.x; e < hl; e += NT) snap[e] = s.heap[KR * 64 + e];
        __syncthreads();
        const uint32_t nk = p.n_knn < ix.knn_dim ? p.n_knn : ix.knn_dim;
        const uint32_t total = hl * nk;
        uint32_t decided_blk = 0xffffffffu;
        for (uint32_t base = 0; base < total; base += p.items_max) {
          const uint32_t n_items = total - base < p.items_max ? total - base : p.items_max;
          if (threadIdx.x == 0) {
            s.st[ST_TMP2] = 0;
            s.st[ST_PULL_L] = 0;
            s.st[ST_NCAND] = 0;
          }
          for (uint32_t ib = 0; ib < n_items; ib += NT) {
            const uint32_t i = ib + threadIdx.x;
            if (i >= n_items) {
              classify_item<VT>(s.st, cb, p.items_max, 0, 0, false);
              continue;
            }
            const uint32_t j = base + i;
            const uint32_t r = j / nk, t = j - r * nk;
            const uint64_t pos = (uint64_t)snap[r] * ix.knn_dim + t;
            bool ok = pos < ix.knn_total;
            const uint32_t nbr = ok ? ix.knn[pos] : 0u;
            ok = ok && nbr < ix.n_docs;
            const uint64_t ref = ok ? ix.doc_ref[nbr] : 0ull;
            const bool vis = !ok || (COUNTED && visited_test(bitmap, nbr));
            cb.it_ref[i] = ref;
            cb.it_doc[i] = nbr | (vis ? 0x80000000u : 0u);
            cb.it_blk[i] = 0;   // no block test in the refinement (replay gets dots == nullptr)
            classify_item<VT>(s.st, cb, p.items_max, i, (uint32_t)ref, !vis);
          }
          __syncthreads();
          score_items<CT, NT, LK, COUNTED, VT>(s, ix, cb, p, spec_docs);
          __syncthreads();
          if (wave == 0) replay_round<KR, COUNTED>(cb, s, p, n_items, bitmap, decided_blk, true, wc, nullptr, LenMask<VT>::v, true);
          __syncthreads();
        }
      }
    }

    // ---- results: best first (into_sorted_vec, src/inverted_index.rs:227-233) ----
    {
      float* os = qb.out_scores + (size_t)q * qb.k_stride;
      uint64_t* oi = qb.out_ids + (size_t)q * qb.k_stride;
      const uint32_t hl = s.st[ST_HLEN];
      for (uint32_t e = threadIdx.x; e < p.k; e += NT) {
        os[e] = e < hl ? __uint_as_float(s.heap[e]) : 0.0f;
        oi[e] = e < hl ? (uint64_t)s.heap[KR * 64 + e] : 0ull;   // (slots past out_n: zero, as sgpu_exact_search_device's)
      }
      if (threadIdx.x == 0) qb.out_n[q] = hl;
      if (COOP && co.enabled && qb.done) {   // (uniform) the rows of this query are in host memory before it counts as finished:
        // a SYSTEM-scope release by every storing wave (write-back of this XCD's L2 + drain). A mere drain is not enough -
        // the rows of a query and the done word of the launch's last query may leave from different XCDs, whose writes
        // to host memory are not ordered with each other (seen: rows of earlier queries missing at the done word).
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
        __syncthreads();
      }
      if (COOP && co.enabled && threadIdx.x == 0) {
        // a query is finished. With a done word to publish the add is acquire-release: the workgroup that counts the LAST
        // query acquires what every other owner released (its rows, written back at system scope above) before it stores
        // the done word at system scope - the chain the host's acquire load of that word completes (ADVICE r04).
        const uint32_t fin = (qb.done ? __hip_atomic_fetch_add(co.counters + 1, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT)
                                      : __hip_atomic_fetch_add(co.counters + 1, 1u, SGPU_RLX)) + 1u;
        // the last one: tell the host that every row of the launch is in its arena (posted writes of one device arrive in
        // order; each workgroup drained its row stores before it counted) - it need not wait for the launch to wind down
        if (qb.done && fin == qb.nq) __hip_atomic_store(qb.done, qb.done_seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
      }
      if (COOP) CO_TRACE(co, 6);
    }
    if (qb.out_stats) write_stats(s, qb, q, nl, spec_docs, wc);
    TICK(9);
    // ---- per-query cleanup: visited bitmap, query bits ----
    if (COUNTED)
      for (uint32_t i = threadIdx.x; i < ix.n_bitmap_words; i += NT) bitmap[i] = 0;
    __threadfence_block();
    __syncthreads();
    TICK(11);
    if (qb.out_stats && threadIdx.x == 0) {
      uint32_t* os = qb.out_stats + (size_t)q * STATS_WORDS + 8;
#pragma unroll
      for (int i = 0; i < 12; ++i) os[i] = clk.prof[i];
      os[12] = blockIdx.x;
#ifdef SGPU_PROF
      if (STREAM) {   // (profiling build, streamed variants) [21] polls of starved scorers [22] polls of the blocked feeder [23] spans << 16 | mean budget
        os[13] = s.st[ST_S_STARVED] | (s.st[ST_S_SKIPPED] << 20);
        os[14] = s.st[ST_S_BLOCKED];
        os[15] = (s.st[ST_S_SPANS] << 16) | (s.st[ST_S_SPANS] ? (s.st[ST_S_BUDGET_SUM] / s.st[ST_S_SPANS]) & 0xffffu : 0u);
      }
#endif
    }
  }
  if (COOP && co.enabled) {
    // the queue is empty: help the workgroups that still own a query, until every query is finished
    coop_help<CT, NT, LK, VT>(s, ix, qb, co, p);
    // The last workgroup out leaves the board as the next launch must find it (all zero): nobody else
    // touches it any more, and the next launch on the stream starts after this one has ended.
    if (threadIdx.x == 0) s.st[ST_CO_FLAG] = __hip_atomic_fetch_add(co.counters + 2, 1u, SGPU_RLX) == gridDim.x - 1 ? 1u : 0u;
    __syncthreads();
    if (s.st[ST_CO_FLAG]) {
      for (uint32_t i = threadIdx.x; i < gridDim.x * (uint32_t)kCoopSlotWords; i += NT) co_st64(co.slots + i, 0ull);
      if (threadIdx.x < 8) co_st64(co.open + threadIdx.x, 0ull);
      if (threadIdx.x < 3) __hip_atomic_store(co.counters + threadIdx.x, 0u, SGPU_RLX);   // ([3]: the sticky protocol-error flag)
    }
  }
}

// ---------------------------------------------------------------------------
// launcher of one kernel family (component type x lookup layout); instantiated by sk_*.hip, one
// translation unit per family so that the 20 variants of each compile in parallel
// ---------------------------------------------------------------------------
template <typename CT, int NT, int KR, int LK, bool COUNTED, int VT, bool COOP, bool STREAM = false>
static hipError_t run_one(const LaunchArgs& a, int* occupancy) {
  auto kern = seismic_search_kernel<CT, NT, KR, LK, COUNTED, VT, COOP, STREAM>;
  hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)a.lds_bytes);
  if (e != hipSuccess) return e;
  if (occupancy) {   // (once per variant and LDS size: the answer is cached by the caller)
    // kernel_has_no_static_lds: the scaled-byte dense lookup reads the weights at LDS address = byte, i.e. it needs the
    // dynamic LDS to start at LDS address 0 (kQscOffset). A static __shared__ object added to the kernel would move it.
    hipFuncAttributes fa;
    e = hipFuncGetAttributes(&fa, (const void*)kern);
    if (e != hipSuccess) return e;
    if (LK == LK_DENSE && fa.sharedSizeBytes != 0) {
      std::fprintf(stderr, "sgpu: the search kernel has %zu bytes of static LDS; the scaled-byte dense lookup needs none\n", (size_t)fa.sharedSizeBytes);
      return hipErrorInvalidConfiguration;
    }
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(occupancy, kern, NT, a.lds_bytes);
  }
  (void)hipGetLastError();   // (this launch is judged alone: an earlier failed call of the thread leaves its error behind)
  if constexpr (COOP)
    hipLaunchKernelGGL(kern, dim3(a.grid), dim3(NT), a.lds_bytes, a.stream, a.ix, a.qb, a.p, a.L, a.queue, a.bitmaps,
                       a.coop);
  else
    hipLaunchKernelGGL(kern, dim3(a.grid), dim3(NT), a.lds_bytes, a.stream, a.ix, a.qb, a.p, a.L, a.queue, a.bitmaps,
                       typename CoopArg<false>::type{});
  return hipGetLastError();
}

// The variants a family instantiates (device_types.hpp: variant_built - 17 per family since r05, 30 before): every heap
// size for 512-thread workgroups, plain and counted; k <= 128 for the 1024-thread workgroups of small launches; the
// cooperative variant up to k = 256. configure() only ever asks for one of these.
template <typename CT, int NT, int LK, bool COUNTED, int VT, bool COOP, int KR_MAX, bool STREAM = false>
static hipError_t run_kr(const LaunchArgs& a, int* occ) {
  const uint32_t kr = heap_variant(a.p.k);
  if (kr == 1) return run_one<CT, NT, 1, LK, COUNTED, VT, COOP, STREAM>(a, occ);
  if (kr == 2) return run_one<CT, NT, 2, LK, COUNTED, VT, COOP, STREAM>(a, occ);
  if constexpr (KR_MAX >= 4)
    if (kr == 4) return run_one<CT, NT, 4, LK, COUNTED, VT, COOP, STREAM>(a, occ);
  if constexpr (KR_MAX >= 16) {
    if (kr == 8) return run_one<CT, NT, 8, LK, COUNTED, VT, COOP, STREAM>(a, occ);
    if (kr == 16) return run_one<CT, NT, 16, LK, COUNTED, VT, COOP, STREAM>(a, occ);
  }
  return hipErrorInvalidConfiguration;   // (not built: configure() checks variant_built first)
}

template <typename CT, int LK, int VT>
static hipError_t run_family(const LaunchArgs& a, int* occ) {
  if (!variant_built(a.block, heap_variant(a.p.k), a.counted != 0, a.coop.enabled != 0, a.streamed != 0)) return hipErrorInvalidConfiguration;
  if (a.streamed) return a.block == 1024 ? run_kr<CT, 1024, LK, false, VT, false, 2, true>(a, occ) : run_kr<CT, 512, LK, false, VT, false, 16, true>(a, occ);
  if (a.counted) return run_kr<CT, 512, LK, true, VT, false, 16>(a, occ);
  if (a.coop.enabled) return a.block == 1024 ? run_kr<CT, 1024, LK, false, VT, true, 2>(a, occ) : run_kr<CT, 512, LK, false, VT, true, 4>(a, occ);
  return a.block == 1024 ? run_kr<CT, 1024, LK, false, VT, false, 2>(a, occ) : run_kr<CT, 512, LK, false, VT, false, 16>(a, occ);
}

}  // namespace sgpu
