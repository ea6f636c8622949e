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
//            out of a ring in LDS - see "stage 2 as a stream" below. The counted pass and the cooperative variant keep the rounds.)
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
#ifndef SGPU_ROWTAB2
#define SGPU_ROWTAB2 1   // stage 1's row directory: two (list, component) pairs per quad and trip (r06)
#endif
#ifndef SGPU_WAVES_PER_EU
#define SGPU_WAVES_PER_EU 4   // 2 workgroups of 512 threads per CU (<= 128 VGPRs)
#endif

// ---------------------------------------------------------------------------
// small helpers
// ---------------------------------------------------------------------------
SGPU_DEV int32_t total_key_dev(float f) {  // Rust f32::total_cmp order
  int32_t b = __float_as_int(f);
  b ^= (int32_t)(((uint32_t)(b >> 31)) >> 1);
  return b;
}

// q * (float)half(packed, hi) with ONE rounding, the product the reference computes after widening
// the stored f16: v_fma_mix_f32 widens the selected half on the fly and adds -0.0, which leaves the
// rounded product untouched, signed zeros and denormals included (tools/ubench/fma_mix_check.hip:
// bit-identical to v_cvt_f32_f16 + v_mul_f32). One instruction instead of convert (+ shift) + multiply.
SGPU_DEV float mul_f32_f16(float q, uint32_t packed, int hi) {
  float r;
  if (hi)
    asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel:[0,1,0] op_sel_hi:[0,1,0]" : "=v"(r) : "v"(q), "v"(packed), "s"(0x80000000u));
  else
    asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel:[0,0,0] op_sel_hi:[0,1,0]" : "=v"(r) : "v"(q), "v"(packed), "s"(0x80000000u));
  return r;
}

SGPU_DEV uint32_t lane_id() { return __lane_id(); }
// device_types.hpp: hash_slot, as two full-rate VALU operations (v_mul_u32_u24, v_lshrrev_b32)
SGPU_DEV uint32_t hash_slot_dev(uint32_t c, uint32_t mult) { return (uint32_t)__umul24(c, mult) >> (32 - kHashBits); }   // (HIP declares __umul24 as returning int)

// value of `v` in lane `l`, l wave-uniform (v_readlane_b32; no LDS round trip)
SGPU_DEV uint32_t readlane_u(uint32_t v, uint32_t l) {
  return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)__builtin_amdgcn_readfirstlane((int)l));
}
SGPU_DEV float readlane_f(float v, uint32_t l) { return __uint_as_float(readlane_u(__float_as_uint(v), l)); }
// lane i receives lane i-1's value, lane 0 keeps its own (DPP wave_shr:1)
SGPU_DEV uint32_t shift_up1_u(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x138, 0xf, 0xf, false);
}
SGPU_DEV float shift_up1_f(float v) { return __uint_as_float(shift_up1_u(__float_as_uint(v))); }

// inclusive scan of one u32 per thread over the whole workgroup.
// `part` points to NT/64 + 1 LDS words. Returns inclusive prefix; *total = sum.
// Inclusive prefix sum over the 64 lanes: four row shifts inside each row of 16, then the row
// totals carried with row_bcast:15 / row_bcast:31 (lanes without a source add 0).
#define SGPU_DPP0(x, ctrl, rows) ((uint32_t)__builtin_amdgcn_update_dpp(0, (int)(x), ctrl, rows, 0xf, false))
SGPU_DEV uint32_t wave_inclusive_scan(uint32_t x) {
  x += SGPU_DPP0(x, 0x111, 0xf);   // row_shr:1
  x += SGPU_DPP0(x, 0x112, 0xf);   // row_shr:2
  x += SGPU_DPP0(x, 0x114, 0xf);   // row_shr:4
  x += SGPU_DPP0(x, 0x118, 0xf);   // row_shr:8
  x += SGPU_DPP0(x, 0x142, 0xa);   // row_bcast:15 into rows 1 and 3
  x += SGPU_DPP0(x, 0x143, 0xc);   // row_bcast:31 into rows 2 and 3
  return x;
}

// the same over max (values >= 0: lanes without a source contribute 0)
SGPU_DEV uint32_t wave_inclusive_max(uint32_t x) {
  uint32_t y;
  y = SGPU_DPP0(x, 0x111, 0xf); x = x > y ? x : y;
  y = SGPU_DPP0(x, 0x112, 0xf); x = x > y ? x : y;
  y = SGPU_DPP0(x, 0x114, 0xf); x = x > y ? x : y;
  y = SGPU_DPP0(x, 0x118, 0xf); x = x > y ? x : y;
  y = SGPU_DPP0(x, 0x142, 0xa); x = x > y ? x : y;
  y = SGPU_DPP0(x, 0x143, 0xc); x = x > y ? x : y;
  return x;
}

// One barrier: the caller guarantees that every thread is past its reads of `part` from the previous
// scan that used it (another barrier lies in between).
template <int NT>
SGPU_DEV uint32_t wg_inclusive_scan(uint32_t v, uint32_t* part, uint32_t* total) {
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t x = wave_inclusive_scan(v);
  if (lane == 63) part[wave] = x;
  __syncthreads();
  uint32_t base = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < NT / 64; ++w) {
    const uint32_t pw = part[w];
    if ((uint32_t)w < wave) base += pw;
    tot += pw;
  }
  *total = tot;
  return x + base;
}

// ---------------------------------------------------------------------------
// LDS view
// ---------------------------------------------------------------------------
struct Lds {
  uint32_t* q_comp;
  float* q_val;
  float* q_sc;          // the weights the scoring loop multiplies with: q_val itself (f16 documents), or
                        // q_val * val_scale in its own area (fixed-u8 documents: the codes are then used as they are)
  uint2* q_word;        // bitmap mode: [ceil(dim/32)] {32 vocabulary bits, rank of the word's first query component}
  uint8_t* q_idx;       // dense mode (same LDS region): [dim] 1 + rank of the component in the query, 0 = absent
  uint32_t* q_bits32;   // split mode (same region): [ceil(dim/32)] bits, followed by
  uint16_t* q_rank16;   //   [ceil(dim/32)] rank of the word's first query component
  uint2* q_ent;         // hash mode (same region as q_idx): [kHashSlots] {component id, weight bits}, empty = {0xffffffff, 0}
  uint32_t* sel_comp;   // [QC] list (component) ids in traversal order
  uint32_t* sel_nb;     // [QC] blocks in the list
  uint32_t* sel_b0;     // [QC] first global block id
  uint32_t* sel_doff;   // [QC+1] offset of the list's dots in `dots`
  uint32_t* sel_r0;     // [QC] first global summary row
  uint32_t* sel_nr;     // [QC] number of summary rows
  uint64_t* rt_start;   // [QC*QN] global entry index of matched row (l, j) (64-bit: > 4 G summary entries)
  uint16_t* rt_mid;     // [QC*QN] split of the row between the list's two block-id halves
  uint32_t* rt_pre;     // [2*QC*(QN+1)] per (list, half): prefix of the rows' 64-entry chunk counts
  float* dots;
  uint16_t* order;
  uint8_t* lookup;      // start of the query lookup table (whichever layout)
  uint8_t* uni;         // union region
  uint32_t* part;       // scan partials [NT/64 + 1]
  uint32_t* heap;       // the top-k between replays: [KR*64] scores, [KR*64] documents
  uint32_t* st;         // state words
  uint32_t idx0;        // LDS byte address of q_idx[0] (VT_DVB + dense lookup: the decoded "components" are table addresses)
};
enum { ST_Q = 0, ST_NLISTS = 1, ST_THR = 2, ST_HLEN = 3, ST_TMP0 = 4, ST_TMP1 = 5, ST_TMP2 = 6, ST_NCAND = 7,
       ST_CAND = 8 /* 64 candidate item indices */, ST_CAND_SORTED = 72 /* 64 */, ST_NSHORT = 136, ST_NLONG = 137,
       ST_PULL_L = 138, ST_NBLK = 139, ST_ENTRIES = 140, ST_ROWS = 141, ST_HMULT = 142,
       // cooperative mode (CoopView)
       ST_ITEMS_DONE = 143 /* items replayed locally for this query */, ST_CO_SLOT = 144, ST_CO_CLAIM_LO = 145,
       ST_CO_CLAIM_HI = 146, ST_CO_NLIVE = 147, ST_CO_THR0 = 148, ST_CO_CUT = 149, ST_CO_QUERY = 150, ST_CO_FLAG = 151,
       ST_CO_NCAND = 152, ST_CO_TAIL = 153, ST_CO_IDLE = 154,
       // dense lookup: 1 = the table in LDS holds SCALED bytes (4 * (1 + rank): the query has <= kScaledMaxNnz components)
       ST_SCALED = 157 };
static_assert(ST_SCALED < kStateWords, "state words");
// Dense lookup table, scaled bytes (r04). The byte of a vocabulary id is 1 + its rank in the query, and the scoring
// loop turns it into the address of the weight with a shift-and-add per document component. A query of at most 63
// components - 98 % of a SPLADE-shaped query stream - can store 4 * (1 + rank) instead: the byte then IS the weight's
// offset from the 0.0 slot, which the host keeps at the start of the dynamic LDS (LdsLayout::q_sc == 0) - LDS address 0,
// the kernel has no static LDS - so the byte is the address: one VALU operation less
// per document component (fixed-u8 documents: 5.57 -> 5.45 ms per 10 000-query launch; f16 documents, bound by
// memory: -0.4 %). Chosen per query (ST_SCALED); both forms of the scoring loops are in the kernel.
constexpr uint32_t kScaledMaxNnz = 63;
constexpr uint32_t kMaxCand = 64;

SGPU_DEV Lds carve(uint8_t* smem, const LdsLayout& L) {
  Lds l;
  l.q_comp = (uint32_t*)(smem + L.q_comp);
  l.q_val = (float*)(smem + L.q_val) + 1;   // q_val[-1] is the 0.0 every non-matching component resolves to
  l.q_sc = (float*)(smem + L.q_sc) + 1;
  l.q_word = (uint2*)(smem + L.q_bits);
  l.q_idx = smem + L.q_bits;
  l.q_bits32 = (uint32_t*)(smem + L.q_bits);
  l.q_rank16 = (uint16_t*)(smem + L.q_rank);
  l.q_ent = (uint2*)(smem + L.q_bits);
  l.sel_comp = (uint32_t*)(smem + L.sel);
  l.sel_nb = l.sel_comp + L.qc;
  l.sel_b0 = l.sel_nb + L.qc;
  l.sel_doff = l.sel_b0 + L.qc;          // qc + 1
  l.sel_r0 = l.sel_doff + L.qc + 1;
  l.sel_nr = l.sel_r0 + L.qc;
  l.rt_start = (uint64_t*)(smem + L.rt_start);
  l.rt_mid = (uint16_t*)(smem + L.rt_mid);
  l.rt_pre = (uint32_t*)(smem + L.rt_pre);
  l.dots = (float*)(smem + L.dots);
  l.order = (uint16_t*)(smem + L.order);
  l.lookup = smem + L.q_bits;
  l.uni = smem + L.uni;
  l.part = (uint32_t*)(smem + L.part);
  l.heap = (uint32_t*)(smem + L.heap);
  l.st = (uint32_t*)(smem + L.st);
  l.idx0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint8_t*)(smem + L.q_bits);
  return l;
}

// ---------------------------------------------------------------------------
// stage 0: query into LDS, choose the lists
// ---------------------------------------------------------------------------
template <int NT>
SGPU_DEV void load_query(const Lds& s, const BatchView& qb, uint32_t q, uint32_t* nnz_out) {
  const uint32_t o0 = qb.q_off[q], o1 = qb.q_off[q + 1];
  const uint32_t nnz = o1 - o0;
  for (uint32_t j = threadIdx.x; j < nnz; j += NT) {
    s.q_comp[j] = qb.q_comp[o0 + j];
    s.q_val[j] = qb.q_val[o0 + j];
  }
  *nnz_out = nnz;
}

// Query lookup table layouts (device_types.hpp: LK_*).
// Fills the query lookup table used by the scoring loop (cleared during stage 1, lookup_clear).
//   dense : one byte per vocabulary id: 1 + rank of the id in the query, 0 = absent
//   bitmap: {32 vocabulary bits, rank of the word's first query component} per 32 ids
template <int NT, int LK>
SGPU_DEV void build_lookup(const Lds& s, uint32_t dim, uint32_t nnz) {
  const uint32_t hm = LK == LK_HASH ? s.st[ST_HMULT] : 1u;   // the query's hash multiplier (host-chosen, collision-free)
  const bool scaled = LK == LK_DENSE && nnz <= kScaledMaxNnz;
  if (LK == LK_DENSE && threadIdx.x == 0) s.st[ST_SCALED] = scaled ? 1u : 0u;   // (read after the barrier below)
  for (uint32_t j = threadIdx.x; j < nnz; j += NT) {
    const uint32_t c = s.q_comp[j];
    if (LK == LK_HASH) {   // the host chose hm so that the query's components fall into distinct slots
      s.q_ent[hash_slot_dev(c, hm)] = make_uint2(c, __float_as_uint(s.q_sc[j]));
    } else if (LK == LK_DENSE) {
      s.q_idx[c] = (uint8_t)(scaled ? 4u * (j + 1) : j + 1);   // (scaled: the weight's byte offset from the 0.0 slot)
    } else if (LK == LK_PACKED) {
      atomicOr(&s.q_word[c >> 5].x, 1u << (c & 31));
      if (j == 0 || (s.q_comp[j - 1] >> 5) != (c >> 5)) s.q_word[c >> 5].y = j;
    } else {   // split: 32 bits + a 16-bit rank per 32 ids (large vocabularies: 6 B instead of 8 B)
      atomicOr(&s.q_bits32[c >> 5], 1u << (c & 31));
      if (j == 0 || (s.q_comp[j - 1] >> 5) != (c >> 5)) s.q_rank16[c >> 5] = (uint16_t)j;
    }
  }
  __syncthreads();
}

// k_largest_by(query_cut, total_cmp) in descending order; ties: ascending component.
template <typename CT, int NT>
SGPU_DEV void select_lists(const Lds& s, const DevView& ix, uint32_t nnz, uint32_t query_cut) {
  const uint32_t nl = nnz < query_cut ? nnz : query_cut;
  for (uint32_t j = threadIdx.x; j < nnz; j += NT) {
    const int32_t kj = total_key_dev(s.q_val[j]);
    uint32_t rank = 0;
    for (uint32_t i = 0; i < nnz; ++i) {
      const int32_t ki = total_key_dev(s.q_val[i]);
      rank += (ki > kj) || (ki == kj && i < j);   // i < j  <=>  smaller component id
    }
    if (rank < nl) {
      const uint32_t c = s.q_comp[j];
      const uint32_t b0 = ix.list_block_start[c], b1 = ix.list_block_start[c + 1];
      uint32_t r0 = 0, r1 = 0;   // (the list's summary rows: only the u32 kernels search them; u16: the row directory)
      if constexpr (sizeof(CT) != 2) {
        r0 = ix.list_row_start[c];
        r1 = ix.list_row_start[c + 1];
      }
      s.sel_comp[rank] = c;
      s.sel_b0[rank] = b0;
      s.sel_nb[rank] = b1 - b0;
      s.sel_r0[rank] = r0;
      s.sel_nr[rank] = r1 - r0;
    }
  }
  if (threadIdx.x == 0) s.st[ST_NLISTS] = nl;
}

// ---------------------------------------------------------------------------
// stage 1: summary dots
// ---------------------------------------------------------------------------
template <typename CT, int NT>
SGPU_DEV void build_row_table(const Lds& s, const DevView& ix, uint32_t nnz, uint32_t l0, uint32_t l1, uint32_t qn) {
  // the row tables of the list group [l0, l1): slot (l - l0) of the rt_* arrays (they hold LdsLayout::qg lists)
  const uint32_t ng = l1 - l0;
  // u16 components: the hashed row directory - every u16 index has one (device_index.hip), so these kernels carry no
  // search and never touch row_comp / list_row_start / row_ptr / row_mid (not even uploaded for them). u32 components:
  // one (list, query component) pair per thread, a binary search of the list's sorted row components.
  if constexpr (sizeof(CT) == 2) {
    // Hashed row directory (r05, DevView::row_dir): FOUR lanes per (list, query component) pair read the four entries of
    // the key's bucket - one 64-byte line, one trip - and the lane that holds the key files the row; a bucket with an
    // empty slot and no hit means the component has no row in this list; a full bucket without the key (rare: the
    // table is at most half full) sends the quad to the next bucket. The lanes of a quad stay together (their loop
    // condition is the quad's ballot).
    const uint32_t q4 = threadIdx.x & 3u;
    const uint4* dir = ix.row_dir;
    const uint32_t n_buckets = ix.row_dir_buckets;
#if SGPU_ROWTAB2
    // (r06: TWO pairs per quad and trip - the buckets of both are requested before either is looked at; a query of 43
    // components over 4 lists has 172 pairs, 128 quads: the second pass used to be a second trip to HBM)
    const uint32_t n_pairs = ng * nnz;
    for (uint32_t t0 = threadIdx.x >> 2; t0 < n_pairs; t0 += NT / 2) {
     uint32_t keyv[2], bv[2];
     uint4 ev[2];
#pragma unroll
     for (int h = 0; h < 2; ++h) {
       const uint32_t t = t0 + (uint32_t)h * (NT / 4);
       const uint32_t tt = t < n_pairs ? t : t0;
       const uint32_t g = tt / nnz, j = tt - g * nnz;
       keyv[h] = (s.sel_comp[l0 + g] << 16) | s.q_comp[j];
       bv[h] = row_dir_bucket(keyv[h], n_buckets);
       ev[h] = dir[(size_t)bv[h] * 4u + q4];
     }
#pragma unroll
     for (int h = 0; h < 2; ++h) {
      const uint32_t t = t0 + (uint32_t)h * (NT / 4);
      if (t >= n_pairs) continue;   // (whole quads)
      const uint32_t g = t / nnz, j = t - g * nnz;
      const uint32_t key = keyv[h];
      uint32_t b = bv[h];
      uint4 e = ev[h];
      uint32_t hits;
      for (;;) {
        const uint32_t shift = lane_id() & ~3u;
        hits = (uint32_t)(__ballot(e.x == key) >> shift) & 15u;
        const uint32_t empties = (uint32_t)(__ballot(e.x == (uint32_t)kRowDirEmpty) >> shift) & 15u;
        if (hits | empties) break;
        b = b + 1u == n_buckets ? 0u : b + 1u;
        e = dir[(size_t)b * 4u + q4];
      }
#else
    for (uint32_t t = threadIdx.x >> 2; t < ng * nnz; t += NT / 4) {
     {
      const uint32_t g = t / nnz, j = t - g * nnz, l = l0 + g;
      const uint32_t key = (s.sel_comp[l] << 16) | s.q_comp[j];
      uint32_t b = row_dir_bucket(key, n_buckets);
      uint4 e;
      uint32_t hits;
      for (;;) {
        e = dir[(size_t)b * 4u + q4];
        const uint32_t shift = lane_id() & ~3u;
        hits = (uint32_t)(__ballot(e.x == key) >> shift) & 15u;
        const uint32_t empties = (uint32_t)(__ballot(e.x == (uint32_t)kRowDirEmpty) >> shift) & 15u;
        if (hits | empties) break;
        b = b + 1u == n_buckets ? 0u : b + 1u;
      }
#endif
      if (e.x == key) {   // (exactly one lane of the quad, if any)
        const uint32_t len = e.z >> 16, mid = e.w & 0xffffu;
        const uint64_t start = ((uint64_t)(e.z & 0xffffu) << 32) | e.y;
        if (len) {   // work counters (entries, matched rows)
          atomicAdd(&s.st[ST_ENTRIES], len);
          atomicAdd(&s.st[ST_ROWS], 1u);
        }
        s.rt_start[g * qn + j] = (start << 16) | (uint64_t)len;
        s.rt_mid[g * qn + j] = (uint16_t)mid;
        s.rt_pre[(2 * g) * (qn + 1) + j + 1] = (mid + 63u) >> 6;
        s.rt_pre[(2 * g + 1) * (qn + 1) + j + 1] = (len - mid + 63u) >> 6;
      } else if (hits == 0 && q4 == 0) {   // no row for this component in this list
        s.rt_start[g * qn + j] = 0ull;
        s.rt_mid[g * qn + j] = 0;
        s.rt_pre[(2 * g) * (qn + 1) + j + 1] = 0;
        s.rt_pre[(2 * g + 1) * (qn + 1) + j + 1] = 0;
      }
     }
    }
  } else {
  const CT* row_comp = (const CT*)ix.row_comp;
  for (uint32_t t = threadIdx.x; t < ng * nnz; t += NT) {
    const uint32_t g = t / nnz, j = t - g * nnz, l = l0 + g;
    const uint32_t target = s.q_comp[j];
    uint32_t lo = s.sel_r0[l], hi = lo + s.sel_nr[l];
    while (lo < hi) {
      const uint32_t mid = (lo + hi) >> 1;
      const uint32_t c = (uint32_t)row_comp[mid];
      if (c < target) lo = mid + 1; else hi = mid;
    }
    uint64_t start = 0;
    uint32_t len = 0, mid = 0;
    if (lo < s.sel_r0[l] + s.sel_nr[l] && (uint32_t)row_comp[lo] == target) {
      start = ix.row_ptr[lo];
      len = (uint32_t)(ix.row_ptr[lo + 1] - start);
      mid = ix.row_mid[lo];
    }
    if (len) {   // work counters (entries, matched rows)
      atomicAdd(&s.st[ST_ENTRIES], len);
      atomicAdd(&s.st[ST_ROWS], 1u);
    }
    s.rt_start[g * qn + j] = (start << 16) | (uint64_t)len;   // a row has at most one entry per block: len <= 65535
    s.rt_mid[g * qn + j] = (uint16_t)mid;
    // 64-entry chunks of the two halves [0, mid) and [mid, len); turned into prefixes below
    s.rt_pre[(2 * g) * (qn + 1) + j + 1] = (mid + 63u) >> 6;
    s.rt_pre[(2 * g + 1) * (qn + 1) + j + 1] = (len - mid + 63u) >> 6;
  }
  }
  __syncthreads();
  // per-stream prefix over the query components (wave w handles streams w, w+NW, ...)
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (uint32_t l = wave; l < 2 * ng; l += NT / 64) {
    uint32_t* pre = s.rt_pre + l * (qn + 1);
    uint32_t carry = 0;
    for (uint32_t j0 = 0; j0 < nnz; j0 += 64) {
      const uint32_t j = j0 + lane;
      const uint32_t x = wave_inclusive_scan(j < nnz ? pre[j + 1] : 0);
      if (j < nnz) pre[j + 1] = x + carry;
      carry += readlane_u(x, 63);
    }
    if (lane == 0) pre[0] = 0;
  }
  __syncthreads();
}

// Lists are processed in GROUPS whose block dots fit the LDS area together (all of a query's lists
// at once at the benchmark configurations; one or two lists at a time when lists have thousands of
// blocks, e.g. docs/Guidelines.md:44-70 with query_cut 10). Returns the end of the group that
// starts at list l0 and lays out the group's dots; a group always holds at least one list (the host
// sized the area for the largest list of the batch) and at most `qg` (the row tables of stage 1 are sized
// for that many: with query_cut 16 the tables of ALL lists - 29 KB at 96 query components - cost the second
// workgroup per CU, r04).
template <int NT>
SGPU_DEV uint32_t plan_list_group(const Lds& s, uint32_t l0, uint32_t nl, uint32_t dots_cap, uint32_t qg) {
  if (threadIdx.x == 0) {
    uint32_t o = 0, l = l0;
    while (l < nl && (l == l0 || (o + s.sel_nb[l] <= dots_cap && l - l0 < qg))) {
      s.sel_doff[l] = o;
      o += s.sel_nb[l];
      ++l;
    }
    s.sel_doff[l] = o;
    s.st[ST_TMP0] = l;
  }
  __syncthreads();
  return s.st[ST_TMP0];
}

// QuantizedSummary::distances for lists [0, nl): one wavefront per list streams the list's matched
// rows in ascending query-component order, 64 entries (one chunk of one row) per step:
//     acc[block] += (code * quant + min) * query_weight          (src/quantized_summary.rs:96-108)
// `code * quant + min` is computed once at upload with the reference's roundings (sum_deq); the
// product and the addition are separately rounded (no FMA). Block ids are distinct within a row,
// so the lanes of a step never collide, and a wavefront's LDS operations execute in issue order,
// so every accumulator sees its additions in ascending component order - the reference's order,
// bit for bit. The (block id, value) loads of the next kDepth steps are in flight while a step
// accumulates, so the HBM latency is paid once per list rather than once per row.
// Wavefronts without a list clear the query lookup table meanwhile (lookup_clear).
template <int LK>
SGPU_DEV void lookup_clear(const Lds& s, uint32_t dim, uint32_t tid, uint32_t nthreads) {
  uint32_t* z = (uint32_t*)s.lookup;
  const uint32_t words = dim / 32 + 1;   // one past the last id: the word of the padding sentinel `dim`
  if (LK == LK_HASH) {   // every slot empty: {0xffffffff (matches no component), 0.0}
    uint2* e = (uint2*)s.lookup;
    for (uint32_t i = tid; i < (uint32_t)kHashSlots; i += nthreads) e[i] = make_uint2(0xffffffffu, 0u);
    return;
  }
  const uint32_t nz = LK == LK_DENSE ? (dim + 1 + 3) / 4 : (LK == LK_PACKED ? 2 * words : words);   // split: bits only
  for (uint32_t i = tid; i < nz; i += nthreads) z[i] = 0;
}

#ifndef SGPU_STREAM_DEPTH
#define SGPU_STREAM_DEPTH 16
#endif

SGPU_DEV uint32_t uniform_u(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

SGPU_DEV void stream_list_dots(const Lds& s, const DevView& ix, uint32_t nnz_, uint32_t qn, uint32_t sl_, uint32_t l0_) {
  constexpr int kDepth = SGPU_STREAM_DEPTH;
  const uint32_t lane = lane_id();
  // wave-uniform values, pinned to scalar registers so that the step bookkeeping runs on the SALU
  // stream sl = (list l, half h): the entries of l's rows whose block id lies in l's lower (h = 0) or
  // upper (h = 1) half. The two streams of a list touch disjoint accumulators.
  // (sl counts the streams of the list GROUP that starts at list l0: the row tables hold the group's lists)
  const uint32_t nnz = uniform_u(nnz_), sl = uniform_u(sl_), g = sl >> 1, h = sl & 1u, l = uniform_u(l0_) + g;
  float* acc = s.dots + s.sel_doff[l];
  const uint64_t* rts = s.rt_start + g * qn;
  const uint16_t* mids = s.rt_mid + g * qn;
  const uint32_t* cpre = s.rt_pre + sl * (qn + 1);
  for (uint32_t jb = 0; jb < nnz; jb += 64) {   // rows in blocks of 64: lane i keeps row jb + i
    const uint32_t nj = nnz - jb < 64u ? nnz - jb : 64u;
    const bool has = lane < nj;
    uint64_t r = 0ull;
    if (has) {   // this half of the row: (first entry) << 16 | entries
      const uint64_t full = rts[jb + lane];
      const uint32_t len = (uint32_t)full & 0xffffu, mid = mids[jb + lane];
      r = h ? ((((full >> 16) + mid) << 16) | (uint64_t)(len - mid)) : (((full >> 16) << 16) | (uint64_t)mid);
    }
    const uint32_t r_lo = (uint32_t)r, r_hi = (uint32_t)(r >> 32);
    const uint32_t c0 = cpre[jb + (has ? lane : nj)];   // first chunk of the row; lanes >= nj hold the block's end
    const float w = has ? s.q_val[jb + lane] : 0.0f;
    const uint32_t t_begin = readlane_u(c0, 0);
    const uint32_t t_end = uniform_u(cpre[jb + nj]);
    for (uint32_t tb = t_begin; tb < t_end; tb += 64) {   // chunks in blocks of 64: lane i describes chunk tb + i
      const uint32_t cnt = t_end - tb < 64u ? t_end - tb : 64u;
      uint32_t d_lo, d_hn;
      float d_q;
      {
        const uint32_t x = tb + lane;
        uint32_t lo = 0, hi = 64;   // the row owning chunk x: the last j with c0[j] <= x
#pragma unroll
        for (int it = 0; it < 6; ++it) {
          const uint32_t mid = (lo + hi) >> 1;
          if ((uint32_t)__shfl((int)c0, (int)mid) <= x) lo = mid; else hi = mid;
        }
        const uint32_t rl = (uint32_t)__shfl((int)r_lo, (int)lo), rh = (uint32_t)__shfl((int)r_hi, (int)lo);
        const uint32_t u = x - (uint32_t)__shfl((int)c0, (int)lo);
        const uint32_t len = rl & 0xffffu;
        const uint64_t g = ((((uint64_t)rh << 32) | rl) >> 16) + (uint64_t)u * 64u;
        uint32_t n = len - u * 64u;
        n = n < 64u ? n : 64u;
        if (lane >= cnt) n = 0;
        d_lo = (uint32_t)g;
        d_hn = (uint32_t)(g >> 32) | (n << 16);   // entry offsets are below 2^48
        d_q = __shfl(w, (int)lo);
      }
      uint32_t bid[kDepth];
      float prod[kDepth];
      bool ok[kDepth];
      auto fetch = [&](uint32_t i, int d) {
        ok[d] = false;
        bid[d] = 0;
        prod[d] = 0.0f;
        if (i < cnt) {
          const uint32_t hn = readlane_u(d_hn, i);
          const uint64_t g = ((((uint64_t)(hn & 0xffffu)) << 32) | readlane_u(d_lo, i)) + lane;
          ok[d] = lane < (hn >> 16);
          if (ok[d]) {
            bid[d] = (uint32_t)ix.sum_bid[g];
            prod[d] = ix.sum_deq[g];   // multiplied by the row's query weight when consumed
          }
        }
      };
#pragma unroll
      for (int d = 0; d < kDepth; ++d) fetch((uint32_t)d, d);
      for (uint32_t i = 0; i < cnt; i += kDepth) {
#pragma unroll
        for (int d = 0; d < kDepth; ++d) {
          // (a return-less LDS float add, ds_add_f32, rounds identically - tools/ubench/lds_fadd_check.hip -
          // but costs ~350 cycles per wavefront instruction against ~100 for this read-add-write;
          // sending the idle lanes to a spare accumulator instead of branching is slower still)
          // (r06, measured once more with the co-resident workgroup's scoring load on the LDS: the return-less add is 5 % / 9 %
          // slower per 10 000-query launch on the headline / clustered collection, profiles/r06_kernel_experiments.txt)
          if (ok[d]) acc[bid[d]] = __fadd_rn(acc[bid[d]], __fmul_rn(prod[d], readlane_f(d_q, i + (uint32_t)d)));
          fetch(i + (uint32_t)d + kDepth, d);
        }
      }
    }
  }
}

template <int NT, int LK>
SGPU_DEV void summary_dots(const Lds& s, const DevView& ix, uint32_t nnz, uint32_t l0, uint32_t l1, uint32_t qn,
                           uint32_t dim, bool want_lookup) {
  const uint32_t wave = threadIdx.x >> 6;
  constexpr uint32_t NW = NT / 64;
  const uint32_t total_blocks = s.sel_doff[l1];
  for (uint32_t i = threadIdx.x; i < total_blocks; i += NT) s.dots[i] = 0.0f;
  __syncthreads();
  const uint32_t ns = 2 * (l1 - l0);         // streams: two block-id halves per list of the group
  const uint32_t busy = ns < NW ? ns : NW;   // wavefronts that own a stream
  if (wave < busy) {
    for (uint32_t sl = wave; sl < ns; sl += NW) stream_list_dots(s, ix, nnz, qn, sl, l0);
  } else if (want_lookup) {
    lookup_clear<LK>(s, dim, threadIdx.x - busy * 64u, NT - busy * 64u);
  }
  __syncthreads();
  if (want_lookup && busy == NW) {
    lookup_clear<LK>(s, dim, threadIdx.x, NT);
    __syncthreads();
  }
}

// descending sort of list 0's blocks by (total_cmp(dot) desc, block id asc) -> s.order
template <int NT>
SGPU_DEV void sort_first_list(const Lds& s, uint32_t nb) {
  uint64_t* keys = (uint64_t*)s.uni;
  uint32_t n2 = 1;
  while (n2 < nb) n2 <<= 1;
  for (uint32_t i = threadIdx.x; i < n2; i += NT) {
    uint64_t k = ~0ull;
    if (i < nb) {
      // ascending u64 order == (dot descending, block ascending)
      const uint32_t uk = (uint32_t)total_key_dev(s.dots[i]) ^ 0x80000000u;   // monotone unsigned
      k = ((uint64_t)(~uk) << 32) | i;
    }
    keys[i] = k;
  }
  __syncthreads();
  for (uint32_t size = 2; size <= n2; size <<= 1) {
    for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
      for (uint32_t t = threadIdx.x; t < n2 / 2; t += NT) {
        const uint32_t i = 2 * t - (t & (stride - 1));
        const uint32_t j = i + stride;
        const bool up = (i & size) == 0;
        const uint64_t a = keys[i], b = keys[j];
        if ((a > b) == up) {
          keys[i] = b;
          keys[j] = a;
        }
      }
      __syncthreads();
    }
  }
  for (uint32_t i = threadIdx.x; i < nb; i += NT) s.order[i] = (uint16_t)(keys[i] & 0xffffu);
  __syncthreads();
}

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
// stage 2 pieces
// ---------------------------------------------------------------------------
struct ChunkBufs {   // carved from the union region
  uint16_t* live_pos;   // [NT] positions (in traversal order) of live blocks
  uint32_t* cb_incl;    // [NT] inclusive item prefix
  uint32_t* cb_p0;      // [NT] first posting of the block
  uint16_t* cb_blk;     // [NT] block id (list-local)
  uint64_t* it_ref;     // [ITEMS] packed doc record ref; high 32 bits reused for the score
  uint32_t* it_doc;     // [ITEMS] doc id | (already visited) << 31
  uint16_t* it_blk;     // [ITEMS] list-local block id (its summary dot is dots[it_blk])
  uint16_t* it_ord;     // [ITEMS] item indices by length class: <= 128 elements from the front, longer from the back
};

template <int NT>
SGPU_DEV ChunkBufs carve_chunk(uint8_t* uni, uint32_t items_max) {
  ChunkBufs c;
  uint8_t* p = uni;
  c.it_ref = (uint64_t*)p;  p += (size_t)items_max * 8;
  c.it_doc = (uint32_t*)p;  p += (size_t)items_max * 4;
  c.cb_incl = (uint32_t*)p; p += NT * 4;
  c.cb_p0 = (uint32_t*)p;   p += NT * 4;
  c.it_blk = (uint16_t*)p;  p += (size_t)items_max * 2;
  c.it_ord = (uint16_t*)p;  p += (size_t)items_max * 2;
  c.live_pos = (uint16_t*)p; p += NT * 2;
  c.cb_blk = (uint16_t*)p;
  return c;
}

SGPU_DEV bool visited_test(const uint32_t* bitmap, uint32_t doc) {
  // written by other waves of this workgroup through L2 atomics: read past the (per-CU,
  // not atomically updated) L1 with an agent-scope load
  const uint32_t w = __hip_atomic_load(bitmap + (doc >> 5), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return (w >> (doc & 31)) & 1u;
}
SGPU_DEV void visited_mark(uint32_t* bitmap, uint32_t doc) {
  __hip_atomic_fetch_or(bitmap + (doc >> 5), 1u << (doc & 31), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// QueryEvaluator::compute_distance for one document by one 16-lane group.
// Canonical order (DESIGN.md): lane j accumulates elements [128 s + 8 j, +8) in
// increasing index, then t[j] += t[j ^ d] for d = 8, 4, 2, 1.
// Non-matching components resolve to the weight 0.0 (slot qn of q_val) and are
// added as +-0.0, which leaves an accumulator that started at +0.0 bit-identical
// to skipping them (x + (+-0) == x, and the accumulator can never be -0.0).
// How a record stores its elements (VT_F16, VT_U8, VT_DVB) and how a slice of 8 is loaded and unpacked: record.hpp.

// VT_DVB with the dense lookup table: slice_components is asked for table ADDRESSES (components + the table's LDS address,
// Lds::idx0), so that the running sums of the gaps ARE the addresses of the bytes to read
template <int LK, int VT>
SGPU_DEV uint32_t dvb_bias(const Lds& s) { return (Vt<VT>::sliced && LK == LK_DENSE) ? s.idx0 : 0u; }

// weight * value i (0..7) of a loaded slice, one rounding
template <int VT>
SGPU_DEV float mul_val(float q, const uint32_t* v, int i) {
  if (Vt<VT>::half) return mul_f32_f16(q, v[i >> 1], i & 1);
  // byte (i & 3) of the word, widened exactly (the compiler selects v_cvt_f32_ubyteN)
  const float c = (float)((v[i >> 2] >> (8 * (i & 3))) & 0xffu);
  return __fmul_rn(q, c);
}

// SC: dense lookup only - the table holds scaled bytes (ST_SCALED; always false for the other layouts)
template <typename CT, int LK, int VT, bool SC>
SGPU_DEV float accumulate_chunk(const Lds& s, const DocChunk<CT, VT>& d, const uint32_t c[8], uint32_t e0, uint32_t len, float acc) {
  const uint32_t v[4] = {d.v.x, d.v.y, d.v.z, d.v.w};
  float qv[8];
  if (LK == LK_HASH) {
    // one {component id, weight} entry per hash slot, ONE LDS read per document component; an empty slot
    // (id 0xffffffff) or a mere slot-mate fails the comparison and gets the weight 0.0 (padding sentinels too)
    const uint32_t hm = uniform_u(s.st[ST_HMULT]);   // (a state word rather than a parameter: the other layouts keep their registers)
    if (sizeof(CT) == 4) {   // u32 records: four entries at a time (eight at once spill next to the slots in flight)
#pragma unroll
      for (int h4 = 0; h4 < 8; h4 += 4) {
        uint2 e[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) e[i] = s.q_ent[hash_slot_dev(c[h4 + i], hm)];
#pragma unroll
        for (int i = 0; i < 4; ++i)
          acc = __fadd_rn(acc, mul_val<VT>(e[i].x == c[h4 + i] ? __uint_as_float(e[i].y) : 0.0f, v, h4 + i));
      }
      return acc;
    }
    uint2 e[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) e[i] = s.q_ent[hash_slot_dev(c[i], hm)];
#pragma unroll
    for (int i = 0; i < 8; ++i) qv[i] = e[i].x == c[i] ? __uint_as_float(e[i].y) : 0.0f;
  } else if (LK == LK_DENSE) {
    // one byte per vocabulary id: 1 + rank in the query, 0 = absent (-> q_val[-1] == 0.0).
    // Padding components carry the sentinel id `dim`, whose byte is always 0: no length test.
    uint32_t r[8];
    if (Vt<VT>::sliced) {   // c[] are the bytes' LDS addresses (dvb_bias)
#pragma unroll
      for (int i = 0; i < 8; ++i) r[i] = *(const __attribute__((address_space(3))) uint8_t*)(uintptr_t)c[i];
    } else {
#pragma unroll
      for (int i = 0; i < 8; ++i) r[i] = s.q_idx[c[i]];
    }
    if (SC) {   // the byte IS the weight's LDS address: the 0.0 slot sits at LDS address 0 - the dynamic LDS starts there (the
                // kernel has no static LDS: checked by the host, kernel_has_no_static_lds) and the host lays the weights
                // out first (kQscOffset == 0). (Adding the array's own address - a link-time 0 - costs a v_add per element.)
      static_assert(kQscOffset == 0, "scaled bytes address the weights from LDS address 0");
#pragma unroll
      for (int i = 0; i < 8; ++i) qv[i] = *(const __attribute__((address_space(3))) float*)(uintptr_t)r[i];
    } else {
#pragma unroll
      for (int i = 0; i < 8; ++i) qv[i] = s.q_sc[(int)r[i] - 1];
    }
  } else {
    // {32 vocabulary bits, rank of the word's first query component} per 32 ids, four elements at a
    // time (the temporaries of eight at once cost spills next to the slots in flight). u32 records
    // pad with the sentinel id `dim`, whose word is always zero (the table has one word to spare);
    // u16 records may not have a sentinel (dim == 65536), so the length is tested there.
#pragma unroll
    for (int h4 = 0; h4 < 8; h4 += 4) {
      uint2 w[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (LK == LK_PACKED) w[i] = s.q_word[c[h4 + i] >> 5];
        else w[i] = make_uint2(s.q_bits32[c[h4 + i] >> 5], (uint32_t)s.q_rank16[c[h4 + i] >> 5]);
      }
      int r[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const uint32_t bit = c[h4 + i] & 31u;
        bool hit = (w[i].x >> bit) & 1u;
        if (sizeof(CT) == 2) hit = hit && (e0 + (uint32_t)(h4 + i) < len);
        r[i] = hit ? (int)(w[i].y + (uint32_t)__popc(w[i].x & ((1u << bit) - 1u))) : -1;
      }
      float q4[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) q4[i] = s.q_sc[r[i]];
#pragma unroll
      for (int i = 0; i < 4; ++i) acc = __fadd_rn(acc, mul_val<VT>(q4[i], v, h4 + i));
    }
    return acc;
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) acc = __fadd_rn(acc, mul_val<VT>(qv[i], v, i));
  return acc;
}

// One pass (record.hpp: load_pass) of one document scored by its 16-lane group, for the loops that take a document at a
// time (cooperative rounds) and for every pass of a VT_DVB document.
template <typename CT, int LK, int VT, bool SC>
SGPU_DEV float score_pass(const Lds& s, const DocChunk<CT, VT>& d, bool raw, uint32_t e, uint32_t len, float a) {
  uint32_t c[8];
  const uint32_t bias = dvb_bias<LK, VT>(s);
  if (Vt<VT>::sliced && raw) {
    raw_pass_components<CT, VT>(d, c, bias);
  } else {
    slice_components<CT, VT>(d, c, bias);
  }
  DocChunk<CT, VT> t = d;
  place_values<CT, VT>(t, raw);
  if (e < len) a = accumulate_chunk<CT, LK, VT, SC>(s, t, c, e, len, a);
  return a;
}

// Sum over the 16 lanes of a group, valid in lane 0 of the group. DPP row rotations (no LDS
// round trip): lane i adds lane (i + d) % 16 for d = 8, 4, 2, 1. For lane 0 every partner is the
// same as in the butterfly t[j] += t[j ^ d] of the canonical order, so the value is bit-identical.
SGPU_DEV float dpp_row_ror(float v, int ctrl8421) {
  const int x = (int)__float_as_uint(v);
  int r;
  switch (ctrl8421) {
    case 8: r = __builtin_amdgcn_update_dpp(0, x, 0x128, 0xf, 0xf, false); break;
    case 4: r = __builtin_amdgcn_update_dpp(0, x, 0x124, 0xf, 0xf, false); break;
    case 2: r = __builtin_amdgcn_update_dpp(0, x, 0x122, 0xf, 0xf, false); break;
    default: r = __builtin_amdgcn_update_dpp(0, x, 0x121, 0xf, 0xf, false); break;
  }
  return __uint_as_float((uint32_t)r);
}
SGPU_DEV float reduce16(float acc) {
  acc = __fadd_rn(acc, dpp_row_ror(acc, 8));
  acc = __fadd_rn(acc, dpp_row_ror(acc, 4));
  acc = __fadd_rn(acc, dpp_row_ror(acc, 2));
  acc = __fadd_rn(acc, dpp_row_ror(acc, 1));
  return acc;
}
// lane 0 of each 16-lane row, broadcast to the row (DPP row_share:0)
SGPU_DEV uint32_t row_bcast0(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x150, 0xf, 0xf, false);
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

// Phase B: speculative scoring of the round's items, 16 lanes per document. Phase A sorted the
// items into two classes by length (ChunkBufs::it_ord): documents of at most 128 elements (one
// slice of 8 elements per lane; two thirds of a SPLADE-shaped collection) occupy one slot of 8
// registers each and a lane group keeps FOUR of them in flight; longer ones take two slices and a
// group keeps two in flight (both ways 128 B per lane, what the register budget of 2 x 512 threads
// per CU allows). The slots ROTATE: as soon as a slot's document is scored the next document's
// loads are issued into it, so the memory pipe stays busy while the other slots are being scored.
// The loads are unconditional (idle lanes re-read the record's first bytes): nothing but
// straight-line code lies between a load and its use, and the compiler's counter waits name
// exactly the slot they need (vmcnt(6), not vmcnt(0)).
// Groups pull documents from a shared counter, a batch ahead. When the heap is already full (and
// no visited bitmap is kept) the items scoring above the round's starting threshold are collected
// for replay_candidates.
template <typename CT, int LK, int ND, int NS, int VT, bool SC>
SGPU_DEV void score_class(const Lds& s, const DevView& ix, const ChunkBufs& cb, const uint16_t* list, int dir,
                              uint32_t n, uint32_t* pull, bool collect, float thr0, uint32_t& spec_docs, uint32_t len_mask) {
  // (len_mask: the bits of a ref's low word that hold the length - a VT_DVB index keeps a format flag above them,
  // also on the records this loop scores in the raw VT_U8 form)
  if (n == 0) return;
  const uint32_t sub = threadIdx.x & 15;
  float* it_score = (float*)cb.it_ref;
  const uint32_t e0 = sub * 8u;
  uint32_t len[ND], item[ND];
  const uint8_t* rec[ND];
  bool rawf[ND];   // (VT_DVB) the document keeps the raw VT_U8 record form: same loop, other addresses, other unpacking
  DocChunk<CT, VT> d[ND][NS];
  auto issue = [&](int u, uint32_t iu) {
    const bool has = iu < n;
    const uint32_t it = (uint32_t)list[(int)(has ? iu : 0u) * dir];
    const uint64_t ref = cb.it_ref[it];
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
        // the same two load instructions for both record forms (straight-line code between a load and its use): 16 bytes
        // of components - a packed slice has 12, the 4 bytes behind it are the next slice's or the values' - and the values
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
      if (Vt<VT>::sliced) {   // (per document: packed slice or raw components)
        a = score_pass<CT, LK, VT, SC>(s, d[u][h], rawf[u], e0 + 128u * h, len[u], a);
        continue;
      }
      uint32_t c[8];
      slice_components<CT, VT>(d[u][h], c, dvb_bias<LK, VT>(s));
      if (e0 + 128u * h < len[u]) a = accumulate_chunk<CT, LK, VT, SC>(s, d[u][h], c, e0 + 128u * h, len[u], a);
    }
    if (NS > 1) {
      // documents longer than 128 NS elements: further passes, the trip count the same for the 16 lanes of the group
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
      if (collect && len[u] != 0 && a > thr0) {
        const uint32_t slot = atomicAdd(&s.st[ST_NCAND], 1u);
        if (slot < kMaxCand) s.st[ST_CAND + slot] = item[u];
      }
    }
  };
  // One pull per wavefront and round of the slots: 4*ND consecutive items, slot u of lane group g
  // takes item base + 4u + g, so that ONE load instruction covers four consecutive items. In the
  // block-major forward store consecutive items of a class are adjacent records: the 128-byte
  // lines on their boundaries are then requested once, inside one instruction, instead of twice
  // hundreds of cycles apart (tools/ubench/record_stream.hip: adjacent records cost no extra lines).
  const uint32_t grp = (threadIdx.x & 63) >> 4;
  uint32_t pulled = 0;
  if ((threadIdx.x & 63) == 0) pulled = atomicAdd(pull, 4u * (uint32_t)ND);
  uint32_t base = uniform_u(pulled);
  if (base >= n) return;
#pragma unroll
  for (int u = 0; u < ND; ++u) issue(u, base + 4u * (uint32_t)u + grp);
  for (;;) {
    if ((threadIdx.x & 63) == 0) pulled = atomicAdd(pull, 4u * (uint32_t)ND);   // the batch that refills the slots
    consume(0);
    base = uniform_u(pulled);
    issue(0, base + grp);
#pragma unroll
    for (int u = 1; u < ND; ++u) {
      consume(u);
      issue(u, base + 4u * (uint32_t)u + grp);
    }
    if (base >= n) break;   // every slot was refilled with nothing
  }
}

#ifndef SGPU_ND_SHORT_U8    // fixed-u8 values: 6 registers per slice
#define SGPU_ND_SHORT_U8 4
#endif
#ifndef SGPU_ND_LONG_U8
#define SGPU_ND_LONG_U8 2
#endif
#ifndef SGPU_ND_SHORT_U32   // documents in flight per lane group, u32 components (12 registers per slice instead of 8)
#define SGPU_ND_SHORT_U32 3
#endif
#ifndef SGPU_ND_LONG_U32
#define SGPU_ND_LONG_U32 2
#endif
#ifndef SGPU_ND_SHORT
#define SGPU_ND_SHORT 4
#endif
#ifndef SGPU_ND_LONG
#define SGPU_ND_LONG 2
#endif
template <typename CT, int NT, int LK, bool COUNTED, int VT, bool SC>
SGPU_DEV void score_items_sc(const Lds& s, const DevView& ix, const ChunkBufs& cb, const KParams& p,
                             uint32_t& spec_docs) {
  const bool collect = !COUNTED && s.st[ST_HLEN] == p.k;   // heap full: only scores above the
  const float thr0 = __uint_as_float(s.st[ST_THR]);            // current k-th best can matter
  const uint32_t n_short = s.st[ST_NSHORT] & 0xffffu, n_long = s.st[ST_NSHORT] >> 16;
  constexpr int kShort = sizeof(CT) == 2 ? (Vt<VT>::half ? SGPU_ND_SHORT : SGPU_ND_SHORT_U8) : SGPU_ND_SHORT_U32;
  constexpr int kLong = sizeof(CT) == 2 ? (Vt<VT>::half ? SGPU_ND_LONG : SGPU_ND_LONG_U8) : SGPU_ND_LONG_U32;
  constexpr uint32_t kMask = LenMask<VT>::v;
  // Half of the wavefronts start with the long class, the others with the short one, and each moves on
  // to the other class when its first is exhausted: the drain of one class (its last loads coming back)
  // overlaps the other's work instead of every wavefront draining, then refilling, at the same time.
  // (Scores do not depend on which wavefront computes them; one copy of each class's code.)
#ifndef SGPU_CLASS_SPLIT
#define SGPU_CLASS_SPLIT 1
#endif
  const bool long_first = SGPU_CLASS_SPLIT && (((threadIdx.x >> 6) & 1u) != 0);
#pragma nounroll
  for (int ph = 0; ph < 2; ++ph) {
    if ((ph == 0) == long_first)
      score_class<CT, LK, kLong, 2, VT, SC>(s, ix, cb, cb.it_ord + (p.items_max - 1), -1, n_long, &s.st[ST_PULL_L], collect, thr0,
                                        spec_docs, kMask);
    else
      score_class<CT, LK, kShort, 1, VT, SC>(s, ix, cb, cb.it_ord, 1, n_short, &s.st[ST_TMP2], collect, thr0, spec_docs, kMask);
  }
}
// (the dense lookup table holds scaled or plain bytes, per query: kScaledMaxNnz; one uniform branch per round)
template <typename CT, int NT, int LK, bool COUNTED, int VT>
SGPU_DEV void score_items(const Lds& s, const DevView& ix, const ChunkBufs& cb, const KParams& p,
                          uint32_t& spec_docs) {
  if (LK == LK_DENSE && uniform_u(s.st[ST_SCALED]) != 0u) score_items_sc<CT, NT, LK, COUNTED, VT, true>(s, ix, cb, p, spec_docs);
  else score_items_sc<CT, NT, LK, COUNTED, VT, false>(s, ix, cb, p, spec_docs);
}

// Phase A's last step: file item i under its length class (wave-aggregated list appends). Items the
// counted pass already knows as visited are not scored at all.
template <int VT>
SGPU_DEV void classify_item(uint32_t* st, const ChunkBufs& cb, uint32_t items_max, uint32_t i, uint32_t ref_lo,
                            bool take) {
  const uint32_t len = ref_lo & LenMask<VT>::v;
  const bool sh = take && len <= 128u, lg = take && len > 128u;   // (VT_DVB: raw-form documents are scored by the same loops)
  const uint64_t ms = __ballot(sh), ml = __ballot(lg);
  const uint32_t lane = lane_id();
  uint32_t both = 0;   // both list lengths live in one word: short | long << 16
  if (lane == 0 && (ms | ml)) both = atomicAdd(&st[ST_NSHORT], (uint32_t)__popcll(ms) | ((uint32_t)__popcll(ml) << 16));
  both = (uint32_t)__builtin_amdgcn_readfirstlane((int)both);
  const uint32_t bs = both & 0xffffu, bl = both >> 16;
  const uint64_t below = (1ull << lane) - 1ull;
  if (sh) cb.it_ord[bs + (uint32_t)__popcll(ms & below)] = (uint16_t)i;
  if (lg) cb.it_ord[items_max - 1u - (bl + (uint32_t)__popcll(ml & below))] = (uint16_t)i;
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

// ---------------------------------------------------------------------------
// stage 2 as a STREAM (r06): one control wavefront (feeder + replayer) and the scoring wavefronts
// ---------------------------------------------------------------------------
// The round loop of stage 2 (the kernel's `while (pos < nb)` below; still what the counted and the cooperative
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
  // odd wavefronts prefer the long class, even ones the short one (SGPU_CLASS_SPLIT of the round loop); each takes
  // whatever there is when its own class has nothing
  const bool long_first = SGPU_CLASS_SPLIT && (((threadIdx.x >> 6) & 1u) != 0);
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
template <int KR, int VT>
SGPU_DEV void stream_control(const Lds& s, const DevView& ix, const BatchView& qb, const Ring& rg, const KParams& p,
                             uint32_t l0, uint32_t l1, uint32_t& budget_io, uint32_t* busy_ticks) {
#ifdef SGPU_PROF   // (profiling build) where the control wavefront's time goes: busy_ticks[0] replay, [1] skip test + tables +
  // block lookup of a batch, [2] posting loads + filing the items, [3] waiting for room, [4] the final replay, [5] skipped windows
  uint64_t tq = clock64();
#define CTICK(i) { const uint64_t t_ = clock64(); busy_ticks[i] += (uint32_t)((t_ - tq) >> 4); tq = t_; }
#else
#define CTICK(i) {}
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
#undef CTICK
  heap.store(s.heap);
  if (lane == 0) {
    s.st[ST_HLEN] = heap.len;
    s.st[ST_THR] = __float_as_uint(heap.len == p.k ? heap.thr : 0.0f);
  }
  budget_io = budget;
}

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
#define SGPU_COOP_FN SGPU_DEV
template <typename CT, int NT, int KR, int LK, int VT>
SGPU_COOP_FN bool wide_round(const Lds& s, const DevView& ix, const BatchView& qb, const CoopView& co, const KParams& p,
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
SGPU_COOP_FN void coop_help(const Lds& s, const DevView& ix, const BatchView& qb, const CoopView& co, const KParams& p) {
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

// STREAM: stage 2 as a stream of items between a feeder, the scorers and a replayer wavefront ("stage 2 as a stream"
// above) instead of the round loop; plain launches only (the counted and the cooperative variants keep the rounds).
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
      {
      const uint32_t ticket = atomicAdd(queue, 1u) - p.queue_base;   // (every workgroup ends on exactly one ticket >= nq: nq + gridDim.x in all)
      // longest-expected-first order prepared by the host (tail balance); identity if absent
      s.st[ST_Q] = ticket < qb.nq ? (qb.q_order ? qb.q_order[ticket] : ticket) : 0xffffffffu;
      // workgroups can only run out of queries while one of the last `gridDim` tickets is being served
      if (COOP) s.st[ST_CO_TAIL] = (uint64_t)ticket + gridDim.x >= qb.nq ? 1u : 0u;
      }
    }
    __syncthreads();
    const uint32_t q = s.st[ST_Q];
    if (q == 0xffffffffu) break;
    if (COOP) CO_TRACE(co, 0);
    // LK_HASH: the multiplier under which this query's components hash without collision (host-chosen)
    if (LK == LK_HASH && threadIdx.x == 0) s.st[ST_HMULT] = qb.q_seed ? hash_mult(qb.q_seed[q]) : 1u;

    // phase clocks (s_memtime): time since the previous TICK goes to bucket i
    uint32_t prof[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) prof[i] = 0;
    uint64_t tprev = clock64();
    (void)tprev;
#ifndef SGPU_PROF   // phase clocks only in the profiling build (make prof): they cost ~2% and 14 registers
#define TICK(i) {}
#else
#define TICK(i)                                   \
  {                                               \
    const uint64_t t_ = clock64();                \
    prof[i] += (uint32_t)((t_ - tprev) >> 4);     \
    tprev = t_;                                   \
  }
#endif
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
#if SGPU_REPLAY_PRIO
          __builtin_amdgcn_s_setprio(SGPU_REPLAY_PRIO);
#endif
          stream_control<KR, VT>(s, ix, qb, rg, p, l0, l1, budget, busy);
          if (lane == 0) s.st[ST_S_BUDGET] = budget;
#if SGPU_REPLAY_PRIO
          __builtin_amdgcn_s_setprio(0);
#endif
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
        prof[7] = prof[7] - (prof[7] < busy[0] + busy[1] + busy[2] + busy[3] ? prof[7] : busy[0] + busy[1] + busy[2] + busy[3]);
        prof[8] += busy[0];
        prof[4] += busy[1];
        prof[5] += busy[2];
        prof[6] += busy[3];
        prof[10] += 1;
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
          prof[10] += 1;
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
#if SGPU_REPLAY_PRIO
              __builtin_amdgcn_s_setprio(SGPU_REPLAY_PRIO);
#endif
              replay_round<KR, COUNTED>(cb, s, p, n_items, bitmap, decided_blk, piece == 0, wc, dots, LenMask<VT>::v, false, idle_fetch);
#if SGPU_REPLAY_PRIO
              __builtin_amdgcn_s_setprio(0);
#endif
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
    if (qb.out_stats) {   // work counters (see DESIGN.md "Algorithmic bytes")
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
      if (lane == 0) atomicAdd(&os[7], sd);
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
      for (int i = 0; i < 12; ++i) os[i] = prof[i];
      os[12] = blockIdx.x;
#ifdef SGPU_PROF
      if (STREAM) {   // (profiling build, streamed variants) [21] polls of starved scorers [22] polls of the blocked feeder [23] spans << 16 | mean budget
        os[13] = s.st[ST_S_STARVED] | (s.st[ST_S_SKIPPED] << 20);
        os[14] = s.st[ST_S_BLOCKED];
        os[15] = (s.st[ST_S_SPANS] << 16) | (s.st[ST_S_SPANS] ? (s.st[ST_S_BUDGET_SUM] / s.st[ST_S_SPANS]) & 0xffffu : 0u);
      }
#endif
    }
#undef TICK
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
