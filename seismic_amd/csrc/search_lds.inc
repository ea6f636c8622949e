// search_lds.inc - part of search_kernel.inc (included there, inside namespace sgpu; not a unit of its own).
// Holds: the lane and workgroup primitives (total_key_dev, mul_f32_f16, readlane_*, uniform_u, the DPP scans, wg_inclusive_scan),
// the kernel's view of its LDS (Lds, carve), the ST_* state words, and the round loop's buffers in the union region
// (ChunkBufs, carve_chunk).
// Called by: every role - the kernel body, stages 0 and 1, the scoring loops, the replay, the stream and the
// cooperative functions all reach their LDS through `Lds` and talk through the ST_* words.

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
// `v` of the first active lane, as a wave-uniform (scalar) value
SGPU_DEV uint32_t uniform_u(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
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
// stage 2's buffers in the union region (round loop)
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
