// search_score.inc - part of search_kernel.inc (included there, inside namespace sgpu; needs search_lds.inc, record.hpp).
// Holds: a document's score by its 16-lane group (mul_val, accumulate_chunk, score_pass, reduce16), the round loop's
// phase B (score_class, score_items and the SGPU_ND_* documents-in-flight defaults) and classify_item.
// Called by: every wavefront of a round-loop workgroup (score_items; the kernel body files the items with
// classify_item); the stream's scorers (search_stream.inc) and the cooperative chunks (search_coop.inc) use
// accumulate_chunk / score_pass / reduce16 with loops of their own.

// ---------------------------------------------------------------------------
// stage 2: scoring a document (16 lanes each) and the round loop's phase B
// ---------------------------------------------------------------------------
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
  const bool long_first = ((threadIdx.x >> 6) & 1u) != 0;
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
