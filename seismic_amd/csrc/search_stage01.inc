// search_stage01.inc - part of search_kernel.inc (included there, inside namespace sgpu; needs search_lds.inc).
// Holds: stage 0 (load_query, select_lists), the query lookup table (build_lookup, lookup_clear), stage 1
// (plan_list_group, build_row_table, stream_list_dots, summary_dots) and sort_first_list.
// Called by: the kernel body, by the whole workgroup, once per query or list group; a cooperative helper
// (search_coop.inc: coop_work) calls load_query, lookup_clear and build_lookup to bring a round's query into its own LDS.

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
