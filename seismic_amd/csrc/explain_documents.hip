// explain_documents.hip — the terms behind a document's score on the device (sgpu_explain_documents).
//
// What score_documents_kernel computes for a candidate, plus the m best of the products it adds. Kept from that kernel:
// the tiles of at most kScoreTile candidates of one query, the query's weight table in LDS (dense or hashed, built and
// cleared the same way), one 16-lane group per candidate reading its record through record.hpp, and the score's order -
// a per-lane accumulator over the passes of 128 elements, then t[j] += t[j ^ s], s = 8, 4, 2, 1, __fmul_rn and
// __fadd_rn - so that the score has the score kernel's bits. A group has ONE candidate in flight (the score kernel: two).
//
//   term    an element e < len whose component has a table weight that is not +-0 (padding elements are never terms, a
//           stored value of 0 is one); its product is the f32 the accumulator adds for it.
//   key     ordered(product bits) << 32 | ~component, a u64: a larger key is an earlier term - product descending in the
//           order of the monotone integer image (-0.0 below +0.0), then component ascending. A document's components are
//           distinct, so the keys of a pair are distinct; 0 is no term's key (it would need the component 2^32 - 1) and
//           stands for "none". The payload of a key is the stored value as an f32 (fixed-u8: the code).
//   list    the group's best m <= 32 keys so far live in REGISTERS, sorted: rank r with its payload in lane r % 16,
//           slot r / 16. After a pass that found terms the group merges: every lane holds its 8 new keys and its 2 list
//           entries, and at most m times the group takes the largest key left (a lane's own maximum, then a max over the
//           16 lanes by xor shuffles), its owner drops it, the payload follows by an or over the lanes, and lane r % 16
//           keeps it as rank r. The loop ends early when no key is left; a pass without terms is not merged.
//   rows    at the end lane l writes ranks l and l + 16 of the candidate's row: the component and product from the key, the
//           document value from the payload, and the query's weight AS GIVEN, found by a binary search of the query's
//           ascending components in global memory (the table holds w * val_scale for fixed-u8 codes). Ranks past the
//           terms are written as zero, so the launch's rows need no clearing.
//   cost    no LDS beyond the weight table, so the table alone decides the workgroups per CU exactly as for the score
//           kernel (one 1024-thread workgroup beside a 128 KiB dense table); the price is registers (kernel resources in
//           DESIGN.md) and 12 shuffles per extracted term.
// Every loop is bounded by the task's own counts (tiles, candidates, passes = ceil(len / 128), m, log2 of the query's
// length; a hash probe ends at an empty slot of a table at most half full); no loop waits on another workgroup; the
// barriers sit in the tile loop, whose bounds and branch (the tile's query) are workgroup-uniform. The shuffles are
// 16 wide and run under conditions that are uniform over the group (len, m, the merged maximum).
#include <hip/hip_runtime.h>

#include <type_traits>

#include "score_lookup.hpp"

namespace sgpu {

namespace {

template <int CW, int VT, bool DENSE>
__global__ __launch_bounds__(1024) void explain_documents_kernel(ExplainArgs a) {
  using CT = typename std::conditional<CW == 2, uint16_t, uint32_t>::type;
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const uint32_t tid = threadIdx.x, nt = blockDim.x;
  const uint32_t ng = nt >> 4, g = tid >> 4, l = tid & 15u;
  const uint32_t slots = 1u << a.slot_bits;
  const uint32_t m = a.m;
  // (the table's block and the ref's decode are written out, as in the parent: through table_fill_query / table_clear_query
  // and doc_ref_of six of this kernel's ten variants compile to other code; the lookup and the reductions are shared)
  const WeightTable tab = weight_table(smem, a.dim, a.slot_bits);
  // the weight table: built, used and cleared as in score_documents_kernel
  if (DENSE) {
    for (uint32_t i = tid; i <= a.dim; i += nt) ((float*)smem)[i] = 0.0f;
  } else {
    for (uint32_t i = tid; i < slots; i += nt) ((uint32_t*)smem)[i] = kHashEmpty;
  }
  uint32_t cur_q = kNoQuery;
  for (uint32_t t = blockIdx.x; t < a.n_tiles; t += gridDim.x) {
    const uint4 tile = a.tiles[t];   // (workgroup-uniform)
    if (tile.x != cur_q) {
      __syncthreads();   // every group is done with the table as it is
      if (cur_q != kNoQuery) {
        if (DENSE) {
          const uint64_t p0 = a.q_off[cur_q], p1 = a.q_off[cur_q + 1];
          for (uint64_t j = p0 + tid; j < p1; j += nt) ((float*)smem)[a.q_comp[j]] = 0.0f;
        } else {
          for (uint32_t i = tid; i < slots; i += nt) ((uint32_t*)smem)[i] = kHashEmpty;
        }
        __syncthreads();
      }
      const uint64_t b0 = a.q_off[tile.x], b1 = a.q_off[tile.x + 1];
      for (uint64_t j = b0 + tid; j < b1; j += nt) {
        const uint32_t c = a.q_comp[j];
        const float w = Vt<VT>::half ? a.q_val[j] : __fmul_rn(a.q_val[j], a.val_scale);
        if (DENSE) {
          ((float*)smem)[c] = w;
        } else {
          uint32_t* keys = (uint32_t*)smem;
          float* wts = (float*)(smem + (size_t)slots * 4u);
          uint32_t slot = (c * 2654435761u) >> (32u - a.slot_bits);
          while (atomicCAS(&keys[slot], kHashEmpty, c) != kHashEmpty) slot = (slot + 1u) & (slots - 1u);
          wts[slot] = w;
        }
      }
      __syncthreads();
      cur_q = tile.x;
    }
    const uint64_t q0 = a.q_off[tile.x], q1 = a.q_off[tile.x + 1];
    for (uint32_t base = 0; base < tile.z; base += ng) {
      const uint32_t idx = base + g;   // (uniform over the group, as is all that follows from it)
      const bool live = idx < tile.z;
      const uint64_t ref = live ? a.doc_ref[a.cand[tile.y + idx]] : 0ull;
      const uint32_t len = (uint32_t)ref & LenMask<VT>::v;
      const bool raw = Vt<VT>::sliced && ((uint32_t)ref & kRawBit) != 0u;
      const uint8_t* rec = a.fwd + (size_t)(ref >> 16) * 16u;
      float acc = 0.0f;
      uint32_t n_terms = 0;
      uint64_t lk[2] = {0, 0};   // the list: ranks l and l + 16
      uint32_t lv[2] = {0, 0};
      for (uint32_t p0 = 0; p0 < len; p0 += 128u) {
        const uint32_t e0 = p0 + l * 8u;
        uint64_t k[10];
        uint32_t v[10];
        uint32_t found = 0;
#pragma unroll
        for (int i = 0; i < 8; ++i) k[i] = 0, v[i] = 0;
        if (e0 < len) {
          DocChunk<CT, VT> d;
          load_pass<CT, VT>(d, rec, len, raw, e0);
          uint32_t c[8];
          if (Vt<VT>::sliced && raw) {
            raw_pass_components<CT, VT>(d, c);
          } else {
            slice_components<CT, VT>(d, c);
          }
          place_values<CT, VT>(d, raw);
          float w[8];
#pragma unroll
          for (int i = 0; i < 8; ++i) w[i] = weight_of<DENSE>(tab, c[i]);
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            const float x = slice_value<VT>(d.v, i);
            const float p = __fmul_rn(w[i], x);
            acc = __fadd_rn(acc, p);
            if (e0 + (uint32_t)i < len && (__float_as_uint(w[i]) & 0x7fffffffu) != 0u) {
              k[i] = ((uint64_t)ordered_u32(p) << 32) | (uint64_t)(~c[i]);
              v[i] = __float_as_uint(x);
              ++found;
            }
          }
        }
        found = group16_sum(found);
        n_terms += found;
        if (found == 0) continue;
        k[8] = lk[0], v[8] = lv[0], k[9] = lk[1], v[9] = lv[1];
        lk[0] = lk[1] = 0;
        lv[0] = lv[1] = 0;
        for (uint32_t r = 0; r < m; ++r) {
          uint64_t bk = k[0];
          uint32_t bv = v[0];
#pragma unroll
          for (int i = 1; i < 10; ++i)
            if (k[i] > bk) bk = k[i], bv = v[i];
          const uint64_t gk = group16_max(bk);
          if (gk == 0) break;   // no key is left
          // (exactly one lane: a pair's keys are distinct because a document's components are strictly ascending -
          // validate_desc in host_index.cpp and build_host_index in builder.cpp refuse anything else)
          const bool mine = bk == gk;
          const uint32_t gv = group16_or(mine ? bv : 0u);
          if (mine) {
#pragma unroll
            for (int i = 0; i < 10; ++i)
              if (k[i] == gk) k[i] = 0;
          }
          if ((r & 15u) == l) {
            if (r < 16u) {
              lk[0] = gk, lv[0] = gv;
            } else {
              lk[1] = gk, lv[1] = gv;
            }
          }
        }
      }
      const float s = group16_sum(acc);
      if (!live) continue;
      const size_t at = (size_t)tile.y + idx;
      if (l == 0) {
        a.scores[at] = s;
        a.n_terms[at] = n_terms;
      }
#pragma unroll
      for (uint32_t u = 0; u < 2; ++u) {
        const uint32_t r = l + 16u * u;
        if (r >= m) continue;
        const uint64_t key = lk[u];
        uint32_t c = 0;
        float qw = 0.0f, dv = 0.0f, p = 0.0f;
        if (key != 0) {
          c = ~(uint32_t)key;
          p = ordered_u32_inv((uint32_t)(key >> 32));
          const float x = __uint_as_float(lv[u]);
          dv = Vt<VT>::half ? x : __fmul_rn(x, a.val_scale);   // (code * 2^e: exact)
          uint64_t lo = q0, hi = q1;   // the query's ascending components hold c: its weight as given
          while (lo < hi) {
            const uint64_t mid = lo + ((hi - lo) >> 1);
            if (a.q_comp[mid] < c) lo = mid + 1; else hi = mid;
          }
          if (lo < q1) qw = a.q_val[lo];
        }
        const size_t o = at * m + r;
        a.comps[o] = c;
        a.q_vals[o] = qw;
        a.d_vals[o] = dv;
        a.products[o] = p;
      }
    }
  }
}

}  // namespace

ExplainKernel explain_kernel(uint32_t cw, uint32_t vt, bool dense) {
  return for_variant(cw, vt, dense, [](auto CW, auto VT, auto D) -> ExplainKernel { return explain_documents_kernel<CW(), VT(), D()>; });
}

}  // namespace sgpu
