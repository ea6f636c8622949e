// diversify_documents.hip — Maximal Marginal Relevance over caller-given candidates on the device
// (sgpu_diversify_documents).
//
// Per query the greedy selection of include/seismic_hip.h: every candidate entry scored against the query (rel), then
// round by round the untaken entry with the largest key (ordered(mmr) descending, id ascending) is selected,
// mmr = fl(fl(lambda * rel) - fl(mu * pen)), and the pen of every entry still untaken is raised to its similarity to
// the selected document. A workgroup of kDiversifyBlock threads owns one query at a time (a plain index range over
// the grid). Its LDS holds ONE weight table - the score kernel's: dense over the vocabulary where dim + 1 floats fit
// kScoreDenseLds, else the open-addressing hash of score_lookup.hpp - and behind it the state of the query's entries
// (id, rel, pen; 12 bytes each, at most 2048 of them).
//
//   table   has one occupant at a time: the query (phase 0) or the document selected last (rounds). Before the next
//           occupant moves in the table is emptied of the previous one - dense: sparsely, by walking the occupant's
//           components again; hash: wholesale. A document moves in decoded once by the workgroup, its passes of 128
//           elements over the 16-lane groups (record.hpp, as expand_queries.hip walks a document), the weight of
//           element e the f32 its stored bits stand for (fixed-u8: fl(fl(code * val_scale) * val_scale), the query
//           weight code * val_scale with the score kernel's fold of val_scale on top); elements e >= len (slice padding)
//           are MASKED, since a padding element repeats a component whose real element another lane holds. A
//           document's components are distinct: dense stores do not collide, the hash arm inserts with the score
//           kernel's CAS loop.
//   stream  both phases score entries against the table exactly as score_documents_kernel does: a 16-lane group per
//           entry, kDivDocs entries per group in flight, load_pass / slice_components / raw_pass_components /
//           place_values / weight_of, accumulator order and shuffle reduction unchanged. Phase 0 writes rel; a round
//           raises pen with fmaxf (pen starts at +0.0, so a negative similarity never lowers it) and skips the taken.
//   argmax  every thread forms the keys of its entries (at most two), a wave reduction by shuffles, the 16 wave maxima
//           through LDS. The entries that carry the selected id are marked taken (pen = kTaken, the bits of no pen: a
//           pen is never negative) in the same step, and the untaken ones counted the same way, so that the round
//           knows whether another follows before it touches the table: the table work and the stream are skipped
//           after the last round.
// Every loop is bounded by the task's own counts (queries of the launch, entries <= cap, k rounds, table entries, the
// elements of a query or document, passes = ceil(len / 128)); no loop waits on another workgroup; every barrier sits
// under workgroup-uniform conditions (the query, the round, the shared count of untaken entries, the occupant).
// Every table index is a stored or validated component (< dim) or a loop index <= dim (hash: < slots); every state
// index is below the query's entry count <= cap; every row index is below k.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "score_lookup.hpp"

namespace sgpu {

namespace {

constexpr uint32_t kDivWaves = kDiversifyBlock / 64u;
constexpr uint32_t kDivGroups = kDiversifyBlock / 16u;
constexpr uint32_t kDivDocs = 2;              // entries a 16-lane group has in flight (the score kernel's)
constexpr uint32_t kTaken = 0xffffffffu;      // pen bits of a taken entry
enum { OCC_NONE = 0, OCC_QUERY = 1, OCC_DOC = 2 };

struct DivState {   // the entries of the workgroup's query, in LDS behind the table
  uint32_t* id;
  float* rel;
  uint32_t* pen;    // f32 bits, or kTaken
};

// The document `ref` into the table (FILL) or out of a dense table again (!FILL), by the whole workgroup.
template <typename CT, int VT, bool DENSE, bool FILL>
__device__ __forceinline__ void table_walk_doc(const DiversifyArgs& a, uint8_t* smem, uint64_t ref) {
  const uint32_t tid = threadIdx.x, g = tid >> 4, l = tid & 15u;
  const uint32_t len = (uint32_t)ref & LenMask<VT>::v;
  const bool raw = Vt<VT>::sliced && ((uint32_t)ref & kRawBit) != 0u;
  const uint8_t* rec = a.fwd + (size_t)(ref >> 16) * 16u;
  const uint32_t slots = 1u << a.slot_bits;
  for (uint32_t p0 = g * 128u; p0 < len; p0 += kDivGroups * 128u) {
    const uint32_t e0 = p0 + l * 8u;
    if (e0 >= len) continue;
    DocChunk<CT, VT> d;
    load_pass<CT, VT>(d, rec, len, raw, e0);
    uint32_t c[8];
    if (Vt<VT>::sliced && raw) {
      raw_pass_components<CT, VT>(d, c);
    } else {
      slice_components<CT, VT>(d, c);
    }
    place_values<CT, VT>(d, raw);
#pragma unroll
    for (int i = 0; i < 8; ++i)
      if (e0 + (uint32_t)i < len) {   // (padding elements are no part of the document)
        if (!FILL) {
          ((float*)smem)[c[i]] = 0.0f;
          continue;
        }
        const float v = slice_value<VT>(d.v, i);
        const float w = Vt<VT>::half ? v : __fmul_rn(__fmul_rn(v, a.val_scale), a.val_scale);
        if (DENSE) {
          ((float*)smem)[c[i]] = w;
        } else {
          uint32_t* keys = (uint32_t*)smem;
          float* wts = (float*)(smem + (size_t)slots * 4u);
          uint32_t slot = (c[i] * 2654435761u) >> (32u - a.slot_bits);
          while (atomicCAS(&keys[slot], kHashEmpty, c[i]) != kHashEmpty) slot = (slot + 1u) & (slots - 1u);
          wts[slot] = w;
        }
      }
  }
}

// Entries [0, n) that are not taken against the table, as score_documents_kernel scores a tile. REL: the result is the
// entry's rel; else its pen is raised to it.
template <typename CT, int VT, bool DENSE, bool REL>
__device__ __forceinline__ void stream_entries(const DiversifyArgs& a, const uint8_t* smem, const DivState& st, uint32_t n) {
  const uint32_t tid = threadIdx.x, g = tid >> 4, l = tid & 15u;
  for (uint32_t base = 0; base < n; base += kDivGroups * kDivDocs) {
    uint32_t len[kDivDocs], idx[kDivDocs];
    const uint8_t* rec[kDivDocs];
    bool raw[kDivDocs], live[kDivDocs];
    float acc[kDivDocs];
    uint32_t max_len = 0;
#pragma unroll
    for (uint32_t u = 0; u < kDivDocs; ++u) {
      idx[u] = base + u * kDivGroups + g;
      live[u] = idx[u] < n && (REL || st.pen[idx[u]] != kTaken);
      const uint64_t ref = live[u] ? a.doc_ref[st.id[idx[u]]] : 0ull;
      len[u] = (uint32_t)ref & LenMask<VT>::v;
      raw[u] = Vt<VT>::sliced && ((uint32_t)ref & kRawBit) != 0u;
      rec[u] = a.fwd + (size_t)(ref >> 16) * 16u;
      acc[u] = 0.0f;
      max_len = max(max_len, len[u]);
    }
    for (uint32_t e0 = l * 8u; e0 < max_len; e0 += 128u) {
      DocChunk<CT, VT> d[kDivDocs];
#pragma unroll
      for (uint32_t u = 0; u < kDivDocs; ++u)
        if (e0 < len[u]) load_pass<CT, VT>(d[u], rec[u], len[u], raw[u], e0);
#pragma unroll
      for (uint32_t u = 0; u < kDivDocs; ++u)
        if (e0 < len[u]) {
          uint32_t c[8];
          if (Vt<VT>::sliced && raw[u]) {
            raw_pass_components<CT, VT>(d[u], c);
          } else {
            slice_components<CT, VT>(d[u], c);
          }
          place_values<CT, VT>(d[u], raw[u]);
          float w[8];
#pragma unroll
          for (int i = 0; i < 8; ++i) w[i] = weight_of<DENSE>(smem, c[i], a.slot_bits);
#pragma unroll
          for (int i = 0; i < 8; ++i) acc[u] = __fadd_rn(acc[u], __fmul_rn(w[i], slice_value<VT>(d[u].v, i)));
        }
    }
#pragma unroll
    for (uint32_t u = 0; u < kDivDocs; ++u) {
      float r = acc[u];
      r = __fadd_rn(r, __shfl_xor(r, 8, 16));
      r = __fadd_rn(r, __shfl_xor(r, 4, 16));
      r = __fadd_rn(r, __shfl_xor(r, 2, 16));
      r = __fadd_rn(r, __shfl_xor(r, 1, 16));
      if (l == 0 && live[u]) {
        if (REL) {
          st.rel[idx[u]] = r;
        } else {
          st.pen[idx[u]] = __float_as_uint(fmaxf(__uint_as_float(st.pen[idx[u]]), r));
        }
      }
    }
  }
}

template <int CW, int VT, bool DENSE>
__global__ __launch_bounds__(kDiversifyBlock) void diversify_documents_kernel(DiversifyArgs a) {
  using CT = typename std::conditional<CW == 2, uint16_t, uint32_t>::type;
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  __shared__ uint64_t s_best[kDivWaves];
  __shared__ uint32_t s_left[kDivWaves];
  __shared__ uint32_t s_pick[2];   // rel and pen bits of the selected entry
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  constexpr uint32_t nt = kDiversifyBlock;
  const uint32_t slots = 1u << a.slot_bits;
  DivState st;
  st.id = (uint32_t*)(smem + a.table_bytes);
  st.rel = (float*)(st.id + a.cap);
  st.pen = (uint32_t*)(st.rel + a.cap);
  const uint32_t k = a.k;

  if (DENSE) {
    for (uint32_t i = tid; i <= a.dim; i += nt) ((float*)smem)[i] = 0.0f;
  } else {
    for (uint32_t i = tid; i < slots; i += nt) ((uint32_t*)smem)[i] = kHashEmpty;
  }
  // the table's occupant (workgroup-uniform): none, a query or a document
  uint32_t occ = OCC_NONE, occ_q = 0;
  uint64_t occ_ref = 0;
  auto table_empty = [&]() {   // (the caller's barriers: nobody reads the table before, everybody sees it empty after)
    if (occ == OCC_NONE) return;
    if (!DENSE) {
      for (uint32_t i = tid; i < slots; i += nt) ((uint32_t*)smem)[i] = kHashEmpty;
    } else if (occ == OCC_QUERY) {
      const uint64_t p0 = a.q_off[occ_q], p1 = a.q_off[occ_q + 1];
      for (uint64_t j = p0 + tid; j < p1; j += nt) ((float*)smem)[a.q_comp[j]] = 0.0f;
    } else {
      table_walk_doc<CT, VT, DENSE, false>(a, smem, occ_ref);
    }
    occ = OCC_NONE;
  };

  for (uint32_t q = a.q_first + blockIdx.x; q < a.q_last; q += gridDim.x) {   // (workgroup-uniform)
    const uint32_t c0 = (uint32_t)(a.cand_off[q] - a.cand_base);
    const uint32_t n = (uint32_t)(a.cand_off[q + 1] - a.cand_off[q]);   // (<= cap: the host's check)
    uint32_t rounds = 0;
    if (n != 0u) {
      __syncthreads();   // the previous query is done with the table and the state
      table_empty();
      for (uint32_t i = tid; i < n; i += nt) st.id[i] = a.cand[c0 + i], st.pen[i] = 0u;
      __syncthreads();
      // phase 0: the query moves in, every entry's rel
      const uint64_t b0 = a.q_off[q], b1 = a.q_off[q + 1];
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
      occ = OCC_QUERY, occ_q = q;
      __syncthreads();
      stream_entries<CT, VT, DENSE, true>(a, smem, st, n);
      __syncthreads();
      // rounds
      for (uint32_t r = 0; r < k; ++r) {   // (left > 0 on entry: n > 0, and a round that leaves nothing ends the loop)
        // (a) the best untaken entry
        uint64_t best = 0;
        for (uint32_t i = tid; i < n; i += nt) {
          const uint32_t pb = st.pen[i];
          if (pb != kTaken) {
            const float mmr = __fsub_rn(__fmul_rn(a.lambda, st.rel[i]), __fmul_rn(a.mu, __uint_as_float(pb)));
            const uint64_t key = ((uint64_t)ordered_u32(mmr) << 32) | (uint64_t)(~st.id[i]);
            best = key > best ? key : best;
          }
        }
#pragma unroll
        for (uint32_t o = 32; o > 0; o >>= 1) {
          const uint64_t other = __shfl_xor(best, (int)o, 64);
          best = other > best ? other : best;
        }
        if (lane == 0u) s_best[wave] = best;
        __syncthreads();
        best = 0;
#pragma unroll
        for (uint32_t x = 0; x < kDivWaves; ++x) best = s_best[x] > best ? s_best[x] : best;
        // (no key: every untaken entry's mmr is a NaN of the image 0, outside the contract - the query ends here, so
        // that `sel` below is always the id of an entry)
        if (best == 0ull) break;   // (uniform: shared)
        const uint32_t sel = ~(uint32_t)best;
        // its entries are taken; what is left is counted
        uint32_t mine = 0;
        for (uint32_t i = tid; i < n; i += nt) {
          const uint32_t pb = st.pen[i];
          if (pb == kTaken) continue;
          if (st.id[i] == sel) {
            // (every entry of the id carries the same rel and pen: the stores below write the same bits)
            s_pick[0] = __float_as_uint(st.rel[i]);
            s_pick[1] = pb;
            st.pen[i] = kTaken;
          } else {
            ++mine;
          }
        }
#pragma unroll
        for (uint32_t o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, (int)o, 64);
        if (lane == 0u) s_left[wave] = mine;
        __syncthreads();
        uint32_t left = 0;
#pragma unroll
        for (uint32_t x = 0; x < kDivWaves; ++x) left += s_left[x];
        // (b) the row slot
        if (tid == 0u) {
          const size_t o = (size_t)q * k + r;
          a.row_ids[o] = (uint64_t)sel;
          a.row_scores[o] = __uint_as_float(s_pick[0]);
          a.row_pen[o] = __uint_as_float(s_pick[1]);
        }
        rounds = r + 1u;
        if (left == 0u || rounds == k) break;   // (uniform: shared counts)
        // (c) the selected document takes the table (everybody is past the barrier above: nobody reads the table)
        table_empty();
        const uint64_t ref = a.doc_ref[sel];
        __syncthreads();   // the table is empty; s_best, s_left and s_pick were read
        table_walk_doc<CT, VT, DENSE, true>(a, smem, ref);
        occ = OCC_DOC, occ_ref = ref;
        __syncthreads();
        // (d) the pen of what is left
        stream_entries<CT, VT, DENSE, false>(a, smem, st, n);
        __syncthreads();
      }
    }
    if (tid == 0u) a.row_n[q] = rounds;
  }
}

using DiversifyKernel = void (*)(DiversifyArgs);
DiversifyKernel diversify_kernel(uint32_t cw, uint32_t vt, bool dense) {
  if (vt == SGPU_VAL_DOTVBYTE) return dense ? diversify_documents_kernel<2, VT_DVB, true> : diversify_documents_kernel<2, VT_DVB, false>;
  if (vt == SGPU_VAL_FIXEDU8) {
    if (cw == 2) return dense ? diversify_documents_kernel<2, VT_U8, true> : diversify_documents_kernel<2, VT_U8, false>;
    return dense ? diversify_documents_kernel<4, VT_U8, true> : diversify_documents_kernel<4, VT_U8, false>;
  }
  if (cw == 2) return dense ? diversify_documents_kernel<2, VT_F16, true> : diversify_documents_kernel<2, VT_F16, false>;
  return dense ? diversify_documents_kernel<4, VT_F16, true> : diversify_documents_kernel<4, VT_F16, false>;
}

}  // namespace

sgpu_status diversify_kernel_fit(uint32_t cw, uint32_t vt, bool dense, uint32_t lds, int* per_cu) {
  DiversifyKernel kern = diversify_kernel(cw, vt, dense);
  HIP_TRY(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(per_cu, kern, (int)kDiversifyBlock, lds));
  return SGPU_OK;
}

sgpu_status diversify_kernel_launch(uint32_t cw, uint32_t vt, bool dense, uint32_t grid, uint32_t lds, hipStream_t stream,
                                    const DiversifyArgs& a) {
  hipLaunchKernelGGL(diversify_kernel(cw, vt, dense), dim3(grid), dim3(kDiversifyBlock), lds, stream, a);
  HIP_TRY(hipGetLastError());
  return SGPU_OK;
}

}  // namespace sgpu
