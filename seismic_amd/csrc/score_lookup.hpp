// score_lookup.hpp — what the kernels of the candidate calls share (score_documents.hip, explain_documents.hip,
// expand_queries.hip, diversify_documents.hip): the weight table in LDS - its two forms, the lookup, the insert, a query
// moving in and out -, a doc_ref word taken apart, the loop in which a 16-lane group scores documents against the
// table, the walk of one document by a whole workgroup; and how a kernel's variant of (component width, value type,
// table form) is chosen, fitted to a CU and launched. The launchers' side of the same calls is score_state.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "device_prims.hpp"
#include "hip_util.hpp"

namespace sgpu {

constexpr uint32_t kScoreTile = 128;             // candidates per tile
constexpr uint32_t kScoreDenseLds = 128u << 10;  // the dense table is used where (dim + 1) floats fit this
constexpr uint32_t kHashEmpty = 0xffffffffu;
constexpr uint32_t kNoQuery = 0xffffffffu;

// ---- the weight table: DENSE, dim + 1 floats indexed by the component; else an open-addressing hash table of
// 2^slot_bits {component, weight} slots (the keys, then the weights), linear probing from the component's home slot, at
// most half full: a probe sequence always meets an empty slot. `tid` of `nt` threads share the loops. The barriers
// around every function here are the caller's.
struct WeightTable {
  uint8_t* smem;
  uint32_t dim, slot_bits, slots;
};
SGPU_DEV WeightTable weight_table(uint8_t* smem, uint32_t dim, uint32_t slot_bits) { return {smem, dim, slot_bits, 1u << slot_bits}; }
SGPU_DEV uint32_t table_home(uint32_t c, uint32_t slot_bits) { return (c * 2654435761u) >> (32u - slot_bits); }

// the table's weight of component c (0.0: it does not hold c)
template <bool DENSE>
SGPU_DEV float weight_of(const WeightTable& t, uint32_t c) {
  if (DENSE) return ((const float*)t.smem)[c];
  const uint32_t* keys = (const uint32_t*)t.smem;
  const float* wts = (const float*)(t.smem + ((size_t)4u << t.slot_bits));
  const uint32_t mask = (1u << t.slot_bits) - 1u;
  uint32_t slot = table_home(c, t.slot_bits);
  for (;;) {
    const uint32_t k = keys[slot];
    if (k == kHashEmpty) return 0.0f;
    if (k == c) return wts[slot];
    slot = (slot + 1u) & mask;
  }
}

// component c, which the table does not hold yet, with the weight w
template <bool DENSE>
SGPU_DEV void table_put(const WeightTable& t, uint32_t c, float w) {
  if (DENSE) {
    ((float*)t.smem)[c] = w;
    return;
  }
  uint32_t* keys = (uint32_t*)t.smem;
  float* wts = (float*)(t.smem + (size_t)t.slots * 4u);
  uint32_t slot = table_home(c, t.slot_bits);
  while (atomicCAS(&keys[slot], kHashEmpty, c) != kHashEmpty) slot = (slot + 1u) & (t.slots - 1u);
  wts[slot] = w;
}

// the whole table: every weight 0.0 / every slot empty
template <bool DENSE>
SGPU_DEV void table_reset(const WeightTable& t, uint32_t tid, uint32_t nt) {
  if (DENSE) {
    for (uint32_t i = tid; i <= t.dim; i += nt) ((float*)t.smem)[i] = 0.0f;
  } else {
    for (uint32_t i = tid; i < t.slots; i += nt) ((uint32_t*)t.smem)[i] = kHashEmpty;
  }
}

// Query q of the call into an empty table, and out of it again (dense: its own entries, hash: wholesale). `a` is any of
// the kernels' argument structs: read are q_off, q_comp, q_val and val_scale.
// (fixed-u8 codes: value = code * val_scale, a power of two folded into the weight (exact), as the search kernels do)
template <int VT, bool DENSE, class Args>
SGPU_DEV void table_fill_query(const WeightTable& t, const Args& a, uint32_t q, uint32_t tid, uint32_t nt) {
  const uint64_t b0 = a.q_off[q], b1 = a.q_off[q + 1];
  for (uint64_t j = b0 + tid; j < b1; j += nt) {
    const uint32_t c = a.q_comp[j];
    table_put<DENSE>(t, c, Vt<VT>::half ? a.q_val[j] : __fmul_rn(a.q_val[j], a.val_scale));
  }
}
template <bool DENSE, class Args>
SGPU_DEV void table_clear_query(const WeightTable& t, const Args& a, uint32_t q, uint32_t tid, uint32_t nt) {
  if (DENSE) {
    const uint64_t p0 = a.q_off[q], p1 = a.q_off[q + 1];
    for (uint64_t j = p0 + tid; j < p1; j += nt) ((float*)t.smem)[a.q_comp[j]] = 0.0f;
  } else {
    table_reset<DENSE>(t, tid, nt);
  }
}

// ---- documents
// A DevView::doc_ref word taken apart: the stored elements, whether a DotVByte index keeps the record in the raw form
// (always false for the other value types), and the record. The word 0 is a document of no elements.
template <int VT>
struct DocRef {
  uint32_t len;
  bool raw;
  const uint8_t* rec;
};
template <int VT>
SGPU_DEV DocRef<VT> doc_ref_of(const uint8_t* fwd, uint64_t ref) {
  return {(uint32_t)ref & LenMask<VT>::v, Vt<VT>::sliced && ((uint32_t)ref & kRawBit) != 0u, fwd + (size_t)(ref >> 16) * 16u};
}

// N documents scored against the table by ONE 16-lane group, all in flight: lane l takes elements [8 l, 8 l + 8) of each
// pass of 128, its accumulator the sum in increasing e, the partials combined by group16_sum - the canonical order of a
// score (score_documents_kernel's loop, which keeps its own text). done(u, score) is called in every lane with document
// u's score, in the order of u; what to do with it, and which documents are live (doc_ref_of(fwd, 0) for the others: no
// elements), is the caller's.
template <typename CT, int VT, bool DENSE, uint32_t N, class F>
SGPU_DEV void group_score(const WeightTable& t, const DocRef<VT> (&doc)[N], uint32_t l, F&& done) {
  float acc[N];
  uint32_t max_len = 0;
#pragma unroll
  for (uint32_t u = 0; u < N; ++u) {
    acc[u] = 0.0f;
    max_len = max(max_len, doc[u].len);
  }
  for (uint32_t e0 = l * 8u; e0 < max_len; e0 += 128u) {
    DocChunk<CT, VT> d[N];
#pragma unroll
    for (uint32_t u = 0; u < N; ++u)
      if (e0 < doc[u].len) load_pass<CT, VT>(d[u], doc[u].rec, doc[u].len, doc[u].raw, e0);
#pragma unroll
    for (uint32_t u = 0; u < N; ++u)
      if (e0 < doc[u].len) {
        uint32_t c[8];
        if (Vt<VT>::sliced && doc[u].raw) {   // (the branch stays at the call: inside a helper the code comes out different)
          raw_pass_components<CT, VT>(d[u], c);
        } else {
          slice_components<CT, VT>(d[u], c);
        }
        place_values<CT, VT>(d[u], doc[u].raw);
        float w[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) w[i] = weight_of<DENSE>(t, c[i]);
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[u] = __fadd_rn(acc[u], __fmul_rn(w[i], slice_value<VT>(d[u].v, i)));
      }
  }
#pragma unroll
  for (uint32_t u = 0; u < N; ++u) done(u, group16_sum(acc[u]));
}

// One document by the whole workgroup of `ng` 16-lane groups, its passes of 128 elements dealt over the groups:
// f(component, value) for every element e < len, the value as slice_value gives it. Elements e >= len (slice padding:
// the last component repeated) are MASKED - their lane would race with the one that holds the component's real element.
// (expand_queries_kernel walks a document the same way in its own text: through this helper one of its probe rows
// measured slower than the parent's spread.)
template <typename CT, int VT, class F>
SGPU_DEV void workgroup_walk_doc(const uint8_t* fwd, uint64_t ref, uint32_t ng, F&& f) {
  const uint32_t g = threadIdx.x >> 4, l = threadIdx.x & 15u;
  const DocRef<VT> doc = doc_ref_of<VT>(fwd, ref);
  for (uint32_t p0 = g * 128u; p0 < doc.len; p0 += ng * 128u) {
    const uint32_t e0 = p0 + l * 8u;
    if (e0 >= doc.len) continue;
    DocChunk<CT, VT> d;
    load_pass<CT, VT>(d, doc.rec, doc.len, doc.raw, e0);
    uint32_t c[8];
    if (Vt<VT>::sliced && doc.raw) {
      raw_pass_components<CT, VT>(d, c);
    } else {
      slice_components<CT, VT>(d, c);
    }
    place_values<CT, VT>(d, doc.raw);
#pragma unroll
    for (int i = 0; i < 8; ++i)
      if (e0 + (uint32_t)i < doc.len) f(c[i], slice_value<VT>(d.v, i));
  }
}

// ---- variants
// f(component width, value type, dense) with the three as std::integral_constants: the ten instances every kernel of
// these calls has (a DotVByte index has u16 components).
template <class F>
auto for_variant(uint32_t cw, uint32_t vt, bool dense, F&& f) {
  auto form = [&](auto CW, auto VT) { return dense ? f(CW, VT, std::true_type{}) : f(CW, VT, std::false_type{}); };
  using W2 = std::integral_constant<int, 2>;
  using W4 = std::integral_constant<int, 4>;
  if (vt == SGPU_VAL_DOTVBYTE) return form(W2{}, std::integral_constant<int, VT_DVB>{});
  if (vt == SGPU_VAL_FIXEDU8) return cw == 2 ? form(W2{}, std::integral_constant<int, VT_U8>{}) : form(W4{}, std::integral_constant<int, VT_U8>{});
  return cw == 2 ? form(W2{}, std::integral_constant<int, VT_F16>{}) : form(W4{}, std::integral_constant<int, VT_F16>{});
}

// workgroups of `block` threads with `lds` bytes of dynamic LDS that fit a CU (sets the kernel's LDS attribute) ...
template <class Args>
sgpu_status kernel_fit(void (*kern)(Args), uint32_t block, uint32_t lds, int* per_cu) {
  HIP_TRY(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(per_cu, kern, (int)block, lds));
  return SGPU_OK;
}
// ... and a launch
template <class Args>
sgpu_status kernel_launch(void (*kern)(Args), uint32_t grid, uint32_t block, uint32_t lds, hipStream_t stream, const Args& a) {
  hipLaunchKernelGGL(kern, dim3(grid), dim3(block), lds, stream, a);
  HIP_TRY(hipGetLastError());
  return SGPU_OK;
}

// ---- explain_documents.hip, whose kernel score_documents.hip's launcher runs in the score kernel's place
struct ExplainArgs {
  const uint8_t* fwd;        // as ScoreArgs (score_documents.hip): the index, the call's staged queries, a launch's tiles and ids
  const uint64_t* doc_ref;
  const uint64_t* q_off;
  const uint32_t* q_comp;
  const float* q_val;
  const uint4* tiles;
  const uint32_t* cand;
  float* scores;             // per candidate of the launch: its score and the number of its terms
  uint32_t* n_terms;
  uint32_t* comps;           // rows of m per candidate of the launch
  float* q_vals;
  float* d_vals;
  float* products;
  uint32_t n_tiles;
  uint32_t dim;
  uint32_t slot_bits;
  uint32_t m;
  float val_scale;
};
using ExplainKernel = void (*)(ExplainArgs);
ExplainKernel explain_kernel(uint32_t cw, uint32_t vt, bool dense);

}  // namespace sgpu
