// score_lookup.hpp — what the kernels that score caller-given documents share (score_documents_kernel in
// score_documents.hip, explain_documents_kernel in explain_documents.hip): the tile, the form of the query's weight table
// in LDS and its lookup; and what score_documents.hip, which runs both kinds of call, sees of explain_documents.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "device_prims.hpp"
#include "hip_util.hpp"

namespace sgpu {

constexpr uint32_t kScoreTile = 128;             // candidates per tile
constexpr uint32_t kScoreDenseLds = 128u << 10;  // the dense table is used where (dim + 1) floats fit this
constexpr uint32_t kHashEmpty = 0xffffffffu;
constexpr uint32_t kNoQuery = 0xffffffffu;

// the query's weight of component c (0.0: the query does not carry it). Dense: tab[c], c <= dim. Hash: linear probing
// from the component's slot; the table is at most half full, so a probe sequence always meets an empty slot.
template <bool DENSE>
__device__ __forceinline__ float weight_of(const uint8_t* smem, uint32_t c, uint32_t slot_bits) {
  if (DENSE) return ((const float*)smem)[c];
  const uint32_t* keys = (const uint32_t*)smem;
  const float* wts = (const float*)(smem + ((size_t)4u << slot_bits));
  const uint32_t mask = (1u << slot_bits) - 1u;
  uint32_t slot = (c * 2654435761u) >> (32u - slot_bits);
  for (;;) {
    const uint32_t k = keys[slot];
    if (k == kHashEmpty) return 0.0f;
    if (k == c) return wts[slot];
    slot = (slot + 1u) & mask;
  }
}

// ---- explain_documents.hip ----
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
// the explain kernel of (component width, value type, lookup form): workgroups of `block` threads with `lds` bytes of
// table that fit a CU (sets the kernel's LDS attribute), and its launch
sgpu_status explain_kernel_fit(uint32_t cw, uint32_t vt, bool dense, uint32_t block, uint32_t lds, int* per_cu);
sgpu_status explain_kernel_launch(uint32_t cw, uint32_t vt, bool dense, uint32_t grid, uint32_t block, uint32_t lds, hipStream_t stream,
                                  const ExplainArgs& a);

// ---- expand_queries.hip ----
constexpr uint32_t kExpandBlock = 1024;   // threads of a workgroup (16 wavefronts: the kernel's wave totals are sized by it)
struct ExpandArgs {
  const uint8_t* fwd;         // the index, as ScoreArgs
  const uint64_t* doc_ref;
  const uint64_t* q_off;      // the call's staged queries and candidate offsets
  const uint32_t* q_comp;
  const float* q_val;
  const uint64_t* cand_off;
  const uint32_t* cand;       // the launch's candidate ids and weights: candidate i of the call at [i - cand_base]
  const float* cand_w;
  float* table;               // !DENSE: gridDim.x tables of dim + 1 floats (DENSE: the table is in LDS)
  uint32_t* out_comps;        // the call's rows [nq x t] and counts
  float* out_vals;
  uint32_t* out_n;
  uint64_t cand_base;
  uint32_t q_first, q_last;   // the launch's queries [q_first, q_last)
  uint32_t dim;
  uint32_t t;
  float alpha;
  float val_scale;
};
// the expand kernel of (component width, value type, table form): as the explain kernel's pair above
sgpu_status expand_kernel_fit(uint32_t cw, uint32_t vt, bool dense, uint32_t lds, int* per_cu);
sgpu_status expand_kernel_launch(uint32_t cw, uint32_t vt, bool dense, uint32_t grid, uint32_t lds, hipStream_t stream, const ExpandArgs& a);

// ---- diversify_documents.hip ----
constexpr uint32_t kDiversifyBlock = 1024;   // threads of a workgroup (16 wavefronts: the kernel's wave maxima are sized by it)
struct DiversifyArgs {
  const uint8_t* fwd;         // the index, as ScoreArgs
  const uint64_t* doc_ref;
  const uint64_t* q_off;      // the call's staged queries and candidate offsets
  const uint32_t* q_comp;
  const float* q_val;
  const uint64_t* cand_off;
  const uint32_t* cand;       // the launch's candidate ids: candidate i of the call at [i - cand_base]
  float* row_scores;          // the call's rows [nq x k] (zeroed before the first launch) and counts
  float* row_pen;
  uint64_t* row_ids;
  uint32_t* row_n;
  uint64_t cand_base;
  uint32_t q_first, q_last;   // the launch's queries [q_first, q_last)
  uint32_t dim;
  uint32_t slot_bits;         // hash table: log2 of its slots (sized for the longest query AND the longest candidate document)
  uint32_t table_bytes;       // LDS: the table, then the entry state - ids, rels, pens of `cap` entries each
  uint32_t cap;               // >= the candidates of every query of the call
  uint32_t k;
  float lambda, mu;
  float val_scale;
};
// the diversify kernel of (component width, value type, table form): as the explain kernel's pair above
sgpu_status diversify_kernel_fit(uint32_t cw, uint32_t vt, bool dense, uint32_t lds, int* per_cu);
sgpu_status diversify_kernel_launch(uint32_t cw, uint32_t vt, bool dense, uint32_t grid, uint32_t lds, hipStream_t stream,
                                    const DiversifyArgs& a);

}  // namespace sgpu
