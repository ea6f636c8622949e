// score_state.hpp — what the launchers of the candidate calls share (score_run in score_documents.hip with the selection of
// rerank_select.hip behind it, expand_run in expand_queries.hip, diversify_run in diversify_documents.hip, collapse_run in
// collapse_documents.hip, fuse_run in fuse_documents.hip): the replica's
// stream, mutex and recycled scratch, and the steps every launcher takes - the form of the weight table, the candidates
// a launch may take, the call's queries and a launch's ids staged, the cut of a call into launches of whole queries,
// the events around a kernel. The kernels' side of the same calls is score_lookup.hpp.
#pragma once
#include <algorithm>
#include <cstdlib>
#include <mutex>
#include <vector>

#include "score_lookup.hpp"

namespace sgpu {

constexpr uint32_t kScoreChunk = 1u << 20;   // candidates per launch (SGPU_SCORE_CHUNK overrides)

// What the last call of one kind measured (the sgpu_debug_*_stats test hooks): device time of its kernels, its launches,
// the table's form, the geometry of its last launch, and two figures of the call's own.
struct CallStats {
  double kernel_ms = 0;
  uint32_t launches = 0, dense = 0, grid = 0, block = 0, lds = 0;
  double extra[2] = {0, 0};
  void begin() { kernel_ms = 0, launches = 0, extra[0] = extra[1] = 0; }   // a call starts: what it sums up
};

struct SelTask {   // rerank_select.hip: one selection task, 32 bytes
  uint32_t kind;       // SEL_RAW: candidates [src, src + n) of the launch; SEL_KEYS: slots [src, src + n)
  uint32_t src, n;
  uint32_t extra;      // SEL_KEYS: a carry slot (0 / 1) that is one more source, or kSelNone
  uint32_t dst_kind;
  uint32_t dst;        // slot, query (its row) or carry slot
  uint32_t pad0, pad1;
};

// Per replica: the candidate calls' stream, their recycled scratch and what the last call of each kind measured.
struct ScoreState {
  int device = -1;
  uint32_t n_cu = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr, ev2 = nullptr;
  std::mutex mu;   // one candidate call at a time on this replica
  DeviceBuffer q_off, q_comp, q_val, cand_off;   // the call's queries, and its candidate offsets where the kernel reads them
  DeviceBuffer tiles, cand, scores;              // a launch's tiles, candidate ids and scores
  // rerank: a launch's selection tasks and k-key slots, the two carry slots, the call's rows (scores, ids, counts)
  DeviceBuffer sel_tasks, slots, carry, row_scores, row_ids, row_n;
  DeviceBuffer terms;   // explain: a launch's term counts and its four arrays of rows
  // expand: the call's rows (components, values, counts), a launch's candidate weights and, where the table does not fit
  // LDS, one table per workgroup
  DeviceBuffer x_comps, x_vals, x_n, x_w, x_table;
  DeviceBuffer d_pen;           // diversify: the call's penalty rows (scores, ids and counts: rerank's row buffers)
  // collapse: a launch's group keys and the queries of its selection launches by tier, the call's rows (group keys, best
  // members' scores, member counts; group scores, best ids and counts: rerank's row buffers)
  DeviceBuffer c_groups, c_tasks, c_row_groups, c_row_best, c_row_members;
  // fuse: a launch's external scores (its queries by tier: collapse's c_tasks), the call's rows (sparse and external scores,
  // both ranks; fused scores, ids and counts: rerank's row buffers)
  DeviceBuffer f_ext, f_row_sparse, f_row_ext, f_row_rank_s, f_row_rank_e;
  std::vector<uint4> h_tiles;   // host staging of a launch
  std::vector<uint32_t> h_ids;
  std::vector<std::vector<SelTask>> sel_rounds;   // [round * tiers + tier]
  std::vector<SelTask> h_sel_tasks;
  std::vector<uint32_t> h_col_tasks;   // collapse, fuse: a launch's queries by tier
  CallStats score_stats;       // score, rerank, explain; extra: device ms of the selection kernels, merge rounds run
  CallStats expand_stats;      // extra: bytes of the global tables
  CallStats diversify_stats;   // extra: rounds of the call's longest query
  CallStats collapse_stats;    // extra: device ms of the selection kernels, selection launches
  CallStats fuse_stats;        // the same
};

// score_documents.hip: the replica's state, made on its first candidate call; and what a sgpu_debug_*_stats hook reports
// from it - out8 = {kernel ms, launches, dense, grid, block, lds, extra[0], extra[1]}, which the hooks with another slot
// order rearrange -, or false where no call has made the state
sgpu_status score_state_of(sgpu_index* idx, uint32_t replica, ScoreState** out);
bool call_stats_out(sgpu_index* idx, uint32_t replica, CallStats ScoreState::*which, double* out8);

inline sgpu_status score_reserve(ScoreState* s, DeviceBuffer& b, uint64_t bytes) { return b.reserve(s->stream, bytes, "scoring documents"); }

// The form of the weight table: dense where the vocabulary fits (test hook SGPU_SCORE_LOOKUP=2: hash although it fits),
// else the hash table sized for `longest`, the most components it has to hold at a time (<= 8192: at most 2^14 slots,
// 128 KiB).
struct LookupForm {
  bool dense;
  uint32_t slot_bits;     // hash: log2 of its slots
  uint32_t table_bytes;   // of the form chosen
};
inline LookupForm lookup_form(const HostIndex& h, uint32_t longest) {
  const uint64_t dense_bytes = ((h.dim + 1) * 4 + 15) & ~15ull;
  bool dense = dense_bytes <= kScoreDenseLds;
  if (test_hooks_on()) {
    const char* v = std::getenv("SGPU_SCORE_LOOKUP");
    if (v && *v == '2') dense = false;
  }
  uint32_t slot_bits = 6;
  while ((1u << slot_bits) < 2u * longest) ++slot_bits;
  return {dense, slot_bits, dense ? (uint32_t)dense_bytes : (8u << slot_bits)};
}

// the candidates a launch may take: `budget` unless SGPU_SCORE_CHUNK says otherwise
inline uint64_t launch_budget(uint64_t budget = kScoreChunk) {
  if (const char* v = std::getenv("SGPU_SCORE_CHUNK"))
    if (*v) budget = std::max<uint64_t>(1, std::strtoull(v, nullptr, 10));
  return std::min<uint64_t>(budget, 1ull << 28);
}

// the workgroups a launch may have, lowered by the test hook `env` (fewer workgroups: each takes many queries in turn)
inline uint64_t hooked_grid(uint64_t max_grid, const char* env) {
  if (test_hooks_on())
    if (const char* v = std::getenv(env))
      if (*v) max_grid = std::max<uint64_t>(1, std::min<uint64_t>(max_grid, std::strtoull(v, nullptr, 10)));
  return max_grid;
}

// the call's queries to s->q_off, q_comp, q_val, and its candidate offsets (null: the kernel does not read them) to
// s->cand_off
inline sgpu_status stage_queries(ScoreState* s, const uint64_t* q_off, const uint32_t* comps, const float* vals, uint32_t nq,
                                 const uint64_t* cand_off) {
  const uint64_t qnnz = q_off[nq];
  sgpu_status st;
  if ((st = score_reserve(s, s->q_off, (uint64_t)(nq + 1) * 8)) != SGPU_OK || (st = score_reserve(s, s->q_comp, qnnz * 4)) != SGPU_OK ||
      (st = score_reserve(s, s->q_val, qnnz * 4)) != SGPU_OK ||
      (cand_off && (st = score_reserve(s, s->cand_off, (uint64_t)(nq + 1) * 8)) != SGPU_OK))
    return st;
  HIP_TRY(hipMemcpyAsync(s->q_off.p, q_off, (uint64_t)(nq + 1) * 8, hipMemcpyHostToDevice, s->stream));
  if (cand_off) HIP_TRY(hipMemcpyAsync(s->cand_off.p, cand_off, (uint64_t)(nq + 1) * 8, hipMemcpyHostToDevice, s->stream));
  if (qnnz) {
    HIP_TRY(hipMemcpyAsync(s->q_comp.p, comps, qnnz * 4, hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipMemcpyAsync(s->q_val.p, vals, qnnz * 4, hipMemcpyHostToDevice, s->stream));
  }
  return SGPU_OK;
}

// candidates [first, first + n) of the call to s->cand, as the u32 the kernels index doc_ref with
inline sgpu_status stage_ids(ScoreState* s, const uint64_t* cand_ids, uint64_t first, uint64_t n) {
  s->h_ids.resize(n);
  for (uint64_t i = 0; i < n; ++i) s->h_ids[i] = (uint32_t)cand_ids[first + i];
  const sgpu_status st = score_reserve(s, s->cand, n * 4);
  if (st != SGPU_OK) return st;
  if (n) HIP_TRY(hipMemcpyAsync(s->cand.p, s->h_ids.data(), n * 4, hipMemcpyHostToDevice, s->stream));
  return SGPU_OK;
}

// The cut of a call into launches of whole queries: the launch that begins at query *q takes the consecutive queries
// whose candidates fit the budget, a query of more candidates than the budget alone. Returns its first query and leaves
// *q behind its last: the launch is [qa, *q), its candidates [cand_off[qa], cand_off[*q]).
inline uint32_t next_whole_queries(const uint64_t* cand_off, uint32_t nq, uint64_t budget, uint32_t* q) {
  const uint32_t qa = *q;
  const uint64_t first = cand_off[qa];
  ++*q;
  while (*q < nq && cand_off[*q + 1] - first <= budget) ++*q;
  return qa;
}

// A kernel between the events ev0 and ev1 on the state's stream; and, after what the launcher enqueued behind it, the
// wait for the stream (the staging vectors and the scratch are the next launch's) and the launch added to the stats.
template <class Args>
sgpu_status launch_timed(ScoreState* s, void (*kern)(Args), uint32_t grid, uint32_t block, uint32_t lds, const Args& a) {
  HIP_TRY(hipEventRecord(s->ev0, s->stream));
  const sgpu_status st = kernel_launch(kern, grid, block, lds, s->stream, a);
  if (st != SGPU_OK) return st;
  HIP_TRY(hipEventRecord(s->ev1, s->stream));
  return SGPU_OK;
}
inline sgpu_status launch_done(ScoreState* s, CallStats* cs) {
  HIP_TRY(hipStreamSynchronize(s->stream));
  float ms = 0.0f;
  HIP_TRY(hipEventElapsedTime(&ms, s->ev0, s->ev1));
  cs->kernel_ms += ms;
  cs->launches += 1;
  return SGPU_OK;
}

// ---- score_documents.hip: the score kernel for a launcher of another file (collapse_documents.hip, fuse_documents.hip).
// score_pass_begin picks the kernel's form and geometry for a call whose queries are staged; score_pass_launch scores the candidates of the whole
// queries [qa, qb) - tiles cut, ids staged, one score per candidate to s->scores in the candidates' order, the kernel
// between ev0 and ev1 -, and what the caller enqueues behind it reads s->scores and s->cand on the same stream.
struct ScorePass {
  LookupForm form;
  uint32_t block = 0, per_cu = 0;
};
sgpu_status score_pass_begin(const HostIndex& h, uint32_t max_nnz, ScorePass* sp);
sgpu_status score_pass_launch(ScoreState* s, const HostIndex& h, const DevView& view, const ScorePass& sp, const uint64_t* cand_off,
                              const uint64_t* cand_ids, uint32_t qa, uint32_t qb, uint32_t* grid);

// ---- rerank_select.hip: the selection behind a rerank call's score kernels
struct SelTier {
  uint32_t cap, team;   // keys per task (a power of two), threads per task (a multiple of 64 dividing the workgroup)
};
struct RerankCall {
  uint32_t k = 0;
  uint32_t chunk = 0;              // C: keys a workgroup-wide team sorts
  uint32_t n_tiers = 0;
  SelTier tiers[3];
  int carry_cur = -1;              // the carry slot the open query's survivors lie in (-1: no query is open)
  float* out_scores = nullptr;
  uint64_t* out_doc_ids = nullptr;
  uint32_t* out_n = nullptr;
};
// chunk and tiers from k (and the test hook SGPU_RERANK_CHUNK)
void rerank_setup(RerankCall* rr);
// the call's rows on the device, zeroed; the selection over one launch's scores - candidates [first, last) of the call,
// the queries from q_first on - enqueued behind its score kernel, ev2 behind it; the rows back to the caller
sgpu_status rerank_rows_begin(ScoreState* s, const RerankCall* rr, uint32_t nq);
sgpu_status rerank_select(ScoreState* s, RerankCall* rr, const uint64_t* cand_off, uint32_t nq, uint32_t q_first, uint64_t first,
                          uint64_t last);
sgpu_status rerank_rows_end(ScoreState* s, const RerankCall* rr, uint32_t nq);

}  // namespace sgpu
