// score_documents.hip — scores of caller-given documents on the device (sgpu_score_documents).
//
// A score is what the search kernels return for the document (search_kernel.inc: score_class), bit for bit: the full
// query's dot product over the document's stored values in the canonical order - 16 accumulators, element e goes to
// accumulator (e / 8) % 16 in increasing e, the partials combined by t[j] += t[j ^ s], s = 8, 4, 2, 1; f32 multiply
// then add, each rounded once. Components the query does not carry resolve to the weight 0.0 and are added as +-0.0,
// which leaves an accumulator that started at +0.0 bit-identical to skipping them; padding elements of a record carry
// the value 0 and do the same.
//
// Unit of work: a TILE of at most kScoreTile candidates of ONE query (the host cuts every query's candidate list into
// tiles; the tiles of all queries of a launch go over the grid). A workgroup keeps the query's weights in LDS - a
// dense f32 table over the vocabulary where dim + 1 floats fit kScoreDenseLds bytes, else an open-addressing hash table
// {component, weight} at most half full - and rebuilds it only when its next tile belongs to another query. Every
// candidate is scored by a 16-lane group: lane l loads elements [8 l, 8 l + 8) of each 128-element round with 16-byte
// loads, kScoreDocs candidates per group in flight. The record forms are those pack_index.cpp writes - raw, and sliced
// for the documents of a DotVByte index that bit 15 of the ref's length field does not mark as raw -; record.hpp
// describes them and decodes them, here as in the search kernels.
//
// sgpu_rerank_documents adds the SELECTION on the device: per query the k best DISTINCT candidates, score descending, id
// ascending. score_documents_kernel is used as it is and leaves a launch's scores in the device scratch; what follows it
// on the same stream is rerank_select_kernel, once per round.
//   key     ordered(score bits) << 32 | ~id, a u64: ordered() is the monotone integer image of an f32 (flip all bits of
//           a negative, the sign bit of the others), so a larger key is a better candidate - higher score, then lower
//           id. A score is never -0.0 (accumulators start at +0.0 and are only added to), so the image's order is the
//           numeric order on finite scores. Equal ids carry equal scores, hence equal keys: after a descending sort a
//           duplicate is a key equal to its predecessor. Key 0 (the image of the NaN 0xffffffff with id 2^32 - 1, which
//           no finite score has) is the padding.
//   task    a TEAM of threads takes at most `cap` keys of ONE query - a chunk of the launch's candidates (keys made from
//           score and id) or the survivors of earlier tasks (k-key slots) -, sorts them in LDS (bitonic, descending,
//           padded to cap with 0), drops the duplicates and the padding, compacts (a prefix sum over the team) and
//           writes the first k: to the query's result row if the task is the query's last, else to a slot, zero-padded.
//   rounds  round 0 holds the chunk tasks of every query part of the launch, round r > 0 merges each part's slots of
//           round r - 1 in groups of floor(C / k) >= 2 until one task is left; rounds are separate launches on the
//           call's stream, which is all the ordering there is (no loop waits on another workgroup). Correct because the
//           distinct top-k of a union is the distinct top-k of the union of the parts' distinct top-k.
//   carry   a query cut by a launch boundary ends its part in one of two carry slots; its next part's first merge task
//           takes that slot as one more source. Only one query can be open at a boundary; the slots alternate, because
//           a launch's last part may write its carry in round 0 while its first part reads the other in a later round.
//   sizes   C = 2048 keys: the smallest C with floor(C / k) >= 2 at k = 1024; 16 KiB of LDS per 256-thread workgroup,
//           so the 8 workgroups that fill a CU's 2048 threads hold 128 of its 160 KiB. A larger C buys fewer merge rounds
//           with more bitonic steps (log2(C) (log2(C) + 1) / 2 barriers each) and fewer workgroups per CU. A task of few
//           keys goes to a smaller tier instead of being padded to C: 128 keys per wave64 (four tasks per workgroup, 28
//           steps of one compare-exchange per lane: the 10 000 x 100 shape) or 512 keys per wave64. Every workgroup has
//           256 threads; the barriers of the tiers' fixed step counts are uniform over it.
//
// sgpu_explain_documents runs through the same launcher (score_run: the staged queries, the tiles, the cuts into launches,
// the per-replica stream, mutex and scratch) with explain_documents.hip's kernel in score_documents_kernel's place; what
// the two kernels share is score_lookup.hpp.
//
// sgpu_expand_queries has a launcher of its own, expand_run, because its unit of work is a whole query and not a tile of
// candidates: it cuts between queries only. It shares ScoreState with score_run - the stream, the mutex, the staged
// queries and ids - and adds the buffers its rows and tables need; the kernel is expand_queries.hip's.
//
// sgpu_diversify_documents (MMR selection) has diversify_run, cut between queries as expand_run cuts: a workgroup of
// diversify_documents.hip's kernel keeps a whole query's entries in LDS. Its rows lie in rerank's row buffers plus one
// for the penalties.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <mutex>
#include <new>
#include <type_traits>
#include <vector>

#include "score_lookup.hpp"

namespace sgpu {

namespace {

constexpr uint32_t kScoreDocs = 2;               // candidates a 16-lane group has in flight
constexpr uint32_t kScoreChunk = 1u << 20;       // candidates per launch (SGPU_SCORE_CHUNK overrides)
constexpr uint64_t kExplainRowBytes = 64ull << 20;   // ... of an explain call: as many as this much of term rows holds

struct ScoreArgs {
  const uint8_t* fwd;        // DevView::fwd (the document-major records lie at its start in both forward layouts)
  const uint64_t* doc_ref;   // DevView::doc_ref
  const uint64_t* q_off;     // the call's queries, staged
  const uint32_t* q_comp;
  const float* q_val;
  const uint4* tiles;        // {query, first candidate of the tile in this launch, candidates, 0}
  const uint32_t* cand;      // the launch's candidate ids
  float* out;                // one score per candidate of the launch
  uint32_t n_tiles;
  uint32_t dim;
  uint32_t slot_bits;        // hash table: log2 of its slots
  float val_scale;
};

template <int CW, int VT, bool DENSE>
__global__ __launch_bounds__(1024) void score_documents_kernel(ScoreArgs a) {
  using CT = typename std::conditional<CW == 2, uint16_t, uint32_t>::type;
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const uint32_t tid = threadIdx.x, nt = blockDim.x;
  const uint32_t ng = nt >> 4, g = tid >> 4, l = tid & 15u;
  const uint32_t slots = 1u << a.slot_bits;
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
        // fixed-u8 codes: value = code * val_scale, a power of two folded into the weight (exact), as the search kernels do
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
    for (uint32_t base = 0; base < tile.z; base += ng * kScoreDocs) {
      uint32_t len[kScoreDocs], idx[kScoreDocs];
      const uint8_t* rec[kScoreDocs];
      bool raw[kScoreDocs];
      float acc[kScoreDocs];
      uint32_t max_len = 0;
#pragma unroll
      for (uint32_t u = 0; u < kScoreDocs; ++u) {
        idx[u] = base + u * ng + g;
        const uint64_t ref = idx[u] < tile.z ? a.doc_ref[a.cand[tile.y + idx[u]]] : 0ull;
        len[u] = (uint32_t)ref & LenMask<VT>::v;
        raw[u] = Vt<VT>::sliced && ((uint32_t)ref & kRawBit) != 0u;
        rec[u] = a.fwd + (size_t)(ref >> 16) * 16u;
        acc[u] = 0.0f;
        max_len = max(max_len, len[u]);
      }
      for (uint32_t e0 = l * 8u; e0 < max_len; e0 += 128u) {
        DocChunk<CT, VT> d[kScoreDocs];
#pragma unroll
        for (uint32_t u = 0; u < kScoreDocs; ++u)
          if (e0 < len[u]) load_pass<CT, VT>(d[u], rec[u], len[u], raw[u], e0);
#pragma unroll
        for (uint32_t u = 0; u < kScoreDocs; ++u)
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
      for (uint32_t u = 0; u < kScoreDocs; ++u) {
        float r = acc[u];
        r = __fadd_rn(r, __shfl_xor(r, 8, 16));
        r = __fadd_rn(r, __shfl_xor(r, 4, 16));
        r = __fadd_rn(r, __shfl_xor(r, 2, 16));
        r = __fadd_rn(r, __shfl_xor(r, 1, 16));
        if (l == 0 && idx[u] < tile.z) a.out[tile.y + idx[u]] = r;
      }
    }
  }
}

using ScoreKernel = void (*)(ScoreArgs);
ScoreKernel score_kernel(uint32_t cw, uint32_t vt, bool dense) {
  if (vt == SGPU_VAL_DOTVBYTE) return dense ? score_documents_kernel<2, VT_DVB, true> : score_documents_kernel<2, VT_DVB, false>;
  if (vt == SGPU_VAL_FIXEDU8) {
    if (cw == 2) return dense ? score_documents_kernel<2, VT_U8, true> : score_documents_kernel<2, VT_U8, false>;
    return dense ? score_documents_kernel<4, VT_U8, true> : score_documents_kernel<4, VT_U8, false>;
  }
  if (cw == 2) return dense ? score_documents_kernel<2, VT_F16, true> : score_documents_kernel<2, VT_F16, false>;
  return dense ? score_documents_kernel<4, VT_F16, true> : score_documents_kernel<4, VT_F16, false>;
}


// ---- selection (sgpu_rerank_documents) ----
constexpr uint32_t kRerankChunk = 2048;   // C: keys a workgroup-wide team sorts (test hook SGPU_RERANK_CHUNK lowers it)
constexpr uint32_t kSelBlock = 256;
constexpr uint32_t kSelNone = 0xffffffffu;
struct SelTier {
  uint32_t cap, team;   // keys per task (a power of two), threads per task (a multiple of 64 dividing kSelBlock)
};
constexpr SelTier kSelTiers[3] = {{128, 64}, {512, 64}, {kRerankChunk, 256}};
enum { SEL_RAW = 0, SEL_KEYS = 1 };             // a task's source
enum { SEL_TO_SLOT = 0, SEL_TO_ROW = 1, SEL_TO_CARRY = 2 };   // ... and its destination

struct SelTask {   // 32 bytes
  uint32_t kind;       // SEL_RAW: candidates [src, src + n) of the launch; SEL_KEYS: slots [src, src + n)
  uint32_t src, n;
  uint32_t extra;      // SEL_KEYS: a carry slot (0 / 1) that is one more source, or kSelNone
  uint32_t dst_kind;
  uint32_t dst;        // slot, query (its row) or carry slot
  uint32_t pad0, pad1;
};

struct SelArgs {
  const SelTask* tasks;
  const float* scores;      // the launch's scores and candidate ids (SEL_RAW)
  const uint32_t* cand;
  uint64_t* slots;          // k keys each
  uint64_t* carry;          // 2 slots
  float* row_scores;        // the call's rows [nq x k], zeroed before the first launch
  uint64_t* row_ids;
  uint32_t* row_n;
  uint32_t n_tasks, cap, team, k;
};

__device__ __forceinline__ uint64_t sel_key(float score, uint32_t id) {
  return ((uint64_t)ordered_u32(score) << 32) | (uint64_t)(~id);
}
__device__ __forceinline__ float sel_key_score(uint64_t key) { return ordered_u32_inv((uint32_t)(key >> 32)); }

__global__ __launch_bounds__(kSelBlock) void rerank_select_kernel(SelArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  __shared__ uint32_t wave_total[kSelBlock / 64];
  const uint32_t tid = threadIdx.x;
  const uint32_t cap = a.cap, team = a.team, k = a.k;
  const uint32_t teams = kSelBlock / team, tm = tid / team, lt = tid % team;
  const uint32_t waves = team / 64u, w = tid >> 6, lane = tid & 63u;
  uint64_t* key = (uint64_t*)smem + (size_t)tm * cap;
  const uint32_t per = cap >= team ? cap / team : 1u;   // consecutive sorted keys a thread looks at
  // (every bound below is workgroup-uniform: a team without a task runs the same barriers over padding)
  for (uint32_t base = blockIdx.x * teams; base < a.n_tasks; base += gridDim.x * teams) {
    const bool live = base + tm < a.n_tasks;
    SelTask t{};
    if (live) t = a.tasks[base + tm];
    const uint32_t n_src = t.kind == SEL_RAW ? t.n : t.n * k;            // keys of the contiguous source
    const uint32_t n_all = n_src + (t.kind == SEL_KEYS && t.extra != kSelNone ? k : 0u);   // (<= cap: the host's cut)
    for (uint32_t i = lt; i < cap; i += team) {
      uint64_t v = 0;
      if (i < n_src) {
        v = t.kind == SEL_RAW ? sel_key(a.scores[t.src + i], a.cand[t.src + i]) : a.slots[(size_t)t.src * k + i];
      } else if (i < n_all) {
        v = a.carry[(size_t)t.extra * k + (i - n_src)];
      }
      key[i] = v;
    }
    __syncthreads();
    // (its barriers are workgroup-uniform because every team of a launch sorts the same cap keys, a team without a task
    // its padding: keep cap a property of the launch, never of the task)
    bitonic_sort_lds<true>(key, cap, lt, team);
    // distinct keys that are no padding, counted per thread over its run of the sorted keys ...
    uint32_t cnt = 0;
    const uint32_t e0 = lt * per;
    if (e0 < cap)
      for (uint32_t e = e0; e < e0 + per; ++e) {
        const uint64_t v = key[e];
        cnt += (v != 0 && (e == 0 || v != key[e - 1])) ? 1u : 0u;
      }
    // ... and their exclusive prefix sum over the team: within a wave by shuffles, across its waves through LDS
    const uint32_t incl = wave_incl_scan(cnt);
    if (lane == 63u) wave_total[w] = incl;
    __syncthreads();
    uint32_t before = incl - cnt, total = 0;
    for (uint32_t x = 0; x < waves; ++x) {
      const uint32_t wt = wave_total[tm * waves + x];
      if (tm * waves + x < w) before += wt;
      total += wt;
    }
    const uint32_t kept = min(total, k);
    if (live) {
      uint64_t* dst_keys = t.dst_kind == SEL_TO_SLOT ? a.slots + (size_t)t.dst * k : a.carry + (size_t)t.dst * k;
      const bool row = t.dst_kind == SEL_TO_ROW;
      if (e0 < cap) {
        uint32_t pos = before;
        for (uint32_t e = e0; e < e0 + per && pos < k; ++e) {
          const uint64_t v = key[e];
          if (v != 0 && (e == 0 || v != key[e - 1])) {
            if (row) {
              a.row_scores[(size_t)t.dst * k + pos] = sel_key_score(v);
              a.row_ids[(size_t)t.dst * k + pos] = (uint64_t)(~(uint32_t)v);
            } else {
              dst_keys[pos] = v;
            }
            ++pos;
          }
        }
      }
      if (row) {
        if (lt == 0) a.row_n[t.dst] = kept;   // (the row's other slots are zero since the call's start)
      } else {
        for (uint32_t i = kept + lt; i < k; i += team) dst_keys[i] = 0;
      }
    }
    __syncthreads();   // the keys and wave_total are the next task's
  }
}
}  // namespace

// Per replica: the score calls' stream, their recycled scratch and what the last call measured.
struct ScoreState {
  int device = -1;
  uint32_t n_cu = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr, ev2 = nullptr;
  std::mutex mu;   // one score or rerank call at a time on this replica
  DeviceBuffer q_off, q_comp, q_val;   // the call's queries
  DeviceBuffer tiles, cand, scores;    // a launch's tiles, candidate ids and scores
  // rerank: a launch's selection tasks and k-key slots, the two carry slots, the call's rows (scores, ids, counts)
  DeviceBuffer sel_tasks, slots, carry, row_scores, row_ids, row_n;
  DeviceBuffer terms;   // explain: a launch's term counts and its four arrays of rows
  // expand: the call's candidate offsets and rows (components, values, counts), a launch's candidate weights and, where
  // the table does not fit LDS, one table per workgroup
  DeviceBuffer x_cand_off, x_comps, x_vals, x_n, x_w, x_table;
  DeviceBuffer d_pen;           // diversify: the call's penalty rows (scores, ids and counts: rerank's row buffers)
  std::vector<uint4> h_tiles;   // host staging of a launch
  std::vector<uint32_t> h_ids;
  std::vector<std::vector<SelTask>> sel_rounds;   // [round * tiers + tier]
  std::vector<SelTask> h_sel_tasks;
  double last_select_ms = 0;    // rerank: device time of the selection kernels, merge rounds run
  uint32_t last_merge_rounds = 0;
  double last_kernel_ms = 0;    // device time of the last call's kernels, its launches and its lookup form (sgpu_debug_score_stats)
  uint32_t last_launches = 0, last_dense = 0, last_grid = 0, last_block = 0, last_lds = 0;
  double x_kernel_ms = 0;       // the same of the last expand call (sgpu_debug_expand_stats)
  uint32_t x_launches = 0, x_dense = 0, x_grid = 0, x_lds = 0;
  uint64_t x_table_bytes = 0;
  double d_kernel_ms = 0;       // the same of the last diversify call (sgpu_debug_diversify_stats)
  uint32_t d_launches = 0, d_dense = 0, d_grid = 0, d_lds = 0, d_rounds = 0;
};

void score_state_free(ScoreState* s) {
  if (!s) return;
  if (s->device >= 0) (void)hipSetDevice(s->device);
  if (s->stream) (void)hipStreamSynchronize(s->stream);
  for (DeviceBuffer* b : {&s->q_off, &s->q_comp, &s->q_val, &s->tiles, &s->cand, &s->scores, &s->sel_tasks, &s->slots, &s->carry,
                          &s->row_scores, &s->row_ids, &s->row_n, &s->terms, &s->x_cand_off, &s->x_comps, &s->x_vals, &s->x_n,
                          &s->x_w, &s->x_table, &s->d_pen})
    b->release();
  if (s->ev0) (void)hipEventDestroy(s->ev0);
  if (s->ev1) (void)hipEventDestroy(s->ev1);
  if (s->ev2) (void)hipEventDestroy(s->ev2);
  if (s->stream) (void)hipStreamDestroy(s->stream);
  delete s;
}

static sgpu_status score_state_init(ScoreState* s, int device) {
  s->device = device;
  HIP_TRY(hipSetDevice(device));
  int n_cu = 0;
  HIP_TRY(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, device));
  s->n_cu = (uint32_t)std::max(n_cu, 1);
  HIP_TRY(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
  HIP_TRY(hipEventCreate(&s->ev0));
  HIP_TRY(hipEventCreate(&s->ev1));
  HIP_TRY(hipEventCreate(&s->ev2));
  return SGPU_OK;
}

static sgpu_status score_reserve(ScoreState* s, DeviceBuffer& b, uint64_t bytes) { return b.reserve(s->stream, bytes, "scoring documents"); }

// A rerank call: what the selection needs beyond a score call (null for sgpu_score_documents).
struct RerankCall {
  uint32_t k = 0;
  uint32_t chunk = kRerankChunk;   // C
  uint32_t n_tiers = 0;
  SelTier tiers[3];
  int carry_cur = -1;              // the carry slot the open query's survivors lie in (-1: no query is open)
  float* out_scores = nullptr;
  uint64_t* out_doc_ids = nullptr;
  uint32_t* out_n = nullptr;
};

static void rerank_setup(RerankCall* rr) {
  uint32_t c = kRerankChunk;
  if (test_hooks_on()) {
    if (const char* v = std::getenv("SGPU_RERANK_CHUNK"))
      if (*v) {
        const uint64_t want = std::min<uint64_t>(std::max<uint64_t>(2, std::strtoull(v, nullptr, 10)), kRerankChunk);
        c = 2;
        while (2ull * c <= want) c *= 2;
        uint32_t k2 = 1;
        while (k2 < rr->k) k2 *= 2;
        if (rr->k > c / 2) c = 2 * k2;   // (the fan-in floor(C / k) stays at least 2; k <= 1024: at most kRerankChunk)
      }
  }
  rr->chunk = c;
  rr->n_tiers = 0;
  for (const SelTier& t : kSelTiers) {
    const uint32_t cap = std::min(t.cap, c);
    if (rr->n_tiers && rr->tiers[rr->n_tiers - 1].cap >= cap) continue;
    rr->tiers[rr->n_tiers++] = SelTier{cap, t.team};
  }
}

// The selection tasks of one launch - candidates [first, last) of the call, the queries from q0 on - by round and tier
// into s->sel_rounds; returns the slots they use.
static uint32_t rerank_plan(ScoreState* s, RerankCall* rr, const uint64_t* cand_off, uint32_t nq, uint32_t q0, uint64_t first,
                            uint64_t last) {
  const uint32_t k = rr->k, c = rr->chunk, fan = c / k, nt = rr->n_tiers;
  s->sel_rounds.clear();
  auto push = [&](uint32_t round, const SelTask& t) {
    const uint32_t keys = t.kind == SEL_RAW ? t.n : (t.n + (t.extra != kSelNone ? 1u : 0u)) * k;
    uint32_t tier = 0;
    while (rr->tiers[tier].cap < keys) ++tier;   // (keys <= c = the last tier's cap)
    if (s->sel_rounds.size() < (size_t)(round + 1) * nt) s->sel_rounds.resize((size_t)(round + 1) * nt);
    s->sel_rounds[(size_t)round * nt + tier].push_back(t);
  };
  uint32_t next_slot = 0;
  for (uint32_t q = q0; q < nq && cand_off[q] < last; ++q) {
    const uint64_t a = std::max(cand_off[q], first), b = std::min(cand_off[q + 1], last);
    if (a >= b) continue;
    const bool has_carry = cand_off[q] < first, ends = cand_off[q + 1] <= last;
    const uint32_t old_carry = has_carry ? (uint32_t)rr->carry_cur : kSelNone;
    // (the other slot than the last one written: a launch's first part may still read that one in a later round)
    const uint32_t new_carry = rr->carry_cur < 0 ? 0u : 1u - (uint32_t)rr->carry_cur;
    if (!ends) rr->carry_cur = (int)new_carry;
    SelTask t{};
    t.extra = kSelNone;
    const uint32_t dst_kind = ends ? SEL_TO_ROW : SEL_TO_CARRY, dst = ends ? q : new_carry;
    const uint32_t len = (uint32_t)(b - a), m = (len + c - 1) / c, at = (uint32_t)(a - first);
    if (m == 1 && !has_carry) {
      t.kind = SEL_RAW, t.src = at, t.n = len, t.dst_kind = dst_kind, t.dst = dst;
      push(0, t);
      continue;
    }
    uint32_t s0 = next_slot, cnt = m, extra = old_carry;
    next_slot += m;
    for (uint32_t j = 0; j < m; ++j) {
      t.kind = SEL_RAW, t.src = at + j * c, t.n = std::min(c, len - j * c), t.dst_kind = SEL_TO_SLOT, t.dst = s0 + j;
      push(0, t);
    }
    t.kind = SEL_KEYS;
    for (uint32_t round = 1;; ++round) {
      const uint32_t e = extra != kSelNone ? 1u : 0u;
      if (cnt + e <= fan) {
        t.src = s0, t.n = cnt, t.extra = extra, t.dst_kind = dst_kind, t.dst = dst;
        push(round, t);
        break;
      }
      const uint32_t out0 = next_slot;
      for (uint32_t pos = 0; pos < cnt;) {
        const uint32_t take = std::min(fan - (pos == 0 ? e : 0u), cnt - pos);
        t.src = s0 + pos, t.n = take, t.extra = pos == 0 ? extra : kSelNone, t.dst_kind = SEL_TO_SLOT, t.dst = next_slot++;
        push(round, t);
        pos += take;
      }
      s0 = out0, cnt = next_slot - out0, extra = kSelNone;
    }
  }
  return next_slot;
}

// The call's rows on the device, zeroed (a selection task writes the slots it fills and the row's count), and what the
// selection launches of the call have in common.
static sgpu_status rerank_rows_begin(ScoreState* s, const RerankCall* rr, uint32_t nq, SelArgs* sel) {
  const uint64_t cells = (uint64_t)nq * rr->k;
  sgpu_status st;
  if ((st = score_reserve(s, s->carry, 2ull * rr->k * 8)) != SGPU_OK || (st = score_reserve(s, s->row_scores, cells * 4)) != SGPU_OK ||
      (st = score_reserve(s, s->row_ids, cells * 8)) != SGPU_OK || (st = score_reserve(s, s->row_n, (uint64_t)nq * 4)) != SGPU_OK)
    return st;
  HIP_TRY(hipMemsetAsync(s->row_scores.p, 0, cells * 4, s->stream));
  HIP_TRY(hipMemsetAsync(s->row_ids.p, 0, cells * 8, s->stream));
  HIP_TRY(hipMemsetAsync(s->row_n.p, 0, (uint64_t)nq * 4, s->stream));
  sel->carry = s->carry.as<uint64_t>();
  sel->row_scores = s->row_scores.as<float>();
  sel->row_ids = s->row_ids.as<uint64_t>();
  sel->row_n = s->row_n.as<uint32_t>();
  sel->k = rr->k;
  HIP_TRY(hipFuncSetAttribute((const void*)rerank_select_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(kRerankChunk * 8u)));
  return SGPU_OK;
}

// The selection over one launch's scores - candidates [first, last) of the call, the queries from q_first on -: one
// launch per round and tier, in the stream's order behind the score kernel.
static sgpu_status rerank_select(ScoreState* s, RerankCall* rr, SelArgs sel, const uint64_t* cand_off, uint32_t nq, uint32_t q_first,
                                 uint64_t first, uint64_t last) {
  const uint32_t n_slots = rerank_plan(s, rr, cand_off, nq, q_first, first, last);
  s->h_sel_tasks.clear();
  for (const auto& v : s->sel_rounds) s->h_sel_tasks.insert(s->h_sel_tasks.end(), v.begin(), v.end());
  sgpu_status st;
  if ((st = score_reserve(s, s->sel_tasks, s->h_sel_tasks.size() * sizeof(SelTask))) != SGPU_OK ||
      (st = score_reserve(s, s->slots, (uint64_t)n_slots * rr->k * 8)) != SGPU_OK)
    return st;
  HIP_TRY(hipMemcpyAsync(s->sel_tasks.p, s->h_sel_tasks.data(), s->h_sel_tasks.size() * sizeof(SelTask), hipMemcpyHostToDevice,
                         s->stream));
  sel.scores = s->scores.as<const float>();
  sel.cand = s->cand.as<const uint32_t>();
  sel.slots = s->slots.as<uint64_t>();
  size_t at = 0;
  for (size_t i = 0; i < s->sel_rounds.size(); ++i) {
    const size_t n = s->sel_rounds[i].size();
    if (!n) continue;
    const SelTier& tier = rr->tiers[i % rr->n_tiers];
    const uint32_t teams = kSelBlock / tier.team;
    sel.tasks = s->sel_tasks.as<const SelTask>() + at;
    sel.n_tasks = (uint32_t)n;
    sel.cap = tier.cap;
    sel.team = tier.team;
    const uint32_t sel_grid = (uint32_t)std::min<uint64_t>((n + teams - 1) / teams, (uint64_t)s->n_cu * (2048u / kSelBlock));
    hipLaunchKernelGGL(rerank_select_kernel, dim3(sel_grid), dim3(kSelBlock), teams * tier.cap * 8u, s->stream, sel);
    HIP_TRY(hipGetLastError());
    at += n;
  }
  HIP_TRY(hipEventRecord(s->ev2, s->stream));
  s->last_merge_rounds += (uint32_t)(s->sel_rounds.size() / rr->n_tiers) - 1u;
  return SGPU_OK;
}

static sgpu_status rerank_rows_end(ScoreState* s, const RerankCall* rr, uint32_t nq) {
  const uint64_t cells = (uint64_t)nq * rr->k;
  HIP_TRY(hipMemcpyAsync(rr->out_scores, s->row_scores.p, cells * 4, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipMemcpyAsync(rr->out_doc_ids, s->row_ids.p, cells * 8, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipMemcpyAsync(rr->out_n, s->row_n.p, (uint64_t)nq * 4, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return SGPU_OK;
}

// An explain call: what it returns beyond a score call (null for the other calls).
struct ExplainCall {
  uint32_t m = 0;
  ExplainOut out{};
};

// A score call (rr, ex null: every candidate's score to out_scores), a rerank call (rr: the selection follows each launch
// on the stream, and the call's rows come back at the end) or an explain call (ex: explain_documents.hip's kernel in the
// score kernel's place, each launch's scores and term rows to ex->out).
static sgpu_status score_run(ScoreState* s, const HostIndex& h, const DevView& view, const uint64_t* q_off, const uint32_t* comps,
                             const float* vals, uint32_t nq, uint32_t max_nnz, const uint64_t* cand_off, const uint64_t* cand_ids,
                             float* out_scores, RerankCall* rr = nullptr, const ExplainCall* ex = nullptr) {
  HIP_TRY(hipSetDevice(s->device));
  s->last_kernel_ms = 0;
  s->last_launches = 0;
  s->last_select_ms = 0;
  s->last_merge_rounds = 0;
  // the lookup form: the dense table where the vocabulary fits, else the hash table sized for the call's longest query
  // (test hook SGPU_SCORE_LOOKUP: 1 = dense where it fits, 2 = hash)
  const uint64_t dense_bytes = ((h.dim + 1) * 4 + 15) & ~15ull;
  bool dense = dense_bytes <= kScoreDenseLds;
  if (test_hooks_on()) {
    const char* v = std::getenv("SGPU_SCORE_LOOKUP");
    if (v && *v == '2') dense = false;
  }
  uint32_t slot_bits = 6;
  while ((1u << slot_bits) < 2u * max_nnz) ++slot_bits;   // (max_nnz <= kScoreMaxQueryNnz = 8192: at most 2^14 slots, 128 KiB)
  const uint32_t lds = dense ? (uint32_t)dense_bytes : (8u << slot_bits);
  const uint32_t block = lds > (40u << 10) ? 1024u : (lds > (20u << 10) ? 512u : 256u);
  ScoreKernel kern = score_kernel(h.comp_width, h.value_type, dense);
  int per_cu = 0;
  if (ex) {
    const sgpu_status fst = explain_kernel_fit(h.comp_width, h.value_type, dense, block, lds, &per_cu);
    if (fst != SGPU_OK) return fst;
  } else {
    HIP_TRY(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, (int)block, lds));
  }
  if (per_cu < 1) return fail(SGPU_ELIMIT, "the score kernel does not fit on a CU (%u bytes of LDS)", lds);
  per_cu = std::min(per_cu, (int)(2048u / block));

  uint64_t budget = ex ? std::min<uint64_t>(kScoreChunk, kExplainRowBytes / (16ull * ex->m)) : kScoreChunk;
  if (const char* v = std::getenv("SGPU_SCORE_CHUNK"))
    if (*v) budget = std::max<uint64_t>(1, std::strtoull(v, nullptr, 10));
  budget = std::min<uint64_t>(budget, 1ull << 28);
  const uint32_t tile_max = (uint32_t)std::min<uint64_t>(kScoreTile, budget);

  const uint64_t qnnz = q_off[nq];
  sgpu_status st;
  if ((st = score_reserve(s, s->q_off, (uint64_t)(nq + 1) * 8)) != SGPU_OK || (st = score_reserve(s, s->q_comp, qnnz * 4)) != SGPU_OK ||
      (st = score_reserve(s, s->q_val, qnnz * 4)) != SGPU_OK)
    return st;
  HIP_TRY(hipMemcpyAsync(s->q_off.p, q_off, (uint64_t)(nq + 1) * 8, hipMemcpyHostToDevice, s->stream));
  if (qnnz) {
    HIP_TRY(hipMemcpyAsync(s->q_comp.p, comps, qnnz * 4, hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipMemcpyAsync(s->q_val.p, vals, qnnz * 4, hipMemcpyHostToDevice, s->stream));
  }
  ScoreArgs a{};
  a.fwd = view.fwd;
  a.doc_ref = view.doc_ref;
  a.q_off = s->q_off.as<const uint64_t>();
  a.q_comp = s->q_comp.as<const uint32_t>();
  a.q_val = s->q_val.as<const float>();
  a.dim = (uint32_t)h.dim;
  a.slot_bits = slot_bits;
  a.val_scale = h.val_scale;
  s->last_dense = dense;
  s->last_block = block;
  s->last_lds = lds;

  ExplainArgs xa{};
  if (ex) {
    xa.fwd = a.fwd, xa.doc_ref = a.doc_ref, xa.q_off = a.q_off, xa.q_comp = a.q_comp, xa.q_val = a.q_val;
    xa.dim = a.dim, xa.slot_bits = a.slot_bits, xa.val_scale = a.val_scale, xa.m = ex->m;
  }

  SelArgs sel{};
  if (rr && (st = rerank_rows_begin(s, rr, nq, &sel)) != SGPU_OK) return st;

  // launches: consecutive tiles (a query's candidates in runs of at most tile_max) while they fit the budget
  uint32_t q = 0;
  uint64_t pos = 0;   // next candidate of the call
  const uint64_t total = cand_off[nq];
  while (pos < total) {
    s->h_tiles.clear();
    s->h_ids.clear();
    const uint64_t first = pos;
    while (pos < total && pos - first < budget) {
      while (cand_off[q + 1] <= pos) ++q;
      const uint32_t n = (uint32_t)std::min<uint64_t>(std::min<uint64_t>(tile_max, cand_off[q + 1] - pos), budget - (pos - first));
      s->h_tiles.push_back(make_uint4(q, (uint32_t)(pos - first), n, 0u));
      pos += n;
    }
    const uint64_t n_cand = pos - first;
    s->h_ids.resize(n_cand);
    for (uint64_t i = 0; i < n_cand; ++i) s->h_ids[i] = (uint32_t)cand_ids[first + i];
    if ((st = score_reserve(s, s->tiles, s->h_tiles.size() * sizeof(uint4))) != SGPU_OK ||
        (st = score_reserve(s, s->cand, n_cand * 4)) != SGPU_OK || (st = score_reserve(s, s->scores, n_cand * 4)) != SGPU_OK)
      return st;
    const uint64_t cells = ex ? n_cand * ex->m : 0;   // of each of a launch's four term arrays, behind its n_cand counts
    if (ex && (st = score_reserve(s, s->terms, (n_cand + 4 * cells) * 4)) != SGPU_OK) return st;
    HIP_TRY(hipMemcpyAsync(s->tiles.p, s->h_tiles.data(), s->h_tiles.size() * sizeof(uint4), hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipMemcpyAsync(s->cand.p, s->h_ids.data(), n_cand * 4, hipMemcpyHostToDevice, s->stream));
    a.tiles = s->tiles.as<const uint4>();
    a.cand = s->cand.as<const uint32_t>();
    a.out = s->scores.as<float>();
    a.n_tiles = (uint32_t)s->h_tiles.size();
    const uint32_t grid = (uint32_t)std::min<uint64_t>(a.n_tiles, (uint64_t)s->n_cu * (uint32_t)per_cu);
    s->last_grid = grid;
    HIP_TRY(hipEventRecord(s->ev0, s->stream));
    if (ex) {
      xa.tiles = a.tiles, xa.cand = a.cand, xa.n_tiles = a.n_tiles, xa.scores = a.out;
      xa.n_terms = s->terms.as<uint32_t>();
      xa.comps = xa.n_terms + n_cand;
      xa.q_vals = (float*)(xa.comps + cells);
      xa.d_vals = xa.q_vals + cells;
      xa.products = xa.d_vals + cells;
      if ((st = explain_kernel_launch(h.comp_width, h.value_type, dense, grid, block, lds, s->stream, xa)) != SGPU_OK) return st;
    } else {
      hipLaunchKernelGGL(kern, dim3(grid), dim3(block), lds, s->stream, a);
      HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(s->ev1, s->stream));
    if (ex) {
      const uint64_t r0 = first * ex->m;
      HIP_TRY(hipMemcpyAsync(ex->out.scores + first, s->scores.p, n_cand * 4, hipMemcpyDeviceToHost, s->stream));
      HIP_TRY(hipMemcpyAsync(ex->out.n_terms + first, xa.n_terms, n_cand * 4, hipMemcpyDeviceToHost, s->stream));
      HIP_TRY(hipMemcpyAsync(ex->out.comps + r0, xa.comps, cells * 4, hipMemcpyDeviceToHost, s->stream));
      HIP_TRY(hipMemcpyAsync(ex->out.q_vals + r0, xa.q_vals, cells * 4, hipMemcpyDeviceToHost, s->stream));
      HIP_TRY(hipMemcpyAsync(ex->out.d_vals + r0, xa.d_vals, cells * 4, hipMemcpyDeviceToHost, s->stream));
      HIP_TRY(hipMemcpyAsync(ex->out.products + r0, xa.products, cells * 4, hipMemcpyDeviceToHost, s->stream));
    } else if (!rr) {
      HIP_TRY(hipMemcpyAsync(out_scores + first, s->scores.p, n_cand * 4, hipMemcpyDeviceToHost, s->stream));
    } else if ((st = rerank_select(s, rr, sel, cand_off, nq, s->h_tiles.front().x, first, pos)) != SGPU_OK) {
      return st;
    }
    HIP_TRY(hipStreamSynchronize(s->stream));   // (the staging vectors and the scratch are the next launch's)
    float ms = 0.0f;
    HIP_TRY(hipEventElapsedTime(&ms, s->ev0, s->ev1));
    s->last_kernel_ms += ms;
    s->last_launches += 1;
    if (rr) {
      HIP_TRY(hipEventElapsedTime(&ms, s->ev1, s->ev2));
      s->last_select_ms += ms;
    }
  }
  return rr ? rerank_rows_end(s, rr, nq) : SGPU_OK;
}

// The replica's score state, made on its first score or rerank call.
static sgpu_status score_state_of(sgpu_index* idx, uint32_t replica, ScoreState** out) {
  return replica_state(idx, idx->score_mu, idx->score, replica, score_state_init, score_state_free, out);
}

sgpu_status score_documents_device(sgpu_index* idx, uint32_t replica, const uint64_t* q_off, const uint32_t* comps,
                                   const float* vals, uint32_t nq, const uint64_t* cand_off, const uint64_t* cand_ids,
                                   float* out_scores) {
  if (!idx) return fail(SGPU_EINVAL, "null argument");
  uint32_t max_nnz = 0;
  const sgpu_status vst = score_check_args(idx->host, q_off, comps, vals, nq, cand_off, cand_ids, out_scores, &max_nnz);
  if (vst != SGPU_OK) return vst;
  ScoreState* s = nullptr;
  const sgpu_status sst = score_state_of(idx, replica, &s);
  if (sst != SGPU_OK) return sst;
  if (nq == 0 || cand_off[nq] == 0) return SGPU_OK;
  std::lock_guard<std::mutex> lk(s->mu);
  try {
    return score_run(s, idx->host, device_index_view(idx->replicas[replica]), q_off, comps, vals, nq, max_nnz, cand_off, cand_ids,
                     out_scores);
  } catch (const std::bad_alloc&) {
    return fail(SGPU_ENOMEM, "out of host memory");
  }
}

sgpu_status rerank_documents_device(sgpu_index* idx, uint32_t replica, const uint64_t* q_off, const uint32_t* comps,
                                    const float* vals, uint32_t nq, const uint64_t* cand_off, const uint64_t* cand_ids, uint32_t k,
                                    float* out_scores, uint64_t* out_doc_ids, uint32_t* out_n) {
  if (!idx) return fail(SGPU_EINVAL, "null argument");
  uint32_t max_nnz = 0;
  const sgpu_status vst =
      rerank_check_args(idx->host, q_off, comps, vals, nq, cand_off, cand_ids, k, out_scores, out_doc_ids, out_n, &max_nnz);
  if (vst != SGPU_OK) return vst;
  ScoreState* s = nullptr;
  const sgpu_status sst = score_state_of(idx, replica, &s);
  if (sst != SGPU_OK) return sst;
  if (nq == 0) return SGPU_OK;
  if (cand_off[nq] == 0) {   // no candidate at all: zeroed rows
    std::fill(out_scores, out_scores + (size_t)nq * k, 0.0f);
    std::fill(out_doc_ids, out_doc_ids + (size_t)nq * k, (uint64_t)0);
    std::fill(out_n, out_n + nq, 0u);
    return SGPU_OK;
  }
  RerankCall rr;
  rr.k = k;
  rr.out_scores = out_scores;
  rr.out_doc_ids = out_doc_ids;
  rr.out_n = out_n;
  rerank_setup(&rr);
  std::lock_guard<std::mutex> lk(s->mu);
  try {
    return score_run(s, idx->host, device_index_view(idx->replicas[replica]), q_off, comps, vals, nq, max_nnz, cand_off, cand_ids,
                     nullptr, &rr);
  } catch (const std::bad_alloc&) {
    return fail(SGPU_ENOMEM, "out of host memory");
  }
}

sgpu_status explain_documents_device(sgpu_index* idx, uint32_t replica, const uint64_t* q_off, const uint32_t* comps,
                                     const float* vals, uint32_t nq, const uint64_t* cand_off, const uint64_t* cand_ids, uint32_t m,
                                     const ExplainOut& out) {
  if (!idx) return fail(SGPU_EINVAL, "null argument");
  uint32_t max_nnz = 0;
  const sgpu_status vst = explain_check_args(idx->host, q_off, comps, vals, nq, cand_off, cand_ids, m, out, &max_nnz);
  if (vst != SGPU_OK) return vst;
  ScoreState* s = nullptr;
  const sgpu_status sst = score_state_of(idx, replica, &s);
  if (sst != SGPU_OK) return sst;
  if (nq == 0 || cand_off[nq] == 0) return SGPU_OK;
  ExplainCall ex;
  ex.m = m;
  ex.out = out;
  std::lock_guard<std::mutex> lk(s->mu);
  try {
    return score_run(s, idx->host, device_index_view(idx->replicas[replica]), q_off, comps, vals, nq, max_nnz, cand_off, cand_ids,
                     nullptr, nullptr, &ex);
  } catch (const std::bad_alloc&) {
    return fail(SGPU_ENOMEM, "out of host memory");
  }
}

// ---- sgpu_expand_queries ----
constexpr uint64_t kExpandTableBytes = 1ull << 30;   // most global scratch the tables of a launch's workgroups take

// An expand call: expand_queries.hip's kernel over the call's queries, staged as score_run stages them. A launch takes
// whole queries - consecutive ones while their candidates fit the budget (SGPU_SCORE_CHUNK), a larger query alone -, so
// no table is carried between launches; the call's rows stay on the device until its end.
static sgpu_status expand_run(ScoreState* s, const HostIndex& h, const DevView& view, const uint64_t* q_off, const uint32_t* comps,
                              const float* vals, uint32_t nq, const uint64_t* cand_off, const uint64_t* cand_ids, const float* cand_w,
                              float alpha, uint32_t t, uint32_t* out_comps, float* out_vals, uint32_t* out_n) {
  HIP_TRY(hipSetDevice(s->device));
  s->x_kernel_ms = 0;
  s->x_launches = 0;
  // the table: in LDS where the vocabulary fits (the score kernel's rule for its dense table; test hook
  // SGPU_SCORE_LOOKUP=2: in global memory although it fits), else one per workgroup in the scratch
  const uint64_t table_bytes = ((h.dim + 1) * 4 + 15) & ~15ull;
  bool dense = table_bytes <= kScoreDenseLds;
  if (test_hooks_on()) {
    const char* v = std::getenv("SGPU_SCORE_LOOKUP");
    if (v && *v == '2') dense = false;
  }
  const uint32_t lds = dense ? (uint32_t)table_bytes : 0u;
  int per_cu = 0;
  sgpu_status st;
  if ((st = expand_kernel_fit(h.comp_width, h.value_type, dense, lds, &per_cu)) != SGPU_OK) return st;
  if (per_cu < 1) return fail(SGPU_ELIMIT, "the expand kernel does not fit on a CU (%u bytes of LDS)", lds);
  per_cu = std::min(per_cu, (int)(2048u / kExpandBlock));
  uint64_t max_grid = (uint64_t)s->n_cu * (uint32_t)per_cu;
  if (!dense) max_grid = std::max<uint64_t>(1, std::min<uint64_t>(max_grid, kExpandTableBytes / ((h.dim + 1) * 4)));
  if (test_hooks_on())   // (test hook SGPU_EXPAND_GRID: fewer workgroups, so that each takes many queries in turn)
    if (const char* v = std::getenv("SGPU_EXPAND_GRID"))
      if (*v) max_grid = std::max<uint64_t>(1, std::min<uint64_t>(max_grid, std::strtoull(v, nullptr, 10)));

  uint64_t budget = kScoreChunk;
  if (const char* v = std::getenv("SGPU_SCORE_CHUNK"))
    if (*v) budget = std::max<uint64_t>(1, std::strtoull(v, nullptr, 10));
  budget = std::min<uint64_t>(budget, 1ull << 28);

  const uint64_t qnnz = q_off[nq], cells = (uint64_t)nq * t;
  if ((st = score_reserve(s, s->q_off, (uint64_t)(nq + 1) * 8)) != SGPU_OK || (st = score_reserve(s, s->q_comp, qnnz * 4)) != SGPU_OK ||
      (st = score_reserve(s, s->q_val, qnnz * 4)) != SGPU_OK || (st = score_reserve(s, s->x_cand_off, (uint64_t)(nq + 1) * 8)) != SGPU_OK ||
      (st = score_reserve(s, s->x_comps, cells * 4)) != SGPU_OK || (st = score_reserve(s, s->x_vals, cells * 4)) != SGPU_OK ||
      (st = score_reserve(s, s->x_n, (uint64_t)nq * 4)) != SGPU_OK)
    return st;
  HIP_TRY(hipMemcpyAsync(s->q_off.p, q_off, (uint64_t)(nq + 1) * 8, hipMemcpyHostToDevice, s->stream));
  HIP_TRY(hipMemcpyAsync(s->x_cand_off.p, cand_off, (uint64_t)(nq + 1) * 8, hipMemcpyHostToDevice, s->stream));
  if (qnnz) {
    HIP_TRY(hipMemcpyAsync(s->q_comp.p, comps, qnnz * 4, hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipMemcpyAsync(s->q_val.p, vals, qnnz * 4, hipMemcpyHostToDevice, s->stream));
  }
  ExpandArgs a{};
  a.fwd = view.fwd;
  a.doc_ref = view.doc_ref;
  a.q_off = s->q_off.as<const uint64_t>();
  a.q_comp = s->q_comp.as<const uint32_t>();
  a.q_val = s->q_val.as<const float>();
  a.cand_off = s->x_cand_off.as<const uint64_t>();
  a.out_comps = s->x_comps.as<uint32_t>();
  a.out_vals = s->x_vals.as<float>();
  a.out_n = s->x_n.as<uint32_t>();
  a.dim = (uint32_t)h.dim;
  a.t = t;
  a.alpha = alpha;
  a.val_scale = h.val_scale;
  s->x_dense = dense;
  s->x_lds = lds;
  s->x_table_bytes = 0;

  for (uint32_t q = 0; q < nq;) {
    const uint32_t qa = q;
    const uint64_t first = cand_off[qa];
    ++q;   // (a query of more candidates than the budget goes alone)
    while (q < nq && cand_off[q + 1] - first <= budget) ++q;
    const uint64_t n_cand = cand_off[q] - first;   // (<= max(budget, kExpandMaxCand) < 2^32)
    s->h_ids.resize(n_cand);
    for (uint64_t i = 0; i < n_cand; ++i) s->h_ids[i] = (uint32_t)cand_ids[first + i];
    const uint32_t grid = (uint32_t)std::min<uint64_t>(q - qa, max_grid);
    if ((st = score_reserve(s, s->cand, n_cand * 4)) != SGPU_OK || (st = score_reserve(s, s->x_w, n_cand * 4)) != SGPU_OK) return st;
    if (!dense) {
      const uint64_t bytes = (uint64_t)grid * (h.dim + 1) * 4;
      if ((st = score_reserve(s, s->x_table, bytes)) != SGPU_OK) return st;
      s->x_table_bytes = std::max(s->x_table_bytes, bytes);
    }
    if (n_cand) {
      HIP_TRY(hipMemcpyAsync(s->cand.p, s->h_ids.data(), n_cand * 4, hipMemcpyHostToDevice, s->stream));
      HIP_TRY(hipMemcpyAsync(s->x_w.p, cand_w + first, n_cand * 4, hipMemcpyHostToDevice, s->stream));
    }
    a.cand = s->cand.as<const uint32_t>();
    a.cand_w = s->x_w.as<const float>();
    a.table = s->x_table.as<float>();
    a.cand_base = first;
    a.q_first = qa;
    a.q_last = q;
    s->x_grid = grid;
    HIP_TRY(hipEventRecord(s->ev0, s->stream));
    if ((st = expand_kernel_launch(h.comp_width, h.value_type, dense, grid, lds, s->stream, a)) != SGPU_OK) return st;
    HIP_TRY(hipEventRecord(s->ev1, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));   // (the staged ids and the scratch are the next launch's)
    float ms = 0.0f;
    HIP_TRY(hipEventElapsedTime(&ms, s->ev0, s->ev1));
    s->x_kernel_ms += ms;
    s->x_launches += 1;
  }
  HIP_TRY(hipMemcpyAsync(out_comps, s->x_comps.p, cells * 4, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipMemcpyAsync(out_vals, s->x_vals.p, cells * 4, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipMemcpyAsync(out_n, s->x_n.p, (uint64_t)nq * 4, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return SGPU_OK;
}

sgpu_status expand_queries_device(sgpu_index* idx, uint32_t replica, const uint64_t* q_off, const uint32_t* comps, const float* vals,
                                  uint32_t nq, const uint64_t* cand_off, const uint64_t* cand_ids, const float* cand_w, float alpha,
                                  uint32_t t, uint32_t* out_comps, float* out_vals, uint32_t* out_n) {
  if (!idx) return fail(SGPU_EINVAL, "null argument");
  uint32_t max_nnz = 0;
  const sgpu_status vst =
      expand_check_args(idx->host, q_off, comps, vals, nq, cand_off, cand_ids, cand_w, alpha, t, out_comps, out_vals, out_n, &max_nnz);
  if (vst != SGPU_OK) return vst;
  ScoreState* s = nullptr;
  const sgpu_status sst = score_state_of(idx, replica, &s);
  if (sst != SGPU_OK) return sst;
  if (nq == 0) return SGPU_OK;
  std::lock_guard<std::mutex> lk(s->mu);
  try {
    return expand_run(s, idx->host, device_index_view(idx->replicas[replica]), q_off, comps, vals, nq, cand_off, cand_ids, cand_w, alpha,
                      t, out_comps, out_vals, out_n);
  } catch (const std::bad_alloc&) {
    return fail(SGPU_ENOMEM, "out of host memory");
  }
}

// ---- sgpu_diversify_documents ----
// A diversify call: diversify_documents.hip's kernel over the call's queries, staged and cut as expand_run stages and
// cuts them - a launch takes whole queries, consecutive ones while their candidates fit the budget (SGPU_SCORE_CHUNK), a
// larger query alone -; the call's rows stay on the device until its end, zeroed before the first launch.
static sgpu_status diversify_run(ScoreState* s, const HostIndex& h, const DevView& view, const uint64_t* q_off, const uint32_t* comps,
                                 const float* vals, uint32_t nq, uint32_t max_nnz, uint32_t max_len, uint32_t max_cand,
                                 const uint64_t* cand_off, const uint64_t* cand_ids, float lambda, float mu, uint32_t k,
                                 const DiversifyOut& out) {
  HIP_TRY(hipSetDevice(s->device));
  s->d_kernel_ms = 0;
  s->d_launches = 0;
  s->d_rounds = 0;
  // the table: the score kernel's rule and its test hook; the hash table holds the longest query or candidate document
  const uint64_t dense_bytes = ((h.dim + 1) * 4 + 15) & ~15ull;
  bool dense = dense_bytes <= kScoreDenseLds;
  if (test_hooks_on()) {
    const char* v = std::getenv("SGPU_SCORE_LOOKUP");
    if (v && *v == '2') dense = false;
  }
  uint32_t slot_bits = 6;
  while ((1u << slot_bits) < 2u * std::max(max_nnz, max_len)) ++slot_bits;   // (both <= 8192: at most 2^14 slots, 128 KiB)
  const uint32_t table_bytes = dense ? (uint32_t)dense_bytes : (8u << slot_bits);
  const uint32_t cap = std::max(64u, (max_cand + 63u) & ~63u);   // (<= 2048: 24 KiB of entry state)
  const uint32_t lds = table_bytes + cap * 12u;
  int per_cu = 0;
  sgpu_status st;
  if ((st = diversify_kernel_fit(h.comp_width, h.value_type, dense, lds, &per_cu)) != SGPU_OK) return st;
  if (per_cu < 1) return fail(SGPU_ELIMIT, "the diversify kernel does not fit on a CU (%u bytes of LDS)", lds);
  per_cu = std::min(per_cu, (int)(2048u / kDiversifyBlock));
  uint64_t max_grid = (uint64_t)s->n_cu * (uint32_t)per_cu;
  if (test_hooks_on())   // (test hook SGPU_DIVERSIFY_GRID: fewer workgroups, so that each takes many queries in turn)
    if (const char* v = std::getenv("SGPU_DIVERSIFY_GRID"))
      if (*v) max_grid = std::max<uint64_t>(1, std::min<uint64_t>(max_grid, std::strtoull(v, nullptr, 10)));

  uint64_t budget = kScoreChunk;
  if (const char* v = std::getenv("SGPU_SCORE_CHUNK"))
    if (*v) budget = std::max<uint64_t>(1, std::strtoull(v, nullptr, 10));
  budget = std::min<uint64_t>(budget, 1ull << 28);

  const uint64_t qnnz = q_off[nq], cells = (uint64_t)nq * k;
  if ((st = score_reserve(s, s->q_off, (uint64_t)(nq + 1) * 8)) != SGPU_OK || (st = score_reserve(s, s->q_comp, qnnz * 4)) != SGPU_OK ||
      (st = score_reserve(s, s->q_val, qnnz * 4)) != SGPU_OK || (st = score_reserve(s, s->x_cand_off, (uint64_t)(nq + 1) * 8)) != SGPU_OK ||
      (st = score_reserve(s, s->row_scores, cells * 4)) != SGPU_OK || (st = score_reserve(s, s->d_pen, cells * 4)) != SGPU_OK ||
      (st = score_reserve(s, s->row_ids, cells * 8)) != SGPU_OK || (st = score_reserve(s, s->row_n, (uint64_t)nq * 4)) != SGPU_OK)
    return st;
  HIP_TRY(hipMemcpyAsync(s->q_off.p, q_off, (uint64_t)(nq + 1) * 8, hipMemcpyHostToDevice, s->stream));
  HIP_TRY(hipMemcpyAsync(s->x_cand_off.p, cand_off, (uint64_t)(nq + 1) * 8, hipMemcpyHostToDevice, s->stream));
  if (qnnz) {
    HIP_TRY(hipMemcpyAsync(s->q_comp.p, comps, qnnz * 4, hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipMemcpyAsync(s->q_val.p, vals, qnnz * 4, hipMemcpyHostToDevice, s->stream));
  }
  HIP_TRY(hipMemsetAsync(s->row_scores.p, 0, cells * 4, s->stream));
  HIP_TRY(hipMemsetAsync(s->d_pen.p, 0, cells * 4, s->stream));
  HIP_TRY(hipMemsetAsync(s->row_ids.p, 0, cells * 8, s->stream));
  HIP_TRY(hipMemsetAsync(s->row_n.p, 0, (uint64_t)nq * 4, s->stream));
  DiversifyArgs a{};
  a.fwd = view.fwd;
  a.doc_ref = view.doc_ref;
  a.q_off = s->q_off.as<const uint64_t>();
  a.q_comp = s->q_comp.as<const uint32_t>();
  a.q_val = s->q_val.as<const float>();
  a.cand_off = s->x_cand_off.as<const uint64_t>();
  a.row_scores = s->row_scores.as<float>();
  a.row_pen = s->d_pen.as<float>();
  a.row_ids = s->row_ids.as<uint64_t>();
  a.row_n = s->row_n.as<uint32_t>();
  a.dim = (uint32_t)h.dim;
  a.slot_bits = slot_bits;
  a.table_bytes = table_bytes;
  a.cap = cap;
  a.k = k;
  a.lambda = lambda;
  a.mu = mu;
  a.val_scale = h.val_scale;
  s->d_dense = dense;
  s->d_lds = lds;

  for (uint32_t q = 0; q < nq;) {
    const uint32_t qa = q;
    const uint64_t first = cand_off[qa];
    ++q;   // (a query of more candidates than the budget goes alone)
    while (q < nq && cand_off[q + 1] - first <= budget) ++q;
    const uint64_t n_cand = cand_off[q] - first;   // (<= max(budget, kDiversifyMaxCand) < 2^32)
    if (n_cand == 0) continue;   // (queries without candidates: their rows are zero already)
    s->h_ids.resize(n_cand);
    for (uint64_t i = 0; i < n_cand; ++i) s->h_ids[i] = (uint32_t)cand_ids[first + i];
    const uint32_t grid = (uint32_t)std::min<uint64_t>(q - qa, max_grid);
    if ((st = score_reserve(s, s->cand, n_cand * 4)) != SGPU_OK) return st;
    HIP_TRY(hipMemcpyAsync(s->cand.p, s->h_ids.data(), n_cand * 4, hipMemcpyHostToDevice, s->stream));
    a.cand = s->cand.as<const uint32_t>();
    a.cand_base = first;
    a.q_first = qa;
    a.q_last = q;
    s->d_grid = grid;
    HIP_TRY(hipEventRecord(s->ev0, s->stream));
    if ((st = diversify_kernel_launch(h.comp_width, h.value_type, dense, grid, lds, s->stream, a)) != SGPU_OK) return st;
    HIP_TRY(hipEventRecord(s->ev1, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));   // (the staged ids are the next launch's)
    float ms = 0.0f;
    HIP_TRY(hipEventElapsedTime(&ms, s->ev0, s->ev1));
    s->d_kernel_ms += ms;
    s->d_launches += 1;
  }
  HIP_TRY(hipMemcpyAsync(out.scores, s->row_scores.p, cells * 4, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipMemcpyAsync(out.penalties, s->d_pen.p, cells * 4, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipMemcpyAsync(out.doc_ids, s->row_ids.p, cells * 8, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipMemcpyAsync(out.n, s->row_n.p, (uint64_t)nq * 4, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  for (uint32_t i = 0; i < nq; ++i) s->d_rounds = std::max(s->d_rounds, out.n[i]);
  return SGPU_OK;
}

sgpu_status diversify_documents_device(sgpu_index* idx, uint32_t replica, const uint64_t* q_off, const uint32_t* comps,
                                       const float* vals, uint32_t nq, const uint64_t* cand_off, const uint64_t* cand_ids, float lambda,
                                       float mu, uint32_t k, const DiversifyOut& out) {
  if (!idx) return fail(SGPU_EINVAL, "null argument");
  uint32_t max_nnz = 0, max_len = 0, max_cand = 0;
  const sgpu_status vst =
      diversify_check_args(idx->host, q_off, comps, vals, nq, cand_off, cand_ids, lambda, mu, k, out, &max_nnz, &max_len, &max_cand);
  if (vst != SGPU_OK) return vst;
  ScoreState* s = nullptr;
  const sgpu_status sst = score_state_of(idx, replica, &s);
  if (sst != SGPU_OK) return sst;
  if (nq == 0) return SGPU_OK;
  std::lock_guard<std::mutex> lk(s->mu);
  try {
    return diversify_run(s, idx->host, device_index_view(idx->replicas[replica]), q_off, comps, vals, nq, max_nnz, max_len, max_cand,
                         cand_off, cand_ids, lambda, mu, k, out);
  } catch (const std::bad_alloc&) {
    return fail(SGPU_ENOMEM, "out of host memory");
  }
}

// (test hook: what the last diversify call on `replica` measured - out8 = {device ms of its kernels, launches, grid of the last
// launch, workgroup size, LDS bytes, 1 = dense table / 0 = hash, rounds of its longest query, 0}. tools/diversify_probe.py)
bool diversify_debug_stats(sgpu_index* idx, uint32_t replica, double* out8) {
  std::lock_guard<std::mutex> lk(idx->score_mu);
  if (replica >= idx->score.size() || !idx->score[replica]) return false;
  ScoreState* s = idx->score[replica];
  std::lock_guard<std::mutex> lk2(s->mu);
  const double v[8] = {s->d_kernel_ms, (double)s->d_launches, (double)s->d_grid, (double)kDiversifyBlock,
                       (double)s->d_lds,  (double)s->d_dense,    (double)s->d_rounds, 0.0};
  for (int i = 0; i < 8; ++i) out8[i] = v[i];
  return true;
}

// (test hook: what the last expand call on `replica` measured - out8 = {device ms of its kernels, launches, 1 = table in LDS /
// 0 = in global memory, grid of the last launch, workgroup size, LDS bytes, bytes of the global tables, 0}. tools/expand_probe.py)
bool expand_debug_stats(sgpu_index* idx, uint32_t replica, double* out8) {
  std::lock_guard<std::mutex> lk(idx->score_mu);
  if (replica >= idx->score.size() || !idx->score[replica]) return false;
  ScoreState* s = idx->score[replica];
  std::lock_guard<std::mutex> lk2(s->mu);
  const double v[8] = {s->x_kernel_ms, (double)s->x_launches, (double)s->x_dense, (double)s->x_grid,
                       (double)kExpandBlock, (double)s->x_lds, (double)s->x_table_bytes, 0.0};
  for (int i = 0; i < 8; ++i) out8[i] = v[i];
  return true;
}

// (test hook: what the last score or rerank call on `replica` measured - out8 = {device ms of its score kernels, launches,
// 1 = dense table / 0 = hash, grid, workgroup size, LDS bytes, device ms of the selection kernels, merge rounds}.
// tools/score_probe.py, tools/rerank_probe.py)
bool score_debug_stats(sgpu_index* idx, uint32_t replica, double* out8) {
  std::lock_guard<std::mutex> lk(idx->score_mu);
  if (replica >= idx->score.size() || !idx->score[replica]) return false;
  ScoreState* s = idx->score[replica];
  std::lock_guard<std::mutex> lk2(s->mu);
  const double v[8] = {s->last_kernel_ms, (double)s->last_launches, (double)s->last_dense, (double)s->last_grid,
                       (double)s->last_block, (double)s->last_lds, s->last_select_ms, (double)s->last_merge_rounds};
  for (int i = 0; i < 8; ++i) out8[i] = v[i];
  return true;
}

}  // namespace sgpu
