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
//           elements over the 16-lane groups (workgroup_walk_doc, as expand_queries.hip walks a document), the weight of
//           element e the f32 its stored bits stand for (fixed-u8: fl(fl(code * val_scale) * val_scale), the query
//           weight code * val_scale with the score kernel's fold of val_scale on top); elements e >= len (slice padding)
//           are MASKED, since a padding element repeats a component whose real element another lane holds. A
//           document's components are distinct: dense stores do not collide, the hash arm inserts with table_put.
//   stream  both phases score entries against the table with score_lookup.hpp's group_score, the score kernel's own
//           loop: a 16-lane group per entry, kDivDocs entries per group in flight. Phase 0 writes rel; a round
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

#include "score_state.hpp"

namespace sgpu {

namespace {

constexpr uint32_t kDiversifyBlock = 1024;   // threads of a workgroup (16 wavefronts: the kernel's wave maxima are sized by it)

struct DiversifyArgs {
  const uint8_t* fwd;         // DevView::fwd and doc_ref
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

// Entries [0, n) that are not taken against the table, as score_documents_kernel scores a tile. REL: the result is the
// entry's rel; else its pen is raised to it.
template <typename CT, int VT, bool DENSE, bool REL>
__device__ __forceinline__ void stream_entries(const DiversifyArgs& a, const WeightTable& tab, const DivState& st, uint32_t n) {
  const uint32_t tid = threadIdx.x, g = tid >> 4, l = tid & 15u;
  for (uint32_t base = 0; base < n; base += kDivGroups * kDivDocs) {
    uint32_t idx[kDivDocs];
    bool live[kDivDocs];
    DocRef<VT> doc[kDivDocs];
#pragma unroll
    for (uint32_t u = 0; u < kDivDocs; ++u) {
      idx[u] = base + u * kDivGroups + g;
      live[u] = idx[u] < n && (REL || st.pen[idx[u]] != kTaken);
      doc[u] = doc_ref_of<VT>(a.fwd, live[u] ? a.doc_ref[st.id[idx[u]]] : 0ull);
    }
    group_score<CT, VT, DENSE>(tab, doc, l, [&](uint32_t u, float score) {
      if (l == 0 && live[u]) {
        if (REL) {
          st.rel[idx[u]] = score;
        } else {
          st.pen[idx[u]] = __float_as_uint(fmaxf(__uint_as_float(st.pen[idx[u]]), score));
        }
      }
    });
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
  DivState st;
  st.id = (uint32_t*)(smem + a.table_bytes);
  st.rel = (float*)(st.id + a.cap);
  st.pen = (uint32_t*)(st.rel + a.cap);
  const uint32_t k = a.k;

  const WeightTable tab = weight_table(smem, a.dim, a.slot_bits);
  table_reset<DENSE>(tab, tid, nt);
  // the table's occupant (workgroup-uniform): none, a query or a document
  uint32_t occ = OCC_NONE, occ_q = 0;
  uint64_t occ_ref = 0;
  auto table_empty = [&]() {   // (the caller's barriers: nobody reads the table before, everybody sees it empty after)
    if (occ == OCC_NONE) return;
    if (!DENSE || occ == OCC_QUERY) {
      table_clear_query<DENSE>(tab, a, occ_q, tid, nt);
    } else {
      workgroup_walk_doc<CT, VT>(a.fwd, occ_ref, kDivGroups, [&](uint32_t c, float) { table_put<DENSE>(tab, c, 0.0f); });
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
      table_fill_query<VT, DENSE>(tab, a, q, tid, nt);
      occ = OCC_QUERY, occ_q = q;
      __syncthreads();
      stream_entries<CT, VT, DENSE, true>(a, tab, st, n);
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
        // (the weight of an element: the f32 its stored bits stand for; fixed-u8: val_scale once for the value, once more
        // as table_fill_query folds it into a query's weight)
        workgroup_walk_doc<CT, VT>(a.fwd, ref, kDivGroups, [&](uint32_t c, float x) {
          table_put<DENSE>(tab, c, Vt<VT>::half ? x : __fmul_rn(__fmul_rn(x, a.val_scale), a.val_scale));
        });
        occ = OCC_DOC, occ_ref = ref;
        __syncthreads();
        // (d) the pen of what is left
        stream_entries<CT, VT, DENSE, false>(a, tab, st, n);
        __syncthreads();
      }
    }
    if (tid == 0u) a.row_n[q] = rounds;
  }
}

using DiversifyKernel = void (*)(DiversifyArgs);
DiversifyKernel diversify_kernel(uint32_t cw, uint32_t vt, bool dense) {
  return for_variant(cw, vt, dense, [](auto CW, auto VT, auto D) -> DiversifyKernel { return diversify_documents_kernel<CW(), VT(), D()>; });
}

// A diversify call: the kernel over the call's queries, a launch taking whole queries (next_whole_queries); the call's
// rows - rerank's row buffers plus one for the penalties - stay on the device until its end, zeroed before the first
// launch.
sgpu_status diversify_run(ScoreState* s, const HostIndex& h, const DevView& view, const uint64_t* q_off, const uint32_t* comps,
                          const float* vals, uint32_t nq, uint32_t max_nnz, uint32_t max_len, uint32_t max_cand, const uint64_t* cand_off,
                          const uint64_t* cand_ids, float lambda, float mu, uint32_t k, const DiversifyOut& out) {
  HIP_TRY(hipSetDevice(s->device));
  CallStats& cs = s->diversify_stats;
  cs.begin();
  const LookupForm form = lookup_form(h, std::max(max_nnz, max_len));   // the hash table holds the longest query or candidate document
  const uint32_t cap = std::max(64u, (max_cand + 63u) & ~63u);   // (<= 2048: 24 KiB of entry state)
  const uint32_t lds = form.table_bytes + cap * 12u;
  const DiversifyKernel kern = diversify_kernel(h.comp_width, h.value_type, form.dense);
  int per_cu = 0;
  sgpu_status st;
  if ((st = kernel_fit(kern, kDiversifyBlock, lds, &per_cu)) != SGPU_OK) return st;
  if (per_cu < 1) return fail(SGPU_ELIMIT, "the diversify kernel does not fit on a CU (%u bytes of LDS)", lds);
  per_cu = std::min(per_cu, (int)(2048u / kDiversifyBlock));
  const uint64_t max_grid = hooked_grid((uint64_t)s->n_cu * (uint32_t)per_cu, "SGPU_DIVERSIFY_GRID");
  const uint64_t budget = launch_budget();

  const uint64_t cells = (uint64_t)nq * k;
  if ((st = stage_queries(s, q_off, comps, vals, nq, cand_off)) != SGPU_OK || (st = score_reserve(s, s->row_scores, cells * 4)) != SGPU_OK ||
      (st = score_reserve(s, s->d_pen, cells * 4)) != SGPU_OK || (st = score_reserve(s, s->row_ids, cells * 8)) != SGPU_OK ||
      (st = score_reserve(s, s->row_n, (uint64_t)nq * 4)) != SGPU_OK)
    return st;
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
  a.cand_off = s->cand_off.as<const uint64_t>();
  a.row_scores = s->row_scores.as<float>();
  a.row_pen = s->d_pen.as<float>();
  a.row_ids = s->row_ids.as<uint64_t>();
  a.row_n = s->row_n.as<uint32_t>();
  a.dim = (uint32_t)h.dim;
  a.slot_bits = form.slot_bits;
  a.table_bytes = form.table_bytes;
  a.cap = cap;
  a.k = k;
  a.lambda = lambda;
  a.mu = mu;
  a.val_scale = h.val_scale;
  cs.dense = form.dense;
  cs.block = kDiversifyBlock;
  cs.lds = lds;

  for (uint32_t q = 0; q < nq;) {
    const uint32_t qa = next_whole_queries(cand_off, nq, budget, &q);
    const uint64_t first = cand_off[qa], n_cand = cand_off[q] - first;   // (<= max(budget, kDiversifyMaxCand) < 2^32)
    if (n_cand == 0) continue;   // (queries without candidates: their rows are zero already)
    const uint32_t grid = (uint32_t)std::min<uint64_t>(q - qa, max_grid);
    if ((st = stage_ids(s, cand_ids, first, n_cand)) != SGPU_OK) return st;
    a.cand = s->cand.as<const uint32_t>();
    a.cand_base = first;
    a.q_first = qa;
    a.q_last = q;
    cs.grid = grid;
    if ((st = launch_timed(s, kern, grid, kDiversifyBlock, lds, a)) != SGPU_OK || (st = launch_done(s, &cs)) != SGPU_OK) return st;
  }
  HIP_TRY(hipMemcpyAsync(out.scores, s->row_scores.p, cells * 4, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipMemcpyAsync(out.penalties, s->d_pen.p, cells * 4, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipMemcpyAsync(out.doc_ids, s->row_ids.p, cells * 8, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipMemcpyAsync(out.n, s->row_n.p, (uint64_t)nq * 4, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  for (uint32_t i = 0; i < nq; ++i) cs.extra[0] = std::max(cs.extra[0], (double)out.n[i]);
  return SGPU_OK;
}

}  // namespace

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
  double v[8];
  if (!call_stats_out(idx, replica, &ScoreState::diversify_stats, v)) return false;
  const double d[8] = {v[0], v[1], v[3], (double)kDiversifyBlock, v[5], v[2], v[6], 0.0};   // (this hook's own slot order)
  for (int i = 0; i < 8; ++i) out8[i] = d[i];
  return true;
}

}  // namespace sgpu
