// score_documents.hip — scores of caller-given documents on the device (sgpu_score_documents), and the launcher that
// sgpu_rerank_documents and sgpu_explain_documents run through as well.
//
// A score is what the search kernels return for the document (search_score.inc: score_class), bit for bit: the full
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
// describes them and decodes them, here as in the search kernels. The table is score_lookup.hpp's; the group's loop stays
// written out here (group_score is the same loop for diversify: called from this kernel it costs its u32 dense variants up
// to six registers and with them a workgroup per CU; profiles/candidate_calls_refactor.txt).
//
// score_run serves three calls: sgpu_score_documents; sgpu_rerank_documents, where the selection of rerank_select.hip
// follows every launch on the stream; and sgpu_explain_documents, with explain_documents.hip's kernel in
// score_documents_kernel's place. The calls whose unit of work is a whole query, not a tile, have launchers of their own
// (expand_queries.hip, diversify_documents.hip); what all launchers share is score_state.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>
#include <new>
#include <type_traits>

#include "score_state.hpp"

namespace sgpu {

namespace {

constexpr uint32_t kScoreDocs = 2;               // candidates a 16-lane group has in flight
constexpr uint64_t kExplainRowBytes = 64ull << 20;   // candidates per launch of an explain call: as many as this much of term rows holds

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
  const WeightTable tab = weight_table(smem, a.dim, a.slot_bits);
  table_reset<DENSE>(tab, tid, nt);
  uint32_t cur_q = kNoQuery;
  for (uint32_t t = blockIdx.x; t < a.n_tiles; t += gridDim.x) {
    const uint4 tile = a.tiles[t];   // (workgroup-uniform)
    if (tile.x != cur_q) {
      __syncthreads();   // every group is done with the table as it is
      if (cur_q != kNoQuery) {
        table_clear_query<DENSE>(tab, a, cur_q, tid, nt);
        __syncthreads();
      }
      table_fill_query<VT, DENSE>(tab, a, tile.x, tid, nt);
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
        const DocRef<VT> doc = doc_ref_of<VT>(a.fwd, ref);
        len[u] = doc.len, raw[u] = doc.raw, rec[u] = doc.rec;
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
            for (int i = 0; i < 8; ++i) w[i] = weight_of<DENSE>(tab, c[i]);
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
  return for_variant(cw, vt, dense, [](auto CW, auto VT, auto D) -> ScoreKernel { return score_documents_kernel<CW(), VT(), D()>; });
}

// An explain call: what it returns beyond a score call (null for the other calls).
struct ExplainCall {
  uint32_t m = 0;
  ExplainOut out{};
};

// A score call (rr, ex null: every candidate's score to out_scores), a rerank call (rr: the selection follows each launch
// on the stream, and the call's rows come back at the end) or an explain call (ex: explain_documents.hip's kernel in the
// score kernel's place, each launch's scores and term rows to ex->out).
sgpu_status score_run(ScoreState* s, const HostIndex& h, const DevView& view, const uint64_t* q_off, const uint32_t* comps,
                      const float* vals, uint32_t nq, uint32_t max_nnz, const uint64_t* cand_off, const uint64_t* cand_ids,
                      float* out_scores, RerankCall* rr = nullptr, const ExplainCall* ex = nullptr) {
  HIP_TRY(hipSetDevice(s->device));
  CallStats& cs = s->score_stats;
  cs.begin();
  const LookupForm form = lookup_form(h, max_nnz);   // the hash table: sized for the call's longest query
  const uint32_t lds = form.table_bytes;
  const uint32_t block = lds > (40u << 10) ? 1024u : (lds > (20u << 10) ? 512u : 256u);
  const ScoreKernel kern = score_kernel(h.comp_width, h.value_type, form.dense);
  const ExplainKernel xkern = explain_kernel(h.comp_width, h.value_type, form.dense);
  int per_cu = 0;
  sgpu_status st = ex ? kernel_fit(xkern, block, lds, &per_cu) : kernel_fit(kern, block, lds, &per_cu);
  if (st != SGPU_OK) return st;
  if (per_cu < 1) return fail(SGPU_ELIMIT, "the score kernel does not fit on a CU (%u bytes of LDS)", lds);
  per_cu = std::min(per_cu, (int)(2048u / block));

  const uint64_t budget = launch_budget(ex ? std::min<uint64_t>(kScoreChunk, kExplainRowBytes / (16ull * ex->m)) : kScoreChunk);
  const uint32_t tile_max = (uint32_t)std::min<uint64_t>(kScoreTile, budget);

  if ((st = stage_queries(s, q_off, comps, vals, nq, nullptr)) != SGPU_OK) return st;
  ScoreArgs a{};
  a.fwd = view.fwd;
  a.doc_ref = view.doc_ref;
  a.q_off = s->q_off.as<const uint64_t>();
  a.q_comp = s->q_comp.as<const uint32_t>();
  a.q_val = s->q_val.as<const float>();
  a.dim = (uint32_t)h.dim;
  a.slot_bits = form.slot_bits;
  a.val_scale = h.val_scale;
  cs.dense = form.dense;
  cs.block = block;
  cs.lds = lds;

  ExplainArgs xa{};
  if (ex) {
    xa.fwd = a.fwd, xa.doc_ref = a.doc_ref, xa.q_off = a.q_off, xa.q_comp = a.q_comp, xa.q_val = a.q_val;
    xa.dim = a.dim, xa.slot_bits = a.slot_bits, xa.val_scale = a.val_scale, xa.m = ex->m;
  }

  if (rr && (st = rerank_rows_begin(s, rr, nq)) != SGPU_OK) return st;

  // launches: consecutive tiles (a query's candidates in runs of at most tile_max) while they fit the budget
  uint32_t q = 0;
  uint64_t pos = 0;   // next candidate of the call
  const uint64_t total = cand_off[nq];
  while (pos < total) {
    s->h_tiles.clear();
    const uint64_t first = pos;
    while (pos < total && pos - first < budget) {
      while (cand_off[q + 1] <= pos) ++q;
      const uint32_t n = (uint32_t)std::min<uint64_t>(std::min<uint64_t>(tile_max, cand_off[q + 1] - pos), budget - (pos - first));
      s->h_tiles.push_back(make_uint4(q, (uint32_t)(pos - first), n, 0u));
      pos += n;
    }
    const uint64_t n_cand = pos - first;
    const uint64_t cells = ex ? n_cand * ex->m : 0;   // of each of a launch's four term arrays, behind its n_cand counts
    if ((st = score_reserve(s, s->tiles, s->h_tiles.size() * sizeof(uint4))) != SGPU_OK || (st = stage_ids(s, cand_ids, first, n_cand)) != SGPU_OK ||
        (st = score_reserve(s, s->scores, n_cand * 4)) != SGPU_OK || (ex && (st = score_reserve(s, s->terms, (n_cand + 4 * cells) * 4)) != SGPU_OK))
      return st;
    HIP_TRY(hipMemcpyAsync(s->tiles.p, s->h_tiles.data(), s->h_tiles.size() * sizeof(uint4), hipMemcpyHostToDevice, s->stream));
    a.tiles = s->tiles.as<const uint4>();
    a.cand = s->cand.as<const uint32_t>();
    a.out = s->scores.as<float>();
    a.n_tiles = (uint32_t)s->h_tiles.size();
    const uint32_t grid = (uint32_t)std::min<uint64_t>(a.n_tiles, (uint64_t)s->n_cu * (uint32_t)per_cu);
    cs.grid = grid;
    if (ex) {
      xa.tiles = a.tiles, xa.cand = a.cand, xa.n_tiles = a.n_tiles, xa.scores = a.out;
      xa.n_terms = s->terms.as<uint32_t>();
      xa.comps = xa.n_terms + n_cand;
      xa.q_vals = (float*)(xa.comps + cells);
      xa.d_vals = xa.q_vals + cells;
      xa.products = xa.d_vals + cells;
      if ((st = launch_timed(s, xkern, grid, block, lds, xa)) != SGPU_OK) return st;
      const uint64_t r0 = first * ex->m;
      HIP_TRY(hipMemcpyAsync(ex->out.scores + first, s->scores.p, n_cand * 4, hipMemcpyDeviceToHost, s->stream));
      HIP_TRY(hipMemcpyAsync(ex->out.n_terms + first, xa.n_terms, n_cand * 4, hipMemcpyDeviceToHost, s->stream));
      HIP_TRY(hipMemcpyAsync(ex->out.comps + r0, xa.comps, cells * 4, hipMemcpyDeviceToHost, s->stream));
      HIP_TRY(hipMemcpyAsync(ex->out.q_vals + r0, xa.q_vals, cells * 4, hipMemcpyDeviceToHost, s->stream));
      HIP_TRY(hipMemcpyAsync(ex->out.d_vals + r0, xa.d_vals, cells * 4, hipMemcpyDeviceToHost, s->stream));
      HIP_TRY(hipMemcpyAsync(ex->out.products + r0, xa.products, cells * 4, hipMemcpyDeviceToHost, s->stream));
    } else {
      if ((st = launch_timed(s, kern, grid, block, lds, a)) != SGPU_OK) return st;
      if (!rr) {
        HIP_TRY(hipMemcpyAsync(out_scores + first, s->scores.p, n_cand * 4, hipMemcpyDeviceToHost, s->stream));
      } else if ((st = rerank_select(s, rr, cand_off, nq, s->h_tiles.front().x, first, pos)) != SGPU_OK) {
        return st;
      }
    }
    if ((st = launch_done(s, &cs)) != SGPU_OK) return st;
    if (rr) {
      float ms = 0.0f;
      HIP_TRY(hipEventElapsedTime(&ms, s->ev1, s->ev2));
      cs.extra[0] += ms;
    }
  }
  return rr ? rerank_rows_end(s, rr, nq) : SGPU_OK;
}

sgpu_status score_state_init(ScoreState* s, int device) {
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

}  // namespace

// the form of the table, the workgroup size that goes with its LDS and the workgroups a CU holds: a score call's
sgpu_status score_pass_begin(const HostIndex& h, uint32_t max_nnz, ScorePass* sp) {
  sp->form = lookup_form(h, max_nnz);
  const uint32_t lds = sp->form.table_bytes;
  sp->block = lds > (40u << 10) ? 1024u : (lds > (20u << 10) ? 512u : 256u);
  int per_cu = 0;
  const sgpu_status st = kernel_fit(score_kernel(h.comp_width, h.value_type, sp->form.dense), sp->block, lds, &per_cu);
  if (st != SGPU_OK) return st;
  if (per_cu < 1) return fail(SGPU_ELIMIT, "the score kernel does not fit on a CU (%u bytes of LDS)", lds);
  sp->per_cu = (uint32_t)std::min(per_cu, (int)(2048u / sp->block));
  return SGPU_OK;
}

sgpu_status score_pass_launch(ScoreState* s, const HostIndex& h, const DevView& view, const ScorePass& sp, const uint64_t* cand_off,
                              const uint64_t* cand_ids, uint32_t qa, uint32_t qb, uint32_t* grid) {
  const uint64_t first = cand_off[qa], n_cand = cand_off[qb] - first;
  s->h_tiles.clear();
  for (uint32_t q = qa; q < qb; ++q)
    for (uint64_t pos = cand_off[q]; pos < cand_off[q + 1]; pos += kScoreTile)
      s->h_tiles.push_back(make_uint4(q, (uint32_t)(pos - first), (uint32_t)std::min<uint64_t>(kScoreTile, cand_off[q + 1] - pos), 0u));
  sgpu_status st;
  if ((st = score_reserve(s, s->tiles, s->h_tiles.size() * sizeof(uint4))) != SGPU_OK || (st = stage_ids(s, cand_ids, first, n_cand)) != SGPU_OK ||
      (st = score_reserve(s, s->scores, n_cand * 4)) != SGPU_OK)
    return st;
  HIP_TRY(hipMemcpyAsync(s->tiles.p, s->h_tiles.data(), s->h_tiles.size() * sizeof(uint4), hipMemcpyHostToDevice, s->stream));
  ScoreArgs a{};
  a.fwd = view.fwd;
  a.doc_ref = view.doc_ref;
  a.q_off = s->q_off.as<const uint64_t>();
  a.q_comp = s->q_comp.as<const uint32_t>();
  a.q_val = s->q_val.as<const float>();
  a.tiles = s->tiles.as<const uint4>();
  a.cand = s->cand.as<const uint32_t>();
  a.out = s->scores.as<float>();
  a.n_tiles = (uint32_t)s->h_tiles.size();
  a.dim = (uint32_t)h.dim;
  a.slot_bits = sp.form.slot_bits;
  a.val_scale = h.val_scale;
  *grid = (uint32_t)std::min<uint64_t>(a.n_tiles, (uint64_t)s->n_cu * sp.per_cu);
  return launch_timed(s, score_kernel(h.comp_width, h.value_type, sp.form.dense), *grid, sp.block, sp.form.table_bytes, a);
}

void score_state_free(ScoreState* s) {
  if (!s) return;
  if (s->device >= 0) (void)hipSetDevice(s->device);
  if (s->stream) (void)hipStreamSynchronize(s->stream);
  for (DeviceBuffer* b : {&s->q_off, &s->q_comp, &s->q_val, &s->cand_off, &s->tiles, &s->cand, &s->scores, &s->sel_tasks, &s->slots,
                          &s->carry, &s->row_scores, &s->row_ids, &s->row_n, &s->terms, &s->x_comps, &s->x_vals, &s->x_n, &s->x_w,
                          &s->x_table, &s->d_pen, &s->c_groups, &s->c_tasks, &s->c_row_groups, &s->c_row_best, &s->c_row_members,
                          &s->f_ext, &s->f_row_sparse, &s->f_row_ext, &s->f_row_rank_s, &s->f_row_rank_e})
    b->release();
  if (s->ev0) (void)hipEventDestroy(s->ev0);
  if (s->ev1) (void)hipEventDestroy(s->ev1);
  if (s->ev2) (void)hipEventDestroy(s->ev2);
  if (s->stream) (void)hipStreamDestroy(s->stream);
  delete s;
}

sgpu_status score_state_of(sgpu_index* idx, uint32_t replica, ScoreState** out) {
  return replica_state(idx, idx->score_mu, idx->score, replica, score_state_init, score_state_free, out);
}

bool call_stats_out(sgpu_index* idx, uint32_t replica, CallStats ScoreState::*which, double* out8) {
  std::lock_guard<std::mutex> lk(idx->score_mu);
  if (replica >= idx->score.size() || !idx->score[replica]) return false;
  ScoreState* s = idx->score[replica];
  std::lock_guard<std::mutex> lk2(s->mu);
  const CallStats& cs = s->*which;
  const double v[8] = {cs.kernel_ms, (double)cs.launches, (double)cs.dense, (double)cs.grid,
                       (double)cs.block, (double)cs.lds,  cs.extra[0],       cs.extra[1]};
  for (int i = 0; i < 8; ++i) out8[i] = v[i];
  return true;
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

// (test hook: what the last score, rerank or explain call on `replica` measured - out8 = {device ms of its score kernels,
// launches, 1 = dense table / 0 = hash, grid, workgroup size, LDS bytes, device ms of the selection kernels, merge rounds}.
// tools/score_probe.py, tools/rerank_probe.py)
bool score_debug_stats(sgpu_index* idx, uint32_t replica, double* out8) {
  return call_stats_out(idx, replica, &ScoreState::score_stats, out8);
}

}  // namespace sgpu
