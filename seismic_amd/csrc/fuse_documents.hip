// fuse_documents.hip — hybrid fusion of each query's candidates on the device (sgpu_fuse_documents): this index's scores
// fused with another retriever's over the union of both lists, by reciprocal ranks, min-max normalised scores or a
// weighted sum; the k best come back with both scores and both ranks.
//
// score_documents_kernel (score_documents.hip) leaves a launch's scores in the device scratch, one per listed entry; what
// follows it on the same stream is fuse_select_kernel, one TEAM of threads per query, everything in LDS:
//   A       id << 32 | entry index of every entry, sorted ascending; padding is all ones and sorts last, so places
//           [0, n) hold the n entries. A place whose predecessor has another id is a HEAD: it stands for one document.
//           Its thread walks the run (the listings of one id) and takes the largest ordered() image among the external
//           scores that are not NaN, 0 where there is none: the document is absent (every float that is no NaN of the
//           full negative payload has an image above 0, and a NaN never gets here). It goes to E at the head's place.
//           The document's sparse score is scores[index of any entry of the run].
//   S       ordered(sparse) << 32 | ~id at the heads' places, 0 elsewhere; X the same with the external image at the
//           places of the heads that are present. Both are sorted descending: places [0, heads) of S and [0, present)
//           of X are the documents best first (a larger key: higher score, then lower id) - the two counts come from
//           LDS atomics over the team. A head finds its own key in either by binary search; the place + 1 is its
//           rank. The ranks go to R at the head's place, two u16 (a rank is at most 4096). The first and last live
//           places of S and X give the largest and smallest score of either kind, which every thread reads into
//           registers before S is overwritten.
//   F       ordered(fused) << 32 | ~id at the heads' places, 0 elsewhere, written over S after a barrier and sorted
//           descending: the first min(k, heads) are the row. Slot j finds its document's head again by binary search
//           in A (sorted by id) and reads E and R there.
// Four sorts; 32 bytes of LDS per entry of the tier's capacity (A, S / F, X: 8 each; E, R: 4 each): 16, 64, 32 and 128 KiB
// per workgroup. A team is a wavefront for queries of at most 128 and of at most 512 entries (four teams per workgroup)
// and the whole workgroup up to 1024 and up to 4096 (collapse_documents.hip's tiers); the queries of a launch go to one
// kernel launch per tier.
// The arithmetic is __fdiv_rn, __fmul_rn, __fadd_rn and __fsub_rn throughout: one rounding per operation, never
// contracted, the bits of the host twin's f32 expressions (score_host.cpp).
// Every loop is bounded by the task's own counts (tasks of the launch, cap, the n <= cap entries of the query, k); the
// four sorts run over cap keys whatever the query holds, so every barrier is workgroup-uniform: cap is a property of
// the launch, never of the task. Every LDS index is a loop index below cap or a binary search's result clamped below n;
// every index into the launch's scores and external scores is c0 + the low half of an A key at a place below n, an
// entry index below n that the first loop wrote. Every row index is below k. No loop waits on another workgroup.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "score_state.hpp"

namespace sgpu {

namespace {

constexpr uint32_t kFuseBlock = 256;
constexpr uint32_t kFuseEntryBytes = 32;   // A, S / F, X: 8 each; E, R: 4 each
constexpr uint32_t kFuseTierCount = 4;
constexpr SelTier kFuseTiers[kFuseTierCount] = {{128, 64}, {512, 64}, {1024, kFuseBlock}, {(uint32_t)kFuseMaxCand, kFuseBlock}};
constexpr uint64_t kFusePad = ~0ull;

struct FuseArgs {
  const uint32_t* tasks;      // the queries of this kernel launch
  const uint64_t* cand_off;   // the call's candidate offsets, staged
  const float* scores;        // the launch's scores, candidate ids and external scores: entry i of the call at [i - cand_base]
  const uint32_t* cand;
  const float* ext;
  float* row_scores;          // the call's rows [nq x k], zeroed before the first launch, and counts
  uint64_t* row_ids;
  float* row_sparse;
  float* row_ext;
  uint32_t* row_rank_s;
  uint32_t* row_rank_e;
  uint32_t* row_n;
  uint64_t cand_base;
  uint32_t n_tasks, cap, team, method, k;
  float w_sparse, w_ext, rrf_c;
};

__device__ __forceinline__ uint64_t doc_key(uint32_t image, uint32_t id) { return ((uint64_t)image << 32) | (uint64_t)(~id); }

// the place of `key` in keys[0, n), sorted descending and holding it: the first place whose key is not above it
__device__ __forceinline__ uint32_t place_desc(const uint64_t* keys, uint32_t n, uint64_t key) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (keys[mid] > key) lo = mid + 1u; else hi = mid;
  }
  return lo;
}

// (v - lo) / (hi - lo), or 1 where all values are one
__device__ __forceinline__ float minmax_norm(float v, float lo, float hi) {
  return hi == lo ? 1.0f : __fdiv_rn(__fsub_rn(v, lo), __fsub_rn(hi, lo));
}

__global__ __launch_bounds__(kFuseBlock) void fuse_select_kernel(FuseArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  __shared__ uint32_t s_heads[kFuseBlock / 64], s_present[kFuseBlock / 64];
  const uint32_t tid = threadIdx.x;
  const uint32_t cap = a.cap, team = a.team, k = a.k, method = a.method;
  const uint32_t teams = kFuseBlock / team, tm = tid / team, lt = tid % team;
  uint64_t* A = (uint64_t*)smem + (size_t)tm * cap;
  uint64_t* S = (uint64_t*)smem + (size_t)(teams + tm) * cap;
  uint64_t* X = (uint64_t*)smem + (size_t)(2u * teams + tm) * cap;
  uint32_t* E = (uint32_t*)((uint64_t*)smem + (size_t)3u * teams * cap) + (size_t)tm * cap;
  uint32_t* R = (uint32_t*)((uint64_t*)smem + (size_t)3u * teams * cap) + (size_t)(teams + tm) * cap;
  // (every bound below is workgroup-uniform: a team without a task runs the same barriers over padding)
  for (uint32_t base = blockIdx.x * teams; base < a.n_tasks; base += gridDim.x * teams) {
    const bool live = base + tm < a.n_tasks;
    uint32_t q = 0, c0 = 0, n = 0;
    if (live) {
      q = a.tasks[base + tm];
      c0 = (uint32_t)(a.cand_off[q] - a.cand_base);
      n = min((uint32_t)(a.cand_off[q + 1] - a.cand_off[q]), cap);   // (<= cap: the host's tier)
    }
    // A: the entries by id
    for (uint32_t i = lt; i < cap; i += team) A[i] = i < n ? ((uint64_t)a.cand[c0 + i] << 32) | (uint64_t)i : kFusePad;
    if (lt == 0u) s_heads[tm] = 0u, s_present[tm] = 0u;
    __syncthreads();
    bitonic_sort_lds<false>(A, cap, lt, team);
    // the heads: each walks its run for the document's external score
    uint32_t heads = 0, present = 0;
    for (uint32_t e = lt; e < cap; e += team) {
      uint64_t sk = 0, xk = 0;
      uint32_t image = 0;
      if (e < n) {
        const uint64_t key = A[e];
        const uint32_t id = (uint32_t)(key >> 32);
        if (e == 0u || (uint32_t)(A[e - 1u] >> 32) != id) {
          for (uint32_t x = e; x < n; ++x) {
            const uint64_t ax = A[x];
            if ((uint32_t)(ax >> 32) != id) break;
            const float v = a.ext[c0 + min((uint32_t)ax, n - 1u)];
            if (v == v) image = max(image, ordered_u32(v));
          }
          sk = doc_key(ordered_u32(a.scores[c0 + min((uint32_t)key, n - 1u)]), id);
          ++heads;
          if (image) xk = doc_key(image, id), ++present;
        }
      }
      S[e] = sk;
      X[e] = xk;
      E[e] = image;
    }
    if (heads) atomicAdd(&s_heads[tm], heads);
    if (present) atomicAdd(&s_present[tm], present);
    __syncthreads();
    bitonic_sort_lds<true>(S, cap, lt, team);
    bitonic_sort_lds<true>(X, cap, lt, team);
    // the ranks: every head's place in either order; and the ends of both
    const uint32_t n_heads = min(s_heads[tm], n), n_present = min(s_present[tm], n_heads);
    float hi_s = 0.0f, lo_s = 0.0f, hi_e = 0.0f, lo_e = 0.0f;
    if (n_heads) hi_s = ordered_u32_inv((uint32_t)(S[0] >> 32)), lo_s = ordered_u32_inv((uint32_t)(S[n_heads - 1u] >> 32));
    if (n_present) hi_e = ordered_u32_inv((uint32_t)(X[0] >> 32)), lo_e = ordered_u32_inv((uint32_t)(X[n_present - 1u] >> 32));
    for (uint32_t e = lt; e < n; e += team) {
      const uint64_t key = A[e];
      const uint32_t id = (uint32_t)(key >> 32);
      if (e == 0u || (uint32_t)(A[e - 1u] >> 32) != id) {
        const float sc = a.scores[c0 + min((uint32_t)key, n - 1u)];
        const uint32_t rs = min(place_desc(S, n_heads, doc_key(ordered_u32(sc), id)), n_heads - 1u) + 1u;
        const uint32_t image = E[e];
        const uint32_t re = image ? min(place_desc(X, n_present, doc_key(image, id)), n_present - 1u) + 1u : 0u;
        R[e] = rs | (re << 16);
      }
    }
    __syncthreads();   // S is read no more
    // F over S: the fused scores
    for (uint32_t e = lt; e < cap; e += team) {
      uint64_t fk = 0;
      if (e < n) {
        const uint64_t key = A[e];
        const uint32_t id = (uint32_t)(key >> 32);
        if (e == 0u || (uint32_t)(A[e - 1u] >> 32) != id) {
          const float sc = a.scores[c0 + min((uint32_t)key, n - 1u)];
          const uint32_t image = E[e], r = R[e];
          const float ex = ordered_u32_inv(image);   // (read where image != 0 only)
          float fused;
          if (method == SGPU_FUSE_RRF) {
            const float te = image ? __fdiv_rn(a.w_ext, __fadd_rn(a.rrf_c, (float)(r >> 16))) : 0.0f;
            fused = __fadd_rn(__fdiv_rn(a.w_sparse, __fadd_rn(a.rrf_c, (float)(r & 0xffffu))), te);
          } else if (method == SGPU_FUSE_MINMAX) {
            const float te = image ? __fmul_rn(a.w_ext, minmax_norm(ex, lo_e, hi_e)) : 0.0f;
            fused = __fadd_rn(__fmul_rn(a.w_sparse, minmax_norm(sc, lo_s, hi_s)), te);
          } else {
            const float te = image ? __fmul_rn(a.w_ext, ex) : 0.0f;
            fused = __fadd_rn(__fmul_rn(a.w_sparse, sc), te);
          }
          fk = doc_key(ordered_u32(fused), id);
        }
      }
      S[e] = fk;
    }
    __syncthreads();
    bitonic_sort_lds<true>(S, cap, lt, team);
    // the row: the first min(k, heads) fused keys, each with its head's record
    const uint32_t kept = min(n_heads, k);
    if (live) {
      for (uint32_t j = lt; j < kept; j += team) {
        const uint64_t f = S[j];
        const uint32_t id = ~(uint32_t)f;
        const uint64_t want = (uint64_t)id << 32;
        uint32_t lo = 0, hi = n;   // the first place of A[0, n) of this id: its head
        while (lo < hi) {
          const uint32_t mid = (lo + hi) >> 1;
          if (A[mid] < want) lo = mid + 1u; else hi = mid;
        }
        const uint32_t p = min(lo, n - 1u);
        const uint32_t image = E[p], r = R[p];
        const size_t o = (size_t)q * k + j;
        a.row_ids[o] = (uint64_t)id;
        a.row_scores[o] = ordered_u32_inv((uint32_t)(f >> 32));
        a.row_sparse[o] = a.scores[c0 + min((uint32_t)A[p], n - 1u)];
        a.row_ext[o] = image ? ordered_u32_inv(image) : 0.0f;
        a.row_rank_s[o] = r & 0xffffu;
        a.row_rank_e[o] = r >> 16;
      }
      if (lt == 0u) a.row_n[q] = kept;   // (the row's other slots are zero since the call's start)
    }
    __syncthreads();   // the arrays and the counts are the next task's
  }
}

// A fuse call: per launch of whole queries (next_whole_queries) the score kernel over their entries, then the selection,
// one kernel launch per tier that has a query; the call's rows stay on the device until its end, zeroed before the first
// launch.
sgpu_status fuse_run(ScoreState* s, const HostIndex& h, const DevView& view, const uint64_t* q_off, const uint32_t* comps,
                     const float* vals, uint32_t nq, uint32_t max_nnz, const uint64_t* cand_off, const uint64_t* cand_ids,
                     const float* cand_ext, uint32_t method, float w_sparse, float w_ext, float rrf_c, uint32_t k, const FuseOut& out) {
  HIP_TRY(hipSetDevice(s->device));
  CallStats& cs = s->fuse_stats;
  cs.begin();
  ScorePass sp;
  sgpu_status st;
  if ((st = score_pass_begin(h, max_nnz, &sp)) != SGPU_OK) return st;
  HIP_TRY(hipFuncSetAttribute((const void*)fuse_select_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)(kFuseMaxCand * kFuseEntryBytes)));
  const uint64_t max_grid = hooked_grid((uint64_t)s->n_cu * (2048u / kFuseBlock), "SGPU_FUSE_GRID");
  const uint64_t budget = launch_budget();

  const uint64_t cells = (uint64_t)nq * k;
  DeviceBuffer* rows4[] = {&s->row_scores, &s->f_row_sparse, &s->f_row_ext, &s->f_row_rank_s, &s->f_row_rank_e};
  if ((st = stage_queries(s, q_off, comps, vals, nq, cand_off)) != SGPU_OK || (st = score_reserve(s, s->row_ids, cells * 8)) != SGPU_OK ||
      (st = score_reserve(s, s->row_n, (uint64_t)nq * 4)) != SGPU_OK)
    return st;
  for (DeviceBuffer* b : rows4)
    if ((st = score_reserve(s, *b, cells * 4)) != SGPU_OK) return st;
  for (DeviceBuffer* b : rows4) HIP_TRY(hipMemsetAsync(b->p, 0, cells * 4, s->stream));
  HIP_TRY(hipMemsetAsync(s->row_ids.p, 0, cells * 8, s->stream));
  HIP_TRY(hipMemsetAsync(s->row_n.p, 0, (uint64_t)nq * 4, s->stream));
  FuseArgs a{};
  a.cand_off = s->cand_off.as<const uint64_t>();
  a.row_scores = s->row_scores.as<float>();
  a.row_ids = s->row_ids.as<uint64_t>();
  a.row_sparse = s->f_row_sparse.as<float>();
  a.row_ext = s->f_row_ext.as<float>();
  a.row_rank_s = s->f_row_rank_s.as<uint32_t>();
  a.row_rank_e = s->f_row_rank_e.as<uint32_t>();
  a.row_n = s->row_n.as<uint32_t>();
  a.method = method;
  a.k = k;
  a.w_sparse = w_sparse;
  a.w_ext = w_ext;
  a.rrf_c = rrf_c;
  cs.dense = sp.form.dense;
  cs.block = sp.block;
  cs.lds = sp.form.table_bytes;

  std::vector<uint32_t>& tasks = s->h_col_tasks;
  for (uint32_t q = 0; q < nq;) {
    const uint32_t qa = next_whole_queries(cand_off, nq, budget, &q);
    const uint64_t first = cand_off[qa], n_cand = cand_off[q] - first;   // (<= max(budget, kFuseMaxCand) < 2^32)
    if (n_cand == 0) continue;   // (queries without candidates: their rows are zero already)
    uint32_t tier_n[kFuseTierCount] = {};
    tasks.clear();
    for (uint32_t t = 0; t < kFuseTierCount; ++t)
      for (uint32_t x = qa; x < q; ++x) {
        const uint64_t len = cand_off[x + 1] - cand_off[x];
        if (len != 0 && len <= kFuseTiers[t].cap && (t == 0 || len > kFuseTiers[t - 1].cap)) tasks.push_back(x), ++tier_n[t];
      }
    if ((st = score_reserve(s, s->f_ext, n_cand * 4)) != SGPU_OK || (st = score_reserve(s, s->c_tasks, tasks.size() * 4)) != SGPU_OK) return st;
    HIP_TRY(hipMemcpyAsync(s->f_ext.p, cand_ext + first, n_cand * 4, hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipMemcpyAsync(s->c_tasks.p, tasks.data(), tasks.size() * 4, hipMemcpyHostToDevice, s->stream));
    if ((st = score_pass_launch(s, h, view, sp, cand_off, cand_ids, qa, q, &cs.grid)) != SGPU_OK) return st;
    a.scores = s->scores.as<const float>();
    a.cand = s->cand.as<const uint32_t>();
    a.ext = s->f_ext.as<const float>();
    a.cand_base = first;
    uint32_t at = 0;
    for (uint32_t t = 0; t < kFuseTierCount; ++t) {
      if (!tier_n[t]) continue;
      const SelTier& tier = kFuseTiers[t];
      const uint32_t teams = kFuseBlock / tier.team;
      a.tasks = s->c_tasks.as<const uint32_t>() + at;
      a.n_tasks = tier_n[t];
      a.cap = tier.cap;
      a.team = tier.team;
      const uint32_t grid = (uint32_t)std::min<uint64_t>((tier_n[t] + teams - 1) / teams, max_grid);
      if ((st = kernel_launch(fuse_select_kernel, grid, kFuseBlock, teams * tier.cap * kFuseEntryBytes, s->stream, a)) != SGPU_OK) return st;
      at += tier_n[t];
      cs.extra[1] += 1.0;
    }
    HIP_TRY(hipEventRecord(s->ev2, s->stream));
    if ((st = launch_done(s, &cs)) != SGPU_OK) return st;
    float ms = 0.0f;
    HIP_TRY(hipEventElapsedTime(&ms, s->ev1, s->ev2));
    cs.extra[0] += ms;
  }
  HIP_TRY(hipMemcpyAsync(out.scores, s->row_scores.p, cells * 4, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipMemcpyAsync(out.doc_ids, s->row_ids.p, cells * 8, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipMemcpyAsync(out.sparse, s->f_row_sparse.p, cells * 4, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipMemcpyAsync(out.ext, s->f_row_ext.p, cells * 4, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipMemcpyAsync(out.rank_sparse, s->f_row_rank_s.p, cells * 4, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipMemcpyAsync(out.rank_ext, s->f_row_rank_e.p, cells * 4, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipMemcpyAsync(out.n, s->row_n.p, (uint64_t)nq * 4, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return SGPU_OK;
}

}  // namespace

sgpu_status fuse_documents_device(sgpu_index* idx, uint32_t replica, const uint64_t* q_off, const uint32_t* comps, const float* vals,
                                  uint32_t nq, const uint64_t* cand_off, const uint64_t* cand_ids, const float* cand_ext,
                                  uint32_t method, float w_sparse, float w_ext, float rrf_c, uint32_t k, const FuseOut& out) {
  if (!idx) return fail(SGPU_EINVAL, "null argument");
  uint32_t max_nnz = 0, max_cand = 0;
  const sgpu_status vst = fuse_check_args(idx->host, q_off, comps, vals, nq, cand_off, cand_ids, cand_ext, method, w_sparse, w_ext,
                                          rrf_c, k, out, &max_nnz, &max_cand);
  if (vst != SGPU_OK) return vst;
  ScoreState* s = nullptr;
  const sgpu_status sst = score_state_of(idx, replica, &s);
  if (sst != SGPU_OK) return sst;
  if (nq == 0) return SGPU_OK;
  std::lock_guard<std::mutex> lk(s->mu);
  try {
    return fuse_run(s, idx->host, device_index_view(idx->replicas[replica]), q_off, comps, vals, nq, max_nnz, cand_off, cand_ids,
                    cand_ext, method, w_sparse, w_ext, rrf_c, k, out);
  } catch (const std::bad_alloc&) {
    return fail(SGPU_ENOMEM, "out of host memory");
  }
}

// (test hook: what the last fuse call on `replica` measured - out8 = {device ms of its score kernels, launches, 1 = dense
// table / 0 = hash, grid, workgroup size and LDS bytes of the score kernel's last launch, device ms of the selection kernels,
// selection kernel launches}. tools/fuse_probe.py)
bool fuse_debug_stats(sgpu_index* idx, uint32_t replica, double* out8) {
  return call_stats_out(idx, replica, &ScoreState::fuse_stats, out8);
}

}  // namespace sgpu
