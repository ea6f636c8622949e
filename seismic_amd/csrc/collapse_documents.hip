// collapse_documents.hip — the k best GROUPS of each query's candidates on the device (sgpu_collapse_documents): field
// collapsing, MaxP and sum-of-the-m-best over caller-given group keys.
//
// score_documents_kernel (score_documents.hip) leaves a launch's scores in the device scratch, one per listed entry; what
// follows it on the same stream is collapse_select_kernel, one TEAM of threads per query, everything in LDS:
//   A       ordered(score) << 32 | ~id of every entry, sorted descending (rerank_select.hip's key: a larger key is a
//           better member - higher score, then lower id). An entry's RANK is the first place its key stands at, found by
//           binary search: the entries of one id carry one score, hence one key and one rank. Padding 0 sorts last;
//           places [0, n) hold the n entries' keys.
//   B       group << 32 | rank of every entry, sorted ascending. A group is then a contiguous run with its members best
//           first, and the listings of one (group, id) pair are EQUAL keys, next to each other. Padding is all ones: a
//           rank is below the entry count <= 4096, so no entry makes it, whatever its group key (0 and 0xffffffff are
//           keys like any other). Places [0, n) hold the entries.
//   heads   a place of B whose predecessor has another group. Its thread walks the run, skips a key equal to its
//           predecessor, counts the distinct members and adds the first m of their scores (A[rank]) in that order, each
//           sum rounded once: the contract's sequential sum, a loop of one thread. The count goes to M at the head's
//           place; the heads are counted over the team (an LDS atomic).
//   C       ordered(group score) << 32 | ~group at the heads' places, 0 elsewhere, sorted descending: the first
//           min(k, heads) are the row. Slot j finds its group's head again by binary search in B (sorted by group),
//           there its best member's rank (the run's first key) and the member count.
// A team is a wavefront for queries of at most 128 and of at most 512 entries (four teams per workgroup) and the whole
// workgroup up to 1024 and up to 4096; the queries of a launch go to one kernel launch per tier. 28 bytes of LDS per
// entry of the tier's capacity: 14 KiB, 56 KiB, 28 KiB and 112 KiB per workgroup.
// Every loop is bounded by the task's own counts (tasks of the launch, cap, the n <= cap entries of the query, k); the
// three sorts run over cap keys whatever the query holds, so every barrier is workgroup-uniform: cap is a property of
// the launch, never of the task (rerank_select.hip). Every LDS index is a loop index below cap, a binary search's result
// clamped below n, or a rank - the low half of a B key at a place below n, which such a search wrote. Every row index is
// below k. No loop waits on another workgroup.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "score_state.hpp"

namespace sgpu {

namespace {

constexpr uint32_t kColBlock = 256;
constexpr uint32_t kColEntryBytes = 28;   // A, B, C: 8 each; M: 4
constexpr uint32_t kColTierCount = 4;
constexpr SelTier kColTiers[kColTierCount] = {{128, 64}, {512, 64}, {1024, kColBlock}, {(uint32_t)kCollapseMaxCand, kColBlock}};
constexpr uint64_t kColPad = ~0ull;

struct CollapseArgs {
  const uint32_t* tasks;      // the queries of this kernel launch
  const uint64_t* cand_off;   // the call's candidate offsets, staged
  const float* scores;        // the launch's scores, candidate ids and group keys: entry i of the call at [i - cand_base]
  const uint32_t* cand;
  const uint32_t* groups;
  uint32_t* row_groups;       // the call's rows [nq x k], zeroed before the first launch, and counts
  float* row_scores;
  uint64_t* row_ids;
  float* row_best;
  uint32_t* row_members;
  uint32_t* row_n;
  uint64_t cand_base;
  uint32_t n_tasks, cap, team, m, k;
};

__device__ __forceinline__ uint64_t member_key(float score, uint32_t id) {
  return ((uint64_t)ordered_u32(score) << 32) | (uint64_t)(~id);
}
__device__ __forceinline__ float key_score(uint64_t key) { return ordered_u32_inv((uint32_t)(key >> 32)); }

__global__ __launch_bounds__(kColBlock) void collapse_select_kernel(CollapseArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  __shared__ uint32_t s_heads[kColBlock / 64];
  const uint32_t tid = threadIdx.x;
  const uint32_t cap = a.cap, team = a.team, m = a.m, k = a.k;
  const uint32_t teams = kColBlock / team, tm = tid / team, lt = tid % team;
  uint64_t* A = (uint64_t*)smem + (size_t)tm * cap;
  uint64_t* B = (uint64_t*)smem + (size_t)(teams + tm) * cap;
  uint64_t* Ck = (uint64_t*)smem + (size_t)(2u * teams + tm) * cap;
  uint32_t* M = (uint32_t*)((uint64_t*)smem + (size_t)3u * teams * cap) + (size_t)tm * cap;
  // (every bound below is workgroup-uniform: a team without a task runs the same barriers over padding)
  for (uint32_t base = blockIdx.x * teams; base < a.n_tasks; base += gridDim.x * teams) {
    const bool live = base + tm < a.n_tasks;
    uint32_t q = 0, c0 = 0, n = 0;
    if (live) {
      q = a.tasks[base + tm];
      c0 = (uint32_t)(a.cand_off[q] - a.cand_base);
      n = min((uint32_t)(a.cand_off[q + 1] - a.cand_off[q]), cap);   // (<= cap: the host's tier)
    }
    // A: the members' keys, best first
    for (uint32_t i = lt; i < cap; i += team) A[i] = i < n ? member_key(a.scores[c0 + i], a.cand[c0 + i]) : 0ull;
    if (lt == 0u) s_heads[tm] = 0u;
    __syncthreads();
    bitonic_sort_lds<true>(A, cap, lt, team);
    // B: every entry's group and rank
    for (uint32_t i = lt; i < cap; i += team) {
      uint64_t v = kColPad;
      if (i < n) {
        const uint64_t key = member_key(a.scores[c0 + i], a.cand[c0 + i]);
        uint32_t lo = 0, hi = n;   // the first place of A[0, n) whose key is not above this one: the key's own
        while (lo < hi) {
          const uint32_t mid = (lo + hi) >> 1;
          if (A[mid] > key) lo = mid + 1u; else hi = mid;
        }
        v = ((uint64_t)a.groups[c0 + i] << 32) | (uint64_t)min(lo, n - 1u);
      }
      B[i] = v;
    }
    __syncthreads();
    bitonic_sort_lds<false>(B, cap, lt, team);
    // the heads: each walks its run
    uint32_t heads = 0;
    for (uint32_t e = lt; e < cap; e += team) {
      uint64_t ck = 0;
      if (e < n) {
        const uint64_t b = B[e];
        const uint32_t g = (uint32_t)(b >> 32);
        if (e == 0u || (uint32_t)(B[e - 1u] >> 32) != g) {
          float sum = 0.0f;
          uint32_t cnt = 0;
          uint64_t prev = kColPad;   // (no entry's key)
          for (uint32_t x = e; x < n; ++x) {
            const uint64_t bx = B[x];
            if ((uint32_t)(bx >> 32) != g) break;
            if (bx != prev) {
              ++cnt;
              if (cnt <= m) {
                const float sc = key_score(A[(uint32_t)bx]);
                sum = cnt == 1u ? sc : __fadd_rn(sum, sc);
              }
            }
            prev = bx;
          }
          M[e] = cnt;
          ck = ((uint64_t)ordered_u32(sum) << 32) | (uint64_t)(~g);
          ++heads;
        }
      }
      Ck[e] = ck;
    }
    if (heads) atomicAdd(&s_heads[tm], heads);
    __syncthreads();
    bitonic_sort_lds<true>(Ck, cap, lt, team);
    // the row: the first min(k, heads) group keys, each with its head's record
    const uint32_t kept = min(min(s_heads[tm], n), k);
    if (live) {
      for (uint32_t j = lt; j < kept; j += team) {
        const uint64_t c = Ck[j];
        const uint32_t g = ~(uint32_t)c;
        const uint64_t want = (uint64_t)g << 32;
        uint32_t lo = 0, hi = n;   // the first place of B[0, n) of group g: its head
        while (lo < hi) {
          const uint32_t mid = (lo + hi) >> 1;
          if (B[mid] < want) lo = mid + 1u; else hi = mid;
        }
        const uint32_t p = min(lo, n - 1u);
        const uint64_t best = A[min((uint32_t)B[p], n - 1u)];
        const size_t o = (size_t)q * k + j;
        a.row_groups[o] = g;
        a.row_scores[o] = key_score(c);
        a.row_ids[o] = (uint64_t)(~(uint32_t)best);
        a.row_best[o] = key_score(best);
        a.row_members[o] = M[p];
      }
      if (lt == 0u) a.row_n[q] = kept;   // (the row's other slots are zero since the call's start)
    }
    __syncthreads();   // the arrays and s_heads are the next task's
  }
}

// A collapse call: per launch of whole queries (next_whole_queries) the score kernel over their entries, then the
// selection, one kernel launch per tier that has a query; the call's rows stay on the device until its end, zeroed before
// the first launch.
sgpu_status collapse_run(ScoreState* s, const HostIndex& h, const DevView& view, const uint64_t* q_off, const uint32_t* comps,
                         const float* vals, uint32_t nq, uint32_t max_nnz, const uint64_t* cand_off, const uint64_t* cand_ids,
                         const uint32_t* cand_groups, uint32_t m, uint32_t k, const CollapseOut& out) {
  HIP_TRY(hipSetDevice(s->device));
  CallStats& cs = s->collapse_stats;
  cs.begin();
  ScorePass sp;
  sgpu_status st;
  if ((st = score_pass_begin(h, max_nnz, &sp)) != SGPU_OK) return st;
  HIP_TRY(hipFuncSetAttribute((const void*)collapse_select_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)(kCollapseMaxCand * kColEntryBytes)));
  const uint64_t max_grid = hooked_grid((uint64_t)s->n_cu * (2048u / kColBlock), "SGPU_COLLAPSE_GRID");
  const uint64_t budget = launch_budget();

  const uint64_t cells = (uint64_t)nq * k;
  if ((st = stage_queries(s, q_off, comps, vals, nq, cand_off)) != SGPU_OK || (st = score_reserve(s, s->c_row_groups, cells * 4)) != SGPU_OK ||
      (st = score_reserve(s, s->row_scores, cells * 4)) != SGPU_OK || (st = score_reserve(s, s->row_ids, cells * 8)) != SGPU_OK ||
      (st = score_reserve(s, s->c_row_best, cells * 4)) != SGPU_OK || (st = score_reserve(s, s->c_row_members, cells * 4)) != SGPU_OK ||
      (st = score_reserve(s, s->row_n, (uint64_t)nq * 4)) != SGPU_OK)
    return st;
  HIP_TRY(hipMemsetAsync(s->c_row_groups.p, 0, cells * 4, s->stream));
  HIP_TRY(hipMemsetAsync(s->row_scores.p, 0, cells * 4, s->stream));
  HIP_TRY(hipMemsetAsync(s->row_ids.p, 0, cells * 8, s->stream));
  HIP_TRY(hipMemsetAsync(s->c_row_best.p, 0, cells * 4, s->stream));
  HIP_TRY(hipMemsetAsync(s->c_row_members.p, 0, cells * 4, s->stream));
  HIP_TRY(hipMemsetAsync(s->row_n.p, 0, (uint64_t)nq * 4, s->stream));
  CollapseArgs a{};
  a.cand_off = s->cand_off.as<const uint64_t>();
  a.row_groups = s->c_row_groups.as<uint32_t>();
  a.row_scores = s->row_scores.as<float>();
  a.row_ids = s->row_ids.as<uint64_t>();
  a.row_best = s->c_row_best.as<float>();
  a.row_members = s->c_row_members.as<uint32_t>();
  a.row_n = s->row_n.as<uint32_t>();
  a.m = m;
  a.k = k;
  cs.dense = sp.form.dense;
  cs.block = sp.block;
  cs.lds = sp.form.table_bytes;

  std::vector<uint32_t>& tasks = s->h_col_tasks;
  for (uint32_t q = 0; q < nq;) {
    const uint32_t qa = next_whole_queries(cand_off, nq, budget, &q);
    const uint64_t first = cand_off[qa], n_cand = cand_off[q] - first;   // (<= max(budget, kCollapseMaxCand) < 2^32)
    if (n_cand == 0) continue;   // (queries without candidates: their rows are zero already)
    uint32_t tier_n[kColTierCount] = {};
    tasks.clear();
    for (uint32_t t = 0; t < kColTierCount; ++t)
      for (uint32_t x = qa; x < q; ++x) {
        const uint64_t len = cand_off[x + 1] - cand_off[x];
        if (len != 0 && len <= kColTiers[t].cap && (t == 0 || len > kColTiers[t - 1].cap)) tasks.push_back(x), ++tier_n[t];
      }
    if ((st = score_reserve(s, s->c_groups, n_cand * 4)) != SGPU_OK || (st = score_reserve(s, s->c_tasks, tasks.size() * 4)) != SGPU_OK) return st;
    HIP_TRY(hipMemcpyAsync(s->c_groups.p, cand_groups + first, n_cand * 4, hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipMemcpyAsync(s->c_tasks.p, tasks.data(), tasks.size() * 4, hipMemcpyHostToDevice, s->stream));
    if ((st = score_pass_launch(s, h, view, sp, cand_off, cand_ids, qa, q, &cs.grid)) != SGPU_OK) return st;
    a.scores = s->scores.as<const float>();
    a.cand = s->cand.as<const uint32_t>();
    a.groups = s->c_groups.as<const uint32_t>();
    a.cand_base = first;
    uint32_t at = 0;
    for (uint32_t t = 0; t < kColTierCount; ++t) {
      if (!tier_n[t]) continue;
      const SelTier& tier = kColTiers[t];
      const uint32_t teams = kColBlock / tier.team;
      a.tasks = s->c_tasks.as<const uint32_t>() + at;
      a.n_tasks = tier_n[t];
      a.cap = tier.cap;
      a.team = tier.team;
      const uint32_t grid = (uint32_t)std::min<uint64_t>((tier_n[t] + teams - 1) / teams, max_grid);
      if ((st = kernel_launch(collapse_select_kernel, grid, kColBlock, teams * tier.cap * kColEntryBytes, s->stream, a)) != SGPU_OK) return st;
      at += tier_n[t];
      cs.extra[1] += 1.0;
    }
    HIP_TRY(hipEventRecord(s->ev2, s->stream));
    if ((st = launch_done(s, &cs)) != SGPU_OK) return st;
    float ms = 0.0f;
    HIP_TRY(hipEventElapsedTime(&ms, s->ev1, s->ev2));
    cs.extra[0] += ms;
  }
  HIP_TRY(hipMemcpyAsync(out.groups, s->c_row_groups.p, cells * 4, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipMemcpyAsync(out.scores, s->row_scores.p, cells * 4, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipMemcpyAsync(out.best_ids, s->row_ids.p, cells * 8, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipMemcpyAsync(out.best_scores, s->c_row_best.p, cells * 4, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipMemcpyAsync(out.members, s->c_row_members.p, cells * 4, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipMemcpyAsync(out.n, s->row_n.p, (uint64_t)nq * 4, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return SGPU_OK;
}

}  // namespace

sgpu_status collapse_documents_device(sgpu_index* idx, uint32_t replica, const uint64_t* q_off, const uint32_t* comps,
                                      const float* vals, uint32_t nq, const uint64_t* cand_off, const uint64_t* cand_ids,
                                      const uint32_t* cand_groups, uint32_t m, uint32_t k, const CollapseOut& out) {
  if (!idx) return fail(SGPU_EINVAL, "null argument");
  uint32_t max_nnz = 0, max_cand = 0;
  const sgpu_status vst = collapse_check_args(idx->host, q_off, comps, vals, nq, cand_off, cand_ids, cand_groups, m, k, out, &max_nnz, &max_cand);
  if (vst != SGPU_OK) return vst;
  ScoreState* s = nullptr;
  const sgpu_status sst = score_state_of(idx, replica, &s);
  if (sst != SGPU_OK) return sst;
  if (nq == 0) return SGPU_OK;
  std::lock_guard<std::mutex> lk(s->mu);
  try {
    return collapse_run(s, idx->host, device_index_view(idx->replicas[replica]), q_off, comps, vals, nq, max_nnz, cand_off, cand_ids,
                        cand_groups, m, k, out);
  } catch (const std::bad_alloc&) {
    return fail(SGPU_ENOMEM, "out of host memory");
  }
}

// (test hook: what the last collapse call on `replica` measured - out8 = {device ms of its score kernels, launches, 1 = dense
// table / 0 = hash, grid, workgroup size and LDS bytes of the score kernel's last launch, device ms of the selection kernels,
// selection kernel launches}. tools/collapse_probe.py)
bool collapse_debug_stats(sgpu_index* idx, uint32_t replica, double* out8) {
  return call_stats_out(idx, replica, &ScoreState::collapse_stats, out8);
}

}  // namespace sgpu
