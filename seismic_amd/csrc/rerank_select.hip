// rerank_select.hip — the SELECTION of sgpu_rerank_documents on the device: per query the k best DISTINCT candidates,
// score descending, id ascending. score_documents_kernel (score_documents.hip) leaves a launch's scores in the device
// scratch; what follows it on the same stream is rerank_select_kernel, once per round.
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
#include <hip/hip_runtime.h>

#include <algorithm>

#include "score_state.hpp"

namespace sgpu {

namespace {

constexpr uint32_t kRerankChunk = 2048;   // C: keys a workgroup-wide team sorts (test hook SGPU_RERANK_CHUNK lowers it)
constexpr uint32_t kSelBlock = 256;
constexpr uint32_t kSelNone = 0xffffffffu;
constexpr SelTier kSelTiers[3] = {{128, 64}, {512, 64}, {kRerankChunk, 256}};
enum { SEL_RAW = 0, SEL_KEYS = 1 };             // a task's source
enum { SEL_TO_SLOT = 0, SEL_TO_ROW = 1, SEL_TO_CARRY = 2 };   // ... and its destination

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

// The selection tasks of one launch - candidates [first, last) of the call, the queries from q0 on - by round and tier
// into s->sel_rounds; returns the slots they use.
uint32_t rerank_plan(ScoreState* s, RerankCall* rr, const uint64_t* cand_off, uint32_t nq, uint32_t q0, uint64_t first, uint64_t last) {
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

}  // namespace

void rerank_setup(RerankCall* rr) {
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

// (a selection task writes the slots it fills and the row's count: the rest of a row stays zero)
sgpu_status rerank_rows_begin(ScoreState* s, const RerankCall* rr, uint32_t nq) {
  const uint64_t cells = (uint64_t)nq * rr->k;
  sgpu_status st;
  if ((st = score_reserve(s, s->carry, 2ull * rr->k * 8)) != SGPU_OK || (st = score_reserve(s, s->row_scores, cells * 4)) != SGPU_OK ||
      (st = score_reserve(s, s->row_ids, cells * 8)) != SGPU_OK || (st = score_reserve(s, s->row_n, (uint64_t)nq * 4)) != SGPU_OK)
    return st;
  HIP_TRY(hipMemsetAsync(s->row_scores.p, 0, cells * 4, s->stream));
  HIP_TRY(hipMemsetAsync(s->row_ids.p, 0, cells * 8, s->stream));
  HIP_TRY(hipMemsetAsync(s->row_n.p, 0, (uint64_t)nq * 4, s->stream));
  HIP_TRY(hipFuncSetAttribute((const void*)rerank_select_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(kRerankChunk * 8u)));
  return SGPU_OK;
}

// one launch per round and tier, in the stream's order behind the score kernel
sgpu_status rerank_select(ScoreState* s, RerankCall* rr, const uint64_t* cand_off, uint32_t nq, uint32_t q_first, uint64_t first,
                          uint64_t last) {
  const uint32_t n_slots = rerank_plan(s, rr, cand_off, nq, q_first, first, last);
  s->h_sel_tasks.clear();
  for (const auto& v : s->sel_rounds) s->h_sel_tasks.insert(s->h_sel_tasks.end(), v.begin(), v.end());
  sgpu_status st;
  if ((st = score_reserve(s, s->sel_tasks, s->h_sel_tasks.size() * sizeof(SelTask))) != SGPU_OK ||
      (st = score_reserve(s, s->slots, (uint64_t)n_slots * rr->k * 8)) != SGPU_OK)
    return st;
  HIP_TRY(hipMemcpyAsync(s->sel_tasks.p, s->h_sel_tasks.data(), s->h_sel_tasks.size() * sizeof(SelTask), hipMemcpyHostToDevice,
                         s->stream));
  SelArgs sel{};
  sel.scores = s->scores.as<const float>();
  sel.cand = s->cand.as<const uint32_t>();
  sel.slots = s->slots.as<uint64_t>();
  sel.carry = s->carry.as<uint64_t>();
  sel.row_scores = s->row_scores.as<float>();
  sel.row_ids = s->row_ids.as<uint64_t>();
  sel.row_n = s->row_n.as<uint32_t>();
  sel.k = rr->k;
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
    const sgpu_status lst = kernel_launch(rerank_select_kernel, sel_grid, kSelBlock, teams * tier.cap * 8u, s->stream, sel);
    if (lst != SGPU_OK) return lst;
    at += n;
  }
  HIP_TRY(hipEventRecord(s->ev2, s->stream));
  s->score_stats.extra[1] += (double)((uint32_t)(s->sel_rounds.size() / rr->n_tiers) - 1u);
  return SGPU_OK;
}

sgpu_status rerank_rows_end(ScoreState* s, const RerankCall* rr, uint32_t nq) {
  const uint64_t cells = (uint64_t)nq * rr->k;
  HIP_TRY(hipMemcpyAsync(rr->out_scores, s->row_scores.p, cells * 4, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipMemcpyAsync(rr->out_doc_ids, s->row_ids.p, cells * 8, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipMemcpyAsync(rr->out_n, s->row_n.p, (uint64_t)nq * 4, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return SGPU_OK;
}

}  // namespace sgpu
