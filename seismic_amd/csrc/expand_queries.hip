// expand_queries.hip — Rocchio feedback queries built on the device (sgpu_expand_queries).
//
// Per query the dense f32 table W over the vocabulary of include/seismic_hip.h: cleared, the query's fl(alpha * w)
// written, every feedback document added in the order given, then the t best components with W > 0 selected and
// written in ascending component order. A workgroup of kExpandBlock threads owns one query at a time (a plain index
// range over the grid) and keeps W in LDS where dim + 1 floats fit kScoreDenseLds (DENSE: one workgroup per CU, the
// score kernel's rule), else in its own slice of the call's global scratch; both are arms of one kernel.
//
//   add     the documents of a query are taken strictly in order, a workgroup barrier before each: W[c] = W[c] + p is
//           not associative, and the order of the documents is the only order the contract fixes (a document's
//           components are distinct, so its own additions touch different entries). A document's passes of 128
//           elements go over the workgroup's 16-lane groups, decoded through record.hpp as the score kernel decodes
//           them; an element e >= len (slice padding: the last component repeated) is MASKED, not added as +-0: its
//           lane would race with the lane that holds the component's real element. The next document's ref and weight
//           are loaded before the barrier.
//   select  key(c) = ordered(W[c] bits) where W[c] > 0, else 0 (no term; ordered() sets the top bit of a positive, so 0
//           is no term's key). A histogram over the keys' top byte also counts the terms; where there are more than t,
//           a radix select of four 8-bit steps over the table (exact_device.hip's, device_prims.hpp's pick) leaves the
//           t-th largest key `thr` and how many of the entries equal to it are still needed.
//   emit    one more pass in component order: the entries above thr and the first `need` equal to it. Each wavefront
//           takes a contiguous segment of the table, 64 entries at a time; it counts what it keeps (ballots), the
//           totals of the 16 wavefronts go through LDS, and a second pass over the segment places every kept entry at
//           (kept entries above thr before it) + min(entries equal to thr before it, need). Ascending components and
//           the tie rule (smaller component first) both follow from the pass order. Slots past the terms are zeroed.
// Every loop is bounded by the task's own counts (queries of the launch, table entries, the query's elements and
// candidates, passes = ceil(len / 128), four radix steps); no loop waits on another workgroup; every barrier sits under
// conditions that are workgroup-uniform (the query, its candidate count, the radix step, the shared term count).
// Every table index is a stored component (< dim: validate_desc) or a loop index <= dim; every row index is below t.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "score_state.hpp"

namespace sgpu {

namespace {

constexpr uint32_t kExpandBlock = 1024;   // threads of a workgroup (16 wavefronts: the kernel's wave totals are sized by it)
constexpr uint64_t kExpandTableBytes = 1ull << 30;   // most global scratch the tables of a launch's workgroups take

struct ExpandArgs {
  const uint8_t* fwd;         // DevView::fwd and doc_ref
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

constexpr uint32_t kExpandWaves = kExpandBlock / 64u;

__device__ __forceinline__ uint32_t expand_key(float w) { return w > 0.0f ? ordered_u32(w) : 0u; }

template <int CW, int VT, bool DENSE>
__global__ __launch_bounds__(kExpandBlock) void expand_queries_kernel(ExpandArgs a) {
  using CT = typename std::conditional<CW == 2, uint16_t, uint32_t>::type;
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  __shared__ uint32_t hist[256];
  __shared__ uint32_t s_sel[4];
  __shared__ uint32_t s_total;
  __shared__ uint32_t s_cnt[2 * kExpandWaves];   // per wavefront: entries above the threshold, entries equal to it
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t g = tid >> 4, l = tid & 15u;
  constexpr uint32_t nt = kExpandBlock, ng = kExpandBlock / 16u;
  const uint32_t n_tab = a.dim + 1u;
  float* W = DENSE ? (float*)smem : a.table + (size_t)blockIdx.x * n_tab;
  const uint32_t seg = (n_tab + kExpandWaves - 1u) / kExpandWaves;
  const uint32_t s0 = min(wave * seg, n_tab), s1 = min(s0 + seg, n_tab);   // this wavefront's segment of the table
  const uint32_t t = a.t;

  for (uint32_t q = a.q_first + blockIdx.x; q < a.q_last; q += gridDim.x) {   // (workgroup-uniform)
    // 1. clear, 2. the query
    for (uint32_t i = tid; i < n_tab; i += nt) W[i] = 0.0f;
    __syncthreads();
    const uint64_t q0 = a.q_off[q], q1 = a.q_off[q + 1];
    for (uint64_t j = q0 + tid; j < q1; j += nt) W[a.q_comp[j]] = __fmul_rn(a.alpha, a.q_val[j]);   // (distinct components)
    // 3. the documents, in order
    const uint32_t c0 = (uint32_t)(a.cand_off[q] - a.cand_base), c1 = (uint32_t)(a.cand_off[q + 1] - a.cand_base);
    uint64_t ref_next = 0;
    float w_next = 0.0f;
    if (c0 < c1) ref_next = a.doc_ref[a.cand[c0]], w_next = a.cand_w[c0];
    for (uint32_t i = c0; i < c1; ++i) {
      const uint64_t ref = ref_next;
      const float wd = Vt<VT>::half ? w_next : __fmul_rn(w_next, a.val_scale);
      if (i + 1u < c1) ref_next = a.doc_ref[a.cand[i + 1u]], w_next = a.cand_w[i + 1u];
      __syncthreads();   // the query's weights and the documents before this one are in the table
      const uint32_t len = (uint32_t)ref & LenMask<VT>::v;
      const bool raw = Vt<VT>::sliced && ((uint32_t)ref & kRawBit) != 0u;
      const uint8_t* rec = a.fwd + (size_t)(ref >> 16) * 16u;
      for (uint32_t p0 = g * 128u; p0 < len; p0 += ng * 128u) {
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
        for (int k = 0; k < 8; ++k)
          if (e0 + (uint32_t)k < len) {   // (padding elements add nothing)
            const float p = __fmul_rn(wd, slice_value<VT>(d.v, k));
            W[c[k]] = __fadd_rn(W[c[k]], p);
          }
      }
    }
    __syncthreads();
    // 4. select: the t-th largest key, if there are more than t terms
    uint32_t prefix = 0, mask = 0, need = t;
    bool all = false;
    for (int shift = 24; shift >= 0; shift -= 8) {
      if (tid < 256u) hist[tid] = 0;
      __syncthreads();
      for (uint32_t i = tid; i < n_tab; i += nt) {
        const uint32_t key = expand_key(W[i]);
        if (key != 0u && (key & mask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
      }
      __syncthreads();
      if (tid < 64u) {
        if (shift == 24) {   // every term is in this histogram
          const uint32_t s = hist[4u * lane] + hist[4u * lane + 1u] + hist[4u * lane + 2u] + hist[4u * lane + 3u];
          const uint32_t incl = wave_incl_scan(s);
          if (lane == 63u) s_total = incl;
        }
        radix_select_pick(hist, need, lane, s_sel);   // (writes nothing where need exceeds the count: not read then)
      }
      __syncthreads();
      if (shift == 24 && s_total <= t) {   // (uniform: shared) every term is kept
        all = true;
        break;
      }
      prefix |= s_sel[0] << shift;
      mask |= 255u << shift;
      need = s_sel[1];
    }
    const uint32_t n_terms = all ? s_total : t;
    const uint32_t thr = all ? 0u : prefix, take_eq = all ? 0u : need;
    // 5. emit: count per wavefront segment, then place
    uint32_t n_gt = 0, n_eq = 0;
    for (uint32_t b = s0; b < s1; b += 64u) {
      const uint32_t i = b + lane;
      const uint32_t key = i < s1 ? expand_key(W[i]) : 0u;
      n_gt += (uint32_t)__popcll(__ballot(key > thr));
      n_eq += (uint32_t)__popcll(__ballot(!all && key == thr));
    }
    if (lane == 0u) s_cnt[2u * wave] = n_gt, s_cnt[2u * wave + 1u] = n_eq;
    __syncthreads();
    uint32_t gt_before = 0, eq_before = 0;
    for (uint32_t x = 0; x < wave; ++x) gt_before += s_cnt[2u * x], eq_before += s_cnt[2u * x + 1u];
    uint32_t* row_c = a.out_comps + (size_t)q * t;
    float* row_v = a.out_vals + (size_t)q * t;
    const uint64_t below = (1ull << lane) - 1ull;
    for (uint32_t b = s0; b < s1; b += 64u) {
      const uint32_t i = b + lane;
      const float w = i < s1 ? W[i] : 0.0f;
      const uint32_t key = expand_key(w);
      const bool is_gt = key > thr, is_eq = !all && key == thr;
      const uint64_t m_gt = __ballot(is_gt), m_eq = __ballot(is_eq);
      const uint32_t my_gt = gt_before + (uint32_t)__popcll(m_gt & below), my_eq = eq_before + (uint32_t)__popcll(m_eq & below);
      if (is_gt || (is_eq && my_eq < take_eq)) {
        const uint32_t pos = my_gt + min(my_eq, take_eq);
        if (pos < t) row_c[pos] = i, row_v[pos] = w;   // (pos < n_terms <= t by the counts; the guard costs nothing)
      }
      gt_before += (uint32_t)__popcll(m_gt);
      eq_before += (uint32_t)__popcll(m_eq);
    }
    for (uint32_t i = n_terms + tid; i < t; i += nt) row_c[i] = 0u, row_v[i] = 0.0f;
    if (tid == 0u) a.out_n[q] = n_terms;
    __syncthreads();   // the table, hist and the counts are the next query's
  }
}

using ExpandKernel = void (*)(ExpandArgs);
ExpandKernel expand_kernel(uint32_t cw, uint32_t vt, bool dense) {
  return for_variant(cw, vt, dense, [](auto CW, auto VT, auto D) -> ExpandKernel { return expand_queries_kernel<CW(), VT(), D()>; });
}

// An expand call: the kernel over the call's queries. A launch takes whole queries (next_whole_queries), so no table is
// carried between launches; the call's rows stay on the device until its end.
sgpu_status expand_run(ScoreState* s, const HostIndex& h, const DevView& view, const uint64_t* q_off, const uint32_t* comps,
                       const float* vals, uint32_t nq, const uint64_t* cand_off, const uint64_t* cand_ids, const float* cand_w, float alpha,
                       uint32_t t, uint32_t* out_comps, float* out_vals, uint32_t* out_n) {
  HIP_TRY(hipSetDevice(s->device));
  CallStats& cs = s->expand_stats;
  cs.begin();
  // the table: in LDS where the dense form is chosen, else one per workgroup in the global scratch
  const LookupForm form = lookup_form(h, 0);
  const bool dense = form.dense;
  const uint32_t lds = dense ? form.table_bytes : 0u;
  const ExpandKernel kern = expand_kernel(h.comp_width, h.value_type, dense);
  int per_cu = 0;
  sgpu_status st;
  if ((st = kernel_fit(kern, kExpandBlock, lds, &per_cu)) != SGPU_OK) return st;
  if (per_cu < 1) return fail(SGPU_ELIMIT, "the expand kernel does not fit on a CU (%u bytes of LDS)", lds);
  per_cu = std::min(per_cu, (int)(2048u / kExpandBlock));
  uint64_t max_grid = (uint64_t)s->n_cu * (uint32_t)per_cu;
  if (!dense) max_grid = std::max<uint64_t>(1, std::min<uint64_t>(max_grid, kExpandTableBytes / ((h.dim + 1) * 4)));
  max_grid = hooked_grid(max_grid, "SGPU_EXPAND_GRID");
  const uint64_t budget = launch_budget();

  const uint64_t cells = (uint64_t)nq * t;
  if ((st = stage_queries(s, q_off, comps, vals, nq, cand_off)) != SGPU_OK || (st = score_reserve(s, s->x_comps, cells * 4)) != SGPU_OK ||
      (st = score_reserve(s, s->x_vals, cells * 4)) != SGPU_OK || (st = score_reserve(s, s->x_n, (uint64_t)nq * 4)) != SGPU_OK)
    return st;
  ExpandArgs a{};
  a.fwd = view.fwd;
  a.doc_ref = view.doc_ref;
  a.q_off = s->q_off.as<const uint64_t>();
  a.q_comp = s->q_comp.as<const uint32_t>();
  a.q_val = s->q_val.as<const float>();
  a.cand_off = s->cand_off.as<const uint64_t>();
  a.out_comps = s->x_comps.as<uint32_t>();
  a.out_vals = s->x_vals.as<float>();
  a.out_n = s->x_n.as<uint32_t>();
  a.dim = (uint32_t)h.dim;
  a.t = t;
  a.alpha = alpha;
  a.val_scale = h.val_scale;
  cs.dense = dense;
  cs.block = kExpandBlock;
  cs.lds = lds;

  for (uint32_t q = 0; q < nq;) {
    const uint32_t qa = next_whole_queries(cand_off, nq, budget, &q);
    const uint64_t first = cand_off[qa], n_cand = cand_off[q] - first;   // (<= max(budget, kExpandMaxCand) < 2^32)
    const uint32_t grid = (uint32_t)std::min<uint64_t>(q - qa, max_grid);
    if ((st = stage_ids(s, cand_ids, first, n_cand)) != SGPU_OK || (st = score_reserve(s, s->x_w, n_cand * 4)) != SGPU_OK) return st;
    if (!dense) {
      const uint64_t bytes = (uint64_t)grid * (h.dim + 1) * 4;
      if ((st = score_reserve(s, s->x_table, bytes)) != SGPU_OK) return st;
      cs.extra[0] = std::max(cs.extra[0], (double)bytes);
    }
    if (n_cand) HIP_TRY(hipMemcpyAsync(s->x_w.p, cand_w + first, n_cand * 4, hipMemcpyHostToDevice, s->stream));
    a.cand = s->cand.as<const uint32_t>();
    a.cand_w = s->x_w.as<const float>();
    a.table = s->x_table.as<float>();
    a.cand_base = first;
    a.q_first = qa;
    a.q_last = q;
    cs.grid = grid;
    if ((st = launch_timed(s, kern, grid, kExpandBlock, lds, a)) != SGPU_OK || (st = launch_done(s, &cs)) != SGPU_OK) return st;
  }
  HIP_TRY(hipMemcpyAsync(out_comps, s->x_comps.p, cells * 4, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipMemcpyAsync(out_vals, s->x_vals.p, cells * 4, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipMemcpyAsync(out_n, s->x_n.p, (uint64_t)nq * 4, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return SGPU_OK;
}

}  // namespace

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

// (test hook: what the last expand call on `replica` measured - out8 = {device ms of its kernels, launches, 1 = table in LDS /
// 0 = in global memory, grid of the last launch, workgroup size, LDS bytes, bytes of the global tables, 0}. tools/expand_probe.py)
bool expand_debug_stats(sgpu_index* idx, uint32_t replica, double* out8) {
  if (!call_stats_out(idx, replica, &ScoreState::expand_stats, out8)) return false;
  out8[4] = (double)kExpandBlock;   // (a constant, also before the replica's first expand call)
  return true;
}

}  // namespace sgpu
