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

#include "score_lookup.hpp"

namespace sgpu {

namespace {

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
  if (vt == SGPU_VAL_DOTVBYTE) return dense ? expand_queries_kernel<2, VT_DVB, true> : expand_queries_kernel<2, VT_DVB, false>;
  if (vt == SGPU_VAL_FIXEDU8) {
    if (cw == 2) return dense ? expand_queries_kernel<2, VT_U8, true> : expand_queries_kernel<2, VT_U8, false>;
    return dense ? expand_queries_kernel<4, VT_U8, true> : expand_queries_kernel<4, VT_U8, false>;
  }
  if (cw == 2) return dense ? expand_queries_kernel<2, VT_F16, true> : expand_queries_kernel<2, VT_F16, false>;
  return dense ? expand_queries_kernel<4, VT_F16, true> : expand_queries_kernel<4, VT_F16, false>;
}

}  // namespace

sgpu_status expand_kernel_fit(uint32_t cw, uint32_t vt, bool dense, uint32_t lds, int* per_cu) {
  ExpandKernel kern = expand_kernel(cw, vt, dense);
  HIP_TRY(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(per_cu, kern, (int)kExpandBlock, lds));
  return SGPU_OK;
}

sgpu_status expand_kernel_launch(uint32_t cw, uint32_t vt, bool dense, uint32_t grid, uint32_t lds, hipStream_t stream, const ExpandArgs& a) {
  hipLaunchKernelGGL(expand_kernel(cw, vt, dense), dim3(grid), dim3(kExpandBlock), lds, stream, a);
  HIP_TRY(hipGetLastError());
  return SGPU_OK;
}

}  // namespace sgpu
