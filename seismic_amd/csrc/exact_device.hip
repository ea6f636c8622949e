// exact_device.hip — exact top-k over ALL documents on the device (sgpu_exact_search_device).
//
// Same contract as exact.cpp, bit for bit: a document's score starts at +0.0f and takes, for each component it
// shares with the query in ascending component order, score = score + (q * w) with the multiply and the add each
// rounded once; every document is a candidate (those sharing nothing score +0.0f); the k best by (score desc, id asc).
//
// The "exact file", built on a replica at its first exact call and kept until sgpu_index_destroy: the documents are
// cut into ranges of kRange = 32768 (u16 local ids); its entries are keyed by (range, component), one u32 each:
// local id in the low 16 bits, the document value in the index's own encoding in the high 16 (f16 bits or a u8
// code). Offsets: a dense table of n_ranges x (dim + 1) u32 offsets within a range, plus a u64 base per range (the
// first entry of the range's first document in the forward index: the file holds the forward index's entries in
// the same number, regrouped).
//
// A query is one (query, range) task per workgroup: the range's f32 accumulators live in LDS (128 KiB), the
// query's segments are streamed in ascending component order with a workgroup barrier between components (a
// document appears at most once per component, so no two lanes add into one accumulator between two barriers), and
// the next step's entries are loaded before the barrier. The task's top-k over all the range's accumulators is a
// radix select on the 48-bit key (ordered score bits, inverted local id): k candidates per task. A second kernel
// reduces a query's n_ranges x k candidates (64-bit keys: ordered score bits, inverted global id) to its k best.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <mutex>
#include <new>
#include <vector>

#include "device_prims.hpp"
#include "exact_file.hpp"
#include "filter.hpp"
#include "hip_util.hpp"

namespace sgpu {

namespace {

constexpr uint32_t kRangeBits = kExactRangeBits, kRange = kExactRange;   // documents per range (exact_file.hpp)
constexpr uint32_t kBS = 1024;        // threads of the accumulate kernel
constexpr uint32_t kE = 8;            // entries per thread and step
constexpr uint32_t kGroup = 256;      // query components resolved to segments at a time (LDS)
constexpr uint32_t kMergeBS = 256;    // threads of the merge kernel
constexpr uint32_t kMaxK = 1024;
constexpr uint64_t kCandBytes = 256ull << 20;   // candidate buffer per chunk of queries (test hook SGPU_EXACT_CAND_BYTES lowers it)
constexpr uint64_t kMaxTable = 1ull << 28;      // dense offset table entries (1 GiB)

// ---- build -----------------------------------------------------------------------------------------------------
// one wave per document; every (range, component) pair of the forward index counted
__global__ __launch_bounds__(256) void exact_count_kernel(const uint64_t* __restrict__ fo, const uint8_t* __restrict__ fc,
                                                          uint32_t cw, uint64_t n_docs, uint64_t dim1, uint32_t* cnt) {
  const uint64_t nw = ((uint64_t)gridDim.x * blockDim.x) >> 6;
  const uint32_t lane = threadIdx.x & 63;
  for (uint64_t d = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; d < n_docs; d += nw) {
    uint32_t* row = cnt + (d >> kRangeBits) * dim1;
    for (uint64_t i = fo[d] + lane; i < fo[d + 1]; i += 64) {
      const uint32_t c = cw == 2 ? (uint32_t)((const uint16_t*)fc)[i] : ((const uint32_t*)fc)[i];
      atomicAdd(row + c, 1u);
    }
  }
}

// one workgroup per range: exclusive scan of the row's dim + 1 counts (the last is 0: it becomes the range's total),
// written to off and, as the scatter's cursor, over cnt
__global__ __launch_bounds__(1024) void exact_scan_kernel(uint32_t* cnt, uint32_t* off, uint64_t dim1) {
  __shared__ uint32_t wsum[16];
  __shared__ uint32_t carry_s;
  uint32_t* c = cnt + (uint64_t)blockIdx.x * dim1;
  uint32_t* o = off + (uint64_t)blockIdx.x * dim1;
  const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  if (tid == 0) carry_s = 0;
  __syncthreads();
  for (uint64_t base = 0; base < dim1; base += 4 * 1024) {
    uint32_t v[4], s = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const uint64_t j = base + 4 * tid + i;
      v[i] = j < dim1 ? c[j] : 0u;
      s += v[i];
    }
    const uint32_t incl = wave_incl_scan(s);
    if (lane == 63) wsum[w] = incl;
    __syncthreads();
    uint32_t before = carry_s;
    for (uint32_t x = 0; x < w; ++x) before += wsum[x];
    before += incl - s;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const uint64_t j = base + 4 * tid + i;
      if (j < dim1) {
        o[j] = before;
        c[j] = before;
      }
      before += v[i];
    }
    __syncthreads();
    if (tid == 1023) carry_s = before;
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void exact_scatter_kernel(const uint64_t* __restrict__ fo, const uint8_t* __restrict__ fc,
                                                            const uint8_t* __restrict__ fv, uint32_t cw, uint32_t f16,
                                                            uint64_t n_docs, uint64_t dim1, const uint64_t* __restrict__ rbase,
                                                            uint32_t* cur, uint32_t* ent) {
  const uint64_t nw = ((uint64_t)gridDim.x * blockDim.x) >> 6;
  const uint32_t lane = threadIdx.x & 63;
  for (uint64_t d = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; d < n_docs; d += nw) {
    const uint64_t r = d >> kRangeBits;
    uint32_t* row = cur + r * dim1;
    uint32_t* dst = ent + rbase[r];
    const uint32_t local = (uint32_t)(d & (kRange - 1));
    for (uint64_t i = fo[d] + lane; i < fo[d + 1]; i += 64) {
      const uint32_t c = cw == 2 ? (uint32_t)((const uint16_t*)fc)[i] : ((const uint32_t*)fc)[i];
      const uint32_t v = f16 ? (uint32_t)((const uint16_t*)fv)[i] : (uint32_t)fv[i];
      const uint32_t p = atomicAdd(row + c, 1u);
      dst[p] = local | (v << 16);
    }
  }
}

// ---- search ----------------------------------------------------------------------------------------------------
struct AccArgs {
  const uint32_t* ent;
  const uint32_t* off;
  const uint64_t* rbase;
  uint64_t dim1, n_docs;
  uint32_t n_ranges, f16;
  float val_scale;
  const uint64_t* q_off;   // the whole call's offsets; this chunk's queries are q0 ..
  const uint32_t* comps;
  const float* vals;
  uint32_t q0, nq, k;
  uint64_t* cand;          // [query of the chunk][range][k]
  const uint32_t* bits;    // a filter's allowed set (bit d of word d / 32), or null: every document is a candidate
};

// One (query, range) task per workgroup and turn of the grid loop.
__global__ __launch_bounds__(kBS) void exact_accumulate_kernel(AccArgs a) {
  __shared__ __attribute__((aligned(16))) float acc[kRange];
  __shared__ uint32_t s_b[kGroup], s_e[kGroup];
  __shared__ float s_qv[kGroup];
  __shared__ uint32_t hist[256];
  __shared__ uint32_t s_sel[4];
  __shared__ uint32_t s_bm[kRange / 32];   // (filtered calls) the range's allowed documents
  __shared__ uint32_t s_nok;
  const uint32_t tid = threadIdx.x, lane = tid & 63;
  const uint64_t n_tasks = (uint64_t)a.nq * a.n_ranges;
  for (uint64_t task = blockIdx.x; task < n_tasks; task += gridDim.x) {
    const uint32_t ql = (uint32_t)(task / a.n_ranges), r = (uint32_t)(task % a.n_ranges);
    const uint32_t* off = a.off + (uint64_t)r * a.dim1;
    const uint32_t* ent = a.ent + a.rbase[r];
    const uint64_t qb = a.q_off[a.q0 + ql], qe = a.q_off[a.q0 + ql + 1];
    __syncthreads();   // (the previous task's select is done with acc, hist and s_sel)
    {
      float4* a4 = (float4*)acc;
      for (uint32_t i = tid; i < kRange / 4; i += kBS) a4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    for (uint64_t g0 = qb; g0 < qe; g0 += kGroup) {
      const uint32_t gn = (uint32_t)min<uint64_t>(kGroup, qe - g0);
      __syncthreads();   // (zeroing done / the previous group's segments consumed)
      if (tid < gn) {
        const uint32_t c = a.comps[g0 + tid];
        s_b[tid] = off[c];
        s_e[tid] = off[c + 1];
        s_qv[tid] = a.vals[g0 + tid];
      }
      __syncthreads();
      uint32_t j = 0;
      while (j < gn && s_b[j] == s_e[j]) ++j;
      uint32_t pos = 0;
      uint32_t cur[kE];
      if (j < gn) {
        const uint32_t b = s_b[j], e = s_e[j];
#pragma unroll
        for (uint32_t i = 0; i < kE; ++i) {
          const uint32_t x = b + i * kBS + tid;
          cur[i] = x < e ? ent[x] : 0xffffffffu;
        }
      }
      while (j < gn) {
        const float qv = s_qv[j];
        uint32_t nj = j, npos = pos + kE * kBS;
        if (s_b[j] + npos >= s_e[j]) {
          nj = j + 1;
          while (nj < gn && s_b[nj] == s_e[nj]) ++nj;
          npos = 0;
        }
        uint32_t nxt[kE];
        if (nj < gn) {   // the next step's entries are in flight while this step adds and waits at the barrier
          const uint32_t b = s_b[nj] + npos, e = s_e[nj];
#pragma unroll
          for (uint32_t i = 0; i < kE; ++i) {
            const uint32_t x = b + i * kBS + tid;
            nxt[i] = x < e ? ent[x] : 0xffffffffu;
          }
        } else {
#pragma unroll
          for (uint32_t i = 0; i < kE; ++i) nxt[i] = 0xffffffffu;
        }
#pragma unroll
        for (uint32_t i = 0; i < kE; ++i) {
          const uint32_t x = cur[i];
          if (x != 0xffffffffu) {
            const uint32_t l = x & 0xffffu;
            const float w = a.f16 ? half_bits_to_float(x >> 16) : __fmul_rn((float)(x >> 16), a.val_scale);
            acc[l] = __fadd_rn(acc[l], __fmul_rn(qv, w));
          }
        }
        if (nj != j) __syncthreads();   // every addition of component j before any of the next
#pragma unroll
        for (uint32_t i = 0; i < kE; ++i) cur[i] = nxt[i];
        j = nj;
        pos = npos;
      }
    }
    __syncthreads();

    // ---- the task's top-k over all its documents: key = ordered_u32(score) << 16 | (0xffff - local), larger is better
    const uint64_t d0 = (uint64_t)r * kRange;
    const uint32_t nr = (uint32_t)min<uint64_t>(kRange, a.n_docs - d0);
    uint64_t* out = a.cand + task * a.k;
    // the task's candidates: its documents l < nr, and of those only the allowed ones when a filter is given (the words
    // past the range's last document are zero). A range may then yield fewer than min(k, nr): the rest of its slots
    // are 0, below every real key, and the merge takes min(k, |A|) per query.
    uint32_t n_ok = nr;
    if (a.bits) {
      if (tid == 0) s_nok = 0;
      __syncthreads();
      const uint32_t n_words = (nr + 31) / 32;
      uint32_t c = 0;
      for (uint32_t i = tid; i < kRange / 32; i += kBS) {
        const uint32_t w = i < n_words ? a.bits[(d0 >> 5) + i] : 0u;
        s_bm[i] = w;
        c += __popc(w);
      }
      if (c) atomicAdd(&s_nok, c);
      __syncthreads();
      n_ok = s_nok;
    }
    auto candidate = [&](uint32_t l) { return a.bits ? ((s_bm[l >> 5] >> (l & 31u)) & 1u) != 0 : l < nr; };
    if (n_ok <= a.k) {
      if (!a.bits) {
        for (uint32_t l = tid; l < a.k; l += kBS)
          out[l] = l < nr ? ((uint64_t)ordered_u32(acc[l]) << 32) | (uint64_t)(0xffffffffu - (uint32_t)(d0 + l)) : 0ull;
        continue;
      }
      if (tid == 0) s_sel[3] = 0;
      __syncthreads();
      for (uint32_t l = tid; l < nr; l += kBS)
        if (candidate(l)) out[atomicAdd(&s_sel[3], 1u)] = ((uint64_t)ordered_u32(acc[l]) << 32) | (uint64_t)(0xffffffffu - (uint32_t)(d0 + l));
      for (uint32_t l = n_ok + tid; l < a.k; l += kBS) out[l] = 0ull;
      continue;
    }
    uint64_t prefix = 0, mask = 0;
    uint32_t need = a.k;
    for (int shift = 40; shift >= 0; shift -= 8) {
      if (tid < 256) hist[tid] = 0;
      __syncthreads();
      uint32_t run_bin = 0xffffffffu, run_n = 0;
      for (uint32_t it = 0; it < kRange / (4 * kBS); ++it) {
        const uint32_t l0 = it * 4 * kBS + 4 * tid;
        const float4 v = ((const float4*)acc)[l0 / 4];
        const float vs[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (uint32_t e = 0; e < 4; ++e) {
          const uint32_t l = l0 + e;
          const uint64_t key = ((uint64_t)ordered_u32(vs[e]) << 16) | (uint64_t)(0xffffu - l);
          if (candidate(l) && (key & mask) == prefix) {
            const uint32_t bin = (uint32_t)(key >> shift) & 255u;
            if (bin == run_bin) {
              ++run_n;
            } else {
              if (run_n) atomicAdd(&hist[run_bin], run_n);
              run_bin = bin;
              run_n = 1;
            }
          }
        }
      }
      if (run_n) atomicAdd(&hist[run_bin], run_n);
      __syncthreads();
      if (tid < 64) radix_select_pick(hist, need, lane, s_sel);   // the bin where the running count from the top reaches `need`
      __syncthreads();
      const uint32_t b = s_sel[0], hb = s_sel[2];
      need = s_sel[1];
      prefix |= (uint64_t)b << shift;
      mask |= (uint64_t)255 << shift;
      if (hb == need) break;   // the whole bin is taken
    }
    // selected: everything above the bin, and the bin (all of it, or its one document once the key is resolved)
    for (uint32_t it = 0; it < kRange / (4 * kBS); ++it) {
      const uint32_t l0 = it * 4 * kBS + 4 * tid;
      const float4 v = ((const float4*)acc)[l0 / 4];
      const float vs[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (uint32_t e = 0; e < 4; ++e) {
        const uint32_t l = l0 + e;
        const uint32_t fk = ordered_u32(vs[e]);
        const uint64_t key = ((uint64_t)fk << 16) | (uint64_t)(0xffffu - l);
        if (candidate(l) && (key & mask) >= prefix) {
          const uint32_t slot = atomicAdd(&s_sel[3], 1u);
          if (slot < a.k) out[slot] = ((uint64_t)fk << 32) | (uint64_t)(0xffffffffu - (uint32_t)(d0 + l));
        }
      }
    }
  }
}

// One workgroup per query: the k best of its n_ranges x k candidates (keys unique but for the 0 padding), sorted.
__global__ __launch_bounds__(kMergeBS) void exact_merge_kernel(const uint64_t* __restrict__ cand, uint32_t n_ranges,
                                                               uint32_t k, uint32_t out_n, uint32_t q0, float* out_scores,
                                                               uint64_t* out_ids, uint32_t* out_nq) {
  __shared__ uint32_t hist[256];
  __shared__ uint32_t s_sel[4];
  __shared__ uint64_t sel[kMaxK];
  const uint32_t tid = threadIdx.x, lane = tid & 63;
  const uint64_t n = (uint64_t)n_ranges * k;
  const uint64_t* c = cand + (uint64_t)blockIdx.x * n;
  uint64_t prefix = 0, mask = 0;
  uint32_t need = out_n;
  for (int shift = 56; shift >= 0 && need; shift -= 8) {
    hist[tid] = 0;
    __syncthreads();
    for (uint64_t i = tid; i < n; i += kMergeBS) {
      const uint64_t key = c[i];
      if ((key & mask) == prefix) atomicAdd(&hist[(uint32_t)(key >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (tid < 64) radix_select_pick(hist, need, lane, s_sel);
    __syncthreads();
    const uint32_t b = s_sel[0], hb = s_sel[2];
    need = s_sel[1];
    prefix |= (uint64_t)b << shift;
    mask |= (uint64_t)255 << shift;
    __syncthreads();   // (s_sel read by every thread before the next pass writes it)
    if (hb == need) break;
  }
  uint32_t p2 = 1;
  while (p2 < out_n) p2 <<= 1;
  for (uint32_t i = tid; i < p2; i += kMergeBS) sel[i] = 0;
  if (tid == 0) s_sel[3] = 0;
  __syncthreads();
  if (out_n)
    for (uint64_t i = tid; i < n; i += kMergeBS) {
      const uint64_t key = c[i];
      if ((key & mask) >= prefix) {
        const uint32_t slot = atomicAdd(&s_sel[3], 1u);
        if (slot < out_n) sel[slot] = key;
      }
    }
  __syncthreads();
  bitonic_sort_lds<true>(sel, p2, tid, kMergeBS);
  const uint64_t row = (uint64_t)(q0 + blockIdx.x) * k;
  for (uint32_t i = tid; i < k; i += kMergeBS) {
    const uint64_t key = i < out_n ? sel[i] : 0ull;
    out_scores[row + i] = i < out_n ? ordered_u32_inv((uint32_t)(key >> 32)) : 0.0f;
    out_ids[row + i] = i < out_n ? (uint64_t)(0xffffffffu - (uint32_t)key) : 0ull;
  }
  if (tid == 0) out_nq[q0 + blockIdx.x] = out_n;
}

}  // namespace

void exact_file_free(ExactFile* f) {
  if (!f) return;
  (void)hipSetDevice(f->device);
  if (f->stream) (void)hipStreamSynchronize(f->stream);
  for (DeviceBuffer* b : {&f->ent, &f->off, &f->rbase, &f->q_off, &f->q_comp, &f->q_val, &f->cand, &f->out_scores, &f->out_ids, &f->out_n,
                          &f->tf_clauses, &f->tf_within, &f->tf_bits, &f->tf_count})
    b->release();
  if (f->tf_e0) (void)hipEventDestroy(f->tf_e0);
  if (f->tf_e1) (void)hipEventDestroy(f->tf_e1);
  if (f->stream) (void)hipStreamDestroy(f->stream);
  delete f;
}

static sgpu_status ex_reserve(ExactFile* f, DeviceBuffer& b, uint64_t bytes) { return b.reserve(f->stream, bytes, "for exact search"); }

// Builds the file of `h` on `device` (histogram, scan, scatter on the device, from the uploaded forward arrays).
static sgpu_status exact_file_build_on(const HostIndex& h, int device, ExactFile* f) {
  const uint64_t nnz = h.nnz(), n_ranges = (h.n_docs + kRange - 1) / kRange, dim1 = h.dim + 1;
  if (n_ranges * dim1 > kMaxTable)
    return fail(SGPU_ELIMIT, "exact search on the device: %llu ranges x %llu components exceed the offset table",
                (unsigned long long)n_ranges, (unsigned long long)dim1);
  std::vector<uint64_t> rbase(n_ranges + 1);
  for (uint64_t r = 0; r <= n_ranges; ++r) rbase[r] = h.fwd_offsets[std::min<uint64_t>(r * kRange, h.n_docs)];
  for (uint64_t r = 0; r < n_ranges; ++r)
    if (rbase[r + 1] - rbase[r] > 0xffffffffull)
      return fail(SGPU_ELIMIT, "exact search on the device: more than 2^32 entries in a range of documents");
  f->device = device;
  f->n_docs = h.n_docs;
  f->dim = h.dim;
  f->n_ranges = (uint32_t)n_ranges;
  f->f16 = h.value_type == SGPU_VAL_F16;
  f->val_scale = h.val_scale;
  HIP_TRY(hipSetDevice(device));
  int n_cu = 0;
  HIP_TRY(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, device));
  f->n_cu = (uint32_t)std::max(n_cu, 1);
  HIP_TRY(hipStreamCreateWithFlags(&f->stream, hipStreamNonBlocking));
  sgpu_status st;
  const uint64_t table = n_ranges * dim1;
  if ((st = ex_reserve(f, f->ent, nnz * 4)) != SGPU_OK || (st = ex_reserve(f, f->off, table * 4)) != SGPU_OK ||
      (st = ex_reserve(f, f->rbase, (n_ranges + 1) * 8)) != SGPU_OK)
    return st;
  f->bytes = nnz * 4 + table * 4 + (n_ranges + 1) * 8;
  // the forward arrays, and the counts (then the scatter's cursor): freed once the file is built
  DeviceBuffer fwd_off, fwd_comp, fwd_val, cnt;
  auto release = [&]() {
    (void)hipStreamSynchronize(f->stream);
    for (DeviceBuffer* b : {&fwd_off, &fwd_comp, &fwd_val, &cnt}) b->release();
  };
  const uint32_t vb = h.val_bytes();
  if ((st = ex_reserve(f, fwd_off, (h.n_docs + 1) * 8)) != SGPU_OK || (st = ex_reserve(f, fwd_comp, nnz * h.comp_width)) != SGPU_OK ||
      (st = ex_reserve(f, fwd_val, nnz * vb)) != SGPU_OK || (st = ex_reserve(f, cnt, table * 4)) != SGPU_OK) {
    release();
    return st;
  }
  const void* vals = h.value_type == SGPU_VAL_F16 ? (const void*)h.fwd_vals.data() : (const void*)h.fwd_codes.data();
  hipError_t e = hipMemcpyAsync(fwd_off.p, h.fwd_offsets.data(), (h.n_docs + 1) * 8, hipMemcpyHostToDevice, f->stream);
  if (e == hipSuccess && nnz) e = hipMemcpyAsync(fwd_comp.p, h.fwd_comps.data(), nnz * h.comp_width, hipMemcpyHostToDevice, f->stream);
  if (e == hipSuccess && nnz) e = hipMemcpyAsync(fwd_val.p, vals, nnz * vb, hipMemcpyHostToDevice, f->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(f->rbase.p, rbase.data(), (n_ranges + 1) * 8, hipMemcpyHostToDevice, f->stream);
  if (e == hipSuccess) e = hipMemsetAsync(cnt.p, 0, table * 4, f->stream);
  const uint32_t grid = std::max<uint32_t>(1, (uint32_t)std::min<uint64_t>((h.n_docs + 3) / 4, 64ull * f->n_cu));
  if (e == hipSuccess && h.n_docs) {
    hipLaunchKernelGGL(exact_count_kernel, dim3(grid), dim3(256), 0, f->stream, fwd_off.as<const uint64_t>(),
                       fwd_comp.as<const uint8_t>(), h.comp_width, h.n_docs, dim1, cnt.as<uint32_t>());
    e = hipGetLastError();
    if (e == hipSuccess) {
      hipLaunchKernelGGL(exact_scan_kernel, dim3((uint32_t)n_ranges), dim3(1024), 0, f->stream, cnt.as<uint32_t>(),
                         f->off.as<uint32_t>(), dim1);
      e = hipGetLastError();
    }
    if (e == hipSuccess) {
      hipLaunchKernelGGL(exact_scatter_kernel, dim3(grid), dim3(256), 0, f->stream, fwd_off.as<const uint64_t>(),
                         fwd_comp.as<const uint8_t>(), fwd_val.as<const uint8_t>(), h.comp_width, f->f16, h.n_docs, dim1,
                         f->rbase.as<const uint64_t>(), cnt.as<uint32_t>(), f->ent.as<uint32_t>());
      e = hipGetLastError();
    }
  }
  if (e == hipSuccess) e = hipStreamSynchronize(f->stream);
  release();
  if (e != hipSuccess) return fail(SGPU_EDEVICE, "building the exact file failed: %s", hipGetErrorString(e));
  return SGPU_OK;
}

// (bits: a filter's allowed set on this device and its size n_allowed, or null)
static sgpu_status exact_run(ExactFile* f, const uint64_t* q_off, const uint32_t* comps, const float* vals, uint32_t nq,
                             uint32_t k, float* out_scores, uint64_t* out_ids, uint32_t* out_n, const uint32_t* bits,
                             uint64_t n_allowed) {
  HIP_TRY(hipSetDevice(f->device));
  f->last_launches = 0;
  const uint32_t out_nn = (uint32_t)std::min<uint64_t>(k, bits ? n_allowed : f->n_docs);
  if (f->n_ranges == 0) {   // (no documents: nothing to return)
    for (uint32_t q = 0; q < nq; ++q) out_n[q] = 0;
    return SGPU_OK;
  }
  const uint64_t qnnz = q_off[nq];
  const uint64_t per_q = (uint64_t)f->n_ranges * k * 8;
  // (test hook SGPU_EXACT_CAND_BYTES, read per call: a smaller candidate buffer, so that a few queries are several chunks)
  uint64_t cand_bytes = kCandBytes;
  if (test_hooks_on())
    if (const char* v = std::getenv("SGPU_EXACT_CAND_BYTES"))
      if (*v) cand_bytes = std::min<uint64_t>(std::max<uint64_t>(1, std::strtoull(v, nullptr, 10)), kCandBytes);
  const uint32_t chunk = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(nq, cand_bytes / per_q));
  sgpu_status st;
  if ((st = ex_reserve(f, f->q_off, (uint64_t)(nq + 1) * 8)) != SGPU_OK || (st = ex_reserve(f, f->q_comp, qnnz * 4)) != SGPU_OK ||
      (st = ex_reserve(f, f->q_val, qnnz * 4)) != SGPU_OK || (st = ex_reserve(f, f->cand, (uint64_t)chunk * per_q)) != SGPU_OK ||
      (st = ex_reserve(f, f->out_scores, (uint64_t)nq * k * 4)) != SGPU_OK ||
      (st = ex_reserve(f, f->out_ids, (uint64_t)nq * k * 8)) != SGPU_OK || (st = ex_reserve(f, f->out_n, (uint64_t)nq * 4)) != SGPU_OK)
    return st;
  HIP_TRY(hipMemcpyAsync(f->q_off.p, q_off, (uint64_t)(nq + 1) * 8, hipMemcpyHostToDevice, f->stream));
  if (qnnz) {
    HIP_TRY(hipMemcpyAsync(f->q_comp.p, comps, qnnz * 4, hipMemcpyHostToDevice, f->stream));
    HIP_TRY(hipMemcpyAsync(f->q_val.p, vals, qnnz * 4, hipMemcpyHostToDevice, f->stream));
  }
  AccArgs a{};
  a.ent = f->ent.as<const uint32_t>();
  a.off = f->off.as<const uint32_t>();
  a.rbase = f->rbase.as<const uint64_t>();
  a.dim1 = f->dim + 1;
  a.n_docs = f->n_docs;
  a.n_ranges = f->n_ranges;
  a.f16 = f->f16;
  a.val_scale = f->val_scale;
  a.q_off = f->q_off.as<const uint64_t>();
  a.comps = f->q_comp.as<const uint32_t>();
  a.vals = f->q_val.as<const float>();
  a.k = k;
  a.cand = f->cand.as<uint64_t>();
  a.bits = bits;
  for (uint32_t q0 = 0; q0 < nq; q0 += chunk) {
    const uint32_t n = std::min(chunk, nq - q0);
    a.q0 = q0;
    a.nq = n;
    const uint64_t tasks = (uint64_t)n * f->n_ranges;
    const uint32_t grid = (uint32_t)std::min<uint64_t>(tasks, f->n_cu);
    hipLaunchKernelGGL(exact_accumulate_kernel, dim3(grid), dim3(kBS), 0, f->stream, a);
    HIP_TRY(hipGetLastError());
    ++f->last_launches;
    hipLaunchKernelGGL(exact_merge_kernel, dim3(n), dim3(kMergeBS), 0, f->stream, (const uint64_t*)a.cand, f->n_ranges,
                       k, out_nn, q0, f->out_scores.as<float>(), f->out_ids.as<uint64_t>(), f->out_n.as<uint32_t>());
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipMemcpyAsync(out_scores, f->out_scores.p, (uint64_t)nq * k * 4, hipMemcpyDeviceToHost, f->stream));
  HIP_TRY(hipMemcpyAsync(out_ids, f->out_ids.p, (uint64_t)nq * k * 8, hipMemcpyDeviceToHost, f->stream));
  HIP_TRY(hipMemcpyAsync(out_n, f->out_n.p, (uint64_t)nq * 4, hipMemcpyDeviceToHost, f->stream));
  HIP_TRY(hipStreamSynchronize(f->stream));
  return SGPU_OK;
}

sgpu_status exact_file_get(sgpu_index* idx, uint32_t replica, ExactFile** out, bool* built) {
  bool fresh = false;
  const sgpu_status st = replica_state(
      idx, idx->exact_mu, idx->exact, replica,
      [&](ExactFile* nf, int device) {
        fresh = true;
        const auto t0 = std::chrono::steady_clock::now();
        const sgpu_status bst = exact_file_build_on(idx->host, device, nf);
        nf->build_wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        return bst;
      },
      exact_file_free, out);
  if (built) *built = fresh && st == SGPU_OK;
  return st;
}

sgpu_status exact_search_device(sgpu_index* idx, uint32_t replica, const uint64_t* q_off, const uint32_t* comps,
                                const float* vals, uint32_t nq, uint32_t k, float* out_scores, uint64_t* out_ids,
                                uint32_t* out_n, const sgpu_filter* filter) {
  if (!idx || !q_off || !out_scores || !out_ids || !out_n) return fail(SGPU_EINVAL, "null argument");
  {
    uint32_t max_nnz = 0;
    const sgpu_status vst = validate_queries(idx->host.dim, q_off, comps, vals, nq, &max_nnz);
    if (vst != SGPU_OK) return vst;
  }
  if (k == 0) return fail(SGPU_EINVAL, "k == 0");
  if (k > kMaxK) return fail(SGPU_ELIMIT, "k = %u exceeds the limit of %u", k, kMaxK);
  ExactFile* f = nullptr;   // (the replica's exact file, built on its first exact or term-filter call)
  const sgpu_status fst = exact_file_get(idx, replica, &f);
  if (fst != SGPU_OK) return fst;
  const FilterDeviceView* fv = nullptr;
  if (filter) {   // (the filter's view on this replica holds its bitmap there)
    const sgpu_status st = filter_view(filter, replica, &fv);
    if (st != SGPU_OK) return st;
  }
  if (nq == 0) return SGPU_OK;
  std::lock_guard<std::mutex> lk(f->mu);
  return exact_run(f, q_off, comps, vals, nq, k, out_scores, out_ids, out_n, fv ? fv->bits : nullptr, fv ? fv->count : 0);
}

// (test hook: the accumulate launches - chunks of queries - of the last exact call on `replica`; false before its first)
bool exact_debug_launches(sgpu_index* idx, uint32_t replica, uint32_t* out) {
  ExactFile* f = nullptr;
  {
    std::lock_guard<std::mutex> lk(idx->exact_mu);
    if (replica >= idx->exact.size() || !idx->exact[replica]) return false;
    f = idx->exact[replica];
  }
  std::lock_guard<std::mutex> lk(f->mu);
  *out = f->last_launches;
  return true;
}

}  // namespace sgpu
