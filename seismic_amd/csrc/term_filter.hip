// term_filter.hip — term filters on the device (sgpu_filter_create_terms): the bitmap of a must / must-not / should
// query, written by one kernel from the replica's exact file (exact_file.hpp).
//
// The posting lists of the index are pruned (n_postings, doc_cut) and cannot say which documents store a component;
// the exact file is the complete inverted file of the forward index, keyed by (range of 32768 documents, component).
// A clause therefore costs 4 bytes per document of the range that stores its component, and nothing else of the index
// is read.
//
// One workgroup per range. The range's state lives in LDS, one u32 per document (128 KiB):
//   bits  0..15  MUST clauses that matched the document
//   bits 16..30  SHOULD clauses that matched it
//   bit  31      a MUST_NOT clause matched it
// The clauses are streamed in the caller's order; each clause's segment off[range][c] .. off[range][c + 1] is read with
// coalesced dword loads, kTermE per thread and step, the stored value decoded and compared, and the state updated with
// LDS atomics (a document appears at most once per segment, so with at most 1024 clauses neither field overflows; no
// barrier is needed between clauses, because the updates commute). After the last clause each wavefront ballots the
// predicate of 64 documents at a time into two of the range's 1024 output words, ANDs them with `within`'s words when
// given, and counts; one atomic per workgroup adds the range's count to the call's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>
#include <new>
#include <vector>

#include "device_prims.hpp"
#include "exact_file.hpp"
#include "hip_util.hpp"
#include "term_filter.hpp"

namespace sgpu {

namespace {

constexpr uint32_t kTermBS = 1024;   // threads of a workgroup
constexpr uint32_t kTermE = 4;       // entries per thread and step: a workgroup reads kTermBS * kTermE = 4096 entries per step
constexpr uint32_t kMustNotBit = 0x80000000u;

struct TermArgs {
  const uint32_t* ent;
  const uint32_t* off;
  const uint64_t* rbase;
  uint64_t dim1, n_docs, n_words;   // n_words: words of the whole bitmap
  uint32_t f16;
  float val_scale;
  const sgpu_term_clause* clauses;
  uint32_t n_clauses, n_must, min_should;
  const uint32_t* within;   // the words of `within` on this device, or null
  uint32_t* bits;           // out: n_words words
  unsigned long long* count;   // out: documents of the set
};

__global__ __launch_bounds__(kTermBS) void term_filter_kernel(TermArgs a) {
  __shared__ uint32_t st[kExactRange];
  __shared__ uint32_t s_cnt;
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t r = blockIdx.x;
  const uint32_t* off = a.off + (uint64_t)r * a.dim1;
  const uint32_t* ent = a.ent + a.rbase[r];
  {
    uint4* s4 = (uint4*)st;
    for (uint32_t i = tid; i < kExactRange / 4; i += kTermBS) s4[i] = make_uint4(0u, 0u, 0u, 0u);
  }
  if (tid == 0) s_cnt = 0;
  __syncthreads();
  for (uint32_t j = 0; j < a.n_clauses; ++j) {
    const sgpu_term_clause cl = a.clauses[j];
    const uint32_t b = off[cl.component], e = off[cl.component + 1];
    const uint32_t add = cl.occur == SGPU_TERM_MUST ? 1u : cl.occur == SGPU_TERM_SHOULD ? 0x10000u : 0u;
    for (uint32_t x0 = b; x0 < e; x0 += kTermBS * kTermE) {
      uint32_t v[kTermE];
#pragma unroll
      for (uint32_t i = 0; i < kTermE; ++i) {
        const uint32_t x = x0 + i * kTermBS + tid;
        v[i] = x < e ? ent[x] : 0xffffffffu;
      }
#pragma unroll
      for (uint32_t i = 0; i < kTermE; ++i) {
        const uint32_t x = x0 + i * kTermBS + tid;
        if (x < e) {
          const uint32_t l = v[i] & (kExactRange - 1);
          const float w = a.f16 ? half_bits_to_float(v[i] >> 16) : __fmul_rn((float)(v[i] >> 16), a.val_scale);
          if (w >= cl.min_weight) {
            if (add)
              atomicAdd(&st[l], add);
            else
              atomicOr(&st[l], kMustNotBit);
          }
        }
      }
    }
  }
  __syncthreads();
  // the range's documents, 64 per wavefront and turn: bit l of the range = word l / 32 of its 1024 words
  const uint64_t d0 = (uint64_t)r * kExactRange;
  const uint32_t nr = (uint32_t)min<uint64_t>(kExactRange, a.n_docs - d0);
  uint32_t cnt = 0;
  for (uint32_t base = wave * 64; base < nr; base += (kTermBS / 64) * 64) {
    const uint32_t l = base + lane;
    bool ok = false;
    if (l < nr) {
      const uint32_t s = st[l];
      ok = !(s & kMustNotBit) && (s & 0xffffu) == a.n_must && ((s >> 16) & 0x7fffu) >= a.min_should;
    }
    uint64_t m = __ballot(ok);
    const uint64_t w0 = (d0 + base) >> 5;   // (even: base is a multiple of 64)
    const bool two = w0 + 1 < a.n_words;
    if (a.within) m &= (uint64_t)a.within[w0] | (two ? (uint64_t)a.within[w0 + 1] << 32 : 0ull);
    if (lane == 0) a.bits[w0] = (uint32_t)m;
    if (lane == 1 && two) a.bits[w0 + 1] = (uint32_t)(m >> 32);
    cnt += (uint32_t)__popcll(m);
  }
  if (lane == 0 && cnt) atomicAdd(&s_cnt, cnt);
  __syncthreads();
  if (tid == 0 && s_cnt) atomicAdd(a.count, (unsigned long long)s_cnt);
}

}  // namespace

sgpu_status term_filter_device(sgpu_index* idx, uint32_t replica, const sgpu_term_clause* clauses, uint32_t n_clauses,
                               uint32_t min_should, const sgpu_filter* within, sgpu_filter** out) {
  const sgpu_status cst = term_check_args(idx, clauses, n_clauses, within, out);
  if (cst != SGPU_OK) return cst;
  ExactFile* f = nullptr;   // (the replica's exact file, built here if no exact call has)
  const sgpu_status fst = exact_file_get(idx, replica, &f);
  if (fst != SGPU_OK) return fst;
  const uint64_t n_docs = f->n_docs, n_words = std::max<uint64_t>((n_docs + 31) / 32, 1);
  std::vector<uint32_t> bits;
  try {
    bits.assign((size_t)n_words, 0u);
  } catch (const std::bad_alloc&) {
    return fail(SGPU_ENOMEM, "out of host memory");
  }
  uint32_t n_must = 0;
  for (uint32_t i = 0; i < n_clauses; ++i) n_must += clauses[i].occur == SGPU_TERM_MUST;
  unsigned long long count = 0;
  if (f->n_ranges) {
    std::lock_guard<std::mutex> lk(f->mu);
    HIP_TRY(hipSetDevice(f->device));
    if (!f->tf_e0) HIP_TRY(hipEventCreate(&f->tf_e0));
    if (!f->tf_e1) HIP_TRY(hipEventCreate(&f->tf_e1));
    sgpu_status st;
    const char* what = "for a term filter";
    if ((st = f->tf_clauses.reserve(f->stream, (uint64_t)n_clauses * sizeof(sgpu_term_clause), what)) != SGPU_OK ||
        (st = f->tf_bits.reserve(f->stream, n_words * 4, what)) != SGPU_OK || (st = f->tf_count.reserve(f->stream, 8, what)) != SGPU_OK ||
        (within && (st = f->tf_within.reserve(f->stream, n_words * 4, what)) != SGPU_OK))
      return st;
    if (n_clauses)
      HIP_TRY(hipMemcpyAsync(f->tf_clauses.p, clauses, (uint64_t)n_clauses * sizeof(sgpu_term_clause), hipMemcpyHostToDevice, f->stream));
    if (within) HIP_TRY(hipMemcpyAsync(f->tf_within.p, filter_host_bits(within), n_words * 4, hipMemcpyHostToDevice, f->stream));
    HIP_TRY(hipMemsetAsync(f->tf_count.p, 0, 8, f->stream));
    TermArgs a{};
    a.ent = f->ent.as<const uint32_t>();
    a.off = f->off.as<const uint32_t>();
    a.rbase = f->rbase.as<const uint64_t>();
    a.dim1 = f->dim + 1;
    a.n_docs = n_docs;
    a.n_words = n_words;
    a.f16 = f->f16;
    a.val_scale = f->val_scale;
    a.clauses = f->tf_clauses.as<const sgpu_term_clause>();
    a.n_clauses = n_clauses;
    a.n_must = n_must;
    a.min_should = min_should;
    a.within = within ? f->tf_within.as<const uint32_t>() : nullptr;
    a.bits = f->tf_bits.as<uint32_t>();
    a.count = f->tf_count.as<unsigned long long>();
    (void)hipGetLastError();   // (judge this launch alone)
    HIP_TRY(hipEventRecord(f->tf_e0, f->stream));
    hipLaunchKernelGGL(term_filter_kernel, dim3(f->n_ranges), dim3(kTermBS), 0, f->stream, a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(f->tf_e1, f->stream));
    HIP_TRY(hipMemcpyAsync(bits.data(), f->tf_bits.p, n_words * 4, hipMemcpyDeviceToHost, f->stream));
    HIP_TRY(hipMemcpyAsync(&count, f->tf_count.p, 8, hipMemcpyDeviceToHost, f->stream));
    HIP_TRY(hipStreamSynchronize(f->stream));
    HIP_TRY(hipEventElapsedTime(&f->tf_kernel_ms, f->tf_e0, f->tf_e1));
  }
  return filter_from_bits(idx, std::move(bits), (uint64_t)count, out);
}

// (test hook) out4 = {kernel ms of the last term-filter call on `replica`, wall ms of the exact file's build there, the
// file's bytes, its ranges = workgroups of the kernel}; false before the replica has an exact file
bool term_filter_debug_stats(sgpu_index* idx, uint32_t replica, double* out4) {
  ExactFile* f = nullptr;
  {
    std::lock_guard<std::mutex> lk(idx->exact_mu);
    if (replica >= idx->exact.size() || !idx->exact[replica]) return false;
    f = idx->exact[replica];
  }
  std::lock_guard<std::mutex> lk(f->mu);
  out4[0] = f->tf_kernel_ms;
  out4[1] = f->build_wall_ms;
  out4[2] = (double)f->bytes;
  out4[3] = (double)f->n_ranges;
  return true;
}

}  // namespace sgpu
