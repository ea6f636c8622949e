// column_filter.hip — column filters on the device (sgpu_filter_create_columns): the bitmap of a must / must-not / should
// query over range and set predicates on the document columns, written by one kernel; and the replicas' column state
// (ColumnState, columns.hpp): the stream and mutex of the column calls and the device copies of the columns.
//
// One streaming pass over the documents. A workgroup of kColBS threads takes kColDocsPerWg consecutive documents, 64 per
// wavefront and turn. The launcher hands over the plan of column_host.cpp: the clauses in ascending slot order, bounds and
// IN values as keys (one unsigned comparison per type), each IN clause's keys sorted. The clause loop is wave-uniform
// (the clause is read through a uniform address); a column's value is loaded where a slot's first clause stands - one
// coalesced dword load per document and distinct column - and its key kept for the slot's other clauses. The IN keys lie
// in LDS (at most 8192 of them, 32 KiB; clauses that share values repeat them in the plan, and a plan of more keys than
// that is searched in global memory instead); an IN clause is a binary search of at most 14 steps per document. The
// predicate of 64 documents is balloted into two output words, ANDed with `within`'s words when given; a lane past n_docs
// votes false, so no bit at or past n_docs is set. The count is a popcount: one LDS atomic per wavefront, one global
// atomic per workgroup, as term_filter.hip counts.
// Bounds: a document index is below n_docs wherever a column or an output word is addressed (base < nr, l < nr); the word
// index (d0 + base) / 32 is below n_words because d0 + base < n_docs, and word + 1 is checked; key indices stay inside
// [begin, begin + count), which column_check_args holds inside the call's values.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>
#include <new>
#include <vector>

#include "columns.hpp"

namespace sgpu {

namespace {

constexpr uint32_t kColBS = 256;   // threads of a workgroup: 4 wavefronts, 32 turns of 64 documents each

struct ColArgs {
  const ColClause* clauses;
  const uint32_t* keys;
  uint32_t n_clauses, n_keys, keys_in_lds;
  uint32_t n_must, min_should;
  uint64_t n_docs, n_words;
  const uint32_t* within;   // the words of `within` on this device, or null
  uint32_t* bits;           // out: n_words words
  unsigned long long* count;
};

__global__ __launch_bounds__(kColBS) void column_filter_kernel(ColArgs a) {
  __shared__ uint32_t s_keys[kColMaxSetValues];
  __shared__ uint32_t s_cnt;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  if (a.keys_in_lds)
    for (uint32_t i = tid; i < a.n_keys; i += kColBS) s_keys[i] = a.keys[i];
  if (tid == 0) s_cnt = 0;
  __syncthreads();
  const uint32_t* keys = a.keys_in_lds ? s_keys : a.keys;
  const uint64_t d0 = (uint64_t)blockIdx.x * kColDocsPerWg;
  const uint32_t nr = (uint32_t)min<uint64_t>(kColDocsPerWg, a.n_docs - d0);   // (d0 < n_docs: the grid is ceil(n_docs / W))
  uint32_t cnt = 0;
  for (uint32_t base = wave * 64u; base < nr; base += (kColBS / 64u) * 64u) {
    const uint32_t l = base + lane;
    const bool in = l < nr;
    uint32_t must = 0, should = 0, key = 0;
    bool banned = false;
    for (uint32_t j = 0; j < a.n_clauses; ++j) {
      const ColClause cl = a.clauses[j];
      if (cl.fresh) key = column_key(cl.type, in ? cl.col[d0 + l] : 0u);
      bool m;
      if (cl.op == SGPU_COLOP_RANGE) {
        m = cl.lo <= key && key <= cl.hi;
      } else {   // the first key >= key in [begin, begin + count)
        uint32_t lo = cl.begin, hi = cl.begin + cl.count;
        while (lo < hi) {
          const uint32_t mid = lo + ((hi - lo) >> 1);
          if (keys[mid] < key) lo = mid + 1u; else hi = mid;
        }
        m = lo < cl.begin + cl.count && keys[lo] == key;
      }
      if (m) {
        if (cl.occur == SGPU_TERM_MUST) ++must;
        else if (cl.occur == SGPU_TERM_SHOULD) ++should;
        else banned = true;
      }
    }
    const bool ok = in && !banned && must == a.n_must && should >= a.min_should;
    uint64_t m = __ballot(ok);
    const uint64_t w0 = (d0 + base) >> 5;   // (even: d0 and base are multiples of 64)
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

sgpu_status column_state_init(ColumnState* s, int device) {
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

uint64_t state_column_bytes(const ColumnState* s) {
  uint64_t b = 0;
  for (const DeviceBuffer& c : s->col) b += c.bytes;
  return b;
}

}  // namespace

void column_state_free(ColumnState* s) {
  if (!s) return;
  if (s->device >= 0) (void)hipSetDevice(s->device);
  if (s->stream) (void)hipStreamSynchronize(s->stream);
  for (DeviceBuffer& c : s->col) c.release();
  for (DeviceBuffer* b : {&s->f_clauses, &s->f_keys, &s->f_within, &s->f_bits, &s->f_count, &s->c_bits, &s->c_table, &s->c_rows,
                          &s->a_bits, &s->a_parts, &s->a_edges, &s->a_table, &s->t_state, &s->t_hist, &s->t_waves, &s->t_comps, &s->t_rows})
    b->release();
  if (s->ev0) (void)hipEventDestroy(s->ev0);
  if (s->ev1) (void)hipEventDestroy(s->ev1);
  if (s->ev2) (void)hipEventDestroy(s->ev2);
  if (s->stream) (void)hipStreamDestroy(s->stream);
  delete s;
}

sgpu_status column_state_of(sgpu_index* idx, uint32_t replica, ColumnState** out) {
  return replica_state(idx, idx->column_mu, idx->column_state, replica, column_state_init, column_state_free, out);
}

void column_states_locked(sgpu_index* idx, uint32_t slot, bool drop, void (*replace)(void*), void* arg) {
  std::vector<std::unique_lock<std::mutex>> locks;
  for (ColumnState* s : idx->column_state)
    if (s) locks.emplace_back(s->mu);
  replace(arg);
  if (drop)
    for (ColumnState* s : idx->column_state)
      if (s) {   // (no call runs: its mutex is held, and every call drains the stream before it lets go of it)
        (void)hipSetDevice(s->device);
        s->col[slot].release();
        s->col_gen[slot] = 0;
      }
}

uint64_t column_device_bytes(const sgpu_index* cidx) {
  if (!cidx) return 0;
  sgpu_index* idx = const_cast<sgpu_index*>(cidx);   // (the mutexes)
  std::lock_guard<std::mutex> lk(idx->column_mu);
  uint64_t b = 0;
  for (ColumnState* s : idx->column_state)
    if (s) {
      std::lock_guard<std::mutex> lk2(s->mu);
      b += state_column_bytes(s);
    }
  return b;
}

sgpu_status column_device_copy(ColumnState* s, const sgpu_index* idx, uint32_t slot, const uint32_t** out) {
  const HostColumn& hc = idx->columns[slot];
  if (hc.generation == 0) return fail(SGPU_EINVAL, "slot %u holds no column (it was dropped while the call ran)", slot);
  if (s->col_gen[slot] != hc.generation) {
    const uint64_t bytes = (uint64_t)hc.values.size() * 4;
    const sgpu_status st = s->col[slot].reserve(s->stream, bytes, "for a document column");
    if (st != SGPU_OK) return st;
    s->col_gen[slot] = 0;
    if (bytes) HIP_TRY(hipMemcpyAsync(s->col[slot].p, hc.values.data(), bytes, hipMemcpyHostToDevice, s->stream));
    s->col_gen[slot] = hc.generation;
  }
  *out = s->col[slot].as<const uint32_t>();
  return SGPU_OK;
}

sgpu_status column_filter_device(sgpu_index* idx, uint32_t replica, const sgpu_column_clause* clauses, uint32_t n_clauses,
                                 uint32_t min_should, const uint32_t* set_values, uint32_t n_set_values, const sgpu_filter* within,
                                 sgpu_filter** out) {
  const sgpu_status cst = column_check_args(idx, clauses, n_clauses, set_values, n_set_values, within, out);
  if (cst != SGPU_OK) return cst;
  ColumnState* s = nullptr;
  const sgpu_status sst = column_state_of(idx, replica, &s);
  if (sst != SGPU_OK) return sst;
  const uint64_t n_docs = idx->host.n_docs, n_words = std::max<uint64_t>((n_docs + 31) / 32, 1);
  try {
    std::vector<uint32_t> bits((size_t)n_words, 0u);
    unsigned long long count = 0;
    ColPlan plan;   // (outlives the drain of the stream, like bits and count: the copies read and write them)
    if (n_docs) {
      std::lock_guard<std::mutex> lk(s->mu);
      HIP_TRY(hipSetDevice(s->device));
      StreamDrain drain{s->stream};
      // the columns as they are now that no set_column can run: the checks that read them hold for THESE columns
      sgpu_status st = column_check_args(idx, clauses, n_clauses, set_values, n_set_values, within, out);
      if (st != SGPU_OK) return st;
      column_plan(idx, clauses, n_clauses, set_values, &plan);
      for (ColClause& c : plan.clauses)
        if ((st = column_device_copy(s, idx, c.slot, &c.col)) != SGPU_OK) return st;
      const char* what = "for a column filter";
      const uint64_t clause_bytes = plan.clauses.size() * sizeof(ColClause), key_bytes = plan.keys.size() * 4;
      if ((st = s->f_clauses.reserve(s->stream, clause_bytes, what)) != SGPU_OK || (st = s->f_keys.reserve(s->stream, key_bytes, what)) != SGPU_OK ||
          (st = s->f_bits.reserve(s->stream, n_words * 4, what)) != SGPU_OK || (st = s->f_count.reserve(s->stream, 8, what)) != SGPU_OK ||
          (within && (st = s->f_within.reserve(s->stream, n_words * 4, what)) != SGPU_OK))
        return st;
      if (clause_bytes) HIP_TRY(hipMemcpyAsync(s->f_clauses.p, plan.clauses.data(), clause_bytes, hipMemcpyHostToDevice, s->stream));
      if (key_bytes) HIP_TRY(hipMemcpyAsync(s->f_keys.p, plan.keys.data(), key_bytes, hipMemcpyHostToDevice, s->stream));
      if (within) HIP_TRY(hipMemcpyAsync(s->f_within.p, filter_host_bits(within), n_words * 4, hipMemcpyHostToDevice, s->stream));
      HIP_TRY(hipMemsetAsync(s->f_count.p, 0, 8, s->stream));
      ColArgs a{};
      a.clauses = s->f_clauses.as<const ColClause>();
      a.keys = s->f_keys.as<const uint32_t>();
      a.n_clauses = (uint32_t)plan.clauses.size();
      a.n_keys = (uint32_t)plan.keys.size();
      a.keys_in_lds = plan.keys.size() <= kColMaxSetValues;
      a.n_must = plan.n_must;
      a.min_should = min_should;
      a.n_docs = n_docs;
      a.n_words = n_words;
      a.within = within ? s->f_within.as<const uint32_t>() : nullptr;
      a.bits = s->f_bits.as<uint32_t>();
      a.count = s->f_count.as<unsigned long long>();
      const uint32_t grid = (uint32_t)((n_docs + kColDocsPerWg - 1) / kColDocsPerWg);
      (void)hipGetLastError();   // (judge this launch alone)
      HIP_TRY(hipEventRecord(s->ev0, s->stream));
      hipLaunchKernelGGL(column_filter_kernel, dim3(grid), dim3(kColBS), 0, s->stream, a);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipEventRecord(s->ev1, s->stream));
      HIP_TRY(hipMemcpyAsync(bits.data(), s->f_bits.p, n_words * 4, hipMemcpyDeviceToHost, s->stream));
      HIP_TRY(hipMemcpyAsync(&count, s->f_count.p, 8, hipMemcpyDeviceToHost, s->stream));
      HIP_TRY(hipStreamSynchronize(s->stream));
      HIP_TRY(hipEventElapsedTime(&s->filter_ms, s->ev0, s->ev1));
      s->filter_grid = grid;
    }
    return filter_from_bits(idx, std::move(bits), (uint64_t)count, out);
  } catch (const std::bad_alloc&) {
    return fail(SGPU_ENOMEM, "out of host memory");
  }
}

// (test hook) sgpu_debug_column_stats; false before the replica's first column call
bool column_debug_stats(sgpu_index* idx, uint32_t replica, double* out8) {
  std::lock_guard<std::mutex> lk(idx->column_mu);
  if (replica >= idx->column_state.size() || !idx->column_state[replica]) return false;
  ColumnState* s = idx->column_state[replica];
  std::lock_guard<std::mutex> lk2(s->mu);
  const double v[8] = {s->filter_ms, s->facet_ms, (double)s->filter_grid, (double)s->facet_grid, (double)kColDocsPerWg,
                       (double)s->facet_docs_per_wg, (double)s->facet_path, (double)state_column_bytes(s)};
  for (int i = 0; i < 8; ++i) out8[i] = v[i];
  return true;
}

// (test hook) sgpu_debug_facet_kernel_ms: {count kernel ms, select kernel ms} of the replica's last facet call
bool facet_debug_kernel_ms(sgpu_index* idx, uint32_t replica, double* out2) {
  std::lock_guard<std::mutex> lk(idx->column_mu);
  if (replica >= idx->column_state.size() || !idx->column_state[replica]) return false;
  ColumnState* s = idx->column_state[replica];
  std::lock_guard<std::mutex> lk2(s->mu);
  out2[0] = s->facet_count_ms;
  out2[1] = s->facet_select_ms;
  return true;
}

}  // namespace sgpu
