// facet_counts.hip — facet counts on the device (sgpu_facet_counts): how many documents of a filter hold each value of a
// U32 column, and the t most frequent values.
//
// Two kernels on the column calls' stream (ColumnState, columns.hpp), over a table of bins = max + 1 u32 counters in
// global memory (at most 1 << 22 bins = 16 MiB, recycled, zeroed per call):
//   count   a workgroup takes a slice of consecutive documents, 64 per wavefront and turn: the filter's bit (the host words,
//           uploaded for the call), the column's value with one coalesced dword load. Two forms of one kernel:
//           LDS     bins <= kFacetLdsBins: the workgroup counts in an LDS histogram (LDS atomics) and adds its non-zero
//                   bins to the table at the end, one global atomic per non-zero bin;
//           global  otherwise: global atomics into the table; the lanes of a wavefront that hold the value of its first
//                   counted lane add once (one ballot: the cheap case of a skewed column), the others add on their own.
//   select  ONE workgroup over the table. key = the count (0: the value does not occur). A histogram over the keys' top
//           byte also counts the distinct values; where there are more than t, a radix select of four 8-bit steps
//           (device_prims.hpp's pick, as expand_queries.hip selects) leaves the t-th largest count `thr` and how many of the
//           values with that count are still needed. The values above thr go to an LDS array of t <= 1024 pairs through a
//           cursor; of the values equal to thr the first `need` in ascending value order are taken - each wavefront owns
//           a contiguous segment of the table, counts its equals (ballots), the totals of the 16 wavefronts go through
//           LDS, and a second pass places them. The pairs, as (count << 32 | ~value), are sorted descending (bitonic, in
//           LDS): count descending, value ascending. The pairs are distinct, so the order of the atomics decides nothing.
// Counts are integers: the result equals the host twin's (column_host.cpp) exactly.
// Bounds: a document index is below n_docs wherever the column or the filter's words are addressed; a table index is a
// column value checked against bins (the recorded maximum makes that always true) or a loop index below bins; an index
// into the pair array is checked against its 1024 entries; every loop is bounded by the slice, the bins or four radix
// steps, and every barrier sits under workgroup-uniform conditions.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>
#include <new>
#include <vector>

#include "columns.hpp"
#include "device_prims.hpp"
#include "filter.hpp"

namespace sgpu {

namespace {

constexpr uint32_t kFacetBS = 1024;   // threads of a workgroup (16 wavefronts: the select kernel's wave totals are sized by it)
constexpr uint32_t kFacetWaves = kFacetBS / 64u;

struct FacetCountArgs {
  const uint32_t* col;
  const uint32_t* fbits;   // the filter's words on this device, or null: all documents
  uint32_t* table;         // bins counters
  uint64_t n_docs;
  uint32_t bins;
  uint32_t docs_per_wg;    // a multiple of 64
};

template <bool LDS>
__global__ __launch_bounds__(kFacetBS) void facet_count_kernel(FacetCountArgs a) {
  __shared__ uint32_t s_hist[LDS ? kFacetLdsBins : 1];
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  if (LDS) {
    for (uint32_t i = tid; i < a.bins; i += kFacetBS) s_hist[i] = 0;
    __syncthreads();
  }
  const uint64_t d0 = (uint64_t)blockIdx.x * a.docs_per_wg, d1 = min<uint64_t>(d0 + a.docs_per_wg, a.n_docs);
  for (uint64_t b = d0 + (tid - lane); b < d1; b += kFacetBS) {   // (wave-uniform: 64 documents per wavefront and turn)
    const uint64_t d = b + lane;
    bool on = d < d1;
    if (on && a.fbits) on = (a.fbits[d >> 5] >> (d & 31u)) & 1u;
    const uint32_t v = on ? a.col[d] : 0u;
    on = on && v < a.bins;
    if (LDS) {
      if (on) atomicAdd(&s_hist[v], 1u);
    } else {
      const uint64_t act = __ballot(on);
      if (act) {
        const uint32_t first = (uint32_t)__ffsll((long long)act) - 1u;
        const uint32_t v0 = (uint32_t)__shfl((int)v, (int)first, 64);
        const bool shares = on && v == v0;
        const uint64_t same = __ballot(shares);
        if (shares) {
          if (lane == first) atomicAdd(&a.table[v0], (uint32_t)__popcll(same));
        } else if (on) {
          atomicAdd(&a.table[v], 1u);
        }
      }
    }
  }
  if (LDS) {
    __syncthreads();
    for (uint32_t i = tid; i < a.bins; i += kFacetBS) {
      const uint32_t c = s_hist[i];
      if (c) atomicAdd(&a.table[i], c);
    }
  }
}

struct FacetSelectArgs {
  const uint32_t* table;
  uint32_t bins, t;
  uint32_t* rows;   // out: t values, t counts, n, distinct
};

__global__ __launch_bounds__(kFacetBS) void facet_select_kernel(FacetSelectArgs a) {
  __shared__ uint64_t s_pairs[kFacetMaxT];
  __shared__ uint32_t hist[256];
  __shared__ uint32_t s_sel[4];
  __shared__ uint32_t s_total;
  __shared__ uint32_t s_cnt[kFacetWaves];
  __shared__ uint32_t s_cursor;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  constexpr uint32_t nt = kFacetBS;
  const uint32_t bins = a.bins, t = a.t;
  const uint32_t seg = (bins + kFacetWaves - 1u) / kFacetWaves;
  const uint32_t s0 = min(wave * seg, bins), s1 = min(s0 + seg, bins);   // this wavefront's segment of the table
  s_pairs[tid] = 0ull;
  if (tid == 0u) s_cursor = 0u;
  // 1. select: the t-th largest count, if there are more than t values
  uint32_t prefix = 0, mask = 0, need = t;
  bool all = false;
  for (int shift = 24; shift >= 0; shift -= 8) {
    if (tid < 256u) hist[tid] = 0;
    __syncthreads();
    for (uint32_t i = tid; i < bins; i += nt) {
      const uint32_t key = a.table[i];
      if (key != 0u && (key & mask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (tid < 64u) {
      if (shift == 24) {   // every value that occurs is in this histogram
        const uint32_t s = hist[4u * lane] + hist[4u * lane + 1u] + hist[4u * lane + 2u] + hist[4u * lane + 3u];
        const uint32_t incl = wave_incl_scan(s);
        if (lane == 63u) s_total = incl;
      }
      radix_select_pick(hist, need, lane, s_sel);   // (writes nothing where need exceeds the count: not read then)
    }
    __syncthreads();
    if (shift == 24 && s_total <= t) {   // (uniform: shared) every value is kept
      all = true;
      break;
    }
    prefix |= s_sel[0] << shift;
    mask |= 255u << shift;
    need = s_sel[1];
  }
  const uint32_t distinct = s_total;
  const uint32_t n_rows = all ? distinct : t;
  const uint32_t thr = all ? 0u : prefix, take_eq = all ? 0u : need;
  const uint32_t n_gt = n_rows - take_eq;   // the values above thr
  // 2. place: the values above thr through the cursor, the first take_eq equal to it in value order behind them
  uint32_t n_eq = 0;
  for (uint32_t b = s0; b < s1; b += 64u) {
    const uint32_t i = b + lane;
    const uint32_t key = i < s1 ? a.table[i] : 0u;
    n_eq += (uint32_t)__popcll(__ballot(!all && key == thr));
  }
  if (lane == 0u) s_cnt[wave] = n_eq;
  __syncthreads();
  uint32_t eq_before = 0;
  for (uint32_t x = 0; x < wave; ++x) eq_before += s_cnt[x];
  const uint64_t below = (1ull << lane) - 1ull;
  for (uint32_t b = s0; b < s1; b += 64u) {
    const uint32_t i = b + lane;
    const uint32_t key = i < s1 ? a.table[i] : 0u;
    const bool is_gt = key > thr, is_eq = !all && key == thr;
    const uint64_t m_eq = __ballot(is_eq);
    const uint32_t my_eq = eq_before + (uint32_t)__popcll(m_eq & below);
    const uint64_t pair = (uint64_t)key << 32 | (uint32_t)~i;
    if (is_gt) {
      const uint32_t pos = atomicAdd(&s_cursor, 1u);
      if (pos < kFacetMaxT) s_pairs[pos] = pair;   // (pos < n_gt <= t by the counts; the guard costs nothing)
    } else if (is_eq && my_eq < take_eq) {
      const uint32_t pos = n_gt + my_eq;
      if (pos < kFacetMaxT) s_pairs[pos] = pair;
    }
    eq_before += (uint32_t)__popcll(m_eq);
  }
  __syncthreads();
  // 3. order: count descending, value ascending (the slots past the rows hold 0 and sort last)
  uint32_t n_sort = 2;
  while (n_sort < n_rows) n_sort <<= 1;   // (uniform; <= 1024)
  bitonic_sort_lds<true>(s_pairs, n_sort, tid, nt);
  for (uint32_t i = tid; i < t; i += nt) {
    const uint64_t p = s_pairs[i];
    a.rows[i] = i < n_rows ? ~(uint32_t)p : 0u;
    a.rows[t + i] = i < n_rows ? (uint32_t)(p >> 32) : 0u;
  }
  if (tid == 0u) a.rows[2u * t] = n_rows, a.rows[2u * t + 1u] = distinct;
}

uint32_t round_up_64(uint64_t x) { return (uint32_t)((x + 63) / 64 * 64); }

}  // namespace

sgpu_status facet_counts_device(sgpu_index* idx, uint32_t replica, uint32_t slot, const sgpu_filter* filter, uint32_t t,
                                uint32_t* out_values, uint64_t* out_counts, uint32_t* out_n, uint64_t* out_distinct, uint64_t* out_docs) {
  const sgpu_status cst = facet_check_args(idx, slot, filter, t, out_values, out_counts, out_n, out_distinct, out_docs);
  if (cst != SGPU_OK) return cst;
  ColumnState* s = nullptr;
  const sgpu_status sst = column_state_of(idx, replica, &s);
  if (sst != SGPU_OK) return sst;
  const uint64_t n_docs = idx->host.n_docs, n_words = std::max<uint64_t>((n_docs + 31) / 32, 1);
  try {
    std::vector<uint32_t> rows(2 * (size_t)t + 2, 0u);
    {
      std::lock_guard<std::mutex> lk(s->mu);
      HIP_TRY(hipSetDevice(s->device));
      StreamDrain drain{s->stream};
      // the column as it is now that no set_column can run: the checks that read it hold for THIS column
      sgpu_status st = facet_check_args(idx, slot, filter, t, out_values, out_counts, out_n, out_distinct, out_docs);
      if (st != SGPU_OK) return st;
      const uint32_t bins = idx->columns[slot].max_u32 + 1u;
      const uint32_t* col = nullptr;
      const char* what = "for facet counts";
      if ((st = column_device_copy(s, idx, slot, &col)) != SGPU_OK || (st = s->c_table.reserve(s->stream, (uint64_t)bins * 4, what)) != SGPU_OK ||
          (st = s->c_rows.reserve(s->stream, rows.size() * 4, what)) != SGPU_OK ||
          (filter && (st = s->c_bits.reserve(s->stream, n_words * 4, what)) != SGPU_OK))
        return st;
      if (filter) HIP_TRY(hipMemcpyAsync(s->c_bits.p, filter_host_bits(filter), n_words * 4, hipMemcpyHostToDevice, s->stream));
      HIP_TRY(hipMemsetAsync(s->c_table.p, 0, (uint64_t)bins * 4, s->stream));
      const bool lds = bins <= kFacetLdsBins;
      // the slices: one workgroup per CU with its histogram in LDS, four where the table is global; no slice so short
      // that zeroing and adding up a histogram outweighs the counting
      const uint64_t wgs = (uint64_t)s->n_cu * (lds ? 1u : 4u);
      const uint32_t docs_per_wg = round_up_64(std::max<uint64_t>((n_docs + wgs - 1) / wgs, lds ? 4096 : 2048));
      const uint32_t grid = (uint32_t)((n_docs + docs_per_wg - 1) / docs_per_wg);
      FacetCountArgs ca{};
      ca.col = col;
      ca.fbits = filter ? s->c_bits.as<const uint32_t>() : nullptr;
      ca.table = s->c_table.as<uint32_t>();
      ca.n_docs = n_docs;
      ca.bins = bins;
      ca.docs_per_wg = docs_per_wg;
      FacetSelectArgs sa{};
      sa.table = s->c_table.as<const uint32_t>();
      sa.bins = bins;
      sa.t = t;
      sa.rows = s->c_rows.as<uint32_t>();
      (void)hipGetLastError();   // (judge these launches alone)
      HIP_TRY(hipEventRecord(s->ev0, s->stream));
      if (grid) {
        if (lds)
          hipLaunchKernelGGL(facet_count_kernel<true>, dim3(grid), dim3(kFacetBS), 0, s->stream, ca);
        else
          hipLaunchKernelGGL(facet_count_kernel<false>, dim3(grid), dim3(kFacetBS), 0, s->stream, ca);
        HIP_TRY(hipGetLastError());
      }
      HIP_TRY(hipEventRecord(s->ev2, s->stream));
      hipLaunchKernelGGL(facet_select_kernel, dim3(1), dim3(kFacetBS), 0, s->stream, sa);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipEventRecord(s->ev1, s->stream));
      HIP_TRY(hipMemcpyAsync(rows.data(), s->c_rows.p, rows.size() * 4, hipMemcpyDeviceToHost, s->stream));
      HIP_TRY(hipStreamSynchronize(s->stream));
      HIP_TRY(hipEventElapsedTime(&s->facet_ms, s->ev0, s->ev1));
      HIP_TRY(hipEventElapsedTime(&s->facet_count_ms, s->ev0, s->ev2));
      HIP_TRY(hipEventElapsedTime(&s->facet_select_ms, s->ev2, s->ev1));
      s->facet_grid = grid;
      s->facet_docs_per_wg = docs_per_wg;
      s->facet_path = lds ? 0u : 1u;
    }
    for (uint32_t i = 0; i < t; ++i) {
      out_values[i] = rows[i];
      out_counts[i] = rows[(size_t)t + i];
    }
    *out_n = rows[2 * (size_t)t];
    *out_distinct = rows[2 * (size_t)t + 1];
    *out_docs = filter ? filter_count(filter) : n_docs;
    return SGPU_OK;
  } catch (const std::bad_alloc&) {
    return fail(SGPU_ENOMEM, "out of host memory");
  }
}

}  // namespace sgpu
