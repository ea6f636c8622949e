// column_top.hip — the filter's documents ordered by a column, on the device (sgpu_column_top): the first min(t, valid)
// documents by (value in the given order, document id ascending), t <= 1024.
//
// The selection key of a document is sel = key for descending order and ~key for ascending (key = column_key: one unsigned
// order per type), so that the rows are the documents of the LARGEST sel, and among equal sel of the smallest id. A
// document counts where it is below n_docs, in the filter (the host words, uploaded for the call) and not an F32 NaN.
// A workgroup of 256 threads owns a contiguous slice of the documents and each of its four wavefronts a contiguous quarter
// of the slice. Kernels, on the column calls' stream (ColumnState, columns.hpp):
//   hist    (x 4)  a grid-wide radix select over sel, eight bits a pass from the top: the documents whose sel agrees with
//                  the prefix chosen so far are counted by the pass's byte in a 256-bin LDS histogram, and the workgroup
//                  adds its non-zero bins to the global one.
//   pick    (x 4)  one wavefront: device_prims.hpp's radix_select_pick over the global bins extends the prefix by the byte
//                  in which the running count from the top reaches `need`, leaves what is still needed inside it, and
//                  zeroes the bins. The first pick also knows `valid` (the sum of all bins); where valid <= t every document
//                  that counts is a row and the remaining kernels of the select do nothing (state.all).
//   count          after four passes the prefix is the threshold thr (the t-th largest sel) and `need` the number of
//                  documents equal to it that are still wanted. Each wavefront counts the equals of its quarter.
//   emit           the documents above thr are placed through a global cursor; of those equal to thr the first `need` in
//                  id order are taken: a wavefront's equals start at the sum of the counts of all wavefronts before it
//                  (an exclusive scan over the wavefronts of the grid, in slice order = id order), and inside a
//                  wavefront a ballot ranks them. What is placed is the composite (~sel) << 32 | id.
//   sort           one workgroup of 1024 threads sorts the at most 1024 composites ascending (bitonic, in LDS) and writes
//                  the rows: ids, the stored bits, n and valid.
// The launcher knows docs = |filter|: where docs <= t no select runs at all (0 passes; state.all is set by the host) and
// valid is the cursor's final value. The composites are distinct, so the order of the atomics decides nothing.
// Bounds: a document index is below n_docs wherever the column or the filter's words are addressed; a bin index is a byte;
// the wavefronts' counts are indexed below grid * 4, the size of the array; a composite is stored at pos < 1024 only (the
// counts make pos < t; the guard costs nothing); every loop is bounded by the slice, the grid or the sort's steps, and
// every barrier sits under workgroup-uniform conditions.
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

constexpr uint32_t kTopBS = 256, kTopWaves = kTopBS / 64u;
constexpr uint32_t kTopSortBS = 1024;

// the select's state in device memory (u32 each)
enum : uint32_t { kStPrefix = 0, kStMask = 1, kStNeed = 2, kStAll = 3, kStValid = 4, kStCursor = 5, kStWords = 8 };

struct TopArgs {
  const uint32_t* col;
  const uint32_t* fbits;     // the filter's words on this device, or null: all documents
  uint32_t* state;           // kStWords words
  uint32_t* hist;            // 256 bins
  uint32_t* wave_eq;         // grid * kTopWaves counts
  unsigned long long* comps; // kTopMaxT composites
  uint32_t* rows;            // out: t ids, t value bits, n, valid
  uint64_t n_docs;
  uint32_t type, order, t;
  uint32_t docs_per_wg;      // a multiple of 256: a wavefront's quarter is a multiple of 64
  uint32_t grid;
};

// (sel of document d, or false where it does not count)
__device__ __forceinline__ bool top_sel(const TopArgs& a, uint64_t d, uint64_t d1, uint32_t* sel) {
  bool on = d < d1;
  if (on && a.fbits) on = (a.fbits[d >> 5] >> (d & 31u)) & 1u;
  const uint32_t v = on ? a.col[d] : 0u;
  on = on && !column_not_a_value(a.type, v);
  const uint32_t key = column_key(a.type, v);
  *sel = a.order ? key : ~key;
  return on;
}

__global__ __launch_bounds__(kTopBS) void column_top_hist_kernel(TopArgs a, uint32_t shift) {
  __shared__ uint32_t s_hist[256];
  if (a.state[kStAll]) return;   // (uniform: one word for the grid)
  const uint32_t tid = threadIdx.x;
  s_hist[tid] = 0u;
  __syncthreads();
  const uint32_t prefix = a.state[kStPrefix], mask = a.state[kStMask];
  const uint64_t d0 = (uint64_t)blockIdx.x * a.docs_per_wg, d1 = min<uint64_t>(d0 + a.docs_per_wg, a.n_docs);
  for (uint64_t d = d0 + tid; d < d1; d += kTopBS) {
    uint32_t sel;
    if (top_sel(a, d, d1, &sel) && (sel & mask) == prefix) atomicAdd(&s_hist[(sel >> shift) & 255u], 1u);
  }
  __syncthreads();
  const uint32_t c = s_hist[tid];
  if (c) atomicAdd(&a.hist[tid], c);
}

__global__ __launch_bounds__(64) void column_top_pick_kernel(TopArgs a, uint32_t shift, uint32_t first) {
  __shared__ uint32_t s_hist[256];
  __shared__ uint32_t s_sel[4];
  if (a.state[kStAll]) return;
  const uint32_t lane = threadIdx.x;
  uint32_t s = 0;
  for (uint32_t i = 0; i < 4u; ++i) {
    const uint32_t c = a.hist[4u * lane + i];
    s_hist[4u * lane + i] = c;
    a.hist[4u * lane + i] = 0u;   // (for the next pass)
    s += c;
  }
  __syncthreads();
  if (first) {   // every document that counts is in this histogram
    const uint32_t incl = wave_incl_scan(s);
    const uint32_t total = (uint32_t)__shfl((int)incl, 63, 64);
    if (lane == 0u) a.state[kStValid] = total;
    if (total <= a.t) {   // (uniform) every one of them is a row
      if (lane == 0u) a.state[kStAll] = 1u;
      return;
    }
  }
  const uint32_t need = a.state[kStNeed];
  radix_select_pick(s_hist, need, lane, s_sel);
  __syncthreads();
  if (lane == 0u) {
    a.state[kStPrefix] |= s_sel[0] << shift;
    a.state[kStMask] |= 255u << shift;
    a.state[kStNeed] = s_sel[1];
  }
}

__global__ __launch_bounds__(kTopBS) void column_top_count_kernel(TopArgs a) {
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const bool all = a.state[kStAll] != 0u;
  const uint32_t thr = a.state[kStPrefix];
  const uint64_t d0 = (uint64_t)blockIdx.x * a.docs_per_wg, d1 = min<uint64_t>(d0 + a.docs_per_wg, a.n_docs);
  const uint32_t seg = a.docs_per_wg / kTopWaves;
  const uint64_t s0 = min<uint64_t>(d0 + (uint64_t)wave * seg, d1), s1 = min<uint64_t>(s0 + seg, d1);
  uint32_t n_eq = 0;
  if (!all)
    for (uint64_t b = s0; b < s1; b += 64u) {
      uint32_t sel;
      const bool on = top_sel(a, b + lane, s1, &sel);
      n_eq += (uint32_t)__popcll(__ballot(on && sel == thr));
    }
  if (lane == 0u) a.wave_eq[blockIdx.x * kTopWaves + wave] = n_eq;
}

__global__ __launch_bounds__(kTopBS) void column_top_emit_kernel(TopArgs a) {
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const bool all = a.state[kStAll] != 0u;
  const uint32_t thr = all ? 0u : a.state[kStPrefix], take_eq = all ? 0u : a.state[kStNeed];
  const uint32_t n_gt = a.t - take_eq;   // the documents above thr (take_eq <= t: it starts at t and only shrinks)
  const uint64_t d0 = (uint64_t)blockIdx.x * a.docs_per_wg, d1 = min<uint64_t>(d0 + a.docs_per_wg, a.n_docs);
  const uint32_t seg = a.docs_per_wg / kTopWaves;
  const uint64_t s0 = min<uint64_t>(d0 + (uint64_t)wave * seg, d1), s1 = min<uint64_t>(s0 + seg, d1);
  // the equals of all wavefronts before this one, in slice order
  uint32_t eq_before = 0;
  if (!all) {
    const uint32_t me = blockIdx.x * kTopWaves + wave;
    for (uint32_t x = lane; x < me; x += 64u) eq_before += a.wave_eq[x];
#pragma unroll
    for (int sft = 32; sft >= 1; sft >>= 1) eq_before += (uint32_t)__shfl_xor((int)eq_before, sft, 64);
  }
  const uint64_t below = (1ull << lane) - 1ull;
  for (uint64_t b = s0; b < s1; b += 64u) {
    const uint64_t d = b + lane;
    uint32_t sel;
    const bool on = top_sel(a, d, s1, &sel);
    const bool is_gt = on && (all || sel > thr), is_eq = on && !all && sel == thr;
    const uint64_t m_eq = __ballot(is_eq);
    const uint32_t my_eq = eq_before + (uint32_t)__popcll(m_eq & below);
    const unsigned long long comp = (unsigned long long)(~sel) << 32 | (uint32_t)d;
    if (is_gt) {
      const uint32_t pos = atomicAdd(&a.state[kStCursor], 1u);
      if (pos < kTopMaxT) a.comps[pos] = comp;   // (pos < n_gt <= t, or < valid <= t, by the counts)
    } else if (is_eq && my_eq < take_eq) {
      const uint32_t pos = n_gt + my_eq;
      if (pos < kTopMaxT) a.comps[pos] = comp;
    }
    eq_before += (uint32_t)__popcll(m_eq);
  }
}

__global__ __launch_bounds__(kTopSortBS) void column_top_sort_kernel(TopArgs a) {
  __shared__ unsigned long long s_comps[kTopMaxT];
  const uint32_t tid = threadIdx.x;
  const bool all = a.state[kStAll] != 0u;
  const uint32_t cursor = min(a.state[kStCursor], kTopMaxT);
  const uint32_t n_rows = all ? min(cursor, a.t) : a.t;
  const uint32_t valid = all ? cursor : a.state[kStValid];   // (all: every document that counts went through the cursor)
  s_comps[tid] = tid < n_rows ? a.comps[tid] : ~0ull;         // (the slots past the rows sort last)
  __syncthreads();
  uint32_t n_sort = 2;
  while (n_sort < n_rows) n_sort <<= 1;   // (uniform; <= 1024)
  bitonic_sort_lds<false>(s_comps, n_sort, tid, kTopSortBS);
  for (uint32_t i = tid; i < a.t; i += kTopSortBS) {
    const uint32_t id = (uint32_t)s_comps[i];
    const bool row = i < n_rows && id < a.n_docs;
    a.rows[i] = row ? id : 0u;
    a.rows[a.t + i] = row ? a.col[id] : 0u;
  }
  if (tid == 0u) a.rows[2u * a.t] = n_rows, a.rows[2u * a.t + 1u] = valid;
}

uint32_t round_up_256(uint64_t x) { return (uint32_t)((x + 255) / 256 * 256); }

}  // namespace

sgpu_status column_top_device(sgpu_index* idx, uint32_t replica, uint32_t slot, const sgpu_filter* filter, uint32_t t, uint32_t order,
                              uint32_t* out_doc_ids, uint32_t* out_value_bits, uint32_t* out_n, uint64_t* out_valid, uint64_t* out_docs) {
  const sgpu_status cst = top_check_args(idx, slot, filter, t, order, out_doc_ids, out_value_bits, out_n, out_valid, out_docs);
  if (cst != SGPU_OK) return cst;
  ColumnState* s = nullptr;
  const sgpu_status sst = column_state_of(idx, replica, &s);
  if (sst != SGPU_OK) return sst;
  const uint64_t n_docs = idx->host.n_docs, n_words = std::max<uint64_t>((n_docs + 31) / 32, 1);
  const uint64_t docs = filter ? filter_count(filter) : n_docs;
  try {
    std::vector<uint32_t> rows(2 * (size_t)t + 2, 0u);   // (both outlive the drain of the stream: the copies read and write them)
    uint32_t state[kStWords] = {};
    {
      std::lock_guard<std::mutex> lk(s->mu);
      HIP_TRY(hipSetDevice(s->device));
      StreamDrain drain{s->stream};
      // the column as it is now that no set_column can run
      sgpu_status st = top_check_args(idx, slot, filter, t, order, out_doc_ids, out_value_bits, out_n, out_valid, out_docs);
      if (st != SGPU_OK) return st;
      // the slices: four workgroups per CU, none shorter than 2048 documents
      const uint64_t wgs = (uint64_t)s->n_cu * 4u;
      const uint32_t docs_per_wg = round_up_256(std::max<uint64_t>((n_docs + wgs - 1) / wgs, 2048));
      const uint32_t grid = (uint32_t)((n_docs + docs_per_wg - 1) / docs_per_wg);
      const uint32_t* col = nullptr;
      const char* what = "for a column top";
      if ((st = column_device_copy(s, idx, slot, &col)) != SGPU_OK || (st = s->t_state.reserve(s->stream, kStWords * 4, what)) != SGPU_OK ||
          (st = s->t_hist.reserve(s->stream, 256 * 4, what)) != SGPU_OK ||
          (st = s->t_waves.reserve(s->stream, (uint64_t)std::max(grid, 1u) * kTopWaves * 4, what)) != SGPU_OK ||
          (st = s->t_comps.reserve(s->stream, (uint64_t)kTopMaxT * 8, what)) != SGPU_OK ||
          (st = s->t_rows.reserve(s->stream, rows.size() * 4, what)) != SGPU_OK ||
          (filter && (st = s->a_bits.reserve(s->stream, n_words * 4, what)) != SGPU_OK))
        return st;
      if (filter) HIP_TRY(hipMemcpyAsync(s->a_bits.p, filter_host_bits(filter), n_words * 4, hipMemcpyHostToDevice, s->stream));
      const bool select = docs > t;   // (else every document of the filter that is a value is a row)
      state[kStNeed] = t;
      state[kStAll] = select ? 0u : 1u;
      HIP_TRY(hipMemcpyAsync(s->t_state.p, state, sizeof(state), hipMemcpyHostToDevice, s->stream));
      HIP_TRY(hipMemsetAsync(s->t_hist.p, 0, 256 * 4, s->stream));
      HIP_TRY(hipMemsetAsync(s->t_comps.p, 0, (uint64_t)kTopMaxT * 8, s->stream));
      TopArgs a{};
      a.col = col;
      a.fbits = filter ? s->a_bits.as<const uint32_t>() : nullptr;
      a.state = s->t_state.as<uint32_t>();
      a.hist = s->t_hist.as<uint32_t>();
      a.wave_eq = s->t_waves.as<uint32_t>();
      a.comps = s->t_comps.as<unsigned long long>();
      a.rows = s->t_rows.as<uint32_t>();
      a.n_docs = n_docs;
      a.type = idx->columns[slot].type;
      a.order = order;
      a.t = t;
      a.docs_per_wg = docs_per_wg;
      a.grid = grid;
      uint32_t passes = 0;
      (void)hipGetLastError();   // (judge these launches alone)
      HIP_TRY(hipEventRecord(s->ev0, s->stream));
      if (grid) {
        if (select) {
          for (int shift = 24; shift >= 0; shift -= 8) {
            hipLaunchKernelGGL(column_top_hist_kernel, dim3(grid), dim3(kTopBS), 0, s->stream, a, (uint32_t)shift);
            hipLaunchKernelGGL(column_top_pick_kernel, dim3(1), dim3(64), 0, s->stream, a, (uint32_t)shift, shift == 24 ? 1u : 0u);
            HIP_TRY(hipGetLastError());
            ++passes;
          }
          hipLaunchKernelGGL(column_top_count_kernel, dim3(grid), dim3(kTopBS), 0, s->stream, a);
        }
        hipLaunchKernelGGL(column_top_emit_kernel, dim3(grid), dim3(kTopBS), 0, s->stream, a);
        HIP_TRY(hipGetLastError());
      }
      hipLaunchKernelGGL(column_top_sort_kernel, dim3(1), dim3(kTopSortBS), 0, s->stream, a);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipEventRecord(s->ev1, s->stream));
      HIP_TRY(hipMemcpyAsync(rows.data(), s->t_rows.p, rows.size() * 4, hipMemcpyDeviceToHost, s->stream));
      HIP_TRY(hipStreamSynchronize(s->stream));
      HIP_TRY(hipEventElapsedTime(&s->top_ms, s->ev0, s->ev1));
      s->top_grid = grid;
      s->top_docs_per_wg = docs_per_wg;
      s->top_passes = passes;
    }
    for (uint32_t i = 0; i < t; ++i) {
      out_doc_ids[i] = rows[i];
      out_value_bits[i] = rows[(size_t)t + i];
    }
    *out_n = rows[2 * (size_t)t];
    *out_valid = rows[2 * (size_t)t + 1];
    *out_docs = docs;
    return SGPU_OK;
  } catch (const std::bad_alloc&) {
    return fail(SGPU_ENOMEM, "out of host memory");
  }
}

}  // namespace sgpu
