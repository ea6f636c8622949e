// column_aggregate.hip — column statistics and histograms on the device (sgpu_column_stats, sgpu_column_histogram): one
// streaming pass each over the column of `slot` and the filter's words (the host words, uploaded for the call), on the
// column calls' stream (ColumnState, columns.hpp).
//
//   stats      a workgroup of kAggLanes = 256 threads takes ONE tile of kAggTile = 16384 consecutive documents - the tile of
//              the canonical F32 sum (seismic_hip.h): thread j adds (double)v of the documents tile * 16384 + r * 256 + j,
//              r = 0 .. 63 ascending, to its lane sum (a coalesced dword load per turn), the 256 lane sums are folded in
//              LDS by c[j] += c[j + h], h = 128 .. 1, and the tile's sum goes to the tile's slot. min / max key, the count
//              of values and the integer sum are order-free: wave reductions by shuffles, the four wavefronts' results
//              through LDS, one slot per workgroup. The launcher adds the ceil(n_docs / 16384) partials on the host in
//              ascending tile order (stats_combine, column_host.cpp: the host twin's own last step).
//   histogram  a workgroup of 1024 threads takes a slice of consecutive documents, sized as facet_counts_device sizes the
//              slices of its LDS form. The edge keys (at most 4097: 16 KiB) and n_buckets + 3 u32 bins (buckets, below,
//              above, NaN: 16 KiB) lie in LDS; a document is one coalesced dword load, a binary search of at most 13 steps
//              for the number of edges <= its key, and an LDS atomic. A workgroup adds its non-zero bins to the global
//              table (u64) with one atomic each. Counts are integers: the order of the atomics decides nothing.
// Bounds: a document index is below n_docs wherever the column or the filter's words are addressed; a tile's slot is
// blockIdx.x < grid = the number of slots; a bin index is below n_buckets + 3 <= 4099 by construction (the search runs over
// [0, n_edges), its result minus one is clamped to n_buckets - 1); every loop is bounded by the tile, the slice, the
// edges or 13 steps, and every barrier sits under workgroup-uniform conditions.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>
#include <new>
#include <vector>

#include "columns.hpp"
#include "filter.hpp"

namespace sgpu {

namespace {

constexpr uint32_t kHistBS = 1024;
static_assert(kAggTile % kAggLanes == 0 && kAggLanes == 256, "a tile is 64 turns of the stats kernel's 256 threads");

struct StatsArgs {
  const uint32_t* col;
  const uint32_t* fbits;   // the filter's words on this device, or null: all documents
  AggPartial* parts;       // one per tile = workgroup
  uint64_t n_docs;
  uint32_t type;
};

__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, s, 64));
  return v;
}
__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, s, 64));
  return v;
}
__device__ __forceinline__ uint64_t wave_sum(uint64_t v) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) v += (uint64_t)__shfl_xor((long long)v, s, 64);
  return v;
}

__global__ __launch_bounds__(kAggLanes) void column_stats_kernel(StatsArgs a) {
  __shared__ double s_c[kAggLanes];
  __shared__ uint64_t s_sum[kAggLanes / 64u];
  __shared__ uint32_t s_min[kAggLanes / 64u], s_max[kAggLanes / 64u], s_valid[kAggLanes / 64u];
  const uint32_t j = threadIdx.x, lane = j & 63u, wave = j >> 6;
  const uint64_t d0 = (uint64_t)blockIdx.x * kAggTile;
  double c = 0.0;
  uint64_t sum_int = 0;
  uint32_t min_key = 0xffffffffu, max_key = 0u, valid = 0u;
  for (uint32_t r = 0; r < kAggTile / kAggLanes; ++r) {
    const uint64_t d = d0 + (uint64_t)r * kAggLanes + j;
    bool on = d < a.n_docs;
    if (on && a.fbits) on = (a.fbits[d >> 5] >> (d & 31u)) & 1u;
    const uint32_t v = on ? a.col[d] : 0u;
    on = on && !column_not_a_value(a.type, v);
    if (on) {
      const uint32_t key = column_key(a.type, v);
      min_key = min(min_key, key);
      max_key = max(max_key, key);
      ++valid;
      if (a.type == SGPU_COL_F32) c += (double)__uint_as_float(v);
      else sum_int += a.type == SGPU_COL_I32 ? (uint64_t)(int64_t)(int32_t)v : (uint64_t)v;
    }
  }
  s_c[j] = c;
  min_key = wave_min(min_key);
  max_key = wave_max(max_key);
  sum_int = wave_sum(sum_int);
  valid = (uint32_t)wave_sum((uint64_t)valid);
  if (lane == 0u) s_min[wave] = min_key, s_max[wave] = max_key, s_sum[wave] = sum_int, s_valid[wave] = valid;
  __syncthreads();
  for (uint32_t h = kAggLanes / 2u; h >= 1u; h >>= 1) {
    if (j < h) s_c[j] += s_c[j + h];
    __syncthreads();
  }
  if (j == 0u) {
    AggPartial p;
    p.sum = s_c[0];
    p.sum_int = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
    p.min_key = min(min(s_min[0], s_min[1]), min(s_min[2], s_min[3]));
    p.max_key = max(max(s_max[0], s_max[1]), max(s_max[2], s_max[3]));
    p.valid = s_valid[0] + s_valid[1] + s_valid[2] + s_valid[3];
    p.pad = 0u;
    a.parts[blockIdx.x] = p;
  }
}

struct HistArgs {
  const uint32_t* col;
  const uint32_t* fbits;
  const uint32_t* edge_keys;       // n_edges keys, strictly ascending
  unsigned long long* table;       // n_edges + 2 bins: the buckets, below, above, NaN
  uint64_t n_docs;
  uint32_t type, n_edges;
  uint32_t docs_per_wg;            // a multiple of 64
};

__global__ __launch_bounds__(kHistBS) void column_histogram_kernel(HistArgs a) {
  __shared__ uint32_t s_edges[kAggMaxBuckets + 1];
  __shared__ uint32_t s_hist[kAggMaxBuckets + 3];
  const uint32_t tid = threadIdx.x;
  const uint32_t ne = min(a.n_edges, kAggMaxBuckets + 1u), nb = ne - 1u, bins = nb + 3u;
  for (uint32_t i = tid; i < ne; i += kHistBS) s_edges[i] = a.edge_keys[i];
  for (uint32_t i = tid; i < bins; i += kHistBS) s_hist[i] = 0u;
  __syncthreads();
  const uint32_t first = s_edges[0], last = s_edges[nb];
  const uint64_t d0 = (uint64_t)blockIdx.x * a.docs_per_wg, d1 = min<uint64_t>(d0 + a.docs_per_wg, a.n_docs);
  for (uint64_t d = d0 + tid; d < d1; d += kHistBS) {
    if (a.fbits && !((a.fbits[d >> 5] >> (d & 31u)) & 1u)) continue;
    const uint32_t v = a.col[d];
    uint32_t b;
    if (column_not_a_value(a.type, v)) {
      b = nb + 2u;
    } else {
      const uint32_t key = column_key(a.type, v);
      if (key < first) {
        b = nb;
      } else if (key > last) {
        b = nb + 1u;
      } else {   // the number of edges <= key, in [1, ne]
        uint32_t lo = 0u, hi = ne;
        while (lo < hi) {
          const uint32_t mid = lo + ((hi - lo) >> 1);
          if (s_edges[mid] <= key) lo = mid + 1u; else hi = mid;
        }
        b = min(lo - 1u, nb - 1u);   // (the last bucket also takes its upper edge)
      }
    }
    atomicAdd(&s_hist[b], 1u);
  }
  __syncthreads();
  for (uint32_t i = tid; i < bins; i += kHistBS) {
    const uint32_t c = s_hist[i];
    if (c) atomicAdd(&a.table[i], (unsigned long long)c);
  }
}

uint32_t round_up_64(uint64_t x) { return (uint32_t)((x + 63) / 64 * 64); }

}  // namespace

sgpu_status column_stats_device(sgpu_index* idx, uint32_t replica, uint32_t slot, const sgpu_filter* filter, struct sgpu_column_stats* out) {
  const sgpu_status cst = stats_check_args(idx, slot, filter, out);
  if (cst != SGPU_OK) return cst;
  ColumnState* s = nullptr;
  const sgpu_status sst = column_state_of(idx, replica, &s);
  if (sst != SGPU_OK) return sst;
  const uint64_t n_docs = idx->host.n_docs, n_words = std::max<uint64_t>((n_docs + 31) / 32, 1);
  const uint64_t n_tiles = (n_docs + kAggTile - 1) / kAggTile;
  try {
    std::vector<AggPartial> parts((size_t)n_tiles);   // (outlives the drain of the stream: the copy writes it)
    uint32_t type = 0;
    {
      std::lock_guard<std::mutex> lk(s->mu);
      HIP_TRY(hipSetDevice(s->device));
      StreamDrain drain{s->stream};
      // the column as it is now that no set_column can run
      sgpu_status st = stats_check_args(idx, slot, filter, out);
      if (st != SGPU_OK) return st;
      type = idx->columns[slot].type;
      const uint32_t* col = nullptr;
      const char* what = "for column stats";
      if ((st = column_device_copy(s, idx, slot, &col)) != SGPU_OK ||
          (st = s->a_parts.reserve(s->stream, n_tiles * sizeof(AggPartial), what)) != SGPU_OK ||
          (filter && (st = s->a_bits.reserve(s->stream, n_words * 4, what)) != SGPU_OK))
        return st;
      if (filter) HIP_TRY(hipMemcpyAsync(s->a_bits.p, filter_host_bits(filter), n_words * 4, hipMemcpyHostToDevice, s->stream));
      StatsArgs a{};
      a.col = col;
      a.fbits = filter ? s->a_bits.as<const uint32_t>() : nullptr;
      a.parts = s->a_parts.as<AggPartial>();
      a.n_docs = n_docs;
      a.type = type;
      const uint32_t grid = (uint32_t)n_tiles;
      (void)hipGetLastError();   // (judge this launch alone)
      HIP_TRY(hipEventRecord(s->ev0, s->stream));
      if (grid) {
        hipLaunchKernelGGL(column_stats_kernel, dim3(grid), dim3(kAggLanes), 0, s->stream, a);
        HIP_TRY(hipGetLastError());
      }
      HIP_TRY(hipEventRecord(s->ev1, s->stream));
      if (grid) HIP_TRY(hipMemcpyAsync(parts.data(), s->a_parts.p, n_tiles * sizeof(AggPartial), hipMemcpyDeviceToHost, s->stream));
      HIP_TRY(hipStreamSynchronize(s->stream));
      HIP_TRY(hipEventElapsedTime(&s->stats_ms, s->ev0, s->ev1));
      s->stats_grid = grid;
    }
    stats_combine(type, parts.data(), n_tiles, filter ? filter_count(filter) : n_docs, out);
    return SGPU_OK;
  } catch (const std::bad_alloc&) {
    return fail(SGPU_ENOMEM, "out of host memory");
  }
}

sgpu_status column_histogram_device(sgpu_index* idx, uint32_t replica, uint32_t slot, const sgpu_filter* filter, const uint32_t* edges,
                                    uint32_t n_edges, uint64_t* out_counts, uint64_t* out_below, uint64_t* out_above, uint64_t* out_nan,
                                    uint64_t* out_docs) {
  const sgpu_status cst = histogram_check_args(idx, slot, filter, edges, n_edges, out_counts, out_below, out_above, out_nan, out_docs);
  if (cst != SGPU_OK) return cst;
  ColumnState* s = nullptr;
  const sgpu_status sst = column_state_of(idx, replica, &s);
  if (sst != SGPU_OK) return sst;
  const uint64_t n_docs = idx->host.n_docs, n_words = std::max<uint64_t>((n_docs + 31) / 32, 1);
  const uint32_t nb = n_edges - 1u, bins = nb + 3u;
  try {
    std::vector<uint32_t> ek(n_edges);            // (both outlive the drain of the stream: the copies read and write them)
    std::vector<unsigned long long> table(bins, 0ull);
    {
      std::lock_guard<std::mutex> lk(s->mu);
      HIP_TRY(hipSetDevice(s->device));
      StreamDrain drain{s->stream};
      // the column as it is now that no set_column can run: the edges are judged in THIS column's type
      sgpu_status st = histogram_check_args(idx, slot, filter, edges, n_edges, out_counts, out_below, out_above, out_nan, out_docs);
      if (st != SGPU_OK) return st;
      const uint32_t type = idx->columns[slot].type;
      for (uint32_t i = 0; i < n_edges; ++i) ek[i] = column_key(type, edges[i]);
      const uint32_t* col = nullptr;
      const char* what = "for a column histogram";
      if ((st = column_device_copy(s, idx, slot, &col)) != SGPU_OK || (st = s->a_edges.reserve(s->stream, (uint64_t)n_edges * 4, what)) != SGPU_OK ||
          (st = s->a_table.reserve(s->stream, (uint64_t)bins * 8, what)) != SGPU_OK ||
          (filter && (st = s->a_bits.reserve(s->stream, n_words * 4, what)) != SGPU_OK))
        return st;
      if (filter) HIP_TRY(hipMemcpyAsync(s->a_bits.p, filter_host_bits(filter), n_words * 4, hipMemcpyHostToDevice, s->stream));
      HIP_TRY(hipMemcpyAsync(s->a_edges.p, ek.data(), (uint64_t)n_edges * 4, hipMemcpyHostToDevice, s->stream));
      HIP_TRY(hipMemsetAsync(s->a_table.p, 0, (uint64_t)bins * 8, s->stream));
      // the slices of facet_counts_device's LDS form: one workgroup per CU, no slice so short that zeroing and adding up
      // a histogram outweighs the counting
      const uint64_t wgs = s->n_cu;
      const uint32_t docs_per_wg = round_up_64(std::max<uint64_t>((n_docs + wgs - 1) / wgs, 4096));
      const uint32_t grid = (uint32_t)((n_docs + docs_per_wg - 1) / docs_per_wg);
      HistArgs a{};
      a.col = col;
      a.fbits = filter ? s->a_bits.as<const uint32_t>() : nullptr;
      a.edge_keys = s->a_edges.as<const uint32_t>();
      a.table = s->a_table.as<unsigned long long>();
      a.n_docs = n_docs;
      a.type = type;
      a.n_edges = n_edges;
      a.docs_per_wg = docs_per_wg;
      (void)hipGetLastError();   // (judge this launch alone)
      HIP_TRY(hipEventRecord(s->ev0, s->stream));
      if (grid) {
        hipLaunchKernelGGL(column_histogram_kernel, dim3(grid), dim3(kHistBS), 0, s->stream, a);
        HIP_TRY(hipGetLastError());
      }
      HIP_TRY(hipEventRecord(s->ev1, s->stream));
      HIP_TRY(hipMemcpyAsync(table.data(), s->a_table.p, (uint64_t)bins * 8, hipMemcpyDeviceToHost, s->stream));
      HIP_TRY(hipStreamSynchronize(s->stream));
      HIP_TRY(hipEventElapsedTime(&s->hist_ms, s->ev0, s->ev1));
      s->hist_grid = grid;
      s->hist_docs_per_wg = docs_per_wg;
    }
    for (uint32_t b = 0; b < nb; ++b) out_counts[b] = table[b];
    *out_below = table[nb];
    *out_above = table[nb + 1];
    *out_nan = table[nb + 2];
    *out_docs = filter ? filter_count(filter) : n_docs;
    return SGPU_OK;
  } catch (const std::bad_alloc&) {
    return fail(SGPU_ENOMEM, "out of host memory");
  }
}

// (test hook) sgpu_debug_column_agg_stats; false before the replica's first column call
bool column_agg_debug_stats(sgpu_index* idx, uint32_t replica, double* out10) {
  std::lock_guard<std::mutex> lk(idx->column_mu);
  if (replica >= idx->column_state.size() || !idx->column_state[replica]) return false;
  ColumnState* s = idx->column_state[replica];
  std::lock_guard<std::mutex> lk2(s->mu);
  const double v[10] = {s->stats_ms, s->hist_ms, s->top_ms, (double)s->stats_grid, (double)s->hist_grid, (double)s->top_grid,
                        (double)kAggTile, (double)s->top_passes, (double)s->hist_docs_per_wg, (double)s->top_docs_per_wg};
  for (int i = 0; i < 10; ++i) out10[i] = v[i];
  return true;
}

}  // namespace sgpu
