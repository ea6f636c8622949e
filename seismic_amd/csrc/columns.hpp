// columns.hpp — what column_host.cpp (set / get, the checks, the host twins), column_filter.hip, facet_counts.hip,
// column_aggregate.hip and column_top.hip (the device calls) share of the document columns: sgpu_index_set_column,
// sgpu_filter_create_columns[_host], sgpu_facet_counts[_host], sgpu_column_stats / _histogram / _top[_host]. The per-replica state itself (ColumnState: a stream, a mutex, the device copies of the columns
// and the recycled scratch) is column_filter.hip's and is only named here. Compiles without HIP.
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>

#include "host_index.hpp"
#include "term_filter.hpp"

namespace sgpu {

constexpr uint32_t kColMaxClauses = 64;
constexpr uint32_t kColMaxSetValues = 8192;       // the IN values of a call: 32 KiB of LDS
constexpr uint32_t kColDocsPerWg = 8192;          // documents a workgroup of the filter kernel takes
constexpr uint32_t kFacetMaxT = 1024;
constexpr uint32_t kFacetMaxBins = 1u << 22;      // values 0 .. (1 << 22) - 1: a table of 16 MiB
constexpr uint32_t kFacetLdsBins = 32768;         // u32 bins a workgroup counts in LDS (128 KiB)
constexpr uint32_t kAggTile = 16384;              // documents of a tile of the canonical F32 sum: a workgroup of the stats kernel
constexpr uint32_t kAggLanes = 256;               // lane sums of a tile: the threads of that workgroup
constexpr uint32_t kAggMaxBuckets = 4096;         // buckets of a histogram: 4097 edge keys, 16 KiB of LDS
constexpr uint32_t kTopMaxT = 1024;

// The comparison of a column's type as ONE unsigned comparison: key(type, bits) ascends with the value.
//   U32  the value
//   I32  the sign bit flipped
//   F32  -0.0 taken as +0.0, then the sign bit of a non-negative set and all bits of a negative flipped. The keys of the
//        numbers lie in [key(-inf), key(+inf)] = [0x007fffff, 0xff800000] and every NaN's key lies outside: a stored NaN
//        is in no range and equals no set value, since bounds and set values are never NaN (check 2).
// Host and device evaluate the clauses on keys, so they cannot disagree on a comparison.
#ifdef __HIPCC__
__host__ __device__
#endif
inline uint32_t column_key(uint32_t type, uint32_t bits) {
  if (type == SGPU_COL_U32) return bits;
  if (type == SGPU_COL_I32) return bits ^ 0x80000000u;
  if (bits == 0x80000000u) bits = 0u;
  return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
}
#ifdef __HIPCC__
__host__ __device__
#endif
inline bool column_bits_nan(uint32_t bits) { return (bits & 0x7fffffffu) > 0x7f800000u; }
// The bit pattern a key stands for (an f32 zero comes back as +0.0: its key is that of +0.0).
#ifdef __HIPCC__
__host__ __device__
#endif
inline uint32_t column_key_bits(uint32_t type, uint32_t key) {
  if (type == SGPU_COL_U32) return key;
  if (type == SGPU_COL_I32) return key ^ 0x80000000u;
  return (key & 0x80000000u) ? (key & 0x7fffffffu) : ~key;
}
// A stored value that is no value: the NaN of an F32 column (counted apart, never compared).
#ifdef __HIPCC__
__host__ __device__
#endif
inline bool column_not_a_value(uint32_t type, uint32_t bits) { return type == SGPU_COL_F32 && column_bits_nan(bits); }

// A clause as both twins evaluate it: bounds as keys, the IN values as keys sorted ascending in [begin, begin + count) of
// the call's key array. The clauses are in ascending slot order (the counts of a document do not depend on the order);
// `fresh` marks the first clause of a slot: the column's value is loaded there and kept for the slot's other clauses.
struct ColClause {
  const uint32_t* col;   // the column's values: host copy (host twin) or the replica's copy (device call)
  uint32_t slot, type, occur, op;
  uint32_t lo, hi;
  uint32_t begin, count;
  uint32_t fresh, pad;
};
struct ColPlan {
  std::vector<ColClause> clauses;   // col is null: the twin fills it in
  std::vector<uint32_t> keys;
  uint32_t n_must = 0, n_should = 0;
};

// column_host.cpp
// checks 1 - 4 of both filter calls, in the header's order (*out is set to null once it is known not to be)
sgpu_status column_check_args(const sgpu_index* idx, const sgpu_column_clause* clauses, uint32_t n_clauses, const uint32_t* set_values,
                              uint32_t n_set_values, const sgpu_filter* within, sgpu_filter** out);
// (after the checks; may throw std::bad_alloc)
void column_plan(const sgpu_index* idx, const sgpu_column_clause* clauses, uint32_t n_clauses, const uint32_t* set_values, ColPlan* plan);
sgpu_status column_filter_host(sgpu_index* idx, const sgpu_column_clause* clauses, uint32_t n_clauses, uint32_t min_should,
                               const uint32_t* set_values, uint32_t n_set_values, const sgpu_filter* within, uint32_t num_threads,
                               sgpu_filter** out);
// checks 1 - 3 of both facet calls
sgpu_status facet_check_args(const sgpu_index* idx, uint32_t slot, const sgpu_filter* filter, uint32_t t, const uint32_t* out_values,
                             const uint64_t* out_counts, const uint32_t* out_n, const uint64_t* out_distinct, const uint64_t* out_docs);
sgpu_status facet_counts_host(const sgpu_index* idx, uint32_t slot, const sgpu_filter* filter, uint32_t t, uint32_t num_threads,
                              uint32_t* out_values, uint64_t* out_counts, uint32_t* out_n, uint64_t* out_distinct, uint64_t* out_docs);
// the aggregations (sgpu_column_stats / _histogram / _top): the checks of the host twin and of the device call, in the
// header's order, and the host twins
sgpu_status stats_check_args(const sgpu_index* idx, uint32_t slot, const sgpu_filter* filter, const struct sgpu_column_stats* out);
sgpu_status histogram_check_args(const sgpu_index* idx, uint32_t slot, const sgpu_filter* filter, const uint32_t* edges, uint32_t n_edges,
                                 const uint64_t* out_counts, const uint64_t* out_below, const uint64_t* out_above, const uint64_t* out_nan,
                                 const uint64_t* out_docs);
sgpu_status top_check_args(const sgpu_index* idx, uint32_t slot, const sgpu_filter* filter, uint32_t t, uint32_t order,
                           const uint32_t* out_doc_ids, const uint32_t* out_value_bits, const uint32_t* out_n, const uint64_t* out_valid,
                           const uint64_t* out_docs);
// What a tile of the stats contributes; the tiles are combined in ascending tile order by stats_combine (both twins).
struct AggPartial {
  double sum;         // F32: the tile's canonical sum; else +0.0
  uint64_t sum_int;   // U32 / I32: the tile's sum, wrapping (I32 values sign-extended)
  uint32_t min_key, max_key;   // 0xffffffff / 0 where valid == 0
  uint32_t valid, pad;
};
void stats_combine(uint32_t type, const AggPartial* parts, uint64_t n_tiles, uint64_t docs, struct sgpu_column_stats* out);
sgpu_status column_stats_host(const sgpu_index* idx, uint32_t slot, const sgpu_filter* filter, uint32_t num_threads, struct sgpu_column_stats* out);
sgpu_status column_histogram_host(const sgpu_index* idx, uint32_t slot, const sgpu_filter* filter, const uint32_t* edges, uint32_t n_edges,
                                  uint32_t num_threads, uint64_t* out_counts, uint64_t* out_below, uint64_t* out_above, uint64_t* out_nan,
                                  uint64_t* out_docs);
sgpu_status column_top_host(const sgpu_index* idx, uint32_t slot, const sgpu_filter* filter, uint32_t t, uint32_t order, uint32_t num_threads,
                            uint32_t* out_doc_ids, uint32_t* out_value_bits, uint32_t* out_n, uint64_t* out_valid, uint64_t* out_docs);
sgpu_status column_set(sgpu_index* idx, uint32_t slot, uint32_t type, const void* values, uint64_t n);
sgpu_status column_get(const sgpu_index* idx, uint32_t slot, uint32_t* type, const void** values, uint64_t* n);

// column_filter.hip: the replicas' states
// (set_column: every state's mutex taken in replica order, `replace` run, the device copy of `slot` freed where `drop`;
// idx->column_mu is held by the caller)
void column_states_locked(sgpu_index* idx, uint32_t slot, bool drop, void (*replace)(void*), void* arg);
void column_state_free(ColumnState* s);
uint64_t column_device_bytes(const sgpu_index* idx);
bool column_debug_stats(sgpu_index* idx, uint32_t replica, double* out8);
bool facet_debug_kernel_ms(sgpu_index* idx, uint32_t replica, double* out2);
sgpu_status column_filter_device(sgpu_index* idx, uint32_t replica, const sgpu_column_clause* clauses, uint32_t n_clauses,
                                 uint32_t min_should, const uint32_t* set_values, uint32_t n_set_values, const sgpu_filter* within,
                                 sgpu_filter** out);
// facet_counts.hip
sgpu_status facet_counts_device(sgpu_index* idx, uint32_t replica, uint32_t slot, const sgpu_filter* filter, uint32_t t,
                                uint32_t* out_values, uint64_t* out_counts, uint32_t* out_n, uint64_t* out_distinct, uint64_t* out_docs);

// column_aggregate.hip, column_top.hip
sgpu_status column_stats_device(sgpu_index* idx, uint32_t replica, uint32_t slot, const sgpu_filter* filter, struct sgpu_column_stats* out);
sgpu_status column_histogram_device(sgpu_index* idx, uint32_t replica, uint32_t slot, const sgpu_filter* filter, const uint32_t* edges,
                                    uint32_t n_edges, uint64_t* out_counts, uint64_t* out_below, uint64_t* out_above, uint64_t* out_nan,
                                    uint64_t* out_docs);
sgpu_status column_top_device(sgpu_index* idx, uint32_t replica, uint32_t slot, const sgpu_filter* filter, uint32_t t, uint32_t order,
                              uint32_t* out_doc_ids, uint32_t* out_value_bits, uint32_t* out_n, uint64_t* out_valid, uint64_t* out_docs);
bool column_agg_debug_stats(sgpu_index* idx, uint32_t replica, double* out10);

}  // namespace sgpu

#ifdef __HIPCC__
// ---- what only the .hip files of the column calls see: the state itself
#include "hip_util.hpp"

namespace sgpu {

// Per replica: the column calls' stream, the device copies of the columns and the recycled scratch. One column call at a
// time (mu); sgpu_index_set_column takes mu too, so it never frees a copy under a running kernel.
struct ColumnState {
  int device = -1;
  uint32_t n_cu = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr, ev2 = nullptr;
  std::mutex mu;
  DeviceBuffer col[SGPU_MAX_COLUMNS];          // the copies; col_gen: the HostColumn::generation each was made from (0: none)
  uint64_t col_gen[SGPU_MAX_COLUMNS] = {};
  DeviceBuffer f_clauses, f_keys, f_within, f_bits, f_count;   // filter: the plan, `within`'s words, the result
  DeviceBuffer c_bits, c_table, c_rows;                        // facets: the filter's words, the table, the rows
  DeviceBuffer a_bits, a_parts, a_edges, a_table;              // stats / histogram: the filter's words, the tiles' partials, edge keys, bins
  DeviceBuffer t_state, t_hist, t_waves, t_comps, t_rows;      // top: select state, radix bins, the wavefronts' equals, composites, rows
  // what the last launches measured (sgpu_debug_column_stats)
  float filter_ms = 0, facet_ms = 0, facet_count_ms = 0, facet_select_ms = 0;   // facet_ms: both facet kernels
  uint32_t filter_grid = 0, facet_grid = 0, facet_docs_per_wg = 0, facet_path = 0;
  // (sgpu_debug_column_agg_stats)
  float stats_ms = 0, hist_ms = 0, top_ms = 0;
  uint32_t stats_grid = 0, hist_grid = 0, top_grid = 0, hist_docs_per_wg = 0, top_docs_per_wg = 0, top_passes = 0;
};

// Waits for the stream when a call leaves, also on an error: the copies it enqueued read host memory of the call and of
// the index's columns, which are the next set_column's to replace once the mutex is free.
struct StreamDrain {
  hipStream_t s;
  ~StreamDrain() { (void)hipStreamSynchronize(s); }
};

// column_filter.hip: the replica's state, made on its first column call; the replica's copy of column `slot`, made or made
// again where the host column is of another generation (s->mu held; the copy is enqueued on s->stream)
sgpu_status column_state_of(sgpu_index* idx, uint32_t replica, ColumnState** out);
sgpu_status column_device_copy(ColumnState* s, const sgpu_index* idx, uint32_t slot, const uint32_t** out);

}  // namespace sgpu
#endif
