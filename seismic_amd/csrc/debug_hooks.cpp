// debug_hooks.cpp — the test hooks declared in include/seismic_hip_testing.h; NOT part of the boundary (that is abi.cpp).
// Entry points the test suite and the tools use to look at host-side decisions (team size, chunk plan, launch plan,
// packed records, phase clocks, cooperative trace). Like the undocumented environment names they are inert unless
// SGPU_TEST_HOOKS=1 is set: status-returning ones fail with SGPU_EINVAL, the others return 0 / do nothing.
#include <algorithm>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/seismic_hip_testing.h"
#include "call_cut.hpp"
#include "columns.hpp"
#include "device_calls.hpp"
#include "filter.hpp"
#include "host_index.hpp"
#include "launch_config.hpp"
#include "term_filter.hpp"

using namespace sgpu;

#define SGPU_HOOK_OR(ret)                                                                            \
  if (!test_hooks_on()) {                                                                            \
    (void)fail(SGPU_EINVAL, "%s is a test hook: set SGPU_TEST_HOOKS=1 (include/seismic_hip_testing.h)", __func__); \
    return ret;                                                                                      \
  }

// What the last call of some kind on `replica` measured, for the hooks that report it: `get` fills `out` from the replica's
// state, or says that no such call has run there yet.
template <class T>
static sgpu_status last_call(bool (*get)(sgpu_index*, uint32_t, T*), sgpu_index* idx, uint32_t replica, T* out, const char* noun) {
  if (!idx || !out) return fail(SGPU_EINVAL, "null argument");
  if (!get(idx, replica, out)) return fail(SGPU_EINVAL, "no %s call has run on replica %u", noun, replica);
  return SGPU_OK;
}

extern "C" {

// (the team size a host-parallel phase would take for num_threads == 0)
uint32_t sgpu_debug_host_threads(void) {
  SGPU_HOOK_OR(0u);
  return (uint32_t)host_threads();
}

// (not part of the boundary: the smallest chunk and the most chunks of a call - out2 = {chunk_min, chunk_max} - as this
// process applies them to a call that shares its replica with others or not, whose chunks the device would plan or not:
// SGPU_CHUNK_MIN / SGPU_CHUNK_MAX as read once, else the rule. Needs no index and no device)
sgpu_status sgpu_debug_cut_rule(uint32_t shared, uint32_t device_plans, uint32_t* out2) {
  SGPU_HOOK_OR(SGPU_EINVAL);
  if (!out2) return fail(SGPU_EINVAL, "null argument");
  const CutRule r = cut_rule(cut_knobs(), shared != 0, device_plans != 0);
  out2[0] = r.chunk_min, out2[1] = r.chunk_max;
  return SGPU_OK;
}

// (not part of the boundary: how search_segment would cut a call of nq queries when `lanes_free` lanes can be had -
// bounds[2 * j], bounds[2 * j + 1] = the queries [q0, q1) of launch j; returns the number of launches)
uint32_t sgpu_debug_chunk_bounds(uint32_t nq, uint32_t chunk_min, uint32_t chunk_max, uint32_t lanes_free, uint32_t* bounds) {
  SGPU_HOOK_OR(0u);
  return cut_segment(nq, chunk_min, chunk_max, lanes_free, 0, reinterpret_cast<uint32_t(*)[2]>(bounds));
}

// (the same for a call of any size: its segments one after the other, each cut as above - every launch of the call in
// order; at most `cap` launches are written, the number there are is returned)
uint32_t sgpu_debug_call_bounds(uint32_t nq, uint32_t chunk_min, uint32_t chunk_max, uint32_t lanes_free, uint32_t first_pm,
                                uint32_t* bounds, uint32_t cap) {
  SGPU_HOOK_OR(0u);
  return cut_call(nq, chunk_min, chunk_max, lanes_free, first_pm, bounds, cap);
}

// (the last chunk pool lane `lane` of replica 0 served: who planned it and, host-planned, the order it went down with -
// staged.hip debug_lane_chunk; tests/test_gpu_entry_chunks.py)
uint32_t sgpu_debug_lane_chunk(sgpu_index* idx, uint32_t lane, uint32_t* info4, uint32_t* order_out, uint32_t cap) {
  SGPU_HOOK_OR(0u);
  if (!idx || !idx->dev || !info4) return 0u;
  return debug_lane_chunk(idx->dev, lane, info4, order_out, cap);
}

// (not part of the boundary: the forward store as sgpu_index_upload packs it - document-major records - and the ref
// of every document, (record offset / 16) << 16 | length field; out_fwd == null: *out_bytes = the size needed.
// tests/test_abi_and_host.py decodes every record with the oracle's restatement of the layout.)
sgpu_status sgpu_debug_pack_forward(const sgpu_index* idx, uint8_t* out_fwd, uint64_t cap, uint64_t* out_doc_ref, uint64_t* out_bytes) {
  SGPU_HOOK_OR(SGPU_EINVAL);
  if (!idx || !out_bytes) return fail(SGPU_EINVAL, "null argument");
  try {
    std::vector<uint8_t> raw, fwd;
    std::vector<uint64_t> off16, dref;
    pack_dvb_raw_flags(idx->host, &raw);
    pack_record_offsets(idx->host, raw, 128 / 16, &off16);
    *out_bytes = std::max<uint64_t>(off16[idx->host.n_docs] * 16, 16);
    if (!out_fwd) return SGPU_OK;
    if (cap < *out_bytes || !out_doc_ref) return fail(SGPU_EINVAL, "buffer too small");
    pack_records(idx->host, raw, off16, &fwd);
    pack_doc_refs(idx->host, raw, off16, &dref);
    std::memcpy(out_fwd, fwd.data(), fwd.size());
    std::memcpy(out_doc_ref, dref.data(), dref.size() * 8);
  } catch (const std::bad_alloc&) {
    return fail(SGPU_ENOMEM, "out of host memory");
  }
  return SGPU_OK;
}

// (the hashed row directory as sgpu_index_upload builds it: 4 words per slot, 4 slots per bucket; out == null: *n_words
// and *n_buckets only. *n_buckets == 0: this index gets none)
sgpu_status sgpu_debug_row_dir(const sgpu_index* idx, uint32_t* out, uint64_t cap_words, uint64_t* n_words, uint32_t* n_buckets) {
  SGPU_HOOK_OR(SGPU_EINVAL);
  if (!idx || !n_words || !n_buckets) return fail(SGPU_EINVAL, "null argument");
  try {
    std::vector<uint16_t> mid;
    std::vector<uint32_t> dir;
    pack_row_mid(idx->host, &mid);
    *n_buckets = 0;
    if (!pack_row_dir(idx->host, mid, &dir, n_buckets)) *n_buckets = 0;
    *n_words = dir.size();
    if (!out) return SGPU_OK;
    if (cap_words < dir.size()) return fail(SGPU_EINVAL, "buffer too small");
    std::memcpy(out, dir.data(), dir.size() * 4);
  } catch (const std::bad_alloc&) {
    return fail(SGPU_ENOMEM, "out of host memory");
  }
  return SGPU_OK;
}

// (not part of the boundary: the launch plan of a batch - processing order (longest expected first), out3 = {block dots a
// query needs at most, largest list walked first, largest list walked}; needs no device)
sgpu_status sgpu_debug_plan(const sgpu_index* idx, const uint64_t* q_off, const uint32_t* comps, const float* vals, uint32_t nq,
                            uint32_t query_cut, uint32_t* order_out, uint32_t* out3) {
  SGPU_HOOK_OR(SGPU_EINVAL);
  if (!idx || !q_off || !order_out || !out3) return fail(SGPU_EINVAL, "null argument");
  return debug_plan(idx->host, q_off, comps, vals, nq, query_cut, order_out, out3);
}

// (not part of the boundary: the LK_HASH half of the same plan, through the same debug_plan / make_plan - *out_hash_ok = every
// query has a collision-free seed and the index is of the hashed family (u32 components, f16 values, dim < 2^24, no
// SGPU_NO_HASH); seeds_out[q] = the query's seed. The search stops at the first query without one: that query's entry is
// 64 & 63 = 0 and the entries after it were never computed, 0 too; all 0 when the index is not of the family. No device)
sgpu_status sgpu_debug_plan_seeds(const sgpu_index* idx, const uint64_t* q_off, const uint32_t* comps, const float* vals, uint32_t nq,
                                  uint32_t query_cut, uint32_t* out_hash_ok, uint32_t* seeds_out) {
  SGPU_HOOK_OR(SGPU_EINVAL);
  if (!idx || !q_off || !out_hash_ok || !seeds_out) return fail(SGPU_EINVAL, "null argument");
  uint32_t out3[3];
  return debug_plan(idx->host, q_off, comps, vals, nq, query_cut, nullptr, out3, out_hash_ok, seeds_out);
}

// (not part of the boundary: the kernel variant of the last search launch of a lane of `replica` - lane < 0: its main lane,
// else chunk pool lane `lane`, as sgpu_debug_lane_chunk counts them - batch.hip debug_lane_variant)
uint32_t sgpu_debug_lane_variant(sgpu_index* idx, uint32_t replica, int32_t lane, uint32_t* out4) {
  SGPU_HOOK_OR(0u);
  if (!idx || !out4 || replica >= idx->replicas.size()) return 0u;
  return debug_lane_variant(idx->replicas[replica], lane, out4);
}

// (not part of the boundary: the same plan as the DEVICE computes it for staged chunks - plan_kernel.hip; replica 0)
sgpu_status sgpu_debug_device_plan(sgpu_index* idx, const uint64_t* q_off, const uint32_t* comps, const float* vals, uint32_t nq,
                                   uint32_t query_cut, uint32_t* order_out, uint32_t* out3) {
  SGPU_HOOK_OR(SGPU_EINVAL);
  if (!idx || !q_off || !order_out || !out3) return fail(SGPU_EINVAL, "null argument");
  return debug_device_plan(idx->dev, q_off, comps, vals, nq, query_cut, order_out, out3);
}

// (not part of the boundary: the launch configuration - launch_config.cpp - of a launch described by 23 words and
// heap_factor, as 58 words; the knobs come from the environment as a launch reads them. Needs no index and no device)
sgpu_status sgpu_debug_launch_config(const uint32_t* in, uint32_t n_in, float heap_factor, uint32_t* out, uint32_t n_out) {
  SGPU_HOOK_OR(SGPU_EINVAL);
  if (!in || !out) return fail(SGPU_EINVAL, "null argument");
  return debug_launch_config(in, n_in, heap_factor, out, n_out);
}

// (not part of the boundary: the calling thread's staged calls add the wall time of their host-side phases to
// buf[0..7] from now on - see staged.hip: call_timing; null switches it off. tools/shard_probe.py)
void sgpu_debug_call_timing(double* buf8) {
  SGPU_HOOK_OR();
  call_timing() = buf8;
}

// (not part of the boundary: the timeline of a cooperative launch, for tools/coop_trace.py on a trace build)
uint32_t sgpu_debug_coop_trace(sgpu_index* idx, uint64_t* out, uint32_t cap) {
  SGPU_HOOK_OR(0u);
  return idx ? coop_trace_dump(idx->dev, out, cap) : 0;
}

// (not part of the boundary: what the last sgpu_fuse_documents call on `replica` measured - out8 in the slot order of
// sgpu_debug_collapse_stats; SGPU_EINVAL before the replica's first score call. tools/fuse_probe.py)
sgpu_status sgpu_debug_fuse_stats(sgpu_index* idx, uint32_t replica, double* out8) {
  SGPU_HOOK_OR(SGPU_EINVAL);
  return last_call(fuse_debug_stats, idx, replica, out8, "fuse");
}

// (not part of the boundary: what the last sgpu_collapse_documents call on `replica` measured - out8 = {device ms of its score
// kernels, launches, 1 = dense table / 0 = hash table, grid, workgroup size and LDS bytes of the score kernel, device ms of the
// selection kernels, selection kernel launches}; SGPU_EINVAL before the replica's first score call. tools/collapse_probe.py)
sgpu_status sgpu_debug_collapse_stats(sgpu_index* idx, uint32_t replica, double* out8) {
  SGPU_HOOK_OR(SGPU_EINVAL);
  return last_call(collapse_debug_stats, idx, replica, out8, "collapse");
}

// (not part of the boundary: what the last sgpu_diversify_documents call on `replica` measured - out8 = {device ms of its
// kernels, launches, grid of the last launch, workgroup size, LDS bytes, 1 = dense table / 0 = hash, rounds of its longest
// query, 0}; SGPU_EINVAL before the replica's first score call. tools/diversify_probe.py)
sgpu_status sgpu_debug_diversify_stats(sgpu_index* idx, uint32_t replica, double* out8) {
  SGPU_HOOK_OR(SGPU_EINVAL);
  return last_call(diversify_debug_stats, idx, replica, out8, "diversify");
}

// (not part of the boundary: what the last sgpu_expand_queries call on `replica` measured - out8 = {device ms of its kernels,
// launches, 1 = table in LDS / 0 = in global memory, grid of the last launch, workgroup size, LDS bytes, bytes of the
// global tables, 0}; SGPU_EINVAL before the replica's first score or expand call. tools/expand_probe.py)
sgpu_status sgpu_debug_expand_stats(sgpu_index* idx, uint32_t replica, double* out8) {
  SGPU_HOOK_OR(SGPU_EINVAL);
  return last_call(expand_debug_stats, idx, replica, out8, "expand");
}

// (not part of the boundary: what the last sgpu_score_documents / sgpu_rerank_documents / sgpu_explain_documents call on `replica` measured - out8 =
// {device ms of its score kernels, launches, 1 = dense table / 0 = hash table, grid, workgroup size, LDS bytes, device ms of
// the selection kernels, merge rounds}; SGPU_EINVAL before the replica's first score call. tools/score_probe.py,
// tools/rerank_probe.py)
sgpu_status sgpu_debug_score_stats(sgpu_index* idx, uint32_t replica, double* out8) {
  SGPU_HOOK_OR(SGPU_EINVAL);
  return last_call(score_debug_stats, idx, replica, out8, "score");
}

// (not part of the boundary: the accumulate launches of the last sgpu_exact_search_device[_filtered] call on `replica`, one
// per chunk of queries whose candidates fit the candidate buffer - 256 MiB, or what SGPU_EXACT_CAND_BYTES says; SGPU_EINVAL
// before the replica's first exact call. tests/test_gpu_exact_edges.py)
sgpu_status sgpu_debug_exact_launches(sgpu_index* idx, uint32_t replica, uint32_t* out_launches) {
  SGPU_HOOK_OR(SGPU_EINVAL);
  return last_call(exact_debug_launches, idx, replica, out_launches, "exact");
}

// (not part of the boundary: {kernel ms of the last sgpu_filter_create_terms call on `replica`, wall ms of the build of the
// exact file there, the file's bytes, its ranges}; SGPU_EINVAL before the replica has an exact file. tools/term_filter_probe.py)
sgpu_status sgpu_debug_term_filter_stats(sgpu_index* idx, uint32_t replica, double* out4) {
  SGPU_HOOK_OR(SGPU_EINVAL);
  if (!idx || !out4) return fail(SGPU_EINVAL, "null argument");
  if (!term_filter_debug_stats(idx, replica, out4)) return fail(SGPU_EINVAL, "replica %u has no exact file", replica);
  return SGPU_OK;
}

// (not part of the boundary: the column calls of `replica` - out8 = {kernel ms of the last column-filter launch, kernel ms of the
// last facet call, the grid of each, the documents per workgroup of each, the facet path (0 LDS, 1 global), bytes of the
// replica's column copies}; SGPU_EINVAL before the replica's first column call. tools/column_probe.py)
sgpu_status sgpu_debug_column_stats(sgpu_index* idx, uint32_t replica, double* out8) {
  SGPU_HOOK_OR(SGPU_EINVAL);
  return last_call(column_debug_stats, idx, replica, out8, "column");
}

// (not part of the boundary: {count kernel ms, select kernel ms} of the last sgpu_facet_counts call on `replica` - the two
// parts of out8[1] above; SGPU_EINVAL before the replica's first column call. tools/column_probe.py)
sgpu_status sgpu_debug_facet_kernel_ms(sgpu_index* idx, uint32_t replica, double* out2) {
  SGPU_HOOK_OR(SGPU_EINVAL);
  return last_call(facet_debug_kernel_ms, idx, replica, out2, "column");
}

// (not part of the boundary: the column aggregations of `replica` - out10 = {kernel ms of the last sgpu_column_stats /
// _histogram / _top call, the grid of each (top: of its select and emit kernels), kAggTile, the select passes the last top
// call ran, the documents per workgroup of the last histogram and top call}; SGPU_EINVAL before the replica's first column
// call. tools/column_agg_probe.py)
sgpu_status sgpu_debug_column_agg_stats(sgpu_index* idx, uint32_t replica, double* out10) {
  SGPU_HOOK_OR(SGPU_EINVAL);
  return last_call(column_agg_debug_stats, idx, replica, out10, "column");
}

// (not part of the boundary: device and wall milliseconds of the build of the filter's view on `replica`; SGPU_EINVAL
// before it is built. tools/filter_probe.py)
sgpu_status sgpu_debug_filter_build_times(const sgpu_filter* filter, uint32_t replica, double* out2) {
  SGPU_HOOK_OR(SGPU_EINVAL);
  if (!filter || !out2) return fail(SGPU_EINVAL, "null argument");
  if (!filter_build_times(filter, replica, out2)) return fail(SGPU_EINVAL, "the filter has no view on replica %u", replica);
  return SGPU_OK;
}

// (not part of the boundary: the posting arrays a search on `replica` walks, read back from the device - the replica's own
// (filter == null) or those of the filter's view there, built as a search builds it on first use (filter.hip:
// debug_posting_view). tests/test_gpu_filter_view.py compares all of them with a numpy compaction)
sgpu_status sgpu_debug_posting_view(sgpu_index* idx, const sgpu_filter* filter, uint32_t replica, uint32_t* out_block_post_start,
                                    uint64_t cap_starts, uint64_t* out_post_ref, uint32_t* out_post_doc, uint64_t cap_postings,
                                    uint32_t* out_knn, uint64_t cap_knn, uint32_t* out_bits, uint64_t cap_bits, uint64_t* sizes5) {
  SGPU_HOOK_OR(SGPU_EINVAL);
  if (!idx || !sizes5) return fail(SGPU_EINVAL, "null argument");
  const sgpu_status st = foreign_filter(idx, filter);
  if (st != SGPU_OK) return st;
  return debug_posting_view(idx, filter, replica, out_block_post_start, cap_starts, out_post_ref, out_post_doc, cap_postings,
                            out_knn, cap_knn, out_bits, cap_bits, sizes5);
}

}  // extern "C"
