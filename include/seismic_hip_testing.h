/* seismic_hip_testing.h - TEST HOOKS of libseismic_hip.so. Not part of the drop-in boundary (that is seismic_hip.h):
 * these entry points let tests/ and tools/ look at host-side decisions of the library. They are inert unless the
 * environment has SGPU_TEST_HOOKS=1 (as tests/conftest.py sets it): the status-returning ones then fail with
 * SGPU_EINVAL, the others return 0. The undocumented SGPU_* environment names obey the
 * same switch. */
#ifndef SEISMIC_HIP_TESTING_H
#define SEISMIC_HIP_TESTING_H
#include "seismic_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* team size a host-parallel phase takes for num_threads == 0 (hardware threads capped by the cgroup CPU quota) */
uint32_t sgpu_debug_host_threads(void);
/* the smallest chunk and the most chunks sgpu_batch_search cuts a call into, as this process applies them: out2 =
 * {chunk_min, chunk_max} for a call that shares its replica with other calls (shared != 0) or not, and whose chunks the
 * device would plan (device_plans != 0) or not - SGPU_CHUNK_MIN / SGPU_CHUNK_MAX as the process read them once, else the
 * rule (seismic_amd/csrc/call_cut.cpp). Needs no index and no device */
sgpu_status sgpu_debug_cut_rule(uint32_t shared, uint32_t device_plans, uint32_t* out2);
/* how sgpu_batch_search cuts a call of nq queries into launches (call_cut.cpp: cut_segment, with equal chunks): bounds[2j],
 * bounds[2j+1] = queries [q0, q1) of launch j */
uint32_t sgpu_debug_chunk_bounds(uint32_t nq, uint32_t chunk_min, uint32_t chunk_max, uint32_t lanes_free, uint32_t* bounds);
/* the same for a call of any size (more than 8 x 16384 queries are served in segments, one after the other): every launch
 * of the call in order, at most cap of them written; first_pm: the first chunk's share in per mille (0: equal chunks) */
uint32_t sgpu_debug_call_bounds(uint32_t nq, uint32_t chunk_min, uint32_t chunk_max, uint32_t lanes_free, uint32_t first_pm,
                                uint32_t* bounds, uint32_t cap);
/* the last chunk pool lane `lane` (0 ... 7) of replica 0 served: info4 = {queries, first query in the call's batch, planned by
 * 0 the host / 1 the device / 2 nobody (input order), query_cut}; host-planned: its launch order as it went down. 0: none */
uint32_t sgpu_debug_lane_chunk(sgpu_index* idx, uint32_t lane, uint32_t* info4, uint32_t* order_out, uint32_t cap);
/* the forward store as sgpu_index_upload packs it (document-major records) and every document's ref */
sgpu_status sgpu_debug_pack_forward(const sgpu_index* idx, uint8_t* out_fwd, uint64_t cap, uint64_t* out_doc_ref,
                                    uint64_t* out_bytes);
/* the hashed row directory as sgpu_index_upload builds it (4 words per slot, 4 slots per bucket); *n_buckets == 0: none */
sgpu_status sgpu_debug_row_dir(const sgpu_index* idx, uint32_t* out, uint64_t cap_words, uint64_t* n_words, uint32_t* n_buckets);
/* the launch plan of a batch: processing order, out3 = {block dots needed at most, largest first list, largest list} */
sgpu_status sgpu_debug_plan(const sgpu_index* idx, const uint64_t* q_off, const uint32_t* comps, const float* vals,
                            uint32_t nq, uint32_t query_cut, uint32_t* order_out, uint32_t* out3);
/* the hashed-lookup half of that plan (no device; the same code path as sgpu_debug_plan): *out_hash_ok = 1 when a launch of
 * this batch may take the hashed query lookup - the index has u32 components, f16 values and dim < 2^24, SGPU_NO_HASH is not
 * set, and EVERY query has a seed: the first of 64 multipliers that sends its components (at most 1024 of them) to distinct
 * slots of the 4096-slot table. seeds_out[q], nq words: that seed, 0 ... 63. The search stops at the first query without a
 * seed: its entry holds 64 & 63 = 0, the entries of the queries after it were never computed and hold 0 as well, and
 * *out_hash_ok = 0 - the entries before it are real seeds. All entries are 0 where the index is not of that form */
sgpu_status sgpu_debug_plan_seeds(const sgpu_index* idx, const uint64_t* q_off, const uint32_t* comps, const float* vals,
                                  uint32_t nq, uint32_t query_cut, uint32_t* out_hash_ok, uint32_t* seeds_out);
/* the kernel variant of the last search launch of a lane of `replica`: lane < 0 its main lane (sgpu_batch_run /
 * sgpu_batch_run_counted and the calls built on them), else chunk pool lane `lane` (0 ... 7, as sgpu_debug_lane_chunk counts
 * them). out4 = {query lookup layout: 0 packed / 1 dense / 2 split / 3 hashed, streamed stage 2, cooperative: 0 / 1 / 2
 * forced, counted pass} - the words [34], [38], [40], [37] of sgpu_debug_launch_config. Recorded once the launch has been
 * enqueued successfully; a summary-distances (dots) launch and a launch that failed leave the words of the search launch
 * before it. 0: the lane has launched no search yet, or is serving a call */
uint32_t sgpu_debug_lane_variant(sgpu_index* idx, uint32_t replica, int32_t lane, uint32_t* out4);
/* the same plan as the DEVICE computes it for staged chunks (needs an uploaded index; 1 ... 16384 queries, query_cut 1 ... 16) */
sgpu_status sgpu_debug_device_plan(sgpu_index* idx, const uint64_t* q_off, const uint32_t* comps, const float* vals,
                                   uint32_t nq, uint32_t query_cut, uint32_t* order_out, uint32_t* out3);
/* the launch configuration of a search pass, as the library's pure function decides it; needs no index and no device. The
 * SGPU_* names are read from the environment as a launch reads them. n_in must be 23, n_out 58.
 * in:  [0] n_cu [1] LDS bytes per workgroup [2] comp_width [3] value_type [4] dim [5] val_scale (float bits)
 *      [6] cooperative variant switched off for the replica [7] nq [8] longest query [9] k_max [10] staged batch
 *      [11] 1 = a launch plan follows / 0 = none [12] block dots a query needs at most [13] largest first list
 *      [14] largest list [15] every query has a hash seed [16] MODE_DOTS: blocks of the target list
 *      [17] k [18] query_cut [19] n_knn [20] first_sorted [21] mode (0 search, 1 dots, 2 counted)
 *      [22] workgroups the occupancy query allows, n_cu x workgroups per CU (0: no grid wanted)
 * out: [0..19] the LDS layout: byte offsets q_comp q_val q_sc q_bits q_rank sel rt_start rt_mid rt_pre dots order uni part
 *      heap st, then qc qn qg dots_cap total  [20..33] the kernel parameters: k query_cut heap_factor first_sorted mode
 *      items_max items_init items_min rblocks_max n_knn target_list val_scale queue_base ring
 *      [34] lookup [35] workgroup size [36] LDS bytes [37] counted [38] streamed [39] ring [40] cooperative: 0 / 1 / 2 forced
 *      [41..49] max_pos max_cand chunk chunk_min min_items first_reach idle_min idle_ratio poll_sleep
 *      [50] most workgroups of an unforced cooperative launch (0: every slot) [51] grid [52] cooperative grid before the
 *      board's 512 slots cap it [53..57] the board's byte offsets: slots pos cand trace total */
sgpu_status sgpu_debug_launch_config(const uint32_t* in, uint32_t n_in, float heap_factor, uint32_t* out, uint32_t n_out);
/* the calling thread's staged calls add their host-side phase times to buf8[0..7] from now on (NULL: off) */
void sgpu_debug_call_timing(double* buf8);
/* timeline of the last cooperative launch (trace builds) */
uint32_t sgpu_debug_coop_trace(sgpu_index* idx, uint64_t* out, uint32_t cap);
/* what the last sgpu_score_documents / sgpu_rerank_documents call on `replica` measured: out8 = {device ms of its score
 * kernels (HIP events), launches, 1 = dense weight table / 0 = hash table, grid, workgroup size, LDS bytes, device ms of
 * the selection kernels (0 for a score call), merge rounds the selection ran after its chunk round, summed over the
 * call's launches}; SGPU_EINVAL before the first call */
sgpu_status sgpu_debug_score_stats(sgpu_index* idx, uint32_t replica, double* out8);
/* what the last sgpu_expand_queries call on `replica` measured: out8 = {device ms of its kernels (HIP events), launches,
 * 1 = the table in LDS / 0 = in global memory, grid of its last launch, workgroup size, LDS bytes, bytes of the global
 * tables (0 with the table in LDS), 0}; SGPU_EINVAL before the replica's first score or expand call */
sgpu_status sgpu_debug_expand_stats(sgpu_index* idx, uint32_t replica, double* out8);
/* what the last sgpu_diversify_documents call on `replica` measured: out8 = {device ms of its kernels (HIP events),
 * launches, grid of its last launch, workgroup size, LDS bytes (table + entry state), 1 = dense table / 0 = hash, rounds of
 * its longest query, 0}; SGPU_EINVAL before the replica's first score call. The environment name SGPU_DIVERSIFY_GRID, read
 * per call and honoured under the same switch, lowers the grid (each workgroup then takes many queries in turn) */
sgpu_status sgpu_debug_diversify_stats(sgpu_index* idx, uint32_t replica, double* out8);
/* what the last sgpu_collapse_documents call on `replica` measured: out8 = {device ms of its score kernels (HIP events),
 * launches, 1 = dense weight table / 0 = hash table, grid, workgroup size and LDS bytes of the score kernel's last launch,
 * device ms of the selection kernels, selection kernel launches (one per tier of list lengths - up to 128, 512, 1024 and
 * 4096 entries - that a launch has a query in)}; SGPU_EINVAL before the replica's first score call. The environment name
 * SGPU_COLLAPSE_GRID, read per call and honoured under the same switch, lowers the selection's grid (each workgroup then
 * takes many queries in turn) */
sgpu_status sgpu_debug_collapse_stats(sgpu_index* idx, uint32_t replica, double* out8);
/* what the last sgpu_fuse_documents call on `replica` measured: out8 in the slot order of sgpu_debug_collapse_stats (the
 * tiers of list lengths are the same); SGPU_EINVAL before the replica's first score call. The environment name
 * SGPU_FUSE_GRID, read per call and honoured under the same switch, lowers the selection's grid (each workgroup then takes
 * many queries in turn) */
sgpu_status sgpu_debug_fuse_stats(sgpu_index* idx, uint32_t replica, double* out8);
/* the accumulate launches of the last sgpu_exact_search_device[_filtered] call on `replica`: one per chunk of queries whose
 * candidates (n_ranges x k x 8 bytes per query) fit the candidate buffer of 256 MiB; the environment name
 * SGPU_EXACT_CAND_BYTES, read per call and honoured under the same switch, lowers that size. SGPU_EINVAL before the
 * replica's first exact call (0 launches when only sgpu_filter_create_terms has built the replica's exact file so far) */
sgpu_status sgpu_debug_exact_launches(sgpu_index* idx, uint32_t replica, uint32_t* out_launches);
/* {kernel ms of the last sgpu_filter_create_terms call on `replica` (HIP events around its one kernel), wall ms of the
 * build of the replica's exact file, the file's bytes, its ranges of 32768 documents = workgroups of the kernel}.
 * SGPU_EINVAL before the replica has an exact file */
sgpu_status sgpu_debug_term_filter_stats(sgpu_index* idx, uint32_t replica, double* out4);
/* the column calls of `replica`: out8 = {kernel ms of the last sgpu_filter_create_columns launch, kernel ms of the last
 * sgpu_facet_counts call (its count and select kernels together; HIP events), grid of the filter kernel, grid of the facet
 * count kernel, documents per workgroup of the filter kernel (a constant: 8192), documents per workgroup of the facet count
 * kernel, the facet path that ran (0 = LDS histograms, 1 = global atomics), bytes of the replica's column copies}.
 * SGPU_EINVAL before the replica's first column call */
sgpu_status sgpu_debug_column_stats(sgpu_index* idx, uint32_t replica, double* out8);
/* out2 = {count kernel ms, select kernel ms} of the last sgpu_facet_counts call on `replica`: the two parts of out8[1] above */
sgpu_status sgpu_debug_facet_kernel_ms(sgpu_index* idx, uint32_t replica, double* out2);
/* the column aggregations of `replica`: out10 = {kernel ms of the last sgpu_column_stats call, of the last
 * sgpu_column_histogram call, of the last sgpu_column_top call (all its kernels; HIP events), the grid of the stats
 * kernel (one workgroup per tile), of the histogram kernel, of the top call's select and emit kernels, the documents of a
 * tile of the canonical sum (a constant: 16384), the select passes the last top call ran (0 where the filter holds at most
 * t documents, else 4), the documents per workgroup of the last histogram call and of the last top call}.
 * SGPU_EINVAL before the replica's first column call */
sgpu_status sgpu_debug_column_agg_stats(sgpu_index* idx, uint32_t replica, double* out10);
/* the posting arrays a search on `replica` walks, read back from the device: the replica's own (filter == NULL) or those of
 * the filter's view there, which is obtained as a search obtains it - built on first use or after a new upload or graph,
 * under the filter's mutex; no second build path. sizes5 = {block starts (n_blocks + 1), postings, kNN ids (0: no graph),
 * bitmap words, allowed documents} - the last two 0 without a filter. A NULL buffer is skipped (all NULL: the sizes only); a
 * buffer whose capacity (in elements; post_ref and post_doc share cap_postings) is below its array's size: SGPU_EINVAL.
 * SGPU_EDEVICE when the index is not uploaded or the replica is out of range. One blocking copy per array, no state kept. */
sgpu_status sgpu_debug_posting_view(sgpu_index* idx, const sgpu_filter* filter, uint32_t replica, uint32_t* out_block_post_start,
                                    uint64_t cap_starts, uint64_t* out_post_ref, uint32_t* out_post_doc, uint64_t cap_postings,
                                    uint32_t* out_knn, uint64_t cap_knn, uint32_t* out_bits, uint64_t cap_bits, uint64_t* sizes5);

#ifdef __cplusplus
}
#endif
#endif /* SEISMIC_HIP_TESTING_H */
