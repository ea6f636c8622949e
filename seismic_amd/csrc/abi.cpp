// abi.cpp — the extern "C" surface declared in include/seismic_hip.h.
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "host_index.hpp"
#include "term_filter.hpp"

struct sgpu_batch;

namespace sgpu {
// device_index.hip (residency, lanes), launch_plan.hip, batch.hip, staged.hip
struct Lane;
sgpu_status device_index_upload(const HostIndex& h, int device, DeviceIndex** out);
sgpu_status device_index_clone(const DeviceIndex* src, int device, DeviceIndex** out);
void device_index_free(DeviceIndex* d);
uint64_t device_index_bytes(const DeviceIndex* d);
Lane* lane_acquire(DeviceIndex* d);
Lane* lane_try_acquire(DeviceIndex* d);
bool call_enter(DeviceIndex* d);
void call_exit(DeviceIndex* d);
void lane_release(DeviceIndex* d, Lane* l);
Lane* lane_main(DeviceIndex* d);
sgpu_batch** lane_scratch(Lane* l);
sgpu_status batch_create(DeviceIndex* d, Lane* lane, uint64_t dim, const uint64_t* q_off, const uint32_t* comps,
                         const float* vals, uint32_t nq, uint32_t k_max, sgpu_batch** out);
void batch_free(sgpu_batch* b);
sgpu_status batch_run(DeviceIndex* d, Lane* lane, sgpu_batch* b, const sgpu_search_params& sp, uint32_t mode,
                      int sync, sgpu_launch_stats* stats);
sgpu_status batch_sync(DeviceIndex* d, sgpu_launch_stats* stats);
sgpu_status batch_fetch(DeviceIndex* d, Lane* lane, sgpu_batch* b, uint32_t k, float* out_scores, uint64_t* out_ids,
                        uint32_t* out_n);
sgpu_status batch_fetch_stats(DeviceIndex* d, sgpu_batch* b, uint32_t* out);
sgpu_status staged_launch(DeviceIndex* d, Lane* lane, uint64_t dim, const uint64_t* q_off, const uint32_t* comps,
                          const float* vals, uint32_t nq, uint32_t q_base, const sgpu_search_params& sp, sgpu_batch** slot,
                          uint32_t followed,    // (0: nothing behind this chunk; 1: other calls; 2: the call's own next chunk)
                          const FilterRef* flt, uint32_t chunk);   // (chunk: which launch of its call, 0 = the first or only one)
sgpu_status staged_finish(DeviceIndex* d, Lane* lane, sgpu_batch* b, float* out_scores, uint64_t* out_ids, uint32_t* out_n);
sgpu_status summary_distances(DeviceIndex* d, const HostIndex& h, uint32_t list, const uint32_t* comps,
                              const float* vals, uint32_t nnz, float* out_dots, uint32_t* out_nb);
int device_count();
double*& call_timing();
uint32_t device_plan_dots(DeviceIndex* d, const sgpu_search_params& sp, uint32_t nq, uint32_t cut);
sgpu_status debug_device_plan(DeviceIndex* d, const uint64_t* q_off, const uint32_t* comps, const float* vals, uint32_t nq,
                              uint32_t query_cut, uint32_t* order_out, uint32_t* out3);
sgpu_status debug_plan(const HostIndex& h, const uint64_t* q_off, const uint32_t* comps, const float* vals, uint32_t nq,
                       uint32_t query_cut, uint32_t* order_out, uint32_t* out3);
uint32_t coop_trace_dump(DeviceIndex* d, uint64_t* out, uint32_t cap);
uint32_t debug_lane_chunk(DeviceIndex* d, uint32_t lane, uint32_t* info4, uint32_t* order_out, uint32_t cap);
const DeviceIndex* batch_replica(const sgpu_batch* b);
sgpu_status device_index_set_knn(DeviceIndex* d, const std::vector<uint32_t>& knn, uint32_t knn_dim);
sgpu_status build_knn_on_device(DeviceIndex* d, HostIndex& h, uint32_t nknn);
// launch_config.cpp
sgpu_status debug_launch_config(const uint32_t* in, uint32_t n_in, float heap_factor, uint32_t* out, uint32_t n_out);
// exact_device.hip
sgpu_status exact_search_device(sgpu_index* idx, uint32_t replica, const uint64_t* q_off, const uint32_t* comps,
                                const float* vals, uint32_t nq, uint32_t k, float* out_scores, uint64_t* out_ids,
                                uint32_t* out_n, const sgpu_filter* filter);
bool exact_debug_launches(sgpu_index* idx, uint32_t replica, uint32_t* out);
// score_documents.hip
sgpu_status score_documents_device(sgpu_index* idx, uint32_t replica, const uint64_t* q_off, const uint32_t* comps,
                                   const float* vals, uint32_t nq, const uint64_t* cand_off, const uint64_t* cand_ids,
                                   float* out_scores);
sgpu_status rerank_documents_device(sgpu_index* idx, uint32_t replica, const uint64_t* q_off, const uint32_t* comps,
                                    const float* vals, uint32_t nq, const uint64_t* cand_off, const uint64_t* cand_ids, uint32_t k,
                                    float* out_scores, uint64_t* out_doc_ids, uint32_t* out_n);
sgpu_status explain_documents_device(sgpu_index* idx, uint32_t replica, const uint64_t* q_off, const uint32_t* comps,
                                     const float* vals, uint32_t nq, const uint64_t* cand_off, const uint64_t* cand_ids, uint32_t m,
                                     const ExplainOut& out);
bool score_debug_stats(sgpu_index* idx, uint32_t replica, double* out8);
// expand_queries.hip
sgpu_status expand_queries_device(sgpu_index* idx, uint32_t replica, const uint64_t* q_off, const uint32_t* comps, const float* vals,
                                  uint32_t nq, const uint64_t* cand_off, const uint64_t* cand_ids, const float* cand_w, float alpha,
                                  uint32_t t, uint32_t* out_comps, float* out_vals, uint32_t* out_n);
bool expand_debug_stats(sgpu_index* idx, uint32_t replica, double* out8);
// diversify_documents.hip
sgpu_status diversify_documents_device(sgpu_index* idx, uint32_t replica, const uint64_t* q_off, const uint32_t* comps,
                                       const float* vals, uint32_t nq, const uint64_t* cand_off, const uint64_t* cand_ids, float lambda,
                                       float mu, uint32_t k, const DiversifyOut& out);
bool diversify_debug_stats(sgpu_index* idx, uint32_t replica, double* out8);
// collapse_documents.hip
sgpu_status collapse_documents_device(sgpu_index* idx, uint32_t replica, const uint64_t* q_off, const uint32_t* comps,
                                      const float* vals, uint32_t nq, const uint64_t* cand_off, const uint64_t* cand_ids,
                                      const uint32_t* cand_groups, uint32_t m, uint32_t k, const CollapseOut& out);
bool collapse_debug_stats(sgpu_index* idx, uint32_t replica, double* out8);
// fuse_documents.hip
sgpu_status fuse_documents_device(sgpu_index* idx, uint32_t replica, const uint64_t* q_off, const uint32_t* comps, const float* vals,
                                  uint32_t nq, const uint64_t* cand_off, const uint64_t* cand_ids, const float* cand_ext,
                                  uint32_t method, float w_sparse, float w_ext, float rrf_c, uint32_t k, const FuseOut& out);
bool fuse_debug_stats(sgpu_index* idx, uint32_t replica, double* out8);
// filter.hip
sgpu_status filter_create(sgpu_index* idx, const uint32_t* doc_ids, uint64_t n, sgpu_filter** out);
sgpu_status filter_get_bits(const sgpu_filter* f, uint32_t* out_words, uint64_t cap_words, uint64_t* n_words);
uint64_t filter_count(const sgpu_filter* f);
uint64_t filter_device_bytes(const sgpu_filter* f);
void filter_destroy(sgpu_filter* f);
bool filter_build_times(const sgpu_filter* f, uint32_t replica, double* out2);
sgpu_status debug_posting_view(sgpu_index* idx, const sgpu_filter* f, uint32_t replica, uint32_t* out_bps, uint64_t cap_bps,
                               uint64_t* out_ref, uint32_t* out_doc, uint64_t cap_post, uint32_t* out_knn, uint64_t cap_knn,
                               uint32_t* out_bits, uint64_t cap_bits, uint64_t* sizes5);
}  // namespace sgpu

using namespace sgpu;

extern "C" {

const char* sgpu_last_error(void) { return last_error().c_str(); }
uint32_t sgpu_abi_version(void) { return 4; }

sgpu_status sgpu_device_count(int32_t* n) {
  if (!n) return fail(SGPU_EINVAL, "null argument");
  *n = device_count();
  if (*n <= 0) {
    *n = 0;
    return fail(SGPU_EDEVICE, "no HIP device visible");
  }
  return SGPU_OK;
}

sgpu_status sgpu_index_create(const sgpu_index_desc* desc, sgpu_index** out) {
  if (!desc || !out) return fail(SGPU_EINVAL, "null argument");
  sgpu_index* ix = new (std::nothrow) sgpu_index();
  if (!ix) return fail(SGPU_ENOMEM, "out of memory");
  sgpu_status st = host_index_from_desc(*desc, &ix->host);
  if (st != SGPU_OK) {
    delete ix;
    return st;
  }
  *out = ix;
  return SGPU_OK;
}

sgpu_status sgpu_index_build(uint32_t comp_width, uint64_t n_docs, uint64_t dim, const uint64_t* offsets,
                             const void* comps, const float* vals, const sgpu_build_config* cfg,
                             sgpu_index** out) {
  if (!offsets || !cfg || !out || (offsets[n_docs] && (!comps || !vals))) return fail(SGPU_EINVAL, "null argument");
  sgpu_index* ix = new (std::nothrow) sgpu_index();
  if (!ix) return fail(SGPU_ENOMEM, "out of memory");
  sgpu_status st = build_host_index(comp_width, n_docs, dim, offsets, comps, vals, *cfg, &ix->host);
  if (st != SGPU_OK) {
    delete ix;
    return st;
  }
  *out = ix;
  return SGPU_OK;
}

sgpu_status sgpu_index_convert(const sgpu_index* src, uint32_t value_type, sgpu_index** out) {
  if (!src || !out) return fail(SGPU_EINVAL, "null argument");
  sgpu_index* ix = new (std::nothrow) sgpu_index();
  if (!ix) return fail(SGPU_ENOMEM, "out of memory");
  sgpu_status st = host_index_convert(src->host, value_type, &ix->host);
  if (st != SGPU_OK) {
    delete ix;
    return st;
  }
  *out = ix;
  return SGPU_OK;
}

sgpu_status sgpu_index_get_desc(const sgpu_index* idx, sgpu_index_desc* out) {
  if (!idx || !out) return fail(SGPU_EINVAL, "null argument");
  idx->host.fill_desc(out);
  return SGPU_OK;
}

sgpu_status sgpu_index_save(const sgpu_index* idx, const char* path) {
  if (!idx || !path) return fail(SGPU_EINVAL, "null argument");
  return host_index_save(idx->host, path);
}

sgpu_status sgpu_index_load(const char* path, sgpu_index** out) {
  if (!path || !out) return fail(SGPU_EINVAL, "null argument");
  sgpu_index* ix = new (std::nothrow) sgpu_index();
  if (!ix) return fail(SGPU_ENOMEM, "out of memory");
  sgpu_status st = host_index_load(path, &ix->host);
  if (st != SGPU_OK) {
    delete ix;
    return st;
  }
  *out = ix;
  return SGPU_OK;
}

// Moves the index's generation on when it goes out of scope: the filters' views of the device state this call replaces
// are rebuilt on their next use (filter.hip).
struct GenerationBump {
  sgpu_index* idx;
  ~GenerationBump() { idx->generation.fetch_add(1, std::memory_order_acq_rel); }
};

static void drop_replicas(sgpu_index* idx) {
  for (ExactFile* f : idx->exact) exact_file_free(f);
  idx->exact.clear();
  for (ScoreState* s : idx->score) score_state_free(s);
  idx->score.clear();
  for (DeviceIndex* d : idx->replicas) device_index_free(d);
  idx->replicas.clear();
  idx->dev = nullptr;
}

sgpu_status sgpu_index_upload_many(sgpu_index* idx, const int32_t* device_ids, uint32_t n) {
  if (!idx || !device_ids || n == 0) return fail(SGPU_EINVAL, "null argument / no device given");
  GenerationBump bump{idx};
  drop_replicas(idx);
  // replica 0 is packed on the host and copied over PCIe once; the others are copied from it
  // GPU to GPU (hipMemcpyPeer: xGMI on an MI355X node) instead of n more host uploads
  DeviceIndex* first = nullptr;
  sgpu_status st = device_index_upload(idx->host, device_ids[0], &first);
  if (st != SGPU_OK) return st;
  idx->replicas.push_back(first);
  idx->dev = first;
  for (uint32_t i = 1; i < n; ++i) {
    DeviceIndex* r = nullptr;
    st = device_index_clone(first, device_ids[i], &r);
    if (st != SGPU_OK) {
      const std::string msg = last_error();   // the error of the failing replica survives the clean-up
      drop_replicas(idx);
      last_error() = msg;
      return st;
    }
    idx->replicas.push_back(r);
  }
  return SGPU_OK;
}

sgpu_status sgpu_index_upload(sgpu_index* idx, int32_t device) { return sgpu_index_upload_many(idx, &device, 1); }

uint32_t sgpu_index_replicas(const sgpu_index* idx) { return idx ? (uint32_t)idx->replicas.size() : 0; }

sgpu_status sgpu_index_set_knn(sgpu_index* idx, const uint32_t* neighbours, uint64_t n_total, uint32_t knn_dim) {
  if (!idx || (n_total && !neighbours)) return fail(SGPU_EINVAL, "null argument");
  if (n_total && knn_dim == 0) return fail(SGPU_EINVAL, "knn_dim == 0 with a non-empty neighbour array");
  for (uint64_t i = 0; i < n_total; ++i)
    if (neighbours[i] >= idx->host.n_docs) return fail(SGPU_EINVAL, "neighbour id >= n_docs");
  GenerationBump bump{idx};
  try {
    idx->host.knn.assign(neighbours, neighbours + n_total);
  } catch (const std::bad_alloc&) {
    return fail(SGPU_ENOMEM, "out of memory");
  }
  idx->host.knn_dim = n_total ? knn_dim : 0;
  for (DeviceIndex* d : idx->replicas) {
    sgpu_status st = device_index_set_knn(d, idx->host.knn, idx->host.knn_dim);
    if (st != SGPU_OK) return st;
  }
  return SGPU_OK;
}

sgpu_status sgpu_index_get_knn(const sgpu_index* idx, const uint32_t** neighbours, uint64_t* n_total,
                               uint32_t* knn_dim) {
  if (!idx || !neighbours || !n_total || !knn_dim) return fail(SGPU_EINVAL, "null argument");
  *neighbours = idx->host.knn.data();
  *n_total = idx->host.knn.size();
  *knn_dim = idx->host.knn_dim;
  return SGPU_OK;
}

sgpu_status sgpu_index_build_knn(sgpu_index* idx, uint32_t nknn) {
  if (!idx) return fail(SGPU_EINVAL, "null argument");
  GenerationBump bump{idx};
  try {
    sgpu_status st = build_knn_on_device(idx->dev, idx->host, nknn);   // searches run on replica 0
    for (size_t i = 1; st == SGPU_OK && i < idx->replicas.size(); ++i)
      st = device_index_set_knn(idx->replicas[i], idx->host.knn, idx->host.knn_dim);
    return st;
  } catch (const std::exception&) {
    return fail(SGPU_ENOMEM, "out of host memory building the kNN graph");
  }
}

uint64_t sgpu_index_device_bytes(const sgpu_index* idx) { return idx ? device_index_bytes(idx->dev) : 0; }

sgpu_status sgpu_index_stream_stats(const sgpu_index* idx, uint64_t* raw_docs, uint64_t* raw_elements) {
  if (!idx || !raw_docs || !raw_elements) return fail(SGPU_EINVAL, "null argument");
  *raw_docs = *raw_elements = 0;
  try {
    std::vector<uint8_t> raw;
    pack_dvb_raw_flags(idx->host, &raw);   // (empty unless the index is a DotVByte one)
    for (uint64_t d = 0; d < raw.size(); ++d)
      if (raw[d]) {
        *raw_docs += 1;
        *raw_elements += idx->host.fwd_offsets[d + 1] - idx->host.fwd_offsets[d];
      }
  } catch (const std::bad_alloc&) {
    return fail(SGPU_ENOMEM, "out of host memory");
  }
  return SGPU_OK;
}

void sgpu_index_destroy(sgpu_index* idx) {
  if (!idx) return;
  drop_replicas(idx);
  delete idx;
}

static DeviceIndex* replica_of(sgpu_index* idx, uint32_t replica) {
  if (!idx || replica >= idx->replicas.size()) {
    fail(SGPU_EDEVICE, "index is not uploaded to a device (call sgpu_index_upload) / replica out of range");
    return nullptr;
  }
  return idx->replicas[replica];
}
static DeviceIndex* replica_of_batch(sgpu_index* idx, const sgpu_batch* b) {
  for (DeviceIndex* d : idx->replicas)
    if (batch_replica(b) == d) return d;
  fail(SGPU_EINVAL, "batch does not belong to this index");
  return nullptr;
}

sgpu_status sgpu_batch_create_on(sgpu_index* idx, uint32_t replica, const uint64_t* q_off, const uint32_t* comps,
                                 const float* vals, uint32_t nq, uint32_t k_max, sgpu_batch** out) {
  if (!idx || !q_off || !out || (q_off[nq] && (!comps || !vals))) return fail(SGPU_EINVAL, "null argument");
  *out = nullptr;
  DeviceIndex* d = replica_of(idx, replica);
  if (!d) return SGPU_EDEVICE;
  return batch_create(d, lane_main(d), idx->host.dim, q_off, comps, vals, nq, k_max, out);
}

sgpu_status sgpu_batch_create(sgpu_index* idx, const uint64_t* q_off, const uint32_t* comps, const float* vals,
                              uint32_t nq, uint32_t k_max, sgpu_batch** out) {
  return sgpu_batch_create_on(idx, 0, q_off, comps, vals, nq, k_max, out);
}

sgpu_status sgpu_batch_run(sgpu_index* idx, sgpu_batch* batch, const sgpu_search_params* params, int32_t sync,
                           sgpu_launch_stats* stats) {
  if (!idx || !batch || !params) return fail(SGPU_EINVAL, "null argument");
  DeviceIndex* d = replica_of_batch(idx, batch);
  if (!d) return SGPU_EINVAL;
  return batch_run(d, nullptr, batch, *params, 0 /*MODE_SEARCH*/, sync, stats);
}

sgpu_status sgpu_batch_run_counted(sgpu_index* idx, sgpu_batch* batch, const sgpu_search_params* params,
                                   sgpu_launch_stats* stats) {
  if (!idx || !batch || !params) return fail(SGPU_EINVAL, "null argument");
  DeviceIndex* d = replica_of_batch(idx, batch);
  if (!d) return SGPU_EINVAL;
  return batch_run(d, nullptr, batch, *params, 2 /*MODE_COUNTED*/, 1, stats);
}

sgpu_status sgpu_batch_sync(sgpu_index* idx, sgpu_launch_stats* stats) {
  if (!idx) return fail(SGPU_EINVAL, "null argument");
  // every replica's main lane; the statistics are replica 0's
  for (size_t i = idx->replicas.size(); i-- > 1;) {
    sgpu_status st = batch_sync(idx->replicas[i], nullptr);
    if (st != SGPU_OK) return st;
  }
  return batch_sync(idx->dev, stats);
}

sgpu_status sgpu_batch_fetch(sgpu_index* idx, sgpu_batch* batch, uint32_t k, float* out_scores,
                             uint64_t* out_doc_ids, uint32_t* out_n) {
  if (!idx || !batch || !out_scores || !out_doc_ids || !out_n) return fail(SGPU_EINVAL, "null argument");
  DeviceIndex* d = replica_of_batch(idx, batch);
  if (!d) return SGPU_EINVAL;
  return batch_fetch(d, nullptr, batch, k, out_scores, out_doc_ids, out_n);
}

sgpu_status sgpu_batch_fetch_stats(sgpu_index* idx, sgpu_batch* batch, uint32_t* out_counters) {
  if (!idx || !batch || !out_counters) return fail(SGPU_EINVAL, "null argument");
  DeviceIndex* d = replica_of_batch(idx, batch);
  if (!d) return SGPU_EINVAL;
  return batch_fetch_stats(d, batch, out_counters);
}

void sgpu_batch_destroy(sgpu_batch* batch) { batch_free(batch); }

// How a shard of nq queries is cut (pure: tests/test_abi_and_host.py and tests/test_entry_chunks_cpu.py check it through
// sgpu_debug_chunk_bounds / sgpu_debug_call_bounds).
// chunk_jobs: the number of launches wanted before lanes are taken - never fewer than it takes to keep every chunk within
// kChunkQueriesMax (what a lane's arena and a launch plan are sized for), up to the eight lanes of a replica.
// chunk_bounds: the queries [q0, q1) of launch j of n_jobs (first_pm: the first chunk's share of the call in per mille,
// 0 = equal chunks; the others share the rest equally).
// A call of more than 8 x kChunkQueriesMax queries is served in SEGMENTS of at most that many, one after the other
// (call_segments), each cut by the rules above: the bound on a chunk then holds whatever nq is.
static uint32_t chunk_jobs(uint32_t nq, uint32_t chunk_min, uint32_t chunk_max) {
  if (!chunk_min) return 1u;
  const uint32_t by_rule = nq >= 2 * (uint64_t)chunk_min ? std::min<uint32_t>(chunk_max, nq / chunk_min) : 1u;
  const uint32_t by_size = (uint32_t)std::min<uint64_t>(((uint64_t)nq + kChunkQueriesMax - 1) / kChunkQueriesMax, 8u);
  return std::max(by_rule, by_size);
}
static void chunk_bounds(uint32_t nq, uint32_t n_jobs, uint32_t j, uint32_t* q0, uint32_t* q1, uint32_t first_pm = 0) {
  if (first_pm == 0 || first_pm >= 1000 || n_jobs < 2) {
    *q0 = (uint32_t)((uint64_t)nq * j / n_jobs);
    *q1 = (uint32_t)((uint64_t)nq * (j + 1) / n_jobs);
    return;
  }
  const uint32_t first = std::min<uint32_t>(std::max<uint32_t>((uint32_t)((uint64_t)nq * first_pm / 1000), 1u), nq - (n_jobs - 1));
  const uint32_t rest = nq - first;
  *q0 = j == 0 ? 0u : first + (uint32_t)((uint64_t)rest * (j - 1) / (n_jobs - 1));
  *q1 = j == 0 ? first : first + (uint32_t)((uint64_t)rest * j / (n_jobs - 1));
}
static uint32_t call_segments(uint32_t nq) {
  return (uint32_t)std::max<uint64_t>(((uint64_t)nq + 8ull * kChunkQueriesMax - 1) / (8ull * kChunkQueriesMax), 1u);
}

// One shard of a batch on one replica: borrow a lane (its stream and recycled device batch), H2D of
// the queries, one kernel pass, D2H of the results. No allocation once the lane's batch has grown to
// the call's size; calls from different host threads take different lanes and overlap.
// A large shard is cut into chunks on as many lanes (as many as are free): the host side of chunk i+1 (validation,
// launch plan, staging of the H2D) runs while the GPU searches chunk i, and the workgroups of chunk i+1 fill the CUs
// that chunk i's tail leaves idle. Who plans which chunk: chunk 0 goes out unplanned where the device could plan it (input
// order, no kernel ahead of its search), every later chunk is planned HERE, on the calling thread, after the chunk before
// it has been enqueued - the thread would only wait, and the chunk's search is then queued and ready long before the
// previous search's workgroups start to leave (staged_launch, staged.hip); a call that is one launch keeps the
// device plan.
// (flt: the filter of a filtered call and the replica d is, or null; [s0, s1): the queries of the caller's arrays this
// segment serves - offsets, rows and error messages stay the whole shard's)
static sgpu_status search_segment(DeviceIndex* d, uint64_t dim, const uint64_t* q_off, const uint32_t* comps,
                                  const float* vals, uint32_t s0, uint32_t s1, uint32_t q_base, const sgpu_search_params& params,
                                  float* out_scores, uint64_t* out_doc_ids, uint32_t* out_n, const FilterRef* flt, bool shared) {
  static const uint32_t chunk_min = [] {
    const char* v = std::getenv("SGPU_CHUNK_MIN");
    // (600 since r03: a 1250-query call - one rank's shard of a 10 000-query batch on eight GPUs - takes 1115 us in two
    // chunks against 1260 in one, a 2500-query call 1.94 against 2.35 ms: the host side of a chunk, ~0.3 us per query,
    // hides behind the previous chunk's kernel; chunks of ~300 lose to their launch tails. profiles/r03_chunk_probe.txt)
    return v && *v ? (uint32_t)std::strtoul(v, nullptr, 10) : 0xffffffffu;   // (unset: by the rule below; 0: never cut a call)
  }();
  struct Job {
    Lane* lane;
    uint32_t q0, q1;
  };
  // Chunks per call: FOUR when this call is alone on the replica (its host side - validation, plan, staging: ~0.2 us per
  // query - hides behind its own earlier chunks' kernels: 1.44 M queries/s from one request thread against 1.31 / 1.11 M
  // with two / one chunk), TWO when other calls are - or were a moment ago - in flight on it (their kernels hide it, and every extra chunk is a launch
  // tail: 10 000-query calls from two / three request threads 1.670 / 1.683 M queries/s with two chunks against 1.636 /
  // 1.596 M with four - the device-resident rate is 1.685 M; r05, gpurun_out r05y). SGPU_CHUNK_MAX fixes the number.
  static const uint32_t chunk_max_env = [] {
    const char* v = std::getenv("SGPU_CHUNK_MAX");
    const uint32_t n = v && *v ? (uint32_t)std::strtoul(v, nullptr, 10) : 0u;
    return n > 8 ? 8u : n;
  }();
  // (SGPU_CHUNK_FIRST, a test hook: the first chunk's share of a call in per mille; unset or 0: equal chunks)
  static const uint32_t chunk_first_pm = [] {
    const char* v = test_hooks_on() ? std::getenv("SGPU_CHUNK_FIRST") : nullptr;
    return v && *v ? (uint32_t)std::strtoul(v, nullptr, 10) : 0u;
  }();
  const uint32_t nq = s1 - s0;
  // Would chunks of this call be planned on the device? ONE predicate with staged_launch (device_plan_dots), asked with the
  // size of a chunk of the two-way cut that answer leads to.
  // (r06: with the launch plan computed on the device - plan_kernel.hip - a chunk's host side is validation and a copy,
  // ~20 us per 1000 queries: two chunks whoever else is calling - one request thread 1.61 M queries/s against 1.59 / 1.54 M
  // with four / one, two threads 1.71 against 1.69 / 1.68; profiles/r06_entry_point_chunks.txt)
  const bool device_plans = device_plan_dots(d, params, std::min<uint32_t>(std::max<uint32_t>(nq / 2, 1u), kChunkQueriesMax), params.query_cut) != 0;
  const uint32_t chunk_max = chunk_max_env ? chunk_max_env : ((shared || device_plans) ? 2u : 4u);
  Job jobs[8];
  // (r06: 1300 where the chunks are planned on the device - a 1250- or 2500-query call is then ONE launch: from two request
  // threads 864 -> 781 us and 1551 -> 1475 us per call, from one thread no difference; profiles/r06_shard_probe_chunk_min.txt)
  const uint32_t cmin = chunk_min != 0xffffffffu ? chunk_min : (device_plans ? 1300u : 600u);
  uint32_t n_jobs = chunk_jobs(nq, cmin, chunk_max);
  jobs[0].lane = lane_acquire(d);
  for (uint32_t j = 1; j < n_jobs; ++j) {
    jobs[j].lane = lane_try_acquire(d);
    if (!jobs[j].lane) {
      n_jobs = j;
      break;
    }
  }
  std::vector<uint64_t> off;   // a chunk's offsets, rebased (sized here: nothing below allocates host memory)
  for (;;) {
    uint32_t longest = 0;
    for (uint32_t j = 0; j < n_jobs; ++j) {
      chunk_bounds(nq, n_jobs, j, &jobs[j].q0, &jobs[j].q1, chunk_first_pm);
      jobs[j].q0 += s0;
      jobs[j].q1 += s0;
      if (jobs[j].q0 != 0) longest = std::max(longest, jobs[j].q1 - jobs[j].q0);
    }
    if (n_jobs == 1 && s0 == 0) break;
    try {
      off.resize((size_t)longest + 1);
      break;
    } catch (const std::exception&) {
      if (n_jobs == 1) {
        lane_release(d, jobs[0].lane);
        return fail(SGPU_ENOMEM, "out of host memory cutting a query batch");
      }
      for (uint32_t j = 1; j < n_jobs; ++j) lane_release(d, jobs[j].lane);
      n_jobs = 1;
    }
  }
  const uint32_t k = params.k;
  sgpu_status st = SGPU_OK;
  std::string msg;
  uint32_t launched = 0;
  if (n_jobs > 1 || s0 != 0) {   // the offsets of the whole segment hold before a chunk is launched (each chunk checks its own components)
    uint32_t max_nnz = 0;
    st = q_off[0] != 0 ? fail(SGPU_EINVAL, "q_off[0] must be 0") : validate_query_offsets(q_off + s0, nq, q_base + s0, &max_nnz);
    if (st != SGPU_OK) msg = last_error();
  }
  for (uint32_t j = 0; j < n_jobs && st == SGPU_OK; ++j) {
    Job& jb = jobs[j];
    const uint64_t* qo = q_off;
    if (jb.q0 != 0) {   // (a chunk that starts at query 0 uses the caller's offsets as they are)
      for (uint32_t q = jb.q0; q <= jb.q1; ++q) off[q - jb.q0] = q_off[q] - q_off[jb.q0];
      qo = off.data();
    }
    st = staged_launch(d, jb.lane, dim, qo, comps ? comps + q_off[jb.q0] : nullptr, vals ? vals + q_off[jb.q0] : nullptr,
                       jb.q1 - jb.q0, q_base + jb.q0, params, lane_scratch(jb.lane), j + 1 < n_jobs ? 2u : (shared ? 1u : 0u),
                       flt, j);
    if (st == SGPU_OK) ++launched;
    else msg = last_error();
  }
  for (uint32_t j = 0; j < launched; ++j) {   // every launched chunk is waited for, also after an error
    Job& jb = jobs[j];
    const sgpu_status fs = staged_finish(d, jb.lane, *lane_scratch(jb.lane), out_scores + (size_t)jb.q0 * k,
                                         out_doc_ids + (size_t)jb.q0 * k, out_n + jb.q0);
    if (fs != SGPU_OK && st == SGPU_OK) {
      st = fs;
      msg = last_error();
    }
  }
  for (uint32_t j = 0; j < n_jobs; ++j) lane_release(d, jobs[j].lane);
  if (st != SGPU_OK) last_error() = msg;
  return st;
}

static sgpu_status search_shard(DeviceIndex* d, uint64_t dim, const uint64_t* q_off, const uint32_t* comps,
                                const float* vals, uint32_t nq, uint32_t q_base, const sgpu_search_params& params,
                                float* out_scores, uint64_t* out_doc_ids, uint32_t* out_n, const FilterRef* flt) {
  struct InFlight {   // (counts this call on the replica for as long as it runs)
    DeviceIndex* d;
    bool shared;
    explicit InFlight(DeviceIndex* d_) : d(d_), shared(call_enter(d_)) {}
    ~InFlight() { call_exit(d); }
  } in_flight(d);
  const uint32_t n_seg = call_segments(nq);
  sgpu_status st = SGPU_OK;
  for (uint32_t s = 0; s < n_seg && st == SGPU_OK; ++s)
    st = search_segment(d, dim, q_off, comps, vals, (uint32_t)((uint64_t)nq * s / n_seg), (uint32_t)((uint64_t)nq * (s + 1) / n_seg),
                        q_base, params, out_scores, out_doc_ids, out_n, flt, in_flight.shared);
  return st;
}

}  // extern "C"

// sgpu_batch_search, and sgpu_batch_search_filtered once its filter is known to be this index's (filter may be null)
static sgpu_status batch_search(sgpu_index* idx, const uint64_t* q_off, const uint32_t* comps, const float* vals,
                                uint32_t nq, const sgpu_search_params* params, float* out_scores,
                                uint64_t* out_doc_ids, uint32_t* out_n, const sgpu_filter* filter) {
  if (!idx || !params || !q_off || !out_scores || !out_doc_ids || !out_n) return fail(SGPU_EINVAL, "null argument");
  if (params->k == 0) return fail(SGPU_EINVAL, "k must be > 0 (KHeap::new asserts, reference src/utils.rs:23)");
  if (idx->replicas.empty()) return fail(SGPU_EDEVICE, "index is not uploaded to a device (call sgpu_index_upload)");
  if (q_off[nq] && (!comps || !vals)) return fail(SGPU_EINVAL, "null argument");
  const uint32_t n_rep = (uint32_t)idx->replicas.size();
  if (n_rep == 1) {
    const FilterRef fr{filter, 0};
    return search_shard(idx->dev, idx->host.dim, q_off, comps, vals, nq, 0, *params, out_scores, out_doc_ids, out_n,
                        filter ? &fr : nullptr);
  }
  if (nq < 2 * n_rep) {   // too small to shard (single queries of a serving loop): the replicas take such calls in turn
    const uint32_t r = idx->next_replica.fetch_add(1, std::memory_order_relaxed) % n_rep;
    const FilterRef fr{filter, r};
    return search_shard(idx->replicas[r], idx->host.dim, q_off, comps, vals, nq, 0, *params, out_scores, out_doc_ids, out_n,
                        filter ? &fr : nullptr);
  }
  // Index replicated on several GPUs: contiguous shards of the batch, one host thread per GPU, no
  // collective; results land in input order (the reference's rayon loop over queries,
  // src/pylib/mod.rs:629-652, 1129-1145, becomes one shard per device).
  {   // the offsets of the whole batch hold before it is cut (each shard checks its own components)
    uint32_t max_nnz = 0;
    if (q_off[0] != 0) return fail(SGPU_EINVAL, "q_off[0] must be 0");
    const sgpu_status vst = validate_query_offsets(q_off, nq, 0, &max_nnz);
    if (vst != SGPU_OK) return vst;
  }
  const uint32_t k = params->k;
  try {
    std::vector<sgpu_status> sts(n_rep, SGPU_OK);
    std::vector<std::string> msgs(n_rep);
    std::vector<std::vector<uint64_t>> offs(n_rep);   // every shard's offsets, rebased; sized before a thread starts
    for (uint32_t r = 0; r < n_rep; ++r) {
      const uint32_t q0 = (uint32_t)((uint64_t)nq * r / n_rep), q1 = (uint32_t)((uint64_t)nq * (r + 1) / n_rep);
      offs[r].resize(q1 - q0 + 1);
      for (uint32_t q = q0; q <= q1; ++q) offs[r][q - q0] = q_off[q] - q_off[q0];
    }
    auto shard = [&](uint32_t r) {
      const uint32_t q0 = (uint32_t)((uint64_t)nq * r / n_rep), q1 = (uint32_t)((uint64_t)nq * (r + 1) / n_rep);
      try {
        const FilterRef fr{filter, r};
        sts[r] = search_shard(idx->replicas[r], idx->host.dim, offs[r].data(), comps ? comps + q_off[q0] : nullptr,
                              vals ? vals + q_off[q0] : nullptr, q1 - q0, q0, *params, out_scores + (size_t)q0 * k,
                              out_doc_ids + (size_t)q0 * k, out_n + q0, filter ? &fr : nullptr);
        if (sts[r] != SGPU_OK) msgs[r] = last_error();
      } catch (const std::exception&) {
        sts[r] = SGPU_ENOMEM;
      }
    };
    std::vector<std::thread> threads;
    threads.reserve(n_rep);
    for (uint32_t r = 1; r < n_rep; ++r) {
      try {
        threads.emplace_back(shard, r);
      } catch (const std::exception&) {   // no thread to be had: the shard runs on this one
        shard(r);
      }
    }
    shard(0);   // the calling thread drives replica 0
    for (auto& t : threads) t.join();
    for (uint32_t r = 0; r < n_rep; ++r)
      if (sts[r] != SGPU_OK) {
        if (msgs[r].empty()) return fail(sts[r], "out of host memory searching shard %u", r);
        last_error() = msgs[r];
        return sts[r];
      }
  } catch (const std::exception&) {
    return fail(SGPU_ENOMEM, "out of host memory sharding a query batch");
  }
  return SGPU_OK;
}

static sgpu_status foreign_filter(const sgpu_index* idx, const sgpu_filter* filter) {
  return filter && filter_index(filter) != idx ? fail(SGPU_EINVAL, "the filter was created on another index") : SGPU_OK;
}

extern "C" {

sgpu_status sgpu_batch_search(sgpu_index* idx, const uint64_t* q_off, const uint32_t* comps, const float* vals,
                              uint32_t nq, const sgpu_search_params* params, float* out_scores,
                              uint64_t* out_doc_ids, uint32_t* out_n) {
  return batch_search(idx, q_off, comps, vals, nq, params, out_scores, out_doc_ids, out_n, nullptr);
}

sgpu_status sgpu_batch_search_filtered(sgpu_index* idx, const uint64_t* q_off, const uint32_t* comps, const float* vals,
                                       uint32_t nq, const sgpu_search_params* params, float* out_scores,
                                       uint64_t* out_doc_ids, uint32_t* out_n, const sgpu_filter* filter) {
  const sgpu_status st = foreign_filter(idx, filter);
  if (st != SGPU_OK) return st;
  return batch_search(idx, q_off, comps, vals, nq, params, out_scores, out_doc_ids, out_n, filter);
}

sgpu_status sgpu_search_filtered(sgpu_index* idx, const uint32_t* comps, const float* vals, uint32_t nnz,
                                 const sgpu_search_params* params, float* out_scores, uint64_t* out_doc_ids,
                                 uint32_t* out_n, const sgpu_filter* filter) {
  const uint64_t q_off[2] = {0, nnz};
  return sgpu_batch_search_filtered(idx, q_off, comps, vals, 1, params, out_scores, out_doc_ids, out_n, filter);
}

sgpu_status sgpu_filter_create(sgpu_index* idx, const uint32_t* doc_ids, uint64_t n, sgpu_filter** out) {
  return filter_create(idx, doc_ids, n, out);
}
sgpu_status sgpu_filter_create_terms(sgpu_index* idx, uint32_t replica, const sgpu_term_clause* clauses, uint32_t n_clauses,
                                     uint32_t min_should, const sgpu_filter* within, sgpu_filter** out) {
  return term_filter_device(idx, replica, clauses, n_clauses, min_should, within, out);
}
sgpu_status sgpu_filter_create_terms_host(sgpu_index* idx, const sgpu_term_clause* clauses, uint32_t n_clauses, uint32_t min_should,
                                          const sgpu_filter* within, uint32_t num_threads, sgpu_filter** out) {
  return term_filter_host(idx, clauses, n_clauses, min_should, within, num_threads, out);
}
sgpu_status sgpu_filter_get_bits(const sgpu_filter* filter, uint32_t* out_words, uint64_t cap_words, uint64_t* n_words) {
  return filter_get_bits(filter, out_words, cap_words, n_words);
}
uint64_t sgpu_filter_count(const sgpu_filter* filter) { return filter_count(filter); }
uint64_t sgpu_filter_device_bytes(const sgpu_filter* filter) { return filter_device_bytes(filter); }
void sgpu_filter_destroy(sgpu_filter* filter) { filter_destroy(filter); }

sgpu_status sgpu_search(sgpu_index* idx, const uint32_t* comps, const float* vals, uint32_t nnz,
                        const sgpu_search_params* params, float* out_scores, uint64_t* out_doc_ids,
                        uint32_t* out_n) {
  const uint64_t q_off[2] = {0, nnz};
  return sgpu_batch_search(idx, q_off, comps, vals, 1, params, out_scores, out_doc_ids, out_n);
}

// The reference's AQT loop (src/bin/perf_inverted_index.rs:184-216): the queries of a set searched one
// at a time, each through sgpu_search, timed around the whole loop.
sgpu_status sgpu_search_sequential_timed(sgpu_index* idx, const uint64_t* q_off, const uint32_t* comps, const float* vals,
                                         uint32_t nq, const sgpu_search_params* params, float* out_scores,
                                         uint64_t* out_doc_ids, uint32_t* out_n, double* mean_us, double* breakdown_us,
                                         double* per_query_us) {
  if (!idx || !params || !q_off || !out_scores || !out_doc_ids || !out_n) return fail(SGPU_EINVAL, "null argument");
  if (params->k == 0) return fail(SGPU_EINVAL, "k must be > 0 (KHeap::new asserts, reference src/utils.rs:23)");
  double phases[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  double*& slot = call_timing();
  double* const saved = slot;
  if (breakdown_us) slot = phases;
  const uint32_t k = params->k;
  sgpu_status st = SGPU_OK;
  const auto t0 = std::chrono::steady_clock::now();
  for (uint32_t q = 0; q < nq && st == SGPU_OK; ++q) {
    if (q_off[q + 1] < q_off[q] || q_off[q + 1] - q_off[q] > 0xffffffffull) {
      st = fail(SGPU_EINVAL, "query offsets must be monotone (query %u)", q);
      break;
    }
    const auto tq = per_query_us ? std::chrono::steady_clock::now() : t0;
    st = sgpu_search(idx, comps ? comps + q_off[q] : nullptr, vals ? vals + q_off[q] : nullptr,
                     (uint32_t)(q_off[q + 1] - q_off[q]), params, out_scores + (size_t)q * k,
                     out_doc_ids + (size_t)q * k, out_n + q);
    if (per_query_us) per_query_us[q] = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - tq).count();
  }
  const double total = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
  slot = saved;
  if (mean_us) *mean_us = nq ? total / nq : 0.0;
  if (breakdown_us)
    for (int i = 0; i < 8; ++i) breakdown_us[i] = nq ? phases[i] / nq : 0.0;
  return st;
}

sgpu_status sgpu_search_sequential(sgpu_index* idx, const uint64_t* q_off, const uint32_t* comps, const float* vals,
                                   uint32_t nq, const sgpu_search_params* params, float* out_scores,
                                   uint64_t* out_doc_ids, uint32_t* out_n, double* mean_us, double* breakdown_us) {
  return sgpu_search_sequential_timed(idx, q_off, comps, vals, nq, params, out_scores, out_doc_ids, out_n, mean_us,
                                      breakdown_us, nullptr);
}

// ---- test hooks (include/seismic_hip_testing.h; NOT part of the boundary) ---------------------------------------
// Entry points the test suite and the tools use to look at host-side decisions (team size, chunk plan, launch plan,
// packed records, phase clocks, cooperative trace). Like the undocumented environment names they are inert unless
// SGPU_TEST_HOOKS=1 is set: status-returning ones fail with SGPU_EINVAL, the others return 0 / do nothing.
#define SGPU_HOOK_OR(ret)                                                                            \
  if (!test_hooks_on()) {                                                                            \
    (void)fail(SGPU_EINVAL, "%s is a test hook: set SGPU_TEST_HOOKS=1 (include/seismic_hip_testing.h)", __func__); \
    return ret;                                                                                      \
  }

// (the team size a host-parallel phase would take for num_threads == 0)
uint32_t sgpu_debug_host_threads(void) {
  SGPU_HOOK_OR(0u);
  return (uint32_t)host_threads();
}

// (not part of the boundary: how search_shard would cut a call of nq queries when `lanes_free` lanes can be had -
// bounds[2 * j], bounds[2 * j + 1] = the queries [q0, q1) of launch j; returns the number of launches)
uint32_t sgpu_debug_chunk_bounds(uint32_t nq, uint32_t chunk_min, uint32_t chunk_max, uint32_t lanes_free, uint32_t* bounds) {
  SGPU_HOOK_OR(0u);
  uint32_t n_jobs = chunk_jobs(nq, chunk_min, chunk_max < 1 ? 1 : (chunk_max > 8 ? 8 : chunk_max));
  if (lanes_free >= 1 && n_jobs > lanes_free) n_jobs = lanes_free;
  for (uint32_t j = 0; j < n_jobs; ++j) chunk_bounds(nq, n_jobs, j, bounds + 2 * j, bounds + 2 * j + 1);
  return n_jobs;
}

// (the same for a call of any size: its segments one after the other, each cut as above - every launch of the call in
// order; at most `cap` launches are written, the number there are is returned)
uint32_t sgpu_debug_call_bounds(uint32_t nq, uint32_t chunk_min, uint32_t chunk_max, uint32_t lanes_free, uint32_t first_pm,
                                uint32_t* bounds, uint32_t cap) {
  SGPU_HOOK_OR(0u);
  const uint32_t n_seg = call_segments(nq);
  uint32_t n = 0;
  for (uint32_t s = 0; s < n_seg; ++s) {
    const uint32_t s0 = (uint32_t)((uint64_t)nq * s / n_seg), s1 = (uint32_t)((uint64_t)nq * (s + 1) / n_seg);
    uint32_t n_jobs = chunk_jobs(s1 - s0, chunk_min, chunk_max < 1 ? 1 : (chunk_max > 8 ? 8 : chunk_max));
    if (lanes_free >= 1 && n_jobs > lanes_free) n_jobs = lanes_free;
    for (uint32_t j = 0; j < n_jobs; ++j, ++n) {
      uint32_t q0, q1;
      chunk_bounds(s1 - s0, n_jobs, j, &q0, &q1, first_pm);
      if (n < cap) {
        bounds[2 * n] = s0 + q0;
        bounds[2 * n + 1] = s0 + q1;
      }
    }
  }
  return n;
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

sgpu_status sgpu_summary_distances(sgpu_index* idx, uint32_t list, const uint32_t* comps, const float* vals,
                                   uint32_t nnz, float* out_dots, uint32_t* out_n_blocks) {
  if (!idx || !out_dots || !out_n_blocks || (nnz && (!comps || !vals))) return fail(SGPU_EINVAL, "null argument");
  return summary_distances(idx->dev, idx->host, list, comps, vals, nnz, out_dots, out_n_blocks);
}

sgpu_status sgpu_exact_search(const sgpu_index* idx, const uint64_t* q_off, const uint32_t* comps,
                              const float* vals, uint32_t nq, uint32_t k, uint32_t num_threads,
                              float* out_scores, uint64_t* out_doc_ids, uint32_t* out_n) {
  if (!idx || !q_off || !out_scores || !out_doc_ids || !out_n) return fail(SGPU_EINVAL, "null argument");
  return exact_search_host(idx->host, q_off, comps, vals, nq, k, num_threads, out_scores, out_doc_ids, out_n);
}

sgpu_status sgpu_exact_search_filtered(const sgpu_index* idx, const uint64_t* q_off, const uint32_t* comps,
                                       const float* vals, uint32_t nq, uint32_t k, uint32_t num_threads,
                                       float* out_scores, uint64_t* out_doc_ids, uint32_t* out_n,
                                       const sgpu_filter* filter) {
  if (!filter) return sgpu_exact_search(idx, q_off, comps, vals, nq, k, num_threads, out_scores, out_doc_ids, out_n);
  const sgpu_status st = foreign_filter(idx, filter);
  if (st != SGPU_OK) return st;
  if (!idx || !q_off || !out_scores || !out_doc_ids || !out_n) return fail(SGPU_EINVAL, "null argument");
  return exact_search_host(idx->host, q_off, comps, vals, nq, k, num_threads, out_scores, out_doc_ids, out_n,
                           filter_host_bits(filter));
}

sgpu_status sgpu_exact_search_device(sgpu_index* idx, uint32_t replica, const uint64_t* q_off, const uint32_t* comps,
                                     const float* vals, uint32_t nq, uint32_t k, float* out_scores,
                                     uint64_t* out_doc_ids, uint32_t* out_n) {
  return exact_search_device(idx, replica, q_off, comps, vals, nq, k, out_scores, out_doc_ids, out_n, nullptr);
}

sgpu_status sgpu_exact_search_device_filtered(sgpu_index* idx, uint32_t replica, const uint64_t* q_off,
                                              const uint32_t* comps, const float* vals, uint32_t nq, uint32_t k,
                                              float* out_scores, uint64_t* out_doc_ids, uint32_t* out_n,
                                              const sgpu_filter* filter) {
  const sgpu_status st = foreign_filter(idx, filter);
  if (st != SGPU_OK) return st;
  return exact_search_device(idx, replica, q_off, comps, vals, nq, k, out_scores, out_doc_ids, out_n, filter);
}

sgpu_status sgpu_score_documents(sgpu_index* idx, uint32_t replica, const uint64_t* q_off, const uint32_t* comps,
                                 const float* vals, uint32_t nq, const uint64_t* cand_off, const uint64_t* cand_ids,
                                 float* out_scores) {
  return score_documents_device(idx, replica, q_off, comps, vals, nq, cand_off, cand_ids, out_scores);
}

sgpu_status sgpu_score_documents_host(const sgpu_index* idx, const uint64_t* q_off, const uint32_t* comps, const float* vals,
                                      uint32_t nq, const uint64_t* cand_off, const uint64_t* cand_ids, uint32_t num_threads,
                                      float* out_scores) {
  if (!idx) return fail(SGPU_EINVAL, "null argument");
  return score_documents_host(idx->host, q_off, comps, vals, nq, cand_off, cand_ids, num_threads, out_scores);
}

sgpu_status sgpu_rerank_documents(sgpu_index* idx, uint32_t replica, const uint64_t* q_off, const uint32_t* comps,
                                  const float* vals, uint32_t nq, const uint64_t* cand_off, const uint64_t* cand_ids, uint32_t k,
                                  float* out_scores, uint64_t* out_doc_ids, uint32_t* out_n) {
  return rerank_documents_device(idx, replica, q_off, comps, vals, nq, cand_off, cand_ids, k, out_scores, out_doc_ids, out_n);
}

sgpu_status sgpu_rerank_documents_host(const sgpu_index* idx, const uint64_t* q_off, const uint32_t* comps, const float* vals,
                                       uint32_t nq, const uint64_t* cand_off, const uint64_t* cand_ids, uint32_t k,
                                       uint32_t num_threads, float* out_scores, uint64_t* out_doc_ids, uint32_t* out_n) {
  if (!idx) return fail(SGPU_EINVAL, "null argument");
  return rerank_documents_host(idx->host, q_off, comps, vals, nq, cand_off, cand_ids, k, num_threads, out_scores, out_doc_ids,
                               out_n);
}

sgpu_status sgpu_explain_documents(sgpu_index* idx, uint32_t replica, const uint64_t* q_off, const uint32_t* comps,
                                   const float* vals, uint32_t nq, const uint64_t* cand_off, const uint64_t* cand_ids, uint32_t m,
                                   float* out_scores, uint32_t* out_n_terms, uint32_t* out_comps, float* out_q_vals,
                                   float* out_d_vals, float* out_products) {
  const ExplainOut out{out_scores, out_n_terms, out_comps, out_q_vals, out_d_vals, out_products};
  return explain_documents_device(idx, replica, q_off, comps, vals, nq, cand_off, cand_ids, m, out);
}

sgpu_status sgpu_explain_documents_host(const sgpu_index* idx, const uint64_t* q_off, const uint32_t* comps, const float* vals,
                                        uint32_t nq, const uint64_t* cand_off, const uint64_t* cand_ids, uint32_t m,
                                        uint32_t num_threads, float* out_scores, uint32_t* out_n_terms, uint32_t* out_comps,
                                        float* out_q_vals, float* out_d_vals, float* out_products) {
  if (!idx) return fail(SGPU_EINVAL, "null argument");
  const ExplainOut out{out_scores, out_n_terms, out_comps, out_q_vals, out_d_vals, out_products};
  return explain_documents_host(idx->host, q_off, comps, vals, nq, cand_off, cand_ids, m, num_threads, out);
}

sgpu_status sgpu_expand_queries(sgpu_index* idx, uint32_t replica, const uint64_t* q_off, const uint32_t* comps, const float* vals,
                                uint32_t nq, const uint64_t* cand_off, const uint64_t* cand_ids, const float* cand_w, float alpha,
                                uint32_t t, uint32_t* out_comps, float* out_vals, uint32_t* out_n) {
  return expand_queries_device(idx, replica, q_off, comps, vals, nq, cand_off, cand_ids, cand_w, alpha, t, out_comps, out_vals, out_n);
}

sgpu_status sgpu_expand_queries_host(const sgpu_index* idx, const uint64_t* q_off, const uint32_t* comps, const float* vals,
                                     uint32_t nq, const uint64_t* cand_off, const uint64_t* cand_ids, const float* cand_w,
                                     float alpha, uint32_t t, uint32_t num_threads, uint32_t* out_comps, float* out_vals,
                                     uint32_t* out_n) {
  if (!idx) return fail(SGPU_EINVAL, "null argument");
  return expand_queries_host(idx->host, q_off, comps, vals, nq, cand_off, cand_ids, cand_w, alpha, t, num_threads, out_comps,
                             out_vals, out_n);
}

sgpu_status sgpu_diversify_documents(sgpu_index* idx, uint32_t replica, const uint64_t* q_off, const uint32_t* comps,
                                     const float* vals, uint32_t nq, const uint64_t* cand_off, const uint64_t* cand_ids, float lambda,
                                     float mu, uint32_t k, float* out_scores, float* out_penalties, uint64_t* out_doc_ids,
                                     uint32_t* out_n) {
  const DiversifyOut out{out_scores, out_penalties, out_doc_ids, out_n};
  return diversify_documents_device(idx, replica, q_off, comps, vals, nq, cand_off, cand_ids, lambda, mu, k, out);
}

sgpu_status sgpu_diversify_documents_host(const sgpu_index* idx, const uint64_t* q_off, const uint32_t* comps, const float* vals,
                                          uint32_t nq, const uint64_t* cand_off, const uint64_t* cand_ids, float lambda, float mu,
                                          uint32_t k, uint32_t num_threads, float* out_scores, float* out_penalties,
                                          uint64_t* out_doc_ids, uint32_t* out_n) {
  if (!idx) return fail(SGPU_EINVAL, "null argument");
  const DiversifyOut out{out_scores, out_penalties, out_doc_ids, out_n};
  return diversify_documents_host(idx->host, q_off, comps, vals, nq, cand_off, cand_ids, lambda, mu, k, num_threads, out);
}

sgpu_status sgpu_collapse_documents(sgpu_index* idx, uint32_t replica, const uint64_t* q_off, const uint32_t* comps, const float* vals,
                                    uint32_t nq, const uint64_t* cand_off, const uint64_t* cand_ids, const uint32_t* cand_groups,
                                    uint32_t m, uint32_t k, uint32_t* out_groups, float* out_scores, uint64_t* out_best_ids,
                                    float* out_best_scores, uint32_t* out_members, uint32_t* out_n) {
  const CollapseOut out{out_groups, out_scores, out_best_ids, out_best_scores, out_members, out_n};
  return collapse_documents_device(idx, replica, q_off, comps, vals, nq, cand_off, cand_ids, cand_groups, m, k, out);
}

sgpu_status sgpu_collapse_documents_host(const sgpu_index* idx, const uint64_t* q_off, const uint32_t* comps, const float* vals,
                                         uint32_t nq, const uint64_t* cand_off, const uint64_t* cand_ids, const uint32_t* cand_groups,
                                         uint32_t m, uint32_t k, uint32_t num_threads, uint32_t* out_groups, float* out_scores,
                                         uint64_t* out_best_ids, float* out_best_scores, uint32_t* out_members, uint32_t* out_n) {
  if (!idx) return fail(SGPU_EINVAL, "null argument");
  const CollapseOut out{out_groups, out_scores, out_best_ids, out_best_scores, out_members, out_n};
  return collapse_documents_host(idx->host, q_off, comps, vals, nq, cand_off, cand_ids, cand_groups, m, k, num_threads, out);
}

sgpu_status sgpu_fuse_documents(sgpu_index* idx, uint32_t replica, const uint64_t* q_off, const uint32_t* comps, const float* vals,
                                uint32_t nq, const uint64_t* cand_off, const uint64_t* cand_ids, const float* cand_ext, uint32_t method,
                                float w_sparse, float w_ext, float rrf_c, uint32_t k, float* out_scores, uint64_t* out_doc_ids,
                                float* out_sparse, float* out_ext, uint32_t* out_rank_sparse, uint32_t* out_rank_ext, uint32_t* out_n) {
  const FuseOut out{out_scores, out_doc_ids, out_sparse, out_ext, out_rank_sparse, out_rank_ext, out_n};
  return fuse_documents_device(idx, replica, q_off, comps, vals, nq, cand_off, cand_ids, cand_ext, method, w_sparse, w_ext, rrf_c, k, out);
}

sgpu_status sgpu_fuse_documents_host(const sgpu_index* idx, const uint64_t* q_off, const uint32_t* comps, const float* vals,
                                     uint32_t nq, const uint64_t* cand_off, const uint64_t* cand_ids, const float* cand_ext,
                                     uint32_t method, float w_sparse, float w_ext, float rrf_c, uint32_t k, uint32_t num_threads,
                                     float* out_scores, uint64_t* out_doc_ids, float* out_sparse, float* out_ext,
                                     uint32_t* out_rank_sparse, uint32_t* out_rank_ext, uint32_t* out_n) {
  if (!idx) return fail(SGPU_EINVAL, "null argument");
  const FuseOut out{out_scores, out_doc_ids, out_sparse, out_ext, out_rank_sparse, out_rank_ext, out_n};
  return fuse_documents_host(idx->host, q_off, comps, vals, nq, cand_off, cand_ids, cand_ext, method, w_sparse, w_ext, rrf_c, k,
                             num_threads, out);
}

// (not part of the boundary: what the last sgpu_fuse_documents call on `replica` measured - out8 in the slot order of
// sgpu_debug_collapse_stats; SGPU_EINVAL before the replica's first score call. tools/fuse_probe.py)
sgpu_status sgpu_debug_fuse_stats(sgpu_index* idx, uint32_t replica, double* out8) {
  SGPU_HOOK_OR(SGPU_EINVAL);
  if (!idx || !out8) return fail(SGPU_EINVAL, "null argument");
  if (!fuse_debug_stats(idx, replica, out8)) return fail(SGPU_EINVAL, "no fuse call has run on replica %u", replica);
  return SGPU_OK;
}

// (not part of the boundary: what the last sgpu_collapse_documents call on `replica` measured - out8 = {device ms of its score
// kernels, launches, 1 = dense table / 0 = hash table, grid, workgroup size and LDS bytes of the score kernel, device ms of the
// selection kernels, selection kernel launches}; SGPU_EINVAL before the replica's first score call. tools/collapse_probe.py)
sgpu_status sgpu_debug_collapse_stats(sgpu_index* idx, uint32_t replica, double* out8) {
  SGPU_HOOK_OR(SGPU_EINVAL);
  if (!idx || !out8) return fail(SGPU_EINVAL, "null argument");
  if (!collapse_debug_stats(idx, replica, out8)) return fail(SGPU_EINVAL, "no collapse call has run on replica %u", replica);
  return SGPU_OK;
}

// (not part of the boundary: what the last sgpu_diversify_documents call on `replica` measured - out8 = {device ms of its
// kernels, launches, grid of the last launch, workgroup size, LDS bytes, 1 = dense table / 0 = hash, rounds of its longest
// query, 0}; SGPU_EINVAL before the replica's first score call. tools/diversify_probe.py)
sgpu_status sgpu_debug_diversify_stats(sgpu_index* idx, uint32_t replica, double* out8) {
  SGPU_HOOK_OR(SGPU_EINVAL);
  if (!idx || !out8) return fail(SGPU_EINVAL, "null argument");
  if (!diversify_debug_stats(idx, replica, out8)) return fail(SGPU_EINVAL, "no diversify call has run on replica %u", replica);
  return SGPU_OK;
}

// (not part of the boundary: what the last sgpu_expand_queries call on `replica` measured - out8 = {device ms of its kernels,
// launches, 1 = table in LDS / 0 = in global memory, grid of the last launch, workgroup size, LDS bytes, bytes of the
// global tables, 0}; SGPU_EINVAL before the replica's first score or expand call. tools/expand_probe.py)
sgpu_status sgpu_debug_expand_stats(sgpu_index* idx, uint32_t replica, double* out8) {
  SGPU_HOOK_OR(SGPU_EINVAL);
  if (!idx || !out8) return fail(SGPU_EINVAL, "null argument");
  if (!expand_debug_stats(idx, replica, out8)) return fail(SGPU_EINVAL, "no expand call has run on replica %u", replica);
  return SGPU_OK;
}

// (not part of the boundary: what the last sgpu_score_documents / sgpu_rerank_documents / sgpu_explain_documents call on `replica` measured - out8 =
// {device ms of its score kernels, launches, 1 = dense table / 0 = hash table, grid, workgroup size, LDS bytes, device ms of
// the selection kernels, merge rounds}; SGPU_EINVAL before the replica's first score call. tools/score_probe.py,
// tools/rerank_probe.py)
sgpu_status sgpu_debug_score_stats(sgpu_index* idx, uint32_t replica, double* out8) {
  SGPU_HOOK_OR(SGPU_EINVAL);
  if (!idx || !out8) return fail(SGPU_EINVAL, "null argument");
  if (!score_debug_stats(idx, replica, out8)) return fail(SGPU_EINVAL, "no score call has run on replica %u", replica);
  return SGPU_OK;
}

// (not part of the boundary: the accumulate launches of the last sgpu_exact_search_device[_filtered] call on `replica`, one
// per chunk of queries whose candidates fit the candidate buffer - 256 MiB, or what SGPU_EXACT_CAND_BYTES says; SGPU_EINVAL
// before the replica's first exact call. tests/test_gpu_exact_edges.py)
sgpu_status sgpu_debug_exact_launches(sgpu_index* idx, uint32_t replica, uint32_t* out_launches) {
  SGPU_HOOK_OR(SGPU_EINVAL);
  if (!idx || !out_launches) return fail(SGPU_EINVAL, "null argument");
  if (!exact_debug_launches(idx, replica, out_launches)) return fail(SGPU_EINVAL, "no exact call has run on replica %u", replica);
  return SGPU_OK;
}

// (not part of the boundary: {kernel ms of the last sgpu_filter_create_terms call on `replica`, wall ms of the build of the
// exact file there, the file's bytes, its ranges}; SGPU_EINVAL before the replica has an exact file. tools/term_filter_probe.py)
sgpu_status sgpu_debug_term_filter_stats(sgpu_index* idx, uint32_t replica, double* out4) {
  SGPU_HOOK_OR(SGPU_EINVAL);
  if (!idx || !out4) return fail(SGPU_EINVAL, "null argument");
  if (!term_filter_debug_stats(idx, replica, out4)) return fail(SGPU_EINVAL, "replica %u has no exact file", replica);
  return SGPU_OK;
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
