// abi.cpp — the extern "C" surface declared in include/seismic_hip.h: the product entry points and, behind
// sgpu_batch_search, the shards and segments a call is served in. (The test hooks are debug_hooks.cpp.)
#include <algorithm>
#include <chrono>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "call_cut.hpp"
#include "columns.hpp"
#include "device_calls.hpp"
#include "filter.hpp"
#include "host_index.hpp"
#include "term_filter.hpp"

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
  {   // (the column copies of the replicas that go; the host columns stay, and the next column call copies them again)
    std::lock_guard<std::mutex> lk(idx->column_mu);
    for (ColumnState* s : idx->column_state) column_state_free(s);
    idx->column_state.clear();
  }
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

uint64_t sgpu_index_device_bytes(const sgpu_index* idx) { return idx ? device_index_bytes(idx->dev) + column_device_bytes(idx) : 0; }

sgpu_status sgpu_index_set_column(sgpu_index* idx, uint32_t slot, uint32_t type, const void* values, uint64_t n) {
  return column_set(idx, slot, type, values, n);
}
sgpu_status sgpu_index_get_column(const sgpu_index* idx, uint32_t slot, uint32_t* type, const void** values, uint64_t* n) {
  return column_get(idx, slot, type, values, n);
}

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

// One segment of a shard on one replica (how a shard is cut into segments and a segment into chunks: call_cut.hpp): borrow
// a lane (its stream and recycled device batch), H2D of the queries, one kernel pass, D2H of the results. No allocation
// once the lane's batch has grown to the call's size; calls from different host threads take different lanes and overlap.
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
  const uint32_t nq = s1 - s0;
  // Would chunks of this call be planned on the device? ONE predicate with staged_launch (device_plan_dots), asked with the
  // size of a chunk of the two-way cut that answer leads to.
  const bool device_plans = device_plan_dots(d, params, std::min<uint32_t>(std::max<uint32_t>(nq / 2, 1u), kChunkQueriesMax), params.query_cut) != 0;
  const CutRule rule = cut_rule(cut_knobs(), shared, device_plans);
  // the lanes first: one, waited for, and as many more as the cut wants and are free - the cut is then made for them
  Lane* lanes[8];
  const uint32_t wanted = cut_jobs(nq, rule.chunk_min, rule.chunk_max);
  lanes[0] = lane_acquire(d);
  uint32_t n_lanes = 1;
  while (n_lanes < wanted && (lanes[n_lanes] = lane_try_acquire(d)) != nullptr) ++n_lanes;
  uint32_t n_jobs, b[8][2];     // chunk j: queries [s0 + b[j][0], s0 + b[j][1]) on lanes[j]
  std::vector<uint64_t> off;   // a chunk's offsets, rebased (sized here: nothing below allocates host memory)
  for (;;) {
    n_jobs = cut_segment(nq, rule.chunk_min, rule.chunk_max, n_lanes, cut_knobs().first_pm, b);
    uint32_t longest = 0;
    for (uint32_t j = 0; j < n_jobs; ++j)
      if (s0 + b[j][0] != 0) longest = std::max(longest, b[j][1] - b[j][0]);
    if (n_jobs == 1 && s0 == 0) break;
    try {
      off.resize((size_t)longest + 1);
      break;
    } catch (const std::exception&) {
      if (n_lanes == 1) {
        lane_release(d, lanes[0]);
        return fail(SGPU_ENOMEM, "out of host memory cutting a query batch");
      }
      while (n_lanes > 1) lane_release(d, lanes[--n_lanes]);   // (one launch, and another try)
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
    const uint32_t q0 = s0 + b[j][0], q1 = s0 + b[j][1];
    const uint64_t* qo = q_off;
    if (q0 != 0) {   // (a chunk that starts at query 0 uses the caller's offsets as they are)
      rebase_offsets(q_off, q0, q1, off.data());
      qo = off.data();
    }
    st = staged_launch(d, lanes[j], dim, qo, comps ? comps + q_off[q0] : nullptr, vals ? vals + q_off[q0] : nullptr, q1 - q0,
                       q_base + q0, params, lane_scratch(lanes[j]), j + 1 < n_jobs ? 2u : (shared ? 1u : 0u), flt, j);
    if (st == SGPU_OK) ++launched;
    else msg = last_error();
  }
  for (uint32_t j = 0; j < launched; ++j) {   // every launched chunk is waited for, also after an error
    const uint32_t q0 = s0 + b[j][0];
    const sgpu_status fs = staged_finish(d, lanes[j], *lane_scratch(lanes[j]), out_scores + (size_t)q0 * k,
                                         out_doc_ids + (size_t)q0 * k, out_n + q0);
    if (fs != SGPU_OK && st == SGPU_OK) {
      st = fs;
      msg = last_error();
    }
  }
  for (uint32_t j = 0; j < n_lanes; ++j) lane_release(d, lanes[j]);
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
    st = search_segment(d, dim, q_off, comps, vals, split_at(nq, n_seg, s), split_at(nq, n_seg, s + 1), q_base, params, out_scores,
                        out_doc_ids, out_n, flt, in_flight.shared);
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
      const uint32_t q0 = split_at(nq, n_rep, r), q1 = split_at(nq, n_rep, r + 1);
      offs[r].resize(q1 - q0 + 1);
      rebase_offsets(q_off, q0, q1, offs[r].data());
    }
    auto shard = [&](uint32_t r) {
      const uint32_t q0 = split_at(nq, n_rep, r), q1 = split_at(nq, n_rep, r + 1);
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
sgpu_status sgpu_filter_create_columns(sgpu_index* idx, uint32_t replica, const sgpu_column_clause* clauses, uint32_t n_clauses,
                                       uint32_t min_should, const uint32_t* set_values, uint32_t n_set_values, const sgpu_filter* within,
                                       sgpu_filter** out) {
  return column_filter_device(idx, replica, clauses, n_clauses, min_should, set_values, n_set_values, within, out);
}
sgpu_status sgpu_filter_create_columns_host(sgpu_index* idx, const sgpu_column_clause* clauses, uint32_t n_clauses, uint32_t min_should,
                                            const uint32_t* set_values, uint32_t n_set_values, const sgpu_filter* within,
                                            uint32_t num_threads, sgpu_filter** out) {
  return column_filter_host(idx, clauses, n_clauses, min_should, set_values, n_set_values, within, num_threads, out);
}
sgpu_status sgpu_facet_counts(sgpu_index* idx, uint32_t replica, uint32_t slot, const sgpu_filter* filter, uint32_t t,
                              uint32_t* out_values, uint64_t* out_counts, uint32_t* out_n, uint64_t* out_distinct, uint64_t* out_docs) {
  return facet_counts_device(idx, replica, slot, filter, t, out_values, out_counts, out_n, out_distinct, out_docs);
}
sgpu_status sgpu_facet_counts_host(const sgpu_index* idx, uint32_t slot, const sgpu_filter* filter, uint32_t t, uint32_t num_threads,
                                   uint32_t* out_values, uint64_t* out_counts, uint32_t* out_n, uint64_t* out_distinct,
                                   uint64_t* out_docs) {
  return facet_counts_host(idx, slot, filter, t, num_threads, out_values, out_counts, out_n, out_distinct, out_docs);
}
sgpu_status sgpu_column_stats(sgpu_index* idx, uint32_t replica, uint32_t slot, const sgpu_filter* filter, struct sgpu_column_stats* out) {
  return column_stats_device(idx, replica, slot, filter, out);
}
sgpu_status sgpu_column_stats_host(const sgpu_index* idx, uint32_t slot, const sgpu_filter* filter, uint32_t num_threads,
                                   struct sgpu_column_stats* out) {
  return column_stats_host(idx, slot, filter, num_threads, out);
}
sgpu_status sgpu_column_histogram(sgpu_index* idx, uint32_t replica, uint32_t slot, const sgpu_filter* filter, const uint32_t* edges,
                                  uint32_t n_edges, uint64_t* out_counts, uint64_t* out_below, uint64_t* out_above, uint64_t* out_nan,
                                  uint64_t* out_docs) {
  return column_histogram_device(idx, replica, slot, filter, edges, n_edges, out_counts, out_below, out_above, out_nan, out_docs);
}
sgpu_status sgpu_column_histogram_host(const sgpu_index* idx, uint32_t slot, const sgpu_filter* filter, const uint32_t* edges,
                                       uint32_t n_edges, uint32_t num_threads, uint64_t* out_counts, uint64_t* out_below,
                                       uint64_t* out_above, uint64_t* out_nan, uint64_t* out_docs) {
  return column_histogram_host(idx, slot, filter, edges, n_edges, num_threads, out_counts, out_below, out_above, out_nan, out_docs);
}
sgpu_status sgpu_column_top(sgpu_index* idx, uint32_t replica, uint32_t slot, const sgpu_filter* filter, uint32_t t, uint32_t order,
                            uint32_t* out_doc_ids, uint32_t* out_value_bits, uint32_t* out_n, uint64_t* out_valid, uint64_t* out_docs) {
  return column_top_device(idx, replica, slot, filter, t, order, out_doc_ids, out_value_bits, out_n, out_valid, out_docs);
}
sgpu_status sgpu_column_top_host(const sgpu_index* idx, uint32_t slot, const sgpu_filter* filter, uint32_t t, uint32_t order,
                                 uint32_t num_threads, uint32_t* out_doc_ids, uint32_t* out_value_bits, uint32_t* out_n,
                                 uint64_t* out_valid, uint64_t* out_docs) {
  return column_top_host(idx, slot, filter, t, order, num_threads, out_doc_ids, out_value_bits, out_n, out_valid, out_docs);
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

}  // extern "C"
