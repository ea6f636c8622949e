// device_calls.hpp — what the host side (abi.cpp, debug_hooks.cpp) calls of the translation units that hold a resident index
// and launch searches on it: device_index.hip, launch_plan.hip, batch.hip, staged.hip. Each of them sees these declarations
// through device_index.hpp, which has the structs that are only named here. Compiles without HIP.
#pragma once
#include <cstdint>
#include <vector>

#include "host_index.hpp"

struct sgpu_batch;

namespace sgpu {

struct Lane;

// ---- device_index.hip: residency, the lanes calls run on
int device_count();
sgpu_status device_index_upload(const HostIndex& h, int device, DeviceIndex** out);
sgpu_status device_index_clone(const DeviceIndex* src, int device, DeviceIndex** out);
void device_index_free(DeviceIndex* d);
uint64_t device_index_bytes(const DeviceIndex* d);
sgpu_status device_index_set_knn(DeviceIndex* d, const std::vector<uint32_t>& knn, uint32_t knn_dim);
Lane* lane_acquire(DeviceIndex* d);
Lane* lane_try_acquire(DeviceIndex* d);
void lane_release(DeviceIndex* d, Lane* l);
Lane* lane_main(DeviceIndex* d);
sgpu_batch** lane_scratch(Lane* l);
bool call_enter(DeviceIndex* d);
void call_exit(DeviceIndex* d);

// ---- launch_plan.hip (device_plan_dots takes d->mu itself)
uint32_t device_plan_dots(DeviceIndex* d, const sgpu_search_params& sp, uint32_t nq, uint32_t cut);
sgpu_status debug_plan(const HostIndex& h, const uint64_t* q_off, const uint32_t* comps, const float* vals, uint32_t nq,
                       uint32_t query_cut, uint32_t* order_out, uint32_t* out3, uint32_t* hash_ok_out = nullptr,
                       uint32_t* seeds_out = nullptr);
sgpu_status debug_device_plan(DeviceIndex* d, const uint64_t* q_off, const uint32_t* comps, const float* vals, uint32_t nq,
                              uint32_t query_cut, uint32_t* order_out, uint32_t* out3);

// ---- batch.hip: the device-resident batch API, and the calls that run on the main lane
sgpu_status batch_create(DeviceIndex* d, Lane* lane, uint64_t dim, const uint64_t* q_off, const uint32_t* comps,
                         const float* vals, uint32_t nq, uint32_t k_max, sgpu_batch** out);
void batch_free(sgpu_batch* b);
const DeviceIndex* batch_replica(const sgpu_batch* b);
sgpu_status batch_run(DeviceIndex* d, Lane* lane, sgpu_batch* b, const sgpu_search_params& sp, uint32_t mode,
                      int sync, sgpu_launch_stats* stats);
sgpu_status batch_sync(DeviceIndex* d, sgpu_launch_stats* stats);
sgpu_status batch_fetch(DeviceIndex* d, Lane* lane, sgpu_batch* b, uint32_t k, float* out_scores, uint64_t* out_ids,
                        uint32_t* out_n);
sgpu_status batch_fetch_stats(DeviceIndex* d, sgpu_batch* b, uint32_t* out);
uint32_t coop_trace_dump(DeviceIndex* d, uint64_t* out, uint32_t cap);
uint32_t debug_lane_variant(DeviceIndex* d, int32_t lane, uint32_t* out4);
sgpu_status summary_distances(DeviceIndex* d, const HostIndex& h, uint32_t list, const uint32_t* comps,
                              const float* vals, uint32_t nnz, float* out_dots, uint32_t* out_nb);
sgpu_status build_knn_on_device(DeviceIndex* d, HostIndex& h, uint32_t nknn);

// ---- staged.hip: one chunk of an entry-point call on a pool lane
// (followed: 0 nothing behind this chunk, 1 other calls, 2 the call's own next chunk; chunk: which launch of its call,
// 0 = the first or only one)
sgpu_status staged_launch(DeviceIndex* d, Lane* lane, uint64_t dim, const uint64_t* q_off, const uint32_t* comps,
                          const float* vals, uint32_t nq, uint32_t q_base, const sgpu_search_params& sp, sgpu_batch** slot,
                          uint32_t followed, const FilterRef* flt, uint32_t chunk);
sgpu_status staged_finish(DeviceIndex* d, Lane* lane, sgpu_batch* b, float* out_scores, uint64_t* out_ids, uint32_t* out_n);
double*& call_timing();
uint32_t debug_lane_chunk(DeviceIndex* d, uint32_t lane, uint32_t* info4, uint32_t* order_out, uint32_t cap);

}  // namespace sgpu
