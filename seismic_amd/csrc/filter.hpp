// filter.hpp — what the launchers and the C ABI see of a document filter (sgpu_filter, filter.hip). Compiles without HIP.
#pragma once
#include <cstdint>

#include "device_types.hpp"
#include "host_index.hpp"

namespace sgpu {

// A filter's view of the index on one replica: the index's DevView with the three posting arrays (and the kNN graph)
// replaced by compacted copies that hold the allowed documents' postings only; everything else is the replica's own.
struct FilterDeviceView {
  DevView view;
  const uint32_t* bits;   // the allowed set: bit d of word d / 32, ceil(n_docs / 32) words
  uint64_t count;         // |A|
};

// The filter's view on `replica`, built there on first use (or when the index's generation moved on since it was built).
sgpu_status filter_view(const sgpu_filter* f, uint32_t replica, const FilterDeviceView** out);

// The filter calls of the C ABI (sgpu_filter_*) and two test hooks: the build times of the filter's view on `replica`
// (false: not built), and the posting arrays a search on `replica` walks (sgpu_debug_posting_view).
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
