// filter.hpp — what the launchers see of a document filter (sgpu_filter, filter.hip).
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

}  // namespace sgpu
