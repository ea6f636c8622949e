// term_filter.hpp — what term_filter_host.cpp (checks, host twin), term_filter.hip (device call) and filter.hip (the filter
// itself) share of sgpu_filter_create_terms[_host].
#pragma once
#include <cstdint>
#include <vector>

#include "host_index.hpp"

namespace sgpu {

constexpr uint32_t kTermMaxClauses = 1024;

// filter.hip
const sgpu_index* filter_index(const sgpu_filter* f);
const uint32_t* filter_host_bits(const sgpu_filter* f);
// (the check of every entry point that takes an index and a filter, which may be null)
inline sgpu_status foreign_filter(const sgpu_index* idx, const sgpu_filter* filter) {
  return filter && filter_index(filter) != idx ? fail(SGPU_EINVAL, "the filter was created on another index") : SGPU_OK;
}
// A filter of `idx` from a finished bitmap: ceil(n_docs / 32) words (at least one), the bits past n_docs zero; count = its
// popcount. `bits` is moved from.
sgpu_status filter_from_bits(sgpu_index* idx, std::vector<uint32_t>&& bits, uint64_t count, sgpu_filter** out);

// term_filter_host.cpp: checks 1 - 4 of both calls, in the header's order (*out is set to null once it is known not to be)
sgpu_status term_check_args(const sgpu_index* idx, const sgpu_term_clause* clauses, uint32_t n_clauses, const sgpu_filter* within,
                            sgpu_filter** out);
sgpu_status term_filter_host(sgpu_index* idx, const sgpu_term_clause* clauses, uint32_t n_clauses, uint32_t min_should,
                             const sgpu_filter* within, uint32_t num_threads, sgpu_filter** out);
// term_filter.hip
sgpu_status term_filter_device(sgpu_index* idx, uint32_t replica, const sgpu_term_clause* clauses, uint32_t n_clauses,
                               uint32_t min_should, const sgpu_filter* within, sgpu_filter** out);
bool term_filter_debug_stats(sgpu_index* idx, uint32_t replica, double* out4);

}  // namespace sgpu
