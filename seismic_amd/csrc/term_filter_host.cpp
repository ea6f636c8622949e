// term_filter_host.cpp — term filters on the host: the argument checks of sgpu_filter_create_terms[_host] and the host twin,
// a parallel scan over the documents of the host forward arrays. The host twin defines the bits; the device call
// (term_filter.hip) returns the same words.
#include <algorithm>
#include <cmath>
#include <new>
#include <vector>

#include <omp.h>

#include "term_filter.hpp"

namespace sgpu {

sgpu_status term_check_args(const sgpu_index* idx, const sgpu_term_clause* clauses, uint32_t n_clauses, const sgpu_filter* within,
                            sgpu_filter** out) {
  if (!idx || !out || (n_clauses && !clauses)) return fail(SGPU_EINVAL, "null argument");
  *out = nullptr;
  for (uint32_t i = 0; i < n_clauses; ++i) {
    const sgpu_term_clause& c = clauses[i];
    if (c.occur > SGPU_TERM_SHOULD) return fail(SGPU_EINVAL, "term filter: clause %u: occur = %u is not one of SGPU_TERM_*", i, c.occur);
    if (c.component >= idx->host.dim)
      return fail(SGPU_EINVAL, "term filter: clause %u: component %u >= dim = %llu", i, c.component, (unsigned long long)idx->host.dim);
    if (std::isnan(c.min_weight)) return fail(SGPU_EINVAL, "term filter: clause %u: min_weight is NaN", i);
  }
  if (n_clauses > kTermMaxClauses) return fail(SGPU_ELIMIT, "term filter: %u clauses exceed the limit of %u", n_clauses, kTermMaxClauses);
  if (within && filter_index(within) != idx) return fail(SGPU_EINVAL, "the filter was created on another index");
  return SGPU_OK;
}

sgpu_status term_filter_host(sgpu_index* idx, const sgpu_term_clause* clauses, uint32_t n_clauses, uint32_t min_should,
                             const sgpu_filter* within, uint32_t num_threads, sgpu_filter** out) {
  const sgpu_status cst = term_check_args(idx, clauses, n_clauses, within, out);
  if (cst != SGPU_OK) return cst;
  const HostIndex& h = idx->host;
  const uint64_t n_docs = h.n_docs, n_words = std::max<uint64_t>((n_docs + 31) / 32, 1);
  const uint32_t* wbits = within ? filter_host_bits(within) : nullptr;
  const int nt = num_threads ? (int)num_threads : default_host_threads(omp_get_max_threads());
  try {
    // the clauses in ascending component order: a document's components are strictly ascending, so one pass over the
    // sorted clauses with a search in what is left of the document finds every (clause, stored value) pair
    std::vector<sgpu_term_clause> cl(clauses, clauses + n_clauses);
    std::stable_sort(cl.begin(), cl.end(), [](const sgpu_term_clause& a, const sgpu_term_clause& b) { return a.component < b.component; });
    uint32_t n_must = 0, n_should = 0;
    for (const sgpu_term_clause& c : cl) {
      n_must += c.occur == SGPU_TERM_MUST;
      n_should += c.occur == SGPU_TERM_SHOULD;
    }
    std::vector<uint32_t> bits((size_t)n_words, 0u);
    uint64_t count = 0;
    if (min_should <= n_should) {   // (else: the empty set)
#pragma omp parallel for num_threads(nt) schedule(dynamic, 256) reduction(+ : count)
      for (uint64_t w = 0; w < n_words; ++w) {
        uint32_t word = 0;
        const uint64_t d0 = w * 32, d1 = std::min<uint64_t>(d0 + 32, n_docs);
        for (uint64_t d = d0; d < d1; ++d) {
          if (wbits && !((wbits[w] >> (d - d0)) & 1u)) continue;
          uint64_t lo = h.fwd_offsets[d];
          const uint64_t end = h.fwd_offsets[d + 1];
          uint32_t must = 0, should = 0;
          bool banned = false;
          for (size_t j = 0; j < cl.size() && lo < end && !banned;) {
            const uint32_t c = cl[j].component;
            // first stored component >= c in [lo, end)
            uint64_t a = lo, b = end;
            while (a < b) {
              const uint64_t m = a + (b - a) / 2;
              if (h.comp(m) < c) a = m + 1; else b = m;
            }
            lo = a;
            const bool stored = lo < end && h.comp(lo) == c;
            const float v = stored ? h.val(lo) : 0.0f;
            for (; j < cl.size() && cl[j].component == c; ++j) {
              if (!stored || !(v >= cl[j].min_weight)) continue;
              if (cl[j].occur == SGPU_TERM_MUST) ++must;
              else if (cl[j].occur == SGPU_TERM_SHOULD) ++should;
              else banned = true;
            }
          }
          if (!banned && must == n_must && should >= min_should) word |= 1u << (d - d0);
        }
        bits[(size_t)w] = word;
        count += (uint64_t)__builtin_popcount(word);
      }
    }
    return filter_from_bits(idx, std::move(bits), count, out);
  } catch (const std::bad_alloc&) {
    return fail(SGPU_ENOMEM, "out of host memory");
  }
}

}  // namespace sgpu
