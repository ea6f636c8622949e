// column_host.cpp — document columns on the host: sgpu_index_set_column / get_column, the argument checks of the column
// filter and of the facet counts, the plan both twins evaluate (bounds and IN values as keys, columns.hpp) and the two host
// twins. The host twins define the words and the rows; the device calls (column_filter.hip, facet_counts.hip) return the
// same.
#include <algorithm>
#include <new>
#include <vector>

#include <omp.h>

#include "columns.hpp"
#include "filter.hpp"

namespace sgpu {

namespace {

struct Replace {
  HostColumn* col;
  std::vector<uint32_t>* values;   // null: drop
  uint32_t type, max_u32;
  uint64_t generation;
};
void replace_column(void* p) {
  Replace* r = static_cast<Replace*>(p);
  if (r->values) {
    r->col->values.swap(*r->values);
    r->col->type = r->type;
    r->col->max_u32 = r->max_u32;
    r->col->generation = r->generation;
  } else {
    std::vector<uint32_t>().swap(r->col->values);
    r->col->type = 0;
    r->col->max_u32 = 0;
    r->col->generation = 0;
  }
}

}  // namespace

sgpu_status column_set(sgpu_index* idx, uint32_t slot, uint32_t type, const void* values, uint64_t n) {
  if (!idx) return fail(SGPU_EINVAL, "null argument");
  if (slot >= SGPU_MAX_COLUMNS) return fail(SGPU_EINVAL, "column slot %u >= SGPU_MAX_COLUMNS = %u", slot, (uint32_t)SGPU_MAX_COLUMNS);
  const bool drop = !values && n == 0;
  std::vector<uint32_t> copy;
  uint32_t max_u32 = 0;
  if (!drop) {
    if (!values) return fail(SGPU_EINVAL, "null argument");
    if (type > SGPU_COL_F32) return fail(SGPU_EINVAL, "column type %u is not one of SGPU_COL_*", type);
    if (n != idx->host.n_docs)
      return fail(SGPU_EINVAL, "column of %llu values for an index of %llu documents", (unsigned long long)n, (unsigned long long)idx->host.n_docs);
    try {
      const uint32_t* v = static_cast<const uint32_t*>(values);
      copy.assign(v, v + n);
      if (type == SGPU_COL_U32)
        for (uint64_t i = 0; i < n; ++i) max_u32 = std::max(max_u32, v[i]);
    } catch (const std::bad_alloc&) {
      return fail(SGPU_ENOMEM, "out of host memory");
    }
  }
  std::lock_guard<std::mutex> lk(idx->column_mu);
  Replace r{&idx->columns[slot], drop ? nullptr : &copy, type, max_u32, ++idx->column_generation};
  column_states_locked(idx, slot, drop, replace_column, &r);
  return SGPU_OK;
}

sgpu_status column_get(const sgpu_index* idx, uint32_t slot, uint32_t* type, const void** values, uint64_t* n) {
  if (!idx || !type || !values || !n) return fail(SGPU_EINVAL, "null argument");
  if (slot >= SGPU_MAX_COLUMNS) return fail(SGPU_EINVAL, "column slot %u >= SGPU_MAX_COLUMNS = %u", slot, (uint32_t)SGPU_MAX_COLUMNS);
  const HostColumn& c = idx->columns[slot];
  const bool set = c.generation != 0;
  *type = set ? c.type : 0u;
  *values = set ? c.values.data() : nullptr;   // (an index of no documents: a set column of no values)
  *n = set ? c.values.size() : 0;
  return SGPU_OK;
}

sgpu_status column_check_args(const sgpu_index* idx, const sgpu_column_clause* clauses, uint32_t n_clauses, const uint32_t* set_values,
                              uint32_t n_set_values, const sgpu_filter* within, sgpu_filter** out) {
  if (!idx || !out || (n_clauses && !clauses) || (n_set_values && !set_values)) return fail(SGPU_EINVAL, "null argument");
  *out = nullptr;
  for (uint32_t i = 0; i < n_clauses; ++i) {
    const sgpu_column_clause& c = clauses[i];
    if (c.occur > SGPU_TERM_SHOULD) return fail(SGPU_EINVAL, "column filter: clause %u: occur = %u is not one of SGPU_TERM_*", i, c.occur);
    if (c.op > SGPU_COLOP_IN) return fail(SGPU_EINVAL, "column filter: clause %u: op = %u is not one of SGPU_COLOP_*", i, c.op);
    if (c.slot >= SGPU_MAX_COLUMNS)
      return fail(SGPU_EINVAL, "column filter: clause %u: slot %u >= SGPU_MAX_COLUMNS = %u", i, c.slot, (uint32_t)SGPU_MAX_COLUMNS);
    const HostColumn& col = idx->columns[c.slot];
    if (col.generation == 0) return fail(SGPU_EINVAL, "column filter: clause %u: slot %u holds no column", i, c.slot);
    if (c.op == SGPU_COLOP_RANGE) {
      if (col.type == SGPU_COL_F32 && (column_bits_nan(c.lo_bits) || column_bits_nan(c.hi_bits)))
        return fail(SGPU_EINVAL, "column filter: clause %u: a bound is NaN", i);
    } else {
      if ((uint64_t)c.set_begin + c.set_count > n_set_values)
        return fail(SGPU_EINVAL, "column filter: clause %u: set_begin + set_count = %llu > n_set_values = %u", i,
                    (unsigned long long)c.set_begin + c.set_count, n_set_values);
      if (col.type == SGPU_COL_F32)
        for (uint32_t j = 0; j < c.set_count; ++j)
          if (column_bits_nan(set_values[c.set_begin + j])) return fail(SGPU_EINVAL, "column filter: clause %u: set value %u is NaN", i, j);
    }
  }
  if (n_clauses > kColMaxClauses) return fail(SGPU_ELIMIT, "column filter: %u clauses exceed the limit of %u", n_clauses, kColMaxClauses);
  if (n_set_values > kColMaxSetValues)
    return fail(SGPU_ELIMIT, "column filter: %u set values exceed the limit of %u", n_set_values, kColMaxSetValues);
  return foreign_filter(idx, within);
}

void column_plan(const sgpu_index* idx, const sgpu_column_clause* clauses, uint32_t n_clauses, const uint32_t* set_values, ColPlan* plan) {
  std::vector<uint32_t> order(n_clauses);
  for (uint32_t i = 0; i < n_clauses; ++i) order[i] = i;
  std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return clauses[a].slot < clauses[b].slot; });
  plan->clauses.clear();
  plan->keys.clear();
  plan->n_must = plan->n_should = 0;
  for (uint32_t x = 0; x < n_clauses; ++x) {
    const sgpu_column_clause& c = clauses[order[x]];
    const uint32_t type = idx->columns[c.slot].type;
    ColClause p{};
    p.slot = c.slot;
    p.type = type;
    p.occur = c.occur;
    p.op = c.op;
    p.fresh = x == 0 || clauses[order[x - 1]].slot != c.slot;
    if (c.op == SGPU_COLOP_RANGE) {
      p.lo = column_key(type, c.lo_bits);
      p.hi = column_key(type, c.hi_bits);
    } else {
      p.begin = (uint32_t)plan->keys.size();
      p.count = c.set_count;
      for (uint32_t j = 0; j < c.set_count; ++j) plan->keys.push_back(column_key(type, set_values[c.set_begin + j]));
      std::sort(plan->keys.begin() + p.begin, plan->keys.end());
    }
    plan->n_must += c.occur == SGPU_TERM_MUST;
    plan->n_should += c.occur == SGPU_TERM_SHOULD;
    plan->clauses.push_back(p);
  }
}

sgpu_status column_filter_host(sgpu_index* idx, const sgpu_column_clause* clauses, uint32_t n_clauses, uint32_t min_should,
                               const uint32_t* set_values, uint32_t n_set_values, const sgpu_filter* within, uint32_t num_threads,
                               sgpu_filter** out) {
  const sgpu_status cst = column_check_args(idx, clauses, n_clauses, set_values, n_set_values, within, out);
  if (cst != SGPU_OK) return cst;
  const uint64_t n_docs = idx->host.n_docs, n_words = std::max<uint64_t>((n_docs + 31) / 32, 1);
  const uint32_t* wbits = within ? filter_host_bits(within) : nullptr;
  const int nt = num_threads ? (int)num_threads : default_host_threads(omp_get_max_threads());
  try {
    ColPlan plan;
    column_plan(idx, clauses, n_clauses, set_values, &plan);
    for (ColClause& c : plan.clauses) c.col = idx->columns[c.slot].values.data();
    const uint32_t* keys = plan.keys.data();
    std::vector<uint32_t> bits((size_t)n_words, 0u);
    uint64_t count = 0;
    if (min_should <= plan.n_should) {   // (else: the empty set)
#pragma omp parallel for num_threads(nt) schedule(static) reduction(+ : count)
      for (uint64_t w = 0; w < n_words; ++w) {
        uint32_t word = 0;
        const uint64_t d0 = w * 32, d1 = std::min<uint64_t>(d0 + 32, n_docs);
        for (uint64_t d = d0; d < d1; ++d) {
          if (wbits && !((wbits[w] >> (d - d0)) & 1u)) continue;
          uint32_t must = 0, should = 0, key = 0;
          bool banned = false;
          for (const ColClause& c : plan.clauses) {
            if (c.fresh) key = column_key(c.type, c.col[d]);
            const bool m = c.op == SGPU_COLOP_RANGE ? (c.lo <= key && key <= c.hi)
                                                    : std::binary_search(keys + c.begin, keys + c.begin + c.count, key);
            if (!m) continue;
            if (c.occur == SGPU_TERM_MUST) ++must;
            else if (c.occur == SGPU_TERM_SHOULD) ++should;
            else banned = true;
          }
          if (!banned && must == plan.n_must && should >= min_should) word |= 1u << (d - d0);
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

sgpu_status facet_check_args(const sgpu_index* idx, uint32_t slot, const sgpu_filter* filter, uint32_t t, const uint32_t* out_values,
                             const uint64_t* out_counts, const uint32_t* out_n, const uint64_t* out_distinct, const uint64_t* out_docs) {
  if (!idx || !out_values || !out_counts || !out_n || !out_distinct || !out_docs) return fail(SGPU_EINVAL, "null argument");
  if (t == 0 || t > kFacetMaxT) return fail(SGPU_EINVAL, "facet counts: t = %u is outside 1..%u", t, kFacetMaxT);
  if (slot >= SGPU_MAX_COLUMNS) return fail(SGPU_EINVAL, "facet counts: slot %u >= SGPU_MAX_COLUMNS = %u", slot, (uint32_t)SGPU_MAX_COLUMNS);
  const HostColumn& col = idx->columns[slot];
  if (col.generation == 0) return fail(SGPU_EINVAL, "facet counts: slot %u holds no column", slot);
  if (col.type != SGPU_COL_U32) return fail(SGPU_EINVAL, "facet counts: the column of slot %u is not SGPU_COL_U32", slot);
  const sgpu_status fst = foreign_filter(idx, filter);
  if (fst != SGPU_OK) return fst;
  if (col.max_u32 >= kFacetMaxBins)
    return fail(SGPU_ELIMIT, "facet counts: the column's largest value %u is not below the limit of %u (1 << 22)", col.max_u32, kFacetMaxBins);
  return SGPU_OK;
}

sgpu_status facet_counts_host(const sgpu_index* idx, uint32_t slot, const sgpu_filter* filter, uint32_t t, uint32_t num_threads,
                              uint32_t* out_values, uint64_t* out_counts, uint32_t* out_n, uint64_t* out_distinct, uint64_t* out_docs) {
  const sgpu_status cst = facet_check_args(idx, slot, filter, t, out_values, out_counts, out_n, out_distinct, out_docs);
  if (cst != SGPU_OK) return cst;
  const HostColumn& col = idx->columns[slot];
  const uint64_t n_docs = idx->host.n_docs, n_words = (n_docs + 31) / 32;
  const uint32_t* fbits = filter ? filter_host_bits(filter) : nullptr;
  const uint32_t* v = col.values.data();
  const uint32_t bins = col.max_u32 + 1u;
  const int nt = num_threads ? (int)num_threads : default_host_threads(omp_get_max_threads());
  try {
    // the table: the threads add with atomics; small tables (contended: few values) are counted per thread first
    std::vector<uint32_t> table(bins, 0u);
    const bool local = bins <= 65536u;
    std::vector<uint32_t> locals(local ? (size_t)nt * bins : 0, 0u);   // (allocated here: nothing throws inside the team)
#pragma omp parallel num_threads(nt)
    {
      uint32_t* mine = local ? locals.data() + (size_t)omp_get_thread_num() * bins : nullptr;
      uint32_t* dst = local ? mine : table.data();
#pragma omp for schedule(static)
      for (uint64_t w = 0; w < n_words; ++w) {
        const uint64_t d0 = w * 32, d1 = std::min<uint64_t>(d0 + 32, n_docs);
        const uint32_t word = fbits ? fbits[w] : 0xffffffffu;
        if (!word) continue;
        for (uint64_t d = d0; d < d1; ++d) {
          if (!((word >> (d - d0)) & 1u)) continue;
          if (local) ++dst[v[d]];
          else __atomic_fetch_add(&dst[v[d]], 1u, __ATOMIC_RELAXED);
        }
      }
      if (local)
        for (uint32_t b = 0; b < bins; ++b)
          if (mine[b]) __atomic_fetch_add(&table[b], mine[b], __ATOMIC_RELAXED);
    }
    // the rows: (count descending, value ascending) as one descending 64-bit key
    std::vector<uint64_t> keys;
    for (uint32_t b = 0; b < bins; ++b)
      if (table[b]) keys.push_back((uint64_t)table[b] << 32 | (uint32_t)~b);
    const uint32_t n = (uint32_t)std::min<uint64_t>(t, keys.size());
    std::partial_sort(keys.begin(), keys.begin() + n, keys.end(), [](uint64_t a, uint64_t b) { return a > b; });
    for (uint32_t i = 0; i < t; ++i) {
      out_values[i] = i < n ? ~(uint32_t)keys[i] : 0u;
      out_counts[i] = i < n ? keys[i] >> 32 : 0ull;
    }
    *out_n = n;
    *out_distinct = keys.size();
    *out_docs = filter ? filter_count(filter) : n_docs;
    return SGPU_OK;
  } catch (const std::bad_alloc&) {
    return fail(SGPU_ENOMEM, "out of host memory");
  }
}

}  // namespace sgpu
