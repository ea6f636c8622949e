// column_host.cpp — document columns on the host: sgpu_index_set_column / get_column, the argument checks of the column
// filter, of the facet counts and of the aggregations, the plan both filter twins evaluate (bounds and IN values as keys,
// columns.hpp) and the host twins: filter, facet counts, stats, histogram, top. The host twins define the words, the
// rows and the bits; the device calls (column_filter.hip, facet_counts.hip, column_aggregate.hip, column_top.hip) return
// the same.
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

// ---- the aggregations: sgpu_column_stats / _histogram / _top ------------------------------------------------------------
namespace {

// (the part of check 1 the three calls share: the slot; `call` names the call in the message)
sgpu_status agg_check_slot(const sgpu_index* idx, uint32_t slot, const char* call) {
  if (slot >= SGPU_MAX_COLUMNS) return fail(SGPU_EINVAL, "%s: slot %u >= SGPU_MAX_COLUMNS = %u", call, slot, (uint32_t)SGPU_MAX_COLUMNS);
  if (idx->columns[slot].generation == 0) return fail(SGPU_EINVAL, "%s: slot %u holds no column", call, slot);
  return SGPU_OK;
}

inline bool filter_bit(const uint32_t* fbits, uint64_t d) { return !fbits || ((fbits[d >> 5] >> (d & 31u)) & 1u); }

}  // namespace

sgpu_status stats_check_args(const sgpu_index* idx, uint32_t slot, const sgpu_filter* filter, const struct sgpu_column_stats* out) {
  if (!idx || !out) return fail(SGPU_EINVAL, "null argument");
  const sgpu_status st = agg_check_slot(idx, slot, "column stats");
  if (st != SGPU_OK) return st;
  return foreign_filter(idx, filter);
}

sgpu_status histogram_check_args(const sgpu_index* idx, uint32_t slot, const sgpu_filter* filter, const uint32_t* edges, uint32_t n_edges,
                                 const uint64_t* out_counts, const uint64_t* out_below, const uint64_t* out_above, const uint64_t* out_nan,
                                 const uint64_t* out_docs) {
  if (!idx || !edges || !out_counts || !out_below || !out_above || !out_nan || !out_docs) return fail(SGPU_EINVAL, "null argument");
  const sgpu_status st = agg_check_slot(idx, slot, "column histogram");
  if (st != SGPU_OK) return st;
  if (n_edges < 2 || n_edges > kAggMaxBuckets + 1)
    return fail(SGPU_ELIMIT, "column histogram: n_edges = %u is outside 2..%u", n_edges, kAggMaxBuckets + 1);
  const uint32_t type = idx->columns[slot].type;
  for (uint32_t i = 0; i < n_edges; ++i) {
    if (column_not_a_value(type, edges[i])) return fail(SGPU_EINVAL, "column histogram: edge %u is NaN", i);
    if (i && column_key(type, edges[i]) <= column_key(type, edges[i - 1]))
      return fail(SGPU_EINVAL, "column histogram: edge %u is not above edge %u in the column's order", i, i - 1);
  }
  return foreign_filter(idx, filter);
}

sgpu_status top_check_args(const sgpu_index* idx, uint32_t slot, const sgpu_filter* filter, uint32_t t, uint32_t order,
                           const uint32_t* out_doc_ids, const uint32_t* out_value_bits, const uint32_t* out_n, const uint64_t* out_valid,
                           const uint64_t* out_docs) {
  if (!idx || !out_doc_ids || !out_value_bits || !out_n || !out_valid || !out_docs) return fail(SGPU_EINVAL, "null argument");
  if (t == 0 || t > kTopMaxT) return fail(SGPU_EINVAL, "column top: t = %u is outside 1..%u", t, kTopMaxT);
  if (order > 1) return fail(SGPU_EINVAL, "column top: order = %u is neither 0 (ascending) nor 1 (descending)", order);
  const sgpu_status st = agg_check_slot(idx, slot, "column top");
  if (st != SGPU_OK) return st;
  return foreign_filter(idx, filter);
}

void stats_combine(uint32_t type, const AggPartial* parts, uint64_t n_tiles, uint64_t docs, struct sgpu_column_stats* out) {
  double sum = 0.0;
  uint64_t sum_int = 0, valid = 0;
  uint32_t min_key = 0xffffffffu, max_key = 0u;
  for (uint64_t t = 0; t < n_tiles; ++t) {   // (ascending tile order: step 4 of the canonical sum)
    sum += parts[t].sum;
    sum_int += parts[t].sum_int;
    valid += parts[t].valid;
    if (parts[t].valid) {
      min_key = std::min(min_key, parts[t].min_key);
      max_key = std::max(max_key, parts[t].max_key);
    }
  }
  if (type == SGPU_COL_U32) sum = (double)sum_int;
  else if (type == SGPU_COL_I32) sum = (double)(int64_t)sum_int;
  else sum_int = 0;
  if (sum != sum) {
    const uint64_t quiet = 0x7ff8000000000000ull;
    std::memcpy(&sum, &quiet, 8);
  }
  out->docs = docs;
  out->valid = valid;
  out->min_bits = valid ? column_key_bits(type, min_key) : 0u;
  out->max_bits = valid ? column_key_bits(type, max_key) : 0u;
  out->sum_int = sum_int;
  out->sum = sum;
}

sgpu_status column_stats_host(const sgpu_index* idx, uint32_t slot, const sgpu_filter* filter, uint32_t num_threads,
                              struct sgpu_column_stats* out) {
  const sgpu_status cst = stats_check_args(idx, slot, filter, out);
  if (cst != SGPU_OK) return cst;
  const HostColumn& col = idx->columns[slot];
  const uint64_t n_docs = idx->host.n_docs, n_tiles = (n_docs + kAggTile - 1) / kAggTile;
  const uint32_t* fbits = filter ? filter_host_bits(filter) : nullptr;
  const uint32_t* v = col.values.data();
  const uint32_t type = col.type;
  const int nt = num_threads ? (int)num_threads : default_host_threads(omp_get_max_threads());
  try {
    std::vector<AggPartial> parts((size_t)n_tiles);
#pragma omp parallel for num_threads(nt) schedule(static)
    for (uint64_t t = 0; t < n_tiles; ++t) {
      double c[kAggLanes];
      for (uint32_t j = 0; j < kAggLanes; ++j) c[j] = 0.0;
      AggPartial p{0.0, 0, 0xffffffffu, 0u, 0u, 0u};
      const uint64_t d0 = t * kAggTile;
      for (uint32_t r = 0; r < kAggTile / kAggLanes; ++r)
        for (uint32_t j = 0; j < kAggLanes; ++j) {
          const uint64_t d = d0 + (uint64_t)r * kAggLanes + j;
          if (d >= n_docs || !filter_bit(fbits, d) || column_not_a_value(type, v[d])) continue;
          const uint32_t key = column_key(type, v[d]);
          p.min_key = std::min(p.min_key, key);
          p.max_key = std::max(p.max_key, key);
          ++p.valid;
          if (type == SGPU_COL_F32) {
            float f;
            std::memcpy(&f, &v[d], 4);
            c[j] += (double)f;
          } else {
            p.sum_int += type == SGPU_COL_I32 ? (uint64_t)(int64_t)(int32_t)v[d] : (uint64_t)v[d];
          }
        }
      for (uint32_t h = kAggLanes / 2; h >= 1; h >>= 1)
        for (uint32_t j = 0; j < h; ++j) c[j] += c[j + h];
      p.sum = c[0];
      parts[(size_t)t] = p;
    }
    stats_combine(type, parts.data(), n_tiles, filter ? filter_count(filter) : n_docs, out);
    return SGPU_OK;
  } catch (const std::bad_alloc&) {
    return fail(SGPU_ENOMEM, "out of host memory");
  }
}

sgpu_status column_histogram_host(const sgpu_index* idx, uint32_t slot, const sgpu_filter* filter, const uint32_t* edges, uint32_t n_edges,
                                  uint32_t num_threads, uint64_t* out_counts, uint64_t* out_below, uint64_t* out_above, uint64_t* out_nan,
                                  uint64_t* out_docs) {
  const sgpu_status cst = histogram_check_args(idx, slot, filter, edges, n_edges, out_counts, out_below, out_above, out_nan, out_docs);
  if (cst != SGPU_OK) return cst;
  const HostColumn& col = idx->columns[slot];
  const uint64_t n_docs = idx->host.n_docs, n_tiles = (n_docs + kAggTile - 1) / kAggTile;
  const uint32_t* fbits = filter ? filter_host_bits(filter) : nullptr;
  const uint32_t* v = col.values.data();
  const uint32_t type = col.type, nb = n_edges - 1, bins = nb + 3;   // bins nb, nb + 1, nb + 2: below, above, NaN
  const int nt = num_threads ? (int)num_threads : default_host_threads(omp_get_max_threads());
  try {
    std::vector<uint32_t> ek(n_edges);
    for (uint32_t i = 0; i < n_edges; ++i) ek[i] = column_key(type, edges[i]);
    std::vector<uint64_t> locals((size_t)nt * bins, 0ull);   // (allocated here: nothing throws inside the team)
#pragma omp parallel num_threads(nt)
    {
      uint64_t* mine = locals.data() + (size_t)omp_get_thread_num() * bins;
#pragma omp for schedule(static)
      for (uint64_t t = 0; t < n_tiles; ++t) {
        const uint64_t d1 = std::min<uint64_t>((t + 1) * kAggTile, n_docs);
        for (uint64_t d = t * kAggTile; d < d1; ++d) {
          if (!filter_bit(fbits, d)) continue;
          uint32_t b;
          if (column_not_a_value(type, v[d])) {
            b = nb + 2;
          } else {
            const uint32_t key = column_key(type, v[d]);
            if (key < ek[0]) b = nb;
            else if (key > ek[nb]) b = nb + 1;
            else b = std::min<uint32_t>((uint32_t)(std::upper_bound(ek.begin(), ek.end(), key) - ek.begin()) - 1u, nb - 1u);
          }
          ++mine[b];
        }
      }
    }
    std::vector<uint64_t> total(bins, 0ull);
    for (int x = 0; x < nt; ++x)
      for (uint32_t b = 0; b < bins; ++b) total[b] += locals[(size_t)x * bins + b];
    for (uint32_t b = 0; b < nb; ++b) out_counts[b] = total[b];
    *out_below = total[nb];
    *out_above = total[nb + 1];
    *out_nan = total[nb + 2];
    *out_docs = filter ? filter_count(filter) : n_docs;
    return SGPU_OK;
  } catch (const std::bad_alloc&) {
    return fail(SGPU_ENOMEM, "out of host memory");
  }
}

sgpu_status column_top_host(const sgpu_index* idx, uint32_t slot, const sgpu_filter* filter, uint32_t t, uint32_t order, uint32_t num_threads,
                            uint32_t* out_doc_ids, uint32_t* out_value_bits, uint32_t* out_n, uint64_t* out_valid, uint64_t* out_docs) {
  const sgpu_status cst = top_check_args(idx, slot, filter, t, order, out_doc_ids, out_value_bits, out_n, out_valid, out_docs);
  if (cst != SGPU_OK) return cst;
  const HostColumn& col = idx->columns[slot];
  const uint64_t n_docs = idx->host.n_docs, n_tiles = (n_docs + kAggTile - 1) / kAggTile;
  const uint32_t* fbits = filter ? filter_host_bits(filter) : nullptr;
  const uint32_t* v = col.values.data();
  const uint32_t type = col.type;
  const int nt = num_threads ? (int)num_threads : default_host_threads(omp_get_max_threads());
  try {
    // the rows are the t smallest composites (key, or ~key for descending) << 32 | id: distinct, so fully determined.
    // A thread keeps the t smallest of its tiles (cut back whenever 4 t have gathered); the threads' lists are merged.
    std::vector<std::vector<uint64_t>> lists((size_t)nt);
    for (std::vector<uint64_t>& l : lists) l.reserve(4 * (size_t)t + kAggTile);   // (allocated here: nothing throws inside the team)
    uint64_t valid = 0;
#pragma omp parallel num_threads(nt) reduction(+ : valid)
    {
      std::vector<uint64_t>& mine = lists[(size_t)omp_get_thread_num()];
#pragma omp for schedule(static)
      for (uint64_t tl = 0; tl < n_tiles; ++tl) {
        const uint64_t d1 = std::min<uint64_t>((tl + 1) * kAggTile, n_docs);
        for (uint64_t d = tl * kAggTile; d < d1; ++d) {
          if (!filter_bit(fbits, d) || column_not_a_value(type, v[d])) continue;
          ++valid;
          const uint32_t key = column_key(type, v[d]);
          mine.push_back((uint64_t)(order ? ~key : key) << 32 | (uint32_t)d);
        }
        if (mine.size() > 4 * (size_t)t) {
          std::nth_element(mine.begin(), mine.begin() + t, mine.end());
          mine.resize(t);
        }
      }
    }
    std::vector<uint64_t> all;
    for (const std::vector<uint64_t>& l : lists) all.insert(all.end(), l.begin(), l.end());
    const uint32_t n = (uint32_t)std::min<uint64_t>(t, all.size());
    std::partial_sort(all.begin(), all.begin() + n, all.end());
    for (uint32_t i = 0; i < t; ++i) {
      out_doc_ids[i] = i < n ? (uint32_t)all[i] : 0u;
      out_value_bits[i] = i < n ? v[(uint32_t)all[i]] : 0u;
    }
    *out_n = n;
    *out_valid = valid;
    *out_docs = filter ? filter_count(filter) : n_docs;
    return SGPU_OK;
  } catch (const std::bad_alloc&) {
    return fail(SGPU_ENOMEM, "out of host memory");
  }
}

}  // namespace sgpu
