// score_host.cpp — sgpu_score_documents_host, sgpu_rerank_documents_host, sgpu_explain_documents_host,
// sgpu_expand_queries_host, sgpu_diversify_documents_host, sgpu_collapse_documents_host and sgpu_fuse_documents_host, and the
// argument checks they share with the device calls.
//
// The host twin of score_documents.hip: the same score, bit for bit - 16 accumulators, element e of the document to
// accumulator (e / 8) % 16 in increasing e, the partials combined by t[j] += t[j ^ s], s = 8, 4, 2, 1; f32 multiply then
// add (this file is compiled with -ffp-contract=off). A query is scattered into a dense f32 table over the vocabulary
// (one per thread); components it does not carry read 0.0 and are added as +-0.0, which never changes an accumulator
// that started at +0.0. Fixed-u8 codes: the power of two val_scale is folded into the weight, as on the device.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "host_index.hpp"

namespace sgpu {

// Checks 1 - 5 of sgpu_score_documents, in the header's order.
sgpu_status score_check_args(const HostIndex& h, const uint64_t* q_off, const uint32_t* comps, const float* vals, uint32_t nq,
                             const uint64_t* cand_off, const uint64_t* cand_ids, const float* out_scores, uint32_t* max_nnz) {
  if (!q_off || !cand_off || !cand_ids || !out_scores) return fail(SGPU_EINVAL, "null argument");
  const sgpu_status vst = validate_queries(h.dim, q_off, comps, vals, nq, max_nnz);
  if (vst != SGPU_OK) return vst;
  if (cand_off[0] != 0) return fail(SGPU_EINVAL, "cand_off[0] must be 0");
  for (uint32_t q = 0; q < nq; ++q)
    if (cand_off[q + 1] < cand_off[q]) return fail(SGPU_EINVAL, "cand_off not monotone");
  for (uint32_t q = 0; q < nq; ++q)
    for (uint64_t i = cand_off[q]; i < cand_off[q + 1]; ++i)
      if (cand_ids[i] >= h.n_docs)
        return fail(SGPU_EINVAL, "query %u: document id %llu >= n_docs (%llu)", q, (unsigned long long)cand_ids[i],
                    (unsigned long long)h.n_docs);
  if (*max_nnz > kScoreMaxQueryNnz)
    return fail(SGPU_ELIMIT, "a query has %u components (scoring documents: limit %u)", *max_nnz, kScoreMaxQueryNnz);
  return SGPU_OK;
}

static inline float score_one(const HostIndex& h, uint64_t doc, const float* dense) {
  const uint64_t s = h.fwd_offsets[doc], e = h.fwd_offsets[doc + 1];
  float t[16];
  for (int j = 0; j < 16; ++j) t[j] = 0.0f;
  const bool f16 = h.value_type == SGPU_VAL_F16;
  for (uint64_t i = s; i < e; ++i) {
    const float v = f16 ? f16_to_f32(h.fwd_vals[i]) : (float)h.fwd_codes[i];
    const int lane = (int)(((i - s) >> 3) & 15);
    const float p = dense[h.comp(i)] * v;
    t[lane] = t[lane] + p;
  }
  for (int st = 8; st >= 1; st >>= 1) {
    float u[16];
    for (int j = 0; j < 16; ++j) u[j] = t[j] + t[j ^ st];
    for (int j = 0; j < 16; ++j) t[j] = u[j];
  }
  return t[0];
}

sgpu_status score_documents_host(const HostIndex& h, const uint64_t* q_off, const uint32_t* comps, const float* vals, uint32_t nq,
                                 const uint64_t* cand_off, const uint64_t* cand_ids, uint32_t num_threads, float* out_scores) {
  uint32_t max_nnz = 0;
  const sgpu_status vst = score_check_args(h, q_off, comps, vals, nq, cand_off, cand_ids, out_scores, &max_nnz);
  if (vst != SGPU_OK) return vst;
  if (nq == 0 || cand_off[nq] == 0) return SGPU_OK;
  int team = num_threads ? (int)num_threads : host_threads();
  team = (int)std::max<int64_t>(1, std::min<int64_t>(team, (int64_t)nq));
  std::vector<std::vector<float>> tables;
  try {
    tables.assign((size_t)team, std::vector<float>());
    for (auto& t : tables) t.assign(h.dim, 0.0f);
  } catch (const std::bad_alloc&) {
    return fail(SGPU_ENOMEM, "out of host memory");
  }
  const bool f16 = h.value_type == SGPU_VAL_F16;
#pragma omp parallel for schedule(dynamic, 1) num_threads(team)
  for (int64_t q = 0; q < (int64_t)nq; ++q) {
    if (cand_off[q + 1] == cand_off[q]) continue;
#ifdef _OPENMP
    float* dense = tables[(size_t)omp_get_thread_num()].data();
#else
    float* dense = tables[0].data();
#endif
    for (uint64_t j = q_off[q]; j < q_off[q + 1]; ++j) dense[comps[j]] = f16 ? vals[j] : vals[j] * h.val_scale;
    for (uint64_t i = cand_off[q]; i < cand_off[q + 1]; ++i) out_scores[i] = score_one(h, cand_ids[i], dense);
    for (uint64_t j = q_off[q]; j < q_off[q + 1]; ++j) dense[comps[j]] = 0.0f;
  }
  return SGPU_OK;
}

// Checks 1 - 4 of sgpu_rerank_documents, in the header's order.
sgpu_status rerank_check_args(const HostIndex& h, const uint64_t* q_off, const uint32_t* comps, const float* vals, uint32_t nq,
                              const uint64_t* cand_off, const uint64_t* cand_ids, uint32_t k, const float* out_scores,
                              const uint64_t* out_doc_ids, const uint32_t* out_n, uint32_t* max_nnz) {
  if (!out_doc_ids || !out_n) return fail(SGPU_EINVAL, "null argument");
  const sgpu_status vst = score_check_args(h, q_off, comps, vals, nq, cand_off, cand_ids, out_scores, max_nnz);
  if (vst != SGPU_OK) return vst;
  if (k == 0) return fail(SGPU_EINVAL, "k must be at least 1");
  if (k > kRerankMaxK) return fail(SGPU_ELIMIT, "k = %u (reranking documents: limit %u)", k, kRerankMaxK);
  return SGPU_OK;
}

// The host twin of the device's selection (score_documents.hip), the arbiter of its rows: per query the distinct ids of
// its candidates, each scored once by score_one (the scores of sgpu_score_documents_host), ordered by score descending -
// NaN after every number - and id ascending, cut to k. -0.0 never occurs (score_documents.hip), so the numeric order is the
// device's order of the scores' integer images.
sgpu_status rerank_documents_host(const HostIndex& h, const uint64_t* q_off, const uint32_t* comps, const float* vals, uint32_t nq,
                                  const uint64_t* cand_off, const uint64_t* cand_ids, uint32_t k, uint32_t num_threads,
                                  float* out_scores, uint64_t* out_doc_ids, uint32_t* out_n) {
  uint32_t max_nnz = 0;
  const sgpu_status vst = rerank_check_args(h, q_off, comps, vals, nq, cand_off, cand_ids, k, out_scores, out_doc_ids, out_n, &max_nnz);
  if (vst != SGPU_OK) return vst;
  if (nq == 0) return SGPU_OK;
  std::memset(out_scores, 0, (size_t)nq * k * sizeof(float));
  std::memset(out_doc_ids, 0, (size_t)nq * k * sizeof(uint64_t));
  std::memset(out_n, 0, (size_t)nq * sizeof(uint32_t));
  if (cand_off[nq] == 0) return SGPU_OK;
  int team = num_threads ? (int)num_threads : host_threads();
  team = (int)std::max<int64_t>(1, std::min<int64_t>(team, (int64_t)nq));
  struct Item {
    float score;
    uint64_t id;
  };
  std::vector<std::vector<float>> tables;
  std::vector<std::vector<Item>> items;
  uint64_t longest = 0;
  for (uint32_t q = 0; q < nq; ++q) longest = std::max(longest, cand_off[q + 1] - cand_off[q]);
  try {
    tables.assign((size_t)team, std::vector<float>());
    for (auto& t : tables) t.assign(h.dim, 0.0f);
    items.assign((size_t)team, std::vector<Item>());
    for (auto& v : items) v.reserve(longest);
  } catch (const std::bad_alloc&) {
    return fail(SGPU_ENOMEM, "out of host memory");
  }
  const bool f16 = h.value_type == SGPU_VAL_F16;
#pragma omp parallel for schedule(dynamic, 1) num_threads(team)
  for (int64_t q = 0; q < (int64_t)nq; ++q) {
    if (cand_off[q + 1] == cand_off[q]) continue;
#ifdef _OPENMP
    const size_t me = (size_t)omp_get_thread_num();
#else
    const size_t me = 0;
#endif
    float* dense = tables[me].data();
    std::vector<Item>& it = items[me];   // (reserved for the longest list: nothing below allocates)
    it.clear();
    for (uint64_t i = cand_off[q]; i < cand_off[q + 1]; ++i) it.push_back(Item{0.0f, cand_ids[i]});
    std::sort(it.begin(), it.end(), [](const Item& a, const Item& b) { return a.id < b.id; });
    it.erase(std::unique(it.begin(), it.end(), [](const Item& a, const Item& b) { return a.id == b.id; }), it.end());
    for (uint64_t j = q_off[q]; j < q_off[q + 1]; ++j) dense[comps[j]] = f16 ? vals[j] : vals[j] * h.val_scale;
    for (Item& x : it) x.score = score_one(h, x.id, dense);
    for (uint64_t j = q_off[q]; j < q_off[q + 1]; ++j) dense[comps[j]] = 0.0f;
    const size_t n = std::min<size_t>(k, it.size());
    std::partial_sort(it.begin(), it.begin() + (ptrdiff_t)n, it.end(), [](const Item& a, const Item& b) {
      const bool na = std::isnan(a.score), nb = std::isnan(b.score);
      if (na != nb) return nb;
      if (!na && a.score != b.score) return a.score > b.score;
      return a.id < b.id;
    });
    for (size_t i = 0; i < n; ++i) {
      out_scores[(size_t)q * k + i] = it[i].score;
      out_doc_ids[(size_t)q * k + i] = it[i].id;
    }
    out_n[q] = (uint32_t)n;
  }
  return SGPU_OK;
}

// Checks 1 - 4 of sgpu_explain_documents, in the header's order.
sgpu_status explain_check_args(const HostIndex& h, const uint64_t* q_off, const uint32_t* comps, const float* vals, uint32_t nq,
                               const uint64_t* cand_off, const uint64_t* cand_ids, uint32_t m, const ExplainOut& out,
                               uint32_t* max_nnz) {
  if (!out.scores || !out.n_terms || !out.comps || !out.q_vals || !out.d_vals || !out.products) return fail(SGPU_EINVAL, "null argument");
  const sgpu_status vst = score_check_args(h, q_off, comps, vals, nq, cand_off, cand_ids, out.scores, max_nnz);
  if (vst != SGPU_OK) return vst;
  if (m == 0) return fail(SGPU_EINVAL, "m must be at least 1");
  if (m > kExplainMaxTerms) return fail(SGPU_ELIMIT, "m = %u (explaining documents: limit %u)", m, kExplainMaxTerms);
  return SGPU_OK;
}

namespace {
inline uint32_t f32_bits(float x) {
  uint32_t b;
  std::memcpy(&b, &x, 4);
  return b;
}
// the monotone integer image of an f32 (device_prims.hpp: ordered_u32) and its inverse
inline uint32_t ordered_bits(float x) {
  const uint32_t b = f32_bits(x);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
inline float ordered_bits_inv(uint32_t k) {
  const uint32_t b = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
  float x;
  std::memcpy(&x, &b, 4);
  return x;
}
struct Term {
  uint64_t key;   // ordered(product) << 32 | ~component: a larger key is an earlier term
  uint64_t at;    // the element's place in the forward arrays
};
}  // namespace

// score_one that also collects the pair's terms: the elements whose component has a table weight that is not +-0.
static inline float explain_one(const HostIndex& h, uint64_t doc, const float* dense, std::vector<Term>& terms) {
  const uint64_t s = h.fwd_offsets[doc], e = h.fwd_offsets[doc + 1];
  float t[16];
  for (int j = 0; j < 16; ++j) t[j] = 0.0f;
  const bool f16 = h.value_type == SGPU_VAL_F16;
  terms.clear();
  for (uint64_t i = s; i < e; ++i) {
    const float v = f16 ? f16_to_f32(h.fwd_vals[i]) : (float)h.fwd_codes[i];
    const int lane = (int)(((i - s) >> 3) & 15);
    const uint32_t c = h.comp(i);
    const float p = dense[c] * v;
    t[lane] = t[lane] + p;
    if (f32_bits(dense[c]) & 0x7fffffffu) terms.push_back(Term{((uint64_t)ordered_bits(p) << 32) | (uint64_t)(~c), i});
  }
  for (int st = 8; st >= 1; st >>= 1) {
    float u[16];
    for (int j = 0; j < 16; ++j) u[j] = t[j] + t[j ^ st];
    for (int j = 0; j < 16; ++j) t[j] = u[j];
  }
  return t[0];
}

// The host twin of explain_documents.hip, the arbiter of its rows: a plain loop over the pairs, the score accumulated as
// score_one does, the terms ordered by their keys and cut to m.
sgpu_status explain_documents_host(const HostIndex& h, const uint64_t* q_off, const uint32_t* comps, const float* vals, uint32_t nq,
                                   const uint64_t* cand_off, const uint64_t* cand_ids, uint32_t m, uint32_t num_threads,
                                   const ExplainOut& out) {
  uint32_t max_nnz = 0;
  const sgpu_status vst = explain_check_args(h, q_off, comps, vals, nq, cand_off, cand_ids, m, out, &max_nnz);
  if (vst != SGPU_OK) return vst;
  if (nq == 0 || cand_off[nq] == 0) return SGPU_OK;
  int team = num_threads ? (int)num_threads : host_threads();
  team = (int)std::max<int64_t>(1, std::min<int64_t>(team, (int64_t)nq));
  uint64_t longest = 0;
  for (uint64_t i = 0; i < cand_off[nq]; ++i) longest = std::max(longest, h.fwd_offsets[cand_ids[i] + 1] - h.fwd_offsets[cand_ids[i]]);
  std::vector<std::vector<float>> tables;
  std::vector<std::vector<Term>> found;
  try {
    tables.assign((size_t)team, std::vector<float>());
    for (auto& t : tables) t.assign(h.dim, 0.0f);
    found.assign((size_t)team, std::vector<Term>());
    for (auto& v : found) v.reserve(longest);
  } catch (const std::bad_alloc&) {
    return fail(SGPU_ENOMEM, "out of host memory");
  }
  const bool f16 = h.value_type == SGPU_VAL_F16;
#pragma omp parallel for schedule(dynamic, 1) num_threads(team)
  for (int64_t q = 0; q < (int64_t)nq; ++q) {
    if (cand_off[q + 1] == cand_off[q]) continue;
#ifdef _OPENMP
    const size_t me = (size_t)omp_get_thread_num();
#else
    const size_t me = 0;
#endif
    float* dense = tables[me].data();
    std::vector<Term>& terms = found[me];   // (reserved for the longest document: nothing below allocates)
    const uint32_t *qc0 = comps + q_off[q], *qc1 = comps + q_off[q + 1];
    for (uint64_t j = q_off[q]; j < q_off[q + 1]; ++j) dense[comps[j]] = f16 ? vals[j] : vals[j] * h.val_scale;
    for (uint64_t i = cand_off[q]; i < cand_off[q + 1]; ++i) {
      out.scores[i] = explain_one(h, cand_ids[i], dense, terms);
      out.n_terms[i] = (uint32_t)terms.size();
      const size_t n = std::min<size_t>(m, terms.size());
      std::partial_sort(terms.begin(), terms.begin() + (ptrdiff_t)n, terms.end(),
                        [](const Term& a, const Term& b) { return a.key > b.key; });
      for (size_t r = 0; r < m; ++r) {
        const size_t o = (size_t)i * m + r;
        if (r < n) {
          const uint32_t c = ~(uint32_t)terms[r].key;
          out.comps[o] = c;
          out.q_vals[o] = vals[q_off[q] + (uint64_t)(std::lower_bound(qc0, qc1, c) - qc0)];   // (w as given, not the table's)
          out.d_vals[o] = h.val(terms[r].at);
          out.products[o] = ordered_bits_inv((uint32_t)(terms[r].key >> 32));
        } else {
          out.comps[o] = 0;
          out.q_vals[o] = out.d_vals[o] = out.products[o] = 0.0f;
        }
      }
    }
    for (uint64_t j = q_off[q]; j < q_off[q + 1]; ++j) dense[comps[j]] = 0.0f;
  }
  return SGPU_OK;
}

// Checks 1 - 6 of sgpu_expand_queries, in the header's order.
sgpu_status expand_check_args(const HostIndex& h, const uint64_t* q_off, const uint32_t* comps, const float* vals, uint32_t nq,
                              const uint64_t* cand_off, const uint64_t* cand_ids, const float* cand_w, float alpha, uint32_t t,
                              const uint32_t* out_comps, const float* out_vals, const uint32_t* out_n, uint32_t* max_nnz) {
  if (!cand_w || !out_comps || !out_n) return fail(SGPU_EINVAL, "null argument");
  const sgpu_status vst = score_check_args(h, q_off, comps, vals, nq, cand_off, cand_ids, out_vals, max_nnz);
  if (vst != SGPU_OK) return vst;
  if (!std::isfinite(alpha)) return fail(SGPU_EINVAL, "alpha is not finite");
  for (uint32_t q = 0; q < nq; ++q)
    for (uint64_t i = cand_off[q]; i < cand_off[q + 1]; ++i)
      if (!std::isfinite(cand_w[i]))
        return fail(SGPU_EINVAL, "query %u: the weight of candidate %llu (document id %llu) is not finite", q,
                    (unsigned long long)(i - cand_off[q]), (unsigned long long)cand_ids[i]);
  for (uint32_t q = 0; q < nq; ++q)
    if (cand_off[q + 1] - cand_off[q] > kExpandMaxCand)
      return fail(SGPU_ELIMIT, "query %u has %llu feedback documents (expanding queries: limit %llu)", q,
                  (unsigned long long)(cand_off[q + 1] - cand_off[q]), (unsigned long long)kExpandMaxCand);
  if (t == 0) return fail(SGPU_EINVAL, "t must be at least 1");
  if (t > kExpandMaxTerms) return fail(SGPU_ELIMIT, "t = %u (expanding queries: limit %u)", t, kExpandMaxTerms);
  return SGPU_OK;
}

// The host twin of expand_queries.hip, the arbiter of its rows: per query the table W of the header - the query's
// fl(alpha * w) written, then every feedback document added in the order given, multiply then add -, the components with
// W > 0 cut to the t best by (W descending, component ascending) and written in ascending component order. A thread keeps
// one table over the vocabulary and the list of the components it touched, each once (`seen`), so that a query costs
// its own elements and not the vocabulary.
sgpu_status expand_queries_host(const HostIndex& h, const uint64_t* q_off, const uint32_t* comps, const float* vals, uint32_t nq,
                                const uint64_t* cand_off, const uint64_t* cand_ids, const float* cand_w, float alpha, uint32_t t,
                                uint32_t num_threads, uint32_t* out_comps, float* out_vals, uint32_t* out_n) {
  uint32_t max_nnz = 0;
  const sgpu_status vst =
      expand_check_args(h, q_off, comps, vals, nq, cand_off, cand_ids, cand_w, alpha, t, out_comps, out_vals, out_n, &max_nnz);
  if (vst != SGPU_OK) return vst;
  if (nq == 0) return SGPU_OK;
  int team = num_threads ? (int)num_threads : host_threads();
  team = (int)std::max<int64_t>(1, std::min<int64_t>(team, (int64_t)nq));
  struct Scratch {
    std::vector<float> w;
    std::vector<uint8_t> seen;
    std::vector<uint32_t> touched;
  };
  std::vector<Scratch> scratch;
  try {
    scratch.assign((size_t)team, Scratch());
    for (auto& s : scratch) {
      s.w.assign(h.dim, 0.0f);
      s.seen.assign(h.dim, 0);
      s.touched.reserve(h.dim);   // (a component enters once: nothing below allocates)
    }
  } catch (const std::bad_alloc&) {
    return fail(SGPU_ENOMEM, "out of host memory");
  }
  const bool f16 = h.value_type == SGPU_VAL_F16;
#pragma omp parallel for schedule(dynamic, 16) num_threads(team)
  for (int64_t q = 0; q < (int64_t)nq; ++q) {
#ifdef _OPENMP
    Scratch& s = scratch[(size_t)omp_get_thread_num()];
#else
    Scratch& s = scratch[0];
#endif
    float* W = s.w.data();
    uint8_t* seen = s.seen.data();
    std::vector<uint32_t>& touched = s.touched;
    touched.clear();
    auto touch = [&](uint32_t c) {
      if (!seen[c]) {
        seen[c] = 1;
        touched.push_back(c);
      }
    };
    for (uint64_t j = q_off[q]; j < q_off[q + 1]; ++j) {
      touch(comps[j]);
      W[comps[j]] = alpha * vals[j];
    }
    for (uint64_t i = cand_off[q]; i < cand_off[q + 1]; ++i) {
      const uint64_t a = h.fwd_offsets[cand_ids[i]], e = h.fwd_offsets[cand_ids[i] + 1];
      const float wd = f16 ? cand_w[i] : cand_w[i] * h.val_scale;
      for (uint64_t x = a; x < e; ++x) {
        const uint32_t c = h.comp(x);
        const float p = wd * (f16 ? f16_to_f32(h.fwd_vals[x]) : (float)h.fwd_codes[x]);
        touch(c);
        W[c] = W[c] + p;
      }
    }
    // the terms: W > 0, the t best by (W descending, component ascending), then in ascending component order
    size_t n = 0;
    for (size_t i = 0; i < touched.size(); ++i) {
      const uint32_t c = touched[i];
      seen[c] = 0;
      if (W[c] > 0.0f) touched[n++] = c;   // (compacted in place: n <= i)
      else W[c] = 0.0f;
    }
    const size_t keep = std::min<size_t>(t, n);
    if (keep < n)
      std::nth_element(touched.begin(), touched.begin() + (ptrdiff_t)keep, touched.begin() + (ptrdiff_t)n,
                       [W](uint32_t a, uint32_t b) { return W[a] != W[b] ? W[a] > W[b] : a < b; });
    std::sort(touched.begin(), touched.begin() + (ptrdiff_t)keep);
    uint32_t* oc = out_comps + (size_t)q * t;
    float* ov = out_vals + (size_t)q * t;
    for (size_t i = 0; i < keep; ++i) {
      oc[i] = touched[i];
      ov[i] = W[touched[i]];
    }
    for (size_t i = keep; i < t; ++i) {
      oc[i] = 0;
      ov[i] = 0.0f;
    }
    out_n[q] = (uint32_t)keep;
    for (size_t i = 0; i < n; ++i) W[touched[i]] = 0.0f;
  }
  return SGPU_OK;
}

// Checks 1 - 7 of sgpu_diversify_documents, in the header's order.
sgpu_status diversify_check_args(const HostIndex& h, const uint64_t* q_off, const uint32_t* comps, const float* vals, uint32_t nq,
                                 const uint64_t* cand_off, const uint64_t* cand_ids, float lambda, float mu, uint32_t k,
                                 const DiversifyOut& out, uint32_t* max_nnz, uint32_t* max_len, uint32_t* max_cand) {
  if (!out.penalties || !out.doc_ids || !out.n) return fail(SGPU_EINVAL, "null argument");
  const sgpu_status vst = score_check_args(h, q_off, comps, vals, nq, cand_off, cand_ids, out.scores, max_nnz);
  if (vst != SGPU_OK) return vst;
  if (!std::isfinite(lambda)) return fail(SGPU_EINVAL, "lambda is not finite");
  if (!std::isfinite(mu)) return fail(SGPU_EINVAL, "mu is not finite");
  *max_len = 0;
  *max_cand = 0;
  for (uint32_t q = 0; q < nq; ++q) {
    if (cand_off[q + 1] - cand_off[q] > kDiversifyMaxCand)
      return fail(SGPU_ELIMIT, "query %u has %llu candidates (diversifying documents: limit %llu)", q,
                  (unsigned long long)(cand_off[q + 1] - cand_off[q]), (unsigned long long)kDiversifyMaxCand);
    *max_cand = std::max(*max_cand, (uint32_t)(cand_off[q + 1] - cand_off[q]));
  }
  for (uint32_t q = 0; q < nq; ++q)
    for (uint64_t i = cand_off[q]; i < cand_off[q + 1]; ++i) {
      const uint64_t len = h.fwd_offsets[cand_ids[i] + 1] - h.fwd_offsets[cand_ids[i]];
      if (len > kScoreMaxQueryNnz)
        return fail(SGPU_ELIMIT, "query %u: document id %llu has %llu components (diversifying documents: limit %u)", q,
                    (unsigned long long)cand_ids[i], (unsigned long long)len, kScoreMaxQueryNnz);
      *max_len = std::max(*max_len, (uint32_t)len);
    }
  if (k == 0) return fail(SGPU_EINVAL, "k must be at least 1");
  if (k > kDiversifyMaxK) return fail(SGPU_ELIMIT, "k = %u (diversifying documents: limit %u)", k, kDiversifyMaxK);
  return SGPU_OK;
}

// The host twin of diversify_documents.hip, the arbiter of its rows: the greedy selection of the header, entry by entry.
// rel and sim both come from score_one - sim with the selected document's stored vector scattered into the thread's
// table in the query's place (fixed-u8: its value code * val_scale, then the fold of val_scale score_documents_host
// applies to every query weight) -, so a row is made of the bits sgpu_score_documents_host returns.
sgpu_status diversify_documents_host(const HostIndex& h, const uint64_t* q_off, const uint32_t* comps, const float* vals, uint32_t nq,
                                     const uint64_t* cand_off, const uint64_t* cand_ids, float lambda, float mu, uint32_t k,
                                     uint32_t num_threads, const DiversifyOut& out) {
  uint32_t max_nnz = 0, max_len = 0, max_cand = 0;
  const sgpu_status vst =
      diversify_check_args(h, q_off, comps, vals, nq, cand_off, cand_ids, lambda, mu, k, out, &max_nnz, &max_len, &max_cand);
  if (vst != SGPU_OK) return vst;
  if (nq == 0) return SGPU_OK;
  std::memset(out.scores, 0, (size_t)nq * k * sizeof(float));
  std::memset(out.penalties, 0, (size_t)nq * k * sizeof(float));
  std::memset(out.doc_ids, 0, (size_t)nq * k * sizeof(uint64_t));
  std::memset(out.n, 0, (size_t)nq * sizeof(uint32_t));
  if (cand_off[nq] == 0) return SGPU_OK;
  int team = num_threads ? (int)num_threads : host_threads();
  team = (int)std::max<int64_t>(1, std::min<int64_t>(team, (int64_t)nq));
  struct Entry {
    uint64_t id;
    float rel, pen;
    bool taken;
  };
  std::vector<std::vector<float>> tables;
  std::vector<std::vector<Entry>> entries;
  try {
    tables.assign((size_t)team, std::vector<float>());
    for (auto& t : tables) t.assign(h.dim, 0.0f);
    entries.assign((size_t)team, std::vector<Entry>());
    for (auto& v : entries) v.reserve(max_cand);
  } catch (const std::bad_alloc&) {
    return fail(SGPU_ENOMEM, "out of host memory");
  }
  const bool f16 = h.value_type == SGPU_VAL_F16;
#pragma omp parallel for schedule(dynamic, 1) num_threads(team)
  for (int64_t q = 0; q < (int64_t)nq; ++q) {
    if (cand_off[q + 1] == cand_off[q]) continue;
#ifdef _OPENMP
    const size_t me = (size_t)omp_get_thread_num();
#else
    const size_t me = 0;
#endif
    float* dense = tables[me].data();
    std::vector<Entry>& en = entries[me];   // (reserved for the longest list: nothing below allocates)
    en.clear();
    for (uint64_t j = q_off[q]; j < q_off[q + 1]; ++j) dense[comps[j]] = f16 ? vals[j] : vals[j] * h.val_scale;
    for (uint64_t i = cand_off[q]; i < cand_off[q + 1]; ++i) en.push_back(Entry{cand_ids[i], score_one(h, cand_ids[i], dense), 0.0f, false});
    for (uint64_t j = q_off[q]; j < q_off[q + 1]; ++j) dense[comps[j]] = 0.0f;
    size_t left = en.size();
    uint32_t r = 0;
    while (r < k && left) {
      uint64_t best = 0;
      const Entry* pick = nullptr;
      for (const Entry& e : en) {
        if (e.taken) continue;
        const float a = lambda * e.rel, b = mu * e.pen;
        const float mmr = a - b;
        const uint64_t key = ((uint64_t)ordered_bits(mmr) << 32) | (uint64_t)(~(uint32_t)e.id);
        if (!pick || key > best) best = key, pick = &e;
      }
      const uint64_t sel = pick->id;
      out.doc_ids[(size_t)q * k + r] = sel;
      out.scores[(size_t)q * k + r] = pick->rel;
      out.penalties[(size_t)q * k + r] = pick->pen;
      ++r;
      for (Entry& e : en)
        if (!e.taken && e.id == sel) e.taken = true, --left;
      if (r == k || !left) break;
      const uint64_t s0 = h.fwd_offsets[sel], s1 = h.fwd_offsets[sel + 1];
      for (uint64_t x = s0; x < s1; ++x) dense[h.comp(x)] = f16 ? f16_to_f32(h.fwd_vals[x]) : h.val(x) * h.val_scale;
      for (Entry& e : en)
        if (!e.taken) e.pen = std::fmax(e.pen, score_one(h, e.id, dense));
      for (uint64_t x = s0; x < s1; ++x) dense[h.comp(x)] = 0.0f;
    }
    out.n[q] = r;
  }
  return SGPU_OK;
}

// Checks 1 - 7 of sgpu_collapse_documents, in the header's order.
sgpu_status collapse_check_args(const HostIndex& h, const uint64_t* q_off, const uint32_t* comps, const float* vals, uint32_t nq,
                                const uint64_t* cand_off, const uint64_t* cand_ids, const uint32_t* cand_groups, uint32_t m,
                                uint32_t k, const CollapseOut& out, uint32_t* max_nnz, uint32_t* max_cand) {
  if (!cand_groups || !out.groups || !out.best_ids || !out.best_scores || !out.members || !out.n) return fail(SGPU_EINVAL, "null argument");
  const sgpu_status vst = score_check_args(h, q_off, comps, vals, nq, cand_off, cand_ids, out.scores, max_nnz);
  if (vst != SGPU_OK) return vst;
  *max_cand = 0;
  for (uint32_t q = 0; q < nq; ++q) {
    if (cand_off[q + 1] - cand_off[q] > kCollapseMaxCand)
      return fail(SGPU_ELIMIT, "query %u has %llu candidates (collapsing documents: limit %llu)", q,
                  (unsigned long long)(cand_off[q + 1] - cand_off[q]), (unsigned long long)kCollapseMaxCand);
    *max_cand = std::max(*max_cand, (uint32_t)(cand_off[q + 1] - cand_off[q]));
  }
  if (m == 0) return fail(SGPU_EINVAL, "m must be at least 1");
  if (m > kCollapseMaxM) return fail(SGPU_ELIMIT, "m = %u (collapsing documents: limit %u)", m, kCollapseMaxM);
  if (k == 0) return fail(SGPU_EINVAL, "k must be at least 1");
  if (k > kCollapseMaxK) return fail(SGPU_ELIMIT, "k = %u (collapsing documents: limit %u)", k, kCollapseMaxK);
  return SGPU_OK;
}

// The host twin of collapse_documents.hip, the arbiter of its rows: per query the distinct (group key, id) pairs of its
// entries, each scored by score_one; the members of a group ordered by score descending and id ascending, the group's
// score the f32 sum of its first min(m, members) scores added in that order; the groups ordered by that sum descending
// and key ascending, cut to k. "Descending" is the order of the scores' integer images (ordered_bits), which is the
// numeric order wherever scores are finite, since -0.0 never occurs: the device's order.
sgpu_status collapse_documents_host(const HostIndex& h, const uint64_t* q_off, const uint32_t* comps, const float* vals, uint32_t nq,
                                    const uint64_t* cand_off, const uint64_t* cand_ids, const uint32_t* cand_groups, uint32_t m,
                                    uint32_t k, uint32_t num_threads, const CollapseOut& out) {
  uint32_t max_nnz = 0, max_cand = 0;
  const sgpu_status vst = collapse_check_args(h, q_off, comps, vals, nq, cand_off, cand_ids, cand_groups, m, k, out, &max_nnz, &max_cand);
  if (vst != SGPU_OK) return vst;
  if (nq == 0) return SGPU_OK;
  std::memset(out.groups, 0, (size_t)nq * k * sizeof(uint32_t));
  std::memset(out.scores, 0, (size_t)nq * k * sizeof(float));
  std::memset(out.best_ids, 0, (size_t)nq * k * sizeof(uint64_t));
  std::memset(out.best_scores, 0, (size_t)nq * k * sizeof(float));
  std::memset(out.members, 0, (size_t)nq * k * sizeof(uint32_t));
  std::memset(out.n, 0, (size_t)nq * sizeof(uint32_t));
  if (cand_off[nq] == 0) return SGPU_OK;
  int team = num_threads ? (int)num_threads : host_threads();
  team = (int)std::max<int64_t>(1, std::min<int64_t>(team, (int64_t)nq));
  struct Member {
    uint32_t group;
    uint64_t id;
    float score;
  };
  struct Group {
    uint32_t key;
    float score;
    uint64_t best_id;
    float best_score;
    uint32_t members;
  };
  struct Scratch {
    std::vector<float> table;
    std::vector<Member> mem;
    std::vector<Group> groups;
  };
  std::vector<Scratch> scratch;
  try {
    scratch.assign((size_t)team, Scratch());
    for (auto& s : scratch) {
      s.table.assign(h.dim, 0.0f);
      s.mem.reserve(max_cand);
      s.groups.reserve(max_cand);
    }
  } catch (const std::bad_alloc&) {
    return fail(SGPU_ENOMEM, "out of host memory");
  }
  const bool f16 = h.value_type == SGPU_VAL_F16;
#pragma omp parallel for schedule(dynamic, 1) num_threads(team)
  for (int64_t q = 0; q < (int64_t)nq; ++q) {
    if (cand_off[q + 1] == cand_off[q]) continue;
#ifdef _OPENMP
    Scratch& s = scratch[(size_t)omp_get_thread_num()];
#else
    Scratch& s = scratch[0];
#endif
    float* dense = s.table.data();
    std::vector<Member>& mem = s.mem;   // (both reserved for the longest list: nothing below allocates)
    std::vector<Group>& groups = s.groups;
    mem.clear();
    groups.clear();
    for (uint64_t i = cand_off[q]; i < cand_off[q + 1]; ++i) mem.push_back(Member{cand_groups[i], cand_ids[i], 0.0f});
    // the members: the distinct pairs
    std::sort(mem.begin(), mem.end(), [](const Member& a, const Member& b) { return a.group != b.group ? a.group < b.group : a.id < b.id; });
    mem.erase(std::unique(mem.begin(), mem.end(), [](const Member& a, const Member& b) { return a.group == b.group && a.id == b.id; }),
              mem.end());
    for (uint64_t j = q_off[q]; j < q_off[q + 1]; ++j) dense[comps[j]] = f16 ? vals[j] : vals[j] * h.val_scale;
    for (Member& x : mem) x.score = score_one(h, x.id, dense);
    for (uint64_t j = q_off[q]; j < q_off[q + 1]; ++j) dense[comps[j]] = 0.0f;
    // group by group, its members best first
    std::sort(mem.begin(), mem.end(), [](const Member& a, const Member& b) {
      if (a.group != b.group) return a.group < b.group;
      const uint32_t ka = ordered_bits(a.score), kb = ordered_bits(b.score);
      return ka != kb ? ka > kb : a.id < b.id;
    });
    for (size_t a = 0; a < mem.size();) {
      size_t b = a;
      while (b < mem.size() && mem[b].group == mem[a].group) ++b;
      float sum = mem[a].score;
      for (size_t i = a + 1; i < b && i < a + m; ++i) sum = sum + mem[i].score;
      groups.push_back(Group{mem[a].group, sum, mem[a].id, mem[a].score, (uint32_t)(b - a)});
      a = b;
    }
    const size_t n = std::min<size_t>(k, groups.size());
    std::partial_sort(groups.begin(), groups.begin() + (ptrdiff_t)n, groups.end(), [](const Group& a, const Group& b) {
      const uint32_t ka = ordered_bits(a.score), kb = ordered_bits(b.score);
      return ka != kb ? ka > kb : a.key < b.key;
    });
    for (size_t i = 0; i < n; ++i) {
      const size_t o = (size_t)q * k + i;
      out.groups[o] = groups[i].key;
      out.scores[o] = groups[i].score;
      out.best_ids[o] = groups[i].best_id;
      out.best_scores[o] = groups[i].best_score;
      out.members[o] = groups[i].members;
    }
    out.n[q] = (uint32_t)n;
  }
  return SGPU_OK;
}

// Checks 1 - 9 of sgpu_fuse_documents, in the header's order.
sgpu_status fuse_check_args(const HostIndex& h, const uint64_t* q_off, const uint32_t* comps, const float* vals, uint32_t nq,
                            const uint64_t* cand_off, const uint64_t* cand_ids, const float* cand_ext, uint32_t method,
                            float w_sparse, float w_ext, float rrf_c, uint32_t k, const FuseOut& out, uint32_t* max_nnz,
                            uint32_t* max_cand) {
  if (!cand_ext || !out.doc_ids || !out.sparse || !out.ext || !out.rank_sparse || !out.rank_ext || !out.n) return fail(SGPU_EINVAL, "null argument");
  const sgpu_status vst = score_check_args(h, q_off, comps, vals, nq, cand_off, cand_ids, out.scores, max_nnz);
  if (vst != SGPU_OK) return vst;
  for (uint32_t q = 0; q < nq; ++q)
    for (uint64_t i = cand_off[q]; i < cand_off[q + 1]; ++i)
      if (std::isinf(cand_ext[i]))
        return fail(SGPU_EINVAL, "query %u: the external score of candidate %llu (document id %llu) is infinite", q,
                    (unsigned long long)(i - cand_off[q]), (unsigned long long)cand_ids[i]);
  if (method != SGPU_FUSE_RRF && method != SGPU_FUSE_MINMAX && method != SGPU_FUSE_SUM) return fail(SGPU_EINVAL, "unknown fusion method %u", method);
  if (!std::isfinite(w_sparse)) return fail(SGPU_EINVAL, "w_sparse is not finite");
  if (!std::isfinite(w_ext)) return fail(SGPU_EINVAL, "w_ext is not finite");
  if (method == SGPU_FUSE_RRF && !(std::isfinite(rrf_c) && rrf_c >= 0.0f)) return fail(SGPU_EINVAL, "rrf_c is not a finite number >= 0");
  *max_cand = 0;
  for (uint32_t q = 0; q < nq; ++q) {
    if (cand_off[q + 1] - cand_off[q] > kFuseMaxCand)
      return fail(SGPU_ELIMIT, "query %u has %llu candidates (fusing documents: limit %llu)", q,
                  (unsigned long long)(cand_off[q + 1] - cand_off[q]), (unsigned long long)kFuseMaxCand);
    *max_cand = std::max(*max_cand, (uint32_t)(cand_off[q + 1] - cand_off[q]));
  }
  if (k == 0) return fail(SGPU_EINVAL, "k must be at least 1");
  if (k > kFuseMaxK) return fail(SGPU_ELIMIT, "k = %u (fusing documents: limit %u)", k, kFuseMaxK);
  return SGPU_OK;
}

// The host twin of fuse_documents.hip, the arbiter of its rows: per query the distinct ids of its entries, each with the
// largest external score listed for it that is no NaN (by ordered_bits; none: absent) and scored once by score_one; the
// ordinal ranks of both orders from two sorts (ordered_bits descending, id ascending); the fused score of the header in
// plain f32 expressions, one operation per statement (this file is compiled with -ffp-contract=off); the documents
// ordered by ordered_bits(fused) descending and id ascending, cut to k.
sgpu_status fuse_documents_host(const HostIndex& h, const uint64_t* q_off, const uint32_t* comps, const float* vals, uint32_t nq,
                                const uint64_t* cand_off, const uint64_t* cand_ids, const float* cand_ext, uint32_t method,
                                float w_sparse, float w_ext, float rrf_c, uint32_t k, uint32_t num_threads, const FuseOut& out) {
  uint32_t max_nnz = 0, max_cand = 0;
  const sgpu_status vst =
      fuse_check_args(h, q_off, comps, vals, nq, cand_off, cand_ids, cand_ext, method, w_sparse, w_ext, rrf_c, k, out, &max_nnz, &max_cand);
  if (vst != SGPU_OK) return vst;
  if (nq == 0) return SGPU_OK;
  std::memset(out.scores, 0, (size_t)nq * k * sizeof(float));
  std::memset(out.doc_ids, 0, (size_t)nq * k * sizeof(uint64_t));
  std::memset(out.sparse, 0, (size_t)nq * k * sizeof(float));
  std::memset(out.ext, 0, (size_t)nq * k * sizeof(float));
  std::memset(out.rank_sparse, 0, (size_t)nq * k * sizeof(uint32_t));
  std::memset(out.rank_ext, 0, (size_t)nq * k * sizeof(uint32_t));
  std::memset(out.n, 0, (size_t)nq * sizeof(uint32_t));
  if (cand_off[nq] == 0) return SGPU_OK;
  int team = num_threads ? (int)num_threads : host_threads();
  team = (int)std::max<int64_t>(1, std::min<int64_t>(team, (int64_t)nq));
  struct Doc {
    uint64_t id;
    uint32_t ext_key;   // ordered_bits of the external score, 0: absent (an entry: its own, 0 for NaN)
    float sparse, ext, fused;
    uint32_t rank_s, rank_e;
  };
  struct Scratch {
    std::vector<float> table;
    std::vector<Doc> docs;
    std::vector<uint32_t> order;
  };
  std::vector<Scratch> scratch;
  try {
    scratch.assign((size_t)team, Scratch());
    for (auto& s : scratch) {
      s.table.assign(h.dim, 0.0f);
      s.docs.reserve(max_cand);
      s.order.reserve(max_cand);
    }
  } catch (const std::bad_alloc&) {
    return fail(SGPU_ENOMEM, "out of host memory");
  }
  const bool f16 = h.value_type == SGPU_VAL_F16;
#pragma omp parallel for schedule(dynamic, 1) num_threads(team)
  for (int64_t q = 0; q < (int64_t)nq; ++q) {
    if (cand_off[q + 1] == cand_off[q]) continue;
#ifdef _OPENMP
    Scratch& s = scratch[(size_t)omp_get_thread_num()];
#else
    Scratch& s = scratch[0];
#endif
    float* dense = s.table.data();
    std::vector<Doc>& docs = s.docs;   // (both reserved for the longest list: nothing below allocates)
    std::vector<uint32_t>& order = s.order;
    docs.clear();
    for (uint64_t i = cand_off[q]; i < cand_off[q + 1]; ++i)
      docs.push_back(Doc{cand_ids[i], std::isnan(cand_ext[i]) ? 0u : ordered_bits(cand_ext[i]), 0.0f, 0.0f, 0.0f, 0u, 0u});
    // the documents: the distinct ids, each with its largest external key
    std::sort(docs.begin(), docs.end(), [](const Doc& a, const Doc& b) { return a.id != b.id ? a.id < b.id : a.ext_key > b.ext_key; });
    docs.erase(std::unique(docs.begin(), docs.end(), [](const Doc& a, const Doc& b) { return a.id == b.id; }), docs.end());
    for (uint64_t j = q_off[q]; j < q_off[q + 1]; ++j) dense[comps[j]] = f16 ? vals[j] : vals[j] * h.val_scale;
    for (Doc& d : docs) {
      d.sparse = score_one(h, d.id, dense);
      d.ext = d.ext_key ? ordered_bits_inv(d.ext_key) : 0.0f;
    }
    for (uint64_t j = q_off[q]; j < q_off[q + 1]; ++j) dense[comps[j]] = 0.0f;
    // the ranks of both orders, and their ends
    order.clear();
    for (uint32_t i = 0; i < docs.size(); ++i) order.push_back(i);
    std::sort(order.begin(), order.end(), [&docs](uint32_t a, uint32_t b) {
      const uint32_t ka = ordered_bits(docs[a].sparse), kb = ordered_bits(docs[b].sparse);
      return ka != kb ? ka > kb : docs[a].id < docs[b].id;
    });
    for (uint32_t r = 0; r < order.size(); ++r) docs[order[r]].rank_s = r + 1;
    const float hi_s = docs[order.front()].sparse, lo_s = docs[order.back()].sparse;
    order.clear();
    for (uint32_t i = 0; i < docs.size(); ++i)
      if (docs[i].ext_key) order.push_back(i);
    std::sort(order.begin(), order.end(), [&docs](uint32_t a, uint32_t b) {
      return docs[a].ext_key != docs[b].ext_key ? docs[a].ext_key > docs[b].ext_key : docs[a].id < docs[b].id;
    });
    for (uint32_t r = 0; r < order.size(); ++r) docs[order[r]].rank_e = r + 1;
    float hi_e = 0.0f, lo_e = 0.0f;
    if (!order.empty()) hi_e = docs[order.front()].ext, lo_e = docs[order.back()].ext;
    // the fused scores: every operation a statement of its own, rounded once
    const float span_s = hi_s - lo_s, span_e = hi_e - lo_e;
    for (Doc& d : docs) {
      const bool present = d.ext_key != 0;
      float a, b = 0.0f;
      if (method == SGPU_FUSE_RRF) {
        const float ds = rrf_c + (float)d.rank_s;
        a = w_sparse / ds;
        if (present) {
          const float de = rrf_c + (float)d.rank_e;
          b = w_ext / de;
        }
      } else if (method == SGPU_FUSE_MINMAX) {
        float ns = 1.0f, ne = 1.0f;
        if (!(hi_s == lo_s)) {
          const float t = d.sparse - lo_s;
          ns = t / span_s;
        }
        a = w_sparse * ns;
        if (present) {
          if (!(hi_e == lo_e)) {
            const float t = d.ext - lo_e;
            ne = t / span_e;
          }
          b = w_ext * ne;
        }
      } else {
        a = w_sparse * d.sparse;
        if (present) b = w_ext * d.ext;
      }
      d.fused = a + b;
    }
    const size_t n = std::min<size_t>(k, docs.size());
    std::partial_sort(docs.begin(), docs.begin() + (ptrdiff_t)n, docs.end(), [](const Doc& a, const Doc& b) {
      const uint32_t ka = ordered_bits(a.fused), kb = ordered_bits(b.fused);
      return ka != kb ? ka > kb : a.id < b.id;
    });
    for (size_t i = 0; i < n; ++i) {
      const size_t o = (size_t)q * k + i;
      out.scores[o] = docs[i].fused;
      out.doc_ids[o] = docs[i].id;
      out.sparse[o] = docs[i].sparse;
      out.ext[o] = docs[i].ext;
      out.rank_sparse[o] = docs[i].rank_s;
      out.rank_ext[o] = docs[i].rank_e;
    }
    out.n[q] = (uint32_t)n;
  }
  return SGPU_OK;
}

}  // namespace sgpu
