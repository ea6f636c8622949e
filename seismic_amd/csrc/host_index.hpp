// host_index.hpp — canonical host-side index (the arrays of sgpu_index_desc, owned).
#pragma once
#include <cstdint>
#include <atomic>
#include <mutex>
#include <vector>

#include "common.hpp"

namespace sgpu {

struct DeviceIndex;  // device_index.hpp
struct ExactFile;    // exact_file.hpp
struct ScoreState;   // score_state.hpp
struct ColumnState;  // columns.hpp

// One document column (sgpu_index_set_column): the host copy, and which set_column call made it - a replica's device copy
// remembers the generation it was made from (columns.hpp). generation == 0: the slot is empty.
struct HostColumn {
  uint32_t type = 0;
  uint32_t max_u32 = 0;   // U32 columns: the largest value
  uint64_t generation = 0;
  std::vector<uint32_t> values;
};

struct HostIndex {
  uint32_t comp_width = 2;
  uint64_t n_docs = 0, dim = 0;
  std::vector<uint64_t> fwd_offsets;
  std::vector<uint8_t> fwd_comps;  // nnz * comp_width bytes
  std::vector<uint16_t> fwd_vals;   // value_type F16: binary16 bits
  std::vector<uint8_t> fwd_codes;   // value_type FIXEDU8: value = code * val_scale
  uint32_t value_type = SGPU_VAL_F16;
  float val_scale = 0.0f;
  std::vector<uint64_t> list_block_start, block_post_start;
  std::vector<uint32_t> post_doc;
  std::vector<float> blk_min, blk_quant;
  std::vector<uint64_t> list_row_start;
  std::vector<uint8_t> row_comp;  // n_rows * comp_width bytes
  std::vector<uint64_t> row_ptr;
  std::vector<uint16_t> sum_bid;
  std::vector<uint8_t> sum_code;
  // optional kNN graph (reference Knn, src/inverted_index.rs:430-435): neighbour ids flattened in
  // document order, knn_dim per document (the reference flattens the same way, :487-493)
  std::vector<uint32_t> knn;
  uint32_t knn_dim = 0;

  uint64_t nnz() const { return fwd_offsets.empty() ? 0 : fwd_offsets.back(); }
  uint64_t n_blocks() const { return list_block_start.empty() ? 0 : list_block_start.back(); }
  uint64_t n_postings() const { return block_post_start.empty() ? 0 : block_post_start.back(); }
  uint64_t n_rows() const { return list_row_start.empty() ? 0 : list_row_start.back(); }
  uint64_t n_entries() const { return row_ptr.empty() ? 0 : row_ptr.back(); }
  inline uint32_t comp(uint64_t i) const {
    return comp_width == 2 ? (uint32_t)((const uint16_t*)fwd_comps.data())[i]
                           : ((const uint32_t*)fwd_comps.data())[i];
  }
  inline float val(uint64_t i) const {   // document value i as f32 (exact for both value types)
    return value_type == SGPU_VAL_F16 ? f16_to_f32(fwd_vals[i]) : (float)fwd_codes[i] * val_scale;
  }
  inline uint32_t val_bytes() const { return value_type == SGPU_VAL_F16 ? 2u : 1u; }   // (fixed-u8 and DotVByte: u8 codes)
  inline uint32_t rcomp(uint64_t i) const {
    return comp_width == 2 ? (uint32_t)((const uint16_t*)row_comp.data())[i]
                           : ((const uint32_t*)row_comp.data())[i];
  }
  void fill_desc(sgpu_index_desc* d) const;
};

// structural validation of a descriptor (monotone offsets, ids in range, sorted rows ...)
sgpu_status validate_desc(const sgpu_index_desc& d);
sgpu_status host_index_from_desc(const sgpu_index_desc& d, HostIndex* out);
sgpu_status host_index_save(const HostIndex& ix, const char* path);
sgpu_status host_index_load(const char* path, HostIndex* out);
sgpu_status host_index_convert(const HostIndex& src, uint32_t value_type, HostIndex* out);

// CSR query batch: q_off[0] == 0 and monotone, components strictly ascending and < dim, no NaN,
// at most 65535 components per query; *max_nnz = the longest query. Error messages name query q_base + q
// (a chunk or shard of a larger batch reports the caller's numbering).
sgpu_status validate_queries(uint64_t dim, const uint64_t* q_off, const uint32_t* comps, const float* vals,
                             uint32_t nq, uint32_t* max_nnz, uint32_t q_base = 0);
// the offsets alone (monotone, query and batch size limits): what has to hold before a batch is cut
sgpu_status validate_query_offsets(const uint64_t* q_off, uint32_t nq, uint32_t q_base, uint32_t* max_nnz);
// pack_index.cpp: the host half of the upload (HBM layout of DESIGN.md section 2), on all host cores
// (raw: per document, 1 = a DotVByte index keeps the document in the raw record form; empty for the other value types)
void pack_dvb_raw_flags(const HostIndex& h, std::vector<uint8_t>* raw);
void pack_record_offsets(const HostIndex& h, const std::vector<uint8_t>& raw, uint64_t line16, std::vector<uint64_t>* rec_off16);
void pack_records(const HostIndex& h, const std::vector<uint8_t>& raw, const std::vector<uint64_t>& rec_off16, std::vector<uint8_t>* fwd);
void pack_block_sizes(const HostIndex& h, const std::vector<uint8_t>& raw, std::vector<uint64_t>* bsize);
void pack_post_refs(const HostIndex& h, const std::vector<uint8_t>& raw, const std::vector<uint64_t>& rec_off16,
                    const std::vector<uint64_t>& bsize, bool block_major, uint64_t blk_base, std::vector<uint64_t>* pref);
void pack_doc_refs(const HostIndex& h, const std::vector<uint8_t>& raw, const std::vector<uint64_t>& rec_off16, std::vector<uint64_t>* dref);
void pack_narrow(const std::vector<uint64_t>& v, std::vector<uint32_t>* out);
void pack_row_mid(const HostIndex& h, std::vector<uint16_t>* mid);
bool pack_row_dir(const HostIndex& h, const std::vector<uint16_t>& mid, std::vector<uint32_t>* out, uint32_t* n_buckets);
void pack_sum_deq(const HostIndex& h, std::vector<float>* deq);

// builder.cpp
sgpu_status build_host_index(uint32_t comp_width, uint64_t n_docs, uint64_t dim, const uint64_t* offsets,
                             const void* comps, const float* vals, const sgpu_build_config& cfg,
                             HostIndex* out);
// exact.cpp
// (allow: null, or the allowed set as a bitmap - bit d of word d / 32: the other documents are not candidates)
sgpu_status exact_search_host(const HostIndex& ix, const uint64_t* q_off, const uint32_t* comps,
                              const float* vals, uint32_t nq, uint32_t k, uint32_t num_threads,
                              float* out_scores, uint64_t* out_ids, uint32_t* out_n, const uint32_t* allow = nullptr);
// exact_device.hip
void exact_file_free(ExactFile* f);
sgpu_status exact_search_device(sgpu_index* idx, uint32_t replica, const uint64_t* q_off, const uint32_t* comps,
                                const float* vals, uint32_t nq, uint32_t k, float* out_scores, uint64_t* out_ids,
                                uint32_t* out_n, const sgpu_filter* filter);
bool exact_debug_launches(sgpu_index* idx, uint32_t replica, uint32_t* out);
// score_host.cpp: scores of caller-given documents (sgpu_score_documents_host) and the argument checks both calls run
constexpr uint32_t kScoreMaxQueryNnz = 8192;   // components of a query (the device's hash table: 2^14 slots, half full)
sgpu_status score_check_args(const HostIndex& h, const uint64_t* q_off, const uint32_t* comps, const float* vals, uint32_t nq,
                             const uint64_t* cand_off, const uint64_t* cand_ids, const float* out_scores, uint32_t* max_nnz);
sgpu_status score_documents_host(const HostIndex& h, const uint64_t* q_off, const uint32_t* comps, const float* vals, uint32_t nq,
                                 const uint64_t* cand_off, const uint64_t* cand_ids, uint32_t num_threads, float* out_scores);
sgpu_status score_documents_device(sgpu_index* idx, uint32_t replica, const uint64_t* q_off, const uint32_t* comps,
                                   const float* vals, uint32_t nq, const uint64_t* cand_off, const uint64_t* cand_ids,
                                   float* out_scores);
// the k best distinct candidates of each query (sgpu_rerank_documents_host) and checks 1 - 4 both rerank calls run
constexpr uint32_t kRerankMaxK = 1024;
sgpu_status rerank_check_args(const HostIndex& h, const uint64_t* q_off, const uint32_t* comps, const float* vals, uint32_t nq,
                              const uint64_t* cand_off, const uint64_t* cand_ids, uint32_t k, const float* out_scores,
                              const uint64_t* out_doc_ids, const uint32_t* out_n, uint32_t* max_nnz);
sgpu_status rerank_documents_host(const HostIndex& h, const uint64_t* q_off, const uint32_t* comps, const float* vals, uint32_t nq,
                                  const uint64_t* cand_off, const uint64_t* cand_ids, uint32_t k, uint32_t num_threads,
                                  float* out_scores, uint64_t* out_doc_ids, uint32_t* out_n);
sgpu_status rerank_documents_device(sgpu_index* idx, uint32_t replica, const uint64_t* q_off, const uint32_t* comps,
                                    const float* vals, uint32_t nq, const uint64_t* cand_off, const uint64_t* cand_ids, uint32_t k,
                                    float* out_scores, uint64_t* out_doc_ids, uint32_t* out_n);
// the m best terms behind each candidate's score (sgpu_explain_documents_host) and the checks both explain calls run
constexpr uint32_t kExplainMaxTerms = 32;
struct ExplainOut {   // the outputs of an explain call: one score and count per candidate, rows of m per term array
  float* scores;
  uint32_t* n_terms;
  uint32_t* comps;
  float* q_vals;
  float* d_vals;
  float* products;
};
sgpu_status explain_check_args(const HostIndex& h, const uint64_t* q_off, const uint32_t* comps, const float* vals, uint32_t nq,
                               const uint64_t* cand_off, const uint64_t* cand_ids, uint32_t m, const ExplainOut& out,
                               uint32_t* max_nnz);
sgpu_status explain_documents_host(const HostIndex& h, const uint64_t* q_off, const uint32_t* comps, const float* vals, uint32_t nq,
                                   const uint64_t* cand_off, const uint64_t* cand_ids, uint32_t m, uint32_t num_threads,
                                   const ExplainOut& out);
sgpu_status explain_documents_device(sgpu_index* idx, uint32_t replica, const uint64_t* q_off, const uint32_t* comps,
                                     const float* vals, uint32_t nq, const uint64_t* cand_off, const uint64_t* cand_ids, uint32_t m,
                                     const ExplainOut& out);
// Rocchio feedback queries (sgpu_expand_queries_host) and checks 1 - 6 both expand calls run
constexpr uint32_t kExpandMaxTerms = 1024;
constexpr uint64_t kExpandMaxCand = 65536;   // feedback documents of one query
sgpu_status expand_check_args(const HostIndex& h, const uint64_t* q_off, const uint32_t* comps, const float* vals, uint32_t nq,
                              const uint64_t* cand_off, const uint64_t* cand_ids, const float* cand_w, float alpha, uint32_t t,
                              const uint32_t* out_comps, const float* out_vals, const uint32_t* out_n, uint32_t* max_nnz);
sgpu_status expand_queries_host(const HostIndex& h, const uint64_t* q_off, const uint32_t* comps, const float* vals, uint32_t nq,
                                const uint64_t* cand_off, const uint64_t* cand_ids, const float* cand_w, float alpha, uint32_t t,
                                uint32_t num_threads, uint32_t* out_comps, float* out_vals, uint32_t* out_n);
sgpu_status expand_queries_device(sgpu_index* idx, uint32_t replica, const uint64_t* q_off, const uint32_t* comps, const float* vals,
                                  uint32_t nq, const uint64_t* cand_off, const uint64_t* cand_ids, const float* cand_w, float alpha,
                                  uint32_t t, uint32_t* out_comps, float* out_vals, uint32_t* out_n);
// MMR selection of candidates (sgpu_diversify_documents_host) and checks 1 - 7 both diversify calls run
constexpr uint32_t kDiversifyMaxK = 256;
constexpr uint64_t kDiversifyMaxCand = 2048;   // listed candidates of one query (the device keeps their state in LDS)
struct DiversifyOut {   // the outputs of a diversify call: rows of k and a count per query
  float* scores;
  float* penalties;
  uint64_t* doc_ids;
  uint32_t* n;
};
// (*max_len = the stored components of the longest candidate document, *max_cand = the candidates of the longest list)
sgpu_status diversify_check_args(const HostIndex& h, const uint64_t* q_off, const uint32_t* comps, const float* vals, uint32_t nq,
                                 const uint64_t* cand_off, const uint64_t* cand_ids, float lambda, float mu, uint32_t k,
                                 const DiversifyOut& out, uint32_t* max_nnz, uint32_t* max_len, uint32_t* max_cand);
sgpu_status diversify_documents_host(const HostIndex& h, const uint64_t* q_off, const uint32_t* comps, const float* vals, uint32_t nq,
                                     const uint64_t* cand_off, const uint64_t* cand_ids, float lambda, float mu, uint32_t k,
                                     uint32_t num_threads, const DiversifyOut& out);
sgpu_status diversify_documents_device(sgpu_index* idx, uint32_t replica, const uint64_t* q_off, const uint32_t* comps,
                                       const float* vals, uint32_t nq, const uint64_t* cand_off, const uint64_t* cand_ids, float lambda,
                                       float mu, uint32_t k, const DiversifyOut& out);
// the k best groups of each query's candidates (sgpu_collapse_documents_host) and checks 1 - 7 both collapse calls run
constexpr uint32_t kCollapseMaxK = 1024;
constexpr uint32_t kCollapseMaxM = 64;        // members a group's score sums (a sequential sum by contract)
constexpr uint64_t kCollapseMaxCand = 4096;   // listed candidates of one query (the device sorts them in LDS)
struct CollapseOut {   // the outputs of a collapse call: rows of k and a count per query
  uint32_t* groups;
  float* scores;
  uint64_t* best_ids;
  float* best_scores;
  uint32_t* members;
  uint32_t* n;
};
// (*max_cand = the candidates of the longest list)
sgpu_status collapse_check_args(const HostIndex& h, const uint64_t* q_off, const uint32_t* comps, const float* vals, uint32_t nq,
                                const uint64_t* cand_off, const uint64_t* cand_ids, const uint32_t* cand_groups, uint32_t m,
                                uint32_t k, const CollapseOut& out, uint32_t* max_nnz, uint32_t* max_cand);
sgpu_status collapse_documents_host(const HostIndex& h, const uint64_t* q_off, const uint32_t* comps, const float* vals, uint32_t nq,
                                    const uint64_t* cand_off, const uint64_t* cand_ids, const uint32_t* cand_groups, uint32_t m,
                                    uint32_t k, uint32_t num_threads, const CollapseOut& out);
sgpu_status collapse_documents_device(sgpu_index* idx, uint32_t replica, const uint64_t* q_off, const uint32_t* comps,
                                      const float* vals, uint32_t nq, const uint64_t* cand_off, const uint64_t* cand_ids,
                                      const uint32_t* cand_groups, uint32_t m, uint32_t k, const CollapseOut& out);
// hybrid fusion of each query's candidates with another retriever's scores (sgpu_fuse_documents_host) and checks 1 - 9 both
// fuse calls run
constexpr uint32_t kFuseMaxK = 1024;
constexpr uint64_t kFuseMaxCand = 4096;   // listed candidates of one query (the device sorts them in LDS)
struct FuseOut {   // the outputs of a fuse call: rows of k and a count per query
  float* scores;
  uint64_t* doc_ids;
  float* sparse;
  float* ext;
  uint32_t* rank_sparse;
  uint32_t* rank_ext;
  uint32_t* n;
};
// (*max_cand = the candidates of the longest list)
sgpu_status fuse_check_args(const HostIndex& h, const uint64_t* q_off, const uint32_t* comps, const float* vals, uint32_t nq,
                            const uint64_t* cand_off, const uint64_t* cand_ids, const float* cand_ext, uint32_t method,
                            float w_sparse, float w_ext, float rrf_c, uint32_t k, const FuseOut& out, uint32_t* max_nnz,
                            uint32_t* max_cand);
sgpu_status fuse_documents_host(const HostIndex& h, const uint64_t* q_off, const uint32_t* comps, const float* vals, uint32_t nq,
                                const uint64_t* cand_off, const uint64_t* cand_ids, const float* cand_ext, uint32_t method,
                                float w_sparse, float w_ext, float rrf_c, uint32_t k, uint32_t num_threads, const FuseOut& out);
sgpu_status fuse_documents_device(sgpu_index* idx, uint32_t replica, const uint64_t* q_off, const uint32_t* comps, const float* vals,
                                  uint32_t nq, const uint64_t* cand_off, const uint64_t* cand_ids, const float* cand_ext,
                                  uint32_t method, float w_sparse, float w_ext, float rrf_c, uint32_t k, const FuseOut& out);
// score_documents.hip (the state itself: score_state.hpp)
void score_state_free(ScoreState* s);
// what the last candidate call of a kind on `replica` measured (the sgpu_debug_*_stats test hooks; false: none has run) -
// each in the .hip file of its call, score_debug_stats (score, rerank, explain) in score_documents.hip
bool score_debug_stats(sgpu_index* idx, uint32_t replica, double* out8);
bool expand_debug_stats(sgpu_index* idx, uint32_t replica, double* out8);
bool diversify_debug_stats(sgpu_index* idx, uint32_t replica, double* out8);
bool collapse_debug_stats(sgpu_index* idx, uint32_t replica, double* out8);
bool fuse_debug_stats(sgpu_index* idx, uint32_t replica, double* out8);

// filter.hip: which filter a launch searches with (f null: none) and on which replica of the index
struct FilterRef {
  const sgpu_filter* f;
  uint32_t replica;
};

}  // namespace sgpu

// the opaque handle of the C ABI
struct sgpu_index {
  sgpu::HostIndex host;
  std::vector<sgpu::DeviceIndex*> replicas;   // one per device the index was uploaded to
  sgpu::DeviceIndex* dev = nullptr;           // replicas[0] (null before upload)
  std::atomic<uint32_t> next_replica{0};      // calls too small to shard go to the replicas in turn
  std::vector<sgpu::ExactFile*> exact;        // per replica: the exact file (null until its first exact call)
  std::mutex exact_mu;                        // its lazy build
  std::vector<sgpu::ScoreState*> score;       // per replica: stream and scratch of sgpu_score_documents (null until its first call)
  std::mutex score_mu;                        // their creation
  // bumped by every call that replaces device state a filter's views derive from (upload, upload_many, set_knn,
  // build_knn): a view built under an older generation is rebuilt on its next use, never dereferenced (filter.hip)
  std::atomic<uint64_t> generation{0};
  // document columns (columns.hpp): not part of the index file; column_mu guards the creation of the replicas' states and,
  // together with every state's own mutex, the replacement of a column
  sgpu::HostColumn columns[SGPU_MAX_COLUMNS];
  uint64_t column_generation = 0;
  std::vector<sgpu::ColumnState*> column_state;   // per replica (null until its first column call)
  std::mutex column_mu;
};
