/*
 * seismic_hip.h — C ABI of the MI355X-native Seismic search hot path.
 *
 * This is the drop-in boundary. The reference (TusKANNy/seismic, Rust) has no
 * C ABI of its own; its narrowest seam for this path is the Rust method
 *
 *   InvertedIndexBase::<S>::search(&self, query: SparseVectorView<C, f32>,
 *       k, query_cut, heap_factor, n_knn, first_sorted) -> Vec<ScoredVectorDotProduct>
 *   (reference: src/inverted_index.rs:153-234)
 *
 * wrapped by SeismicIndex::search_raw/search (src/inverted_index_wrapper.rs:218-284)
 * and by the PyO3 classes (src/pylib/mod.rs:504-533, 587-655, 1046-1076, 1111-1146).
 * Every entry point below names the reference item it replaces. INTEGRATION.md
 * shows the `extern "C"` block a maintainer of the reference would add to bind it.
 *
 * Conventions
 *   - plain pointers and sizes only; the caller owns every buffer it passes in
 *     or receives results in; the library keeps no pointer past the call
 *     (sgpu_index_create COPIES the descriptor's arrays).
 *   - every function returns an sgpu_status; nothing aborts or throws across
 *     the boundary (the reference panics instead: src/inverted_index.rs:172-175,
 *     src/utils.rs:23).
 *   - results are best-first; fewer than k results is not an error
 *     (src/bin/perf_inverted_index.rs:201-206); out_n[q] gives the valid count.
 *   - the search entry points run on the GPU only. There is no CPU fallback:
 *     without a usable HIP device they return SGPU_EDEVICE.
 */
#ifndef SEISMIC_HIP_H
#define SEISMIC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum sgpu_status {
  SGPU_OK = 0,
  SGPU_EINVAL = 1,   /* bad argument: k==0, unsorted/duplicate query components,
                        component >= dim, inconsistent descriptor */
  SGPU_EDEVICE = 2,  /* HIP failure / no device / index not uploaded */
  SGPU_ENOMEM = 3,   /* host or device allocation failed */
  SGPU_EIO = 4,      /* file could not be read / written / parsed */
  SGPU_ELIMIT = 5    /* a documented capacity limit of the kernel was exceeded */
} sgpu_status;

/* ------------------------------------------------------------------------
 * Index descriptor: the searchable state of the reference's
 * InvertedIndexBase<S> (src/inverted_index.rs:39-52) as flat host SoA arrays.
 *
 *   forward index  (reference: vectorium SparseDataset; call sites
 *                   src/posting_list.rs:203,210, src/inverted_index.rs:231)
 *     doc d = components fwd_comps[fwd_offsets[d] .. fwd_offsets[d+1]) (ascending)
 *             values     fwd_vals [same range], IEEE binary16 bit patterns
 *   posting lists  (reference: PostingList<C>, src/posting_list.rs:68-73)
 *     list c (one per component id) owns blocks
 *             [list_block_start[c], list_block_start[c+1])      (global block ids)
 *     block b owns postings [block_post_start[b], block_post_start[b+1])
 *     posting p refers to document post_doc[p]  (the reference packs
 *             (offset<<16)|len, src/posting_list.rs:32-60; offset/len are
 *             recovered here from fwd_offsets)
 *   quantized summaries (reference: QuantizedSummary<C>, src/quantized_summary.rs:15-24)
 *     blk_min[b], blk_quant[b]: dequantisation of block b's summary
 *     list c owns summary rows [list_row_start[c], list_row_start[c+1]);
 *     row r: component row_comp[r] (ascending within a list), entries
 *            [row_ptr[r], row_ptr[r+1]): sum_bid[e] = block id LOCAL to the list
 *            (ascending within a row), sum_code[e] = u8 code.
 *     (the reference stores the same CSR with Elias-Fano offsets and a packed
 *      BitField of summary ids; the codecs carry no arithmetic.)
 * ---------------------------------------------------------------------- */
/* Document value storage (the reference's value types, src/bin/build_inverted_index.rs:255-292):
 *   SGPU_VAL_F16     half::f16, the default.
 *   SGPU_VAL_FIXEDU8 unsigned 8-bit fixed point: value = code * val_scale. Replaces vectorium's
 *                    FixedU8Q / the value half of DotVByteFixedU8Encoder ("8-bit fixed-point
 *                    quantization (Q0.8)", docs/TomlInstructions.md:100). The codec is not in the
 *                    reference tree: PARITY UNPINNED. Restated as: val_scale = the smallest power of
 *                    two with 255 * val_scale >= the largest value (2^-8, i.e. Q0.8, for values
 *                    below 1); code = min(255, round_half_away(v / val_scale)), negatives -> 0.
 *                    Either component width (the reference's "fixedu8" goes with u16 and u32 components,
 *                    src/bin/perf_inverted_index.rs:110-126; its DotVByte class is u16-only).
 *   SGPU_VAL_DOTVBYTE the forward index of the reference's DotVByte index (SeismicIndexDotVByte,
 *                    src/pylib/dotvbyte.rs:15-22, 208-213; `dotvbyte` value type of the CLI,
 *                    src/bin/perf_inverted_index.rs:110-126): the FIXEDU8 values PLUS a compressed
 *                    component stream. The host-side arrays of the descriptor are those of FIXEDU8 (u16
 *                    components, u8 codes); the compression is the HBM layout: per 8-element slice three dwords
 *                    instead of four (the first component in 16 bits, three 12-bit and four 11-bit gaps), a document
 *                    with a gap that does not fit its field keeps the raw record form. The reference's codec (vectorium's DotVByte, a
 *                    variable-byte gap stream) is not in the tree: PARITY UNPINNED; it is lossless, so results
 *                    are those of the FIXEDU8 index - which is what the tests assert. u16 components only (as the
 *                    reference's class), documents of fewer than 32768 components. */
enum { SGPU_VAL_F16 = 0, SGPU_VAL_FIXEDU8 = 1, SGPU_VAL_DOTVBYTE = 2 };

typedef struct sgpu_index_desc {
  uint32_t comp_width;            /* 2 (SeismicIndex, u16) or 4 (SeismicIndexLV, u32) */
  uint32_t value_type;            /* SGPU_VAL_F16, SGPU_VAL_FIXEDU8 or SGPU_VAL_DOTVBYTE: how fwd_vals stores document values */
  uint64_t n_docs;
  uint64_t dim;                   /* number of components == number of posting lists */
  uint64_t nnz;                   /* fwd_offsets[n_docs] */
  uint64_t n_blocks;              /* list_block_start[dim] */
  uint64_t n_postings;            /* block_post_start[n_blocks] */
  uint64_t n_rows;                /* list_row_start[dim] */
  uint64_t n_entries;             /* row_ptr[n_rows] */
  const uint64_t* fwd_offsets;    /* n_docs + 1 */
  const void* fwd_comps;          /* nnz x comp_width bytes */
  const void* fwd_vals;           /* nnz binary16 bit patterns (F16) or nnz u8 codes (FIXEDU8, DOTVBYTE) */
  const uint64_t* list_block_start; /* dim + 1 */
  const uint64_t* block_post_start; /* n_blocks + 1 */
  const uint32_t* post_doc;       /* n_postings */
  const float* blk_min;           /* n_blocks */
  const float* blk_quant;         /* n_blocks */
  const uint64_t* list_row_start; /* dim + 1 */
  const void* row_comp;           /* n_rows x comp_width bytes */
  const uint64_t* row_ptr;        /* n_rows + 1 */
  const uint16_t* sum_bid;        /* n_entries */
  const uint8_t* sum_code;        /* n_entries */
  float val_scale;                /* FIXEDU8 / DOTVBYTE: value = code * val_scale (a power of two); 0 for F16 */
  uint32_t reserved;
} sgpu_index_desc;

/* Build-time configuration; mirrors Configuration (src/configurations.rs:15-129)
 * restricted to the path the Python API exposes (src/pylib/mod.rs:329-369):
 * GlobalThreshold pruning, RandomKmeansInvertedIndexApprox blocking,
 * EnergyPreserving summaries. Defaults = the reference's Python defaults. */
typedef struct sgpu_build_config {
  uint64_t n_postings;        /* 3500 */
  float centroid_fraction;    /* 0.1  */
  uint32_t min_cluster_size;  /* 2    */
  float summary_energy;       /* 0.4  */
  float max_fraction;         /* 1.5  */
  uint32_t doc_cut;           /* 15   */
  uint32_t num_threads;       /* 0 = all host cores */
  uint32_t use_device;        /* 0 = build on the host cores only; n > 0: the clustering (the k-means
                                 assignment of every posting, src/utils.rs:146-237) and the per-block
                                 summaries (src/posting_list.rs:329-368) run on HIP device n - 1. The
                                 index is byte-identical either way; a missing or failing device is an
                                 error, never a silent host build. */
  uint32_t reserved;
} sgpu_build_config;

/* Query-time knobs of InvertedIndexBase::search (src/inverted_index.rs:153-161). */
typedef struct sgpu_search_params {
  uint32_t k;            /* > 0 */
  uint32_t query_cut;    /* number of heaviest query components whose lists are walked */
  float heap_factor;     /* skip block iff heap full && dot < heap_factor * kth_best */
  uint32_t n_knn;        /* neighbours of each result to rescore (Knn::refine); needs a graph, else ignored */
  int32_t first_sorted;  /* !=0: first list visited by descending summary dot
                            (PostingList::sort_and_search, src/posting_list.rs:149-185) */
} sgpu_search_params;

typedef struct sgpu_index sgpu_index;     /* host + device state of one index */
typedef struct sgpu_batch sgpu_batch;     /* a device-resident query batch + result slab */

/* Per-launch measurements of the search kernel (HIP events on the library's stream). */
typedef struct sgpu_launch_stats {
  float kernel_ms;         /* duration of the last search kernel launch */
  uint32_t n_queries;
  uint32_t grid;           /* workgroups launched */
  uint32_t block;          /* threads per workgroup */
  uint32_t lds_bytes;      /* dynamic LDS per workgroup */
} sgpu_launch_stats;

/* ---- library ---------------------------------------------------------- */
/* Thread-local message for the last non-OK status returned on this thread. */
const char* sgpu_last_error(void);
/* ABI version of this header (bumped on any layout change). */
uint32_t sgpu_abi_version(void);
/* What this binary was built from: "sources <16 hex digits> arch gfx950 extra [<flags>] HIP version: ...". The hex
   digits are the first 64 bits of the SHA-256 of the library's source files in a fixed order (seismic_amd/csrc/Makefile,
   SOURCES); seismic_amd._native.source_fingerprint() recomputes them from a source tree. Static storage. */
const char* sgpu_build_info(void);
/* Number of visible HIP devices; SGPU_EDEVICE (and *n = 0) when none. */
sgpu_status sgpu_device_count(int32_t* n);

/* ---- index life cycle -------------------------------------------------- */
/* Replaces: holding an InvertedIndexBase<S> (src/inverted_index.rs:39-52).
 * Validates the descriptor, copies it, derives the HBM layout. */
sgpu_status sgpu_index_create(const sgpu_index_desc* desc, sgpu_index** out);
/* Replaces: InvertedIndexBase::build (src/inverted_index.rs:603-686) for the
 * Python-exposed configuration. Offline; on the host cores, or with cfg->use_device the clustering and
 * the block summaries on a HIP device (same index, byte for byte). Input = a sparse dataset in
 * CSR form, values already f32 (they are rounded to binary16 as
 * from_f32_saturating does, src/json_utils.rs:64). comps are comp_width bytes each. */
sgpu_status sgpu_index_build(uint32_t comp_width, uint64_t n_docs, uint64_t dim,
                             const uint64_t* offsets, const void* comps,
                             const float* vals, const sgpu_build_config* cfg,
                             sgpu_index** out);
/* Replaces: InvertedIndexBase::convert_dataset_into (call sites src/pylib/dotvbyte.rs:208-213,
 * src/bin/build_inverted_index.rs:294-306): a new index with the same posting lists, blocks and
 * summaries whose forward index stores the documents with another value type (F16 -> FIXEDU8 is what
 * SeismicIndexDotVByte.build does after building the standard index). *out is independent of src. */
sgpu_status sgpu_index_convert(const sgpu_index* src, uint32_t value_type, sgpu_index** out);
/* View of the index's canonical host arrays; valid until sgpu_index_destroy. */
sgpu_status sgpu_index_get_desc(const sgpu_index* idx, sgpu_index_desc* out);
/* Replaces: IndexSerializer::save_index / load_index (src/pylib/mod.rs:186-221).
 * Own flat SoA file format (the reference's wire format lives in un-vendored vectorium). */
sgpu_status sgpu_index_save(const sgpu_index* idx, const char* path);
sgpu_status sgpu_index_load(const char* path, sgpu_index** out);
/* Copies the index into the HBM of HIP device `device` (replaces any earlier upload). */
sgpu_status sgpu_index_upload(sgpu_index* idx, int32_t device);
/* Replicates the index on n devices of this process (index replicated, queries
 * sharded, no collective). Replica 0 is uploaded from the host; the others are copied from it GPU to
 * GPU (hipMemcpyPeer: xGMI on an MI355X node). With more than one replica, sgpu_batch_search shards a
 * batch contiguously over them, one host thread per device, and returns the rows in input order -
 * what the reference's rayon loop over queries does on host cores (src/pylib/mod.rs:629-652, 1129-1145).
 * Calls with fewer than two queries per replica (sgpu_search) are not cut: the replicas take them in turn.
 * A device id may be listed more than once (replicas sharing a device; used to test the path on a
 * single-GPU box). Replaces any earlier upload. */
sgpu_status sgpu_index_upload_many(sgpu_index* idx, const int32_t* device_ids, uint32_t n);
/* Number of device replicas (0 before upload). */
uint32_t sgpu_index_replicas(const sgpu_index* idx);
/* kNN graph — replaces Knn::new / Knn::refine (src/inverted_index.rs:448-500, 551-593).
 * build: every document is searched as a query (k = nknn+1, query_cut 10, heap_factor 0.7) as
 * batches through the GPU kernel; needs an uploaded index. set/get: attach or read the flattened
 * neighbour lists (document d's neighbours at [d*knn_dim, (d+1)*knn_dim)). With a graph attached,
 * sgpu_search_params.n_knn > 0 rescans the first n_knn neighbours of every top-k document after
 * the posting lists; without one n_knn is ignored, as in the reference (src/inverted_index.rs:215-216). */
sgpu_status sgpu_index_build_knn(sgpu_index* idx, uint32_t nknn);
sgpu_status sgpu_index_set_knn(sgpu_index* idx, const uint32_t* neighbours, uint64_t n_total, uint32_t knn_dim);
sgpu_status sgpu_index_get_knn(const sgpu_index* idx, const uint32_t** neighbours, uint64_t* n_total,
                               uint32_t* knn_dim);
/* Bytes resident in HBM after upload (0 before), plus the device copies of document columns on all replicas. */
uint64_t sgpu_index_device_bytes(const sgpu_index* idx);
/* A DotVByte index (SGPU_VAL_DOTVBYTE; reference src/pylib/dotvbyte.rs:15-22) keeps a document whose component gaps do
 * not fit the packed stream's fields in the raw form (2 bytes per component instead of 1.5): how many documents and
 * how many of their elements that is (0, 0 for the other value types). bench.py charges those elements their stored
 * bytes in the algorithmic-byte count. */
sgpu_status sgpu_index_stream_stats(const sgpu_index* idx, uint64_t* raw_docs, uint64_t* raw_elements);
void sgpu_index_destroy(sgpu_index* idx);

/* ---- search ------------------------------------------------------------ */
/* Replaces: InvertedIndexBase::search (src/inverted_index.rs:153-234) /
 * SeismicIndexRaw.search (src/pylib/mod.rs:1046-1076).
 * comps ascending, strictly increasing, < dim (u32 regardless of comp_width).
 * out_scores/out_doc_ids have room for params->k entries. */
sgpu_status sgpu_search(sgpu_index* idx, const uint32_t* comps, const float* vals,
                        uint32_t nnz, const sgpu_search_params* params,
                        float* out_scores, uint64_t* out_doc_ids, uint32_t* out_n);
/* Replaces: SeismicIndexRaw.batch_search (src/pylib/mod.rs:1111-1146) and the
 * per-query loop of SeismicIndex.batch_search (src/pylib/mod.rs:629-652).
 * Queries in CSR form: query q = [q_off[q], q_off[q+1]). Results in input
 * order: out_scores/out_doc_ids are nq x k (slots of row q past out_n[q] are written as zero).
 * Thread safety: sgpu_search / sgpu_batch_search may be called from any number of host threads on one
 * index (the reference's search takes &self and the index is Sync, src/index_traits.rs:106-113). Each
 * call borrows one of a small pool of (stream, recycled device batch) lanes of the replica it runs on,
 * so concurrent calls overlap on the device; a call allocates nothing once its lane's batch has grown
 * to the call's size. Query-time semantics that differ from a panic in the reference: query_cut == 0
 * walks no list and returns no result (k_largest_by(0), src/inverted_index.rs:187-190); any
 * heap_factor is accepted, negative ones included (the skip test is evaluated exactly as
 * src/posting_list.rs:130 does). */
sgpu_status sgpu_batch_search(sgpu_index* idx, const uint64_t* q_off,
                              const uint32_t* comps, const float* vals, uint32_t nq,
                              const sgpu_search_params* params, float* out_scores,
                              uint64_t* out_doc_ids, uint32_t* out_n);

/* Replaces: the sequential AQT loop of perf_inverted_index (src/bin/perf_inverted_index.rs:184-216), the
 * loop behind the reference's published per-query latency: the nq queries of a CSR set are searched ONE
 * AT A TIME, each through sgpu_search (host buffers in, results out, the call returns before the next
 * one starts). *mean_us (may be NULL) = wall time of the loop / nq. breakdown_us (may be NULL) receives 8
 * doubles, the mean microseconds per query the calling thread spent in each host-side phase:
 *   [0] validation + launch plan  [1] staging into the pinned arena  [2] enqueue H2D
 *   [3] launch configuration + kernel launch  [4] enqueue D2H  [5] waiting for the stream (the kernel
 *   runs here)  [6] copying the rows out  [7] reserved. */
sgpu_status sgpu_search_sequential(sgpu_index* idx, const uint64_t* q_off, const uint32_t* comps,
                                   const float* vals, uint32_t nq, const sgpu_search_params* params,
                                   float* out_scores, uint64_t* out_doc_ids, uint32_t* out_n,
                                   double* mean_us, double* breakdown_us);
/* Same loop; per_query_us (may be NULL) additionally receives the wall time of every call, nq doubles - the
 * distribution (p50 / p95 / p99 / max) behind the mean that perf_inverted_index reports
 * (src/bin/perf_inverted_index.rs:184-216 times the whole loop only). */
sgpu_status sgpu_search_sequential_timed(sgpu_index* idx, const uint64_t* q_off, const uint32_t* comps,
                                         const float* vals, uint32_t nq, const sgpu_search_params* params,
                                         float* out_scores, uint64_t* out_doc_ids, uint32_t* out_n,
                                         double* mean_us, double* breakdown_us, double* per_query_us);

/* Device-resident variant (what bench.py times: inputs already in HBM when the
 * timed region starts; results stay in HBM until fetched). */
sgpu_status sgpu_batch_create(sgpu_index* idx, const uint64_t* q_off,
                              const uint32_t* comps, const float* vals, uint32_t nq,
                              uint32_t k_max, sgpu_batch** out);
/* Same, on replica `replica` of an index uploaded with sgpu_index_upload_many (run / fetch / stats
 * find the replica from the batch). */
sgpu_status sgpu_batch_create_on(sgpu_index* idx, uint32_t replica, const uint64_t* q_off,
                                 const uint32_t* comps, const float* vals, uint32_t nq,
                                 uint32_t k_max, sgpu_batch** out);
/* Enqueues one search pass over the batch on the library's stream. With
 * sync != 0 waits for it and fills *stats (may be NULL). */
sgpu_status sgpu_batch_run(sgpu_index* idx, sgpu_batch* batch,
                           const sgpu_search_params* params, int32_t sync,
                           sgpu_launch_stats* stats);
/* Same search, synchronous, but with the reference's visited set materialised as a bitmap in HBM
 * instead of the (exactly equivalent, cheaper) heap-membership test: results are identical, and
 * work counters [5],[6] of sgpu_batch_fetch_stats then exclude re-encountered documents exactly
 * as the reference's FxHashSet does (src/inverted_index.rs:181-184). Used for accounting. */
sgpu_status sgpu_batch_run_counted(sgpu_index* idx, sgpu_batch* batch,
                                   const sgpu_search_params* params, sgpu_launch_stats* stats);
/* Blocks until all enqueued passes (of every replica) are done; *stats (may be NULL) gets the MEAN
 * kernel duration of replica 0's passes enqueued since the previous sync. */
sgpu_status sgpu_batch_sync(sgpu_index* idx, sgpu_launch_stats* stats);
sgpu_status sgpu_batch_fetch(sgpu_index* idx, sgpu_batch* batch, uint32_t k,
                             float* out_scores, uint64_t* out_doc_ids, uint32_t* out_n);
/* Work counters of the batch's LAST pass (every pass starts them from zero), nq x 24 uint32, row q for query q alone:
 *   [0] blocks of the walked lists   [1] summary rows matched   [2] summary entries read
 *   [3] blocks that passed the skip test   [4] postings of those blocks
 *   [5] documents scored (as the reference would; exact after sgpu_batch_run_counted, otherwise
 *       re-encountered documents are included)   [6] sum of their component counts
 *   [7] documents the kernel scored speculatively (>= [5]; the surplus is overhead)
 *   With a kNN graph and n_knn > 0 the neighbours the refine step scores are documents scored: they count in [5], [6]
 *   and [7]. They are no postings of a block: [3] and [4] are those of the posting lists only.
 *   [8..19] kernel phase clocks (shader cycles / 16; zero unless the library was built with
 *           -DSGPU_PROF, `make prof`), [20] workgroup slot, [21..23] reserved
 * Counters [3..6] are exact only after sgpu_batch_run_counted (the default pass skips replay windows
 * that cannot change the heap and does not track re-encountered documents).
 * Counters [0..6] are what the ALGORITHM touches and feed the roofline accounting. */
sgpu_status sgpu_batch_fetch_stats(sgpu_index* idx, sgpu_batch* batch, uint32_t* out_counters);
void sgpu_batch_destroy(sgpu_batch* batch);

/* Hot loop A in isolation — replaces QuantizedSummary::distances
 * (src/quantized_summary.rs:64-160) for posting list `list`: writes one f32
 * per block of that list (out_dots has room for n_blocks(list) entries). */
sgpu_status sgpu_summary_distances(sgpu_index* idx, uint32_t list, const uint32_t* comps,
                                   const float* vals, uint32_t nnz, float* out_dots,
                                   uint32_t* out_n_blocks);

/* ---- host-side helpers around the path (CPU, not on the hot path) ------ */
/* Replaces: SeismicDataset.search (exact, vectorium FlatIndex;
 * src/inverted_index_wrapper.rs:721-742) — ground truth for recall@k.
 * Brute force over the forward index of `idx`, multi-threaded on the host. */
sgpu_status sgpu_exact_search(const sgpu_index* idx, const uint64_t* q_off,
                              const uint32_t* comps, const float* vals, uint32_t nq,
                              uint32_t k, uint32_t num_threads, float* out_scores,
                              uint64_t* out_doc_ids, uint32_t* out_n);
/* The same exact search on the device of replica `replica` of an uploaded index: for every query exactly
 * what sgpu_exact_search returns (out_n, ids and their order, score bits). Scores that are not finite
 * (NaN, or inf from inf query values) may be ordered differently. Host buffers in and out, nq x k
 * row-major; slots past out_n[q] are written as zero. Checks, in this order: the queries (SGPU_EINVAL),
 * k == 0 (SGPU_EINVAL), k > 1024 (SGPU_ELIMIT), index not uploaded or replica out of range
 * (SGPU_EDEVICE), device memory (SGPU_ENOMEM; the index stays usable for search).
 * The first call on a replica builds there an "exact file" of the forward index, kept until
 * sgpu_index_destroy (or a new upload) and not counted by sgpu_index_device_bytes:
 * 4 bytes per stored component plus 4 x ceil(n_docs / 32768) x (dim + 1) bytes of offsets
 * (about 4.2 GB for 8.8M documents of 117 components over a 30K vocabulary). Safe to call while other
 * threads search the same replica: the call has a stream of its own; exact calls on one replica take
 * turns. */
sgpu_status sgpu_exact_search_device(sgpu_index* idx, uint32_t replica, const uint64_t* q_off,
                                     const uint32_t* comps, const float* vals, uint32_t nq, uint32_t k,
                                     float* out_scores, uint64_t* out_doc_ids, uint32_t* out_n);
/* ---- document filters ----------------------------------------------------
 * Restrict a search to a set A of allowed document ids (one tenant's documents, a date range, what a caller may see).
 * No reference counterpart. Contract: filtered search of index I with A returns exactly what unfiltered search returns
 * on I_A, the index I with every posting of a document outside A deleted from its block (blocks that become empty are
 * kept; with a kNN graph, every neighbour outside A replaced by 0xffffffff, which the refine step skips) and nothing
 * else changed - block order, summaries, forward index, knn_dim. Same out_n, ids in the same order, same score bits,
 * for every parameter, value type and launch shape. The summaries still bound the remaining documents from above, so
 * pruning stays sound; as with any approximate search, out_n may be below k even when |A| >= k.
 * Filtered exact search returns the k best documents of A (out_n = min(k, |A|)), host and device bit-identical.
 *
 * A filter belongs to the index it was created on: passing it with another index is SGPU_EINVAL. A NULL filter makes
 * each filtered call exactly its unfiltered counterpart; otherwise, after the check of the filter's index, the
 * unfiltered call's checks run in their order. Destroy every filter before its index.
 * On first use on a replica a filter builds there (on the device) its view: its bitmap, the compacted
 * block_post_start (n_blocks + 1 u32), post_ref (8 B) and post_doc (4 B) of the allowed postings and, with a graph, a
 * masked copy of it (4 B per entry); sgpu_filter_device_bytes counts them. sgpu_index_upload, sgpu_index_upload_many,
 * sgpu_index_set_knn and sgpu_index_build_knn invalidate the views: they are rebuilt on their next use. Filtered and
 * unfiltered calls may run concurrently on one replica; one filter may serve any number of concurrent calls. */
typedef struct sgpu_filter sgpu_filter;
/* A = the n ids of doc_ids (repeats allowed; n == 0: the empty set). An id >= n_docs is SGPU_EINVAL (the message
 * names the first one). Needs no device: works on an index that is not uploaded (host exact search). */
sgpu_status sgpu_filter_create(sgpu_index* idx, const uint32_t* doc_ids, uint64_t n, sgpu_filter** out);
/* |A| (0 for NULL). */
uint64_t sgpu_filter_count(const sgpu_filter* filter);
/* HBM held by the filter's views on all replicas (0 before its first device use). */
uint64_t sgpu_filter_device_bytes(const sgpu_filter* filter);
void sgpu_filter_destroy(sgpu_filter* filter);
/* sgpu_search / sgpu_batch_search restricted to the filter's documents (replicas shard a batch as without one). */
sgpu_status sgpu_search_filtered(sgpu_index* idx, const uint32_t* comps, const float* vals, uint32_t nnz,
                                 const sgpu_search_params* params, float* out_scores, uint64_t* out_doc_ids,
                                 uint32_t* out_n, const sgpu_filter* filter);
sgpu_status sgpu_batch_search_filtered(sgpu_index* idx, const uint64_t* q_off, const uint32_t* comps, const float* vals,
                                       uint32_t nq, const sgpu_search_params* params, float* out_scores,
                                       uint64_t* out_doc_ids, uint32_t* out_n, const sgpu_filter* filter);
/* sgpu_exact_search / sgpu_exact_search_device over the filter's documents only. */
sgpu_status sgpu_exact_search_filtered(const sgpu_index* idx, const uint64_t* q_off, const uint32_t* comps,
                                       const float* vals, uint32_t nq, uint32_t k, uint32_t num_threads,
                                       float* out_scores, uint64_t* out_doc_ids, uint32_t* out_n,
                                       const sgpu_filter* filter);
sgpu_status sgpu_exact_search_device_filtered(sgpu_index* idx, uint32_t replica, const uint64_t* q_off,
                                              const uint32_t* comps, const float* vals, uint32_t nq, uint32_t k,
                                              float* out_scores, uint64_t* out_doc_ids, uint32_t* out_n,
                                              const sgpu_filter* filter);

/* ---- term filters: a filter from must / must-not / should clauses -------------
 * The `bool` query of a lexical engine over the index's own vocabulary (an index component is a token; tags, languages
 * and tenants are often encoded as components too). No reference counterpart. The clauses are evaluated against the
 * forward index - every stored component of every document - not against the pruned posting lists.
 * A clause MATCHES document d iff d stores `component` and its stored value, decoded to f32 (binary16 -> f32; u8 code
 * * val_scale, the product rounded once), is >= min_weight; min_weight = -INFINITY: any stored entry matches.
 * The set: A = { d < n_docs : every MUST clause matches d, no MUST_NOT clause matches d, and the number of SHOULD
 * clauses that match d is >= min_should }, intersected with `within`'s set when `within` is not NULL.
 *  - With no MUST clause and min_should == 0, A is every document except the MUST_NOT matches; documents that store
 *    no component are in it.
 *  - n_clauses == 0 gives all documents (of `within`).
 *  - min_should above the number of SHOULD clauses gives the empty set; it is not an error.
 *  - One component may appear in several clauses; SHOULD clauses are counted per clause, so two SHOULD clauses on one
 *    component with different thresholds count on their own.
 *  - The comparison is the IEEE >= on f32: a stored -0.0 matches min_weight = +0.0.
 *  - A DotVByte index answers as its fixed-u8 twin does.
 * The result is an ordinary sgpu_filter of `idx`: sgpu_filter_count is the number of matching documents, every
 * filtered call takes it, and it stays valid across uploads (it depends on the forward index only).
 * Checks, in this order: (1) NULL idx or out, or NULL clauses with n_clauses > 0: SGPU_EINVAL; (2) an occur outside
 * 0..2, a component >= dim or a NaN min_weight: SGPU_EINVAL, the message names the first offending clause;
 * (3) n_clauses > 1024: SGPU_ELIMIT; (4) a `within` of another index: SGPU_EINVAL; (5, device call only) index not
 * uploaded or replica out of range: SGPU_EDEVICE; the exact file's own limits: SGPU_ELIMIT, as
 * sgpu_exact_search_device reports them; device memory: SGPU_ENOMEM, and the index stays usable.
 * sgpu_filter_create_terms_host needs no upload, scans the host forward arrays with num_threads threads (0 = all) and
 * DEFINES the bits; sgpu_filter_create_terms returns the same words, computed on the device of `replica` from its
 * exact file (see sgpu_exact_search_device: the first call on a replica builds the file if no exact call has), and
 * copies them (n_docs / 8 bytes) to the host. The device call runs on the exact file's stream under its mutex:
 * term-filter calls and exact calls on one replica take turns; searches run beside them. */
enum { SGPU_TERM_MUST = 0, SGPU_TERM_MUST_NOT = 1, SGPU_TERM_SHOULD = 2 };
typedef struct sgpu_term_clause {
  uint32_t component; /* < dim */
  uint32_t occur;     /* SGPU_TERM_* */
  float min_weight;   /* the clause matches d iff d stores the component with a decoded value >= min_weight */
  uint32_t reserved;  /* 0 */
} sgpu_term_clause;
sgpu_status sgpu_filter_create_terms(sgpu_index* idx, uint32_t replica, const sgpu_term_clause* clauses,
                                     uint32_t n_clauses, uint32_t min_should, const sgpu_filter* within,
                                     sgpu_filter** out);
sgpu_status sgpu_filter_create_terms_host(sgpu_index* idx, const sgpu_term_clause* clauses, uint32_t n_clauses,
                                          uint32_t min_should, const sgpu_filter* within, uint32_t num_threads,
                                          sgpu_filter** out);
/* The allowed set of any filter as ceil(n_docs / 32) words (at least one), bit d of word d / 32, bits past n_docs
 * zero. *n_words (may be NULL) is set to the number of words; cap_words below it is SGPU_EINVAL (nothing written). */
sgpu_status sgpu_filter_get_bits(const sgpu_filter* filter, uint32_t* out_words, uint64_t cap_words, uint64_t* n_words);

/* ---- document columns: range and set filters, facet counts --------------------
 * Up to SGPU_MAX_COLUMNS per-document attributes of 32 bits each (a tenant, a category, a timestamp, a price), held with
 * the index on the host and, once a device call needs them, on the device. No reference counterpart.
 * sgpu_index_set_column: `values` holds one 32-bit value per document, in the index's document order; n must equal
 * n_docs (SGPU_EINVAL otherwise). values == NULL with n == 0 drops the column. slot >= SGPU_MAX_COLUMNS or an unknown
 * type is SGPU_EINVAL. The library copies the values; setting a slot again replaces the column, and its type may
 * change. For a U32 column the largest value is recorded while it is copied (sgpu_facet_counts checks it). Needs no
 * upload. Filters made earlier are bitmaps and stay valid.
 * sgpu_index_get_column: a view of the host copy, valid until the next sgpu_index_set_column of that slot or
 * sgpu_index_destroy; an empty slot gives *n = 0 and *values = NULL and is not an error (*type is then 0).
 * A replica's copy of a column is made by the first device call that needs it there, and made again after
 * sgpu_index_set_column replaced the column or sgpu_index_upload[_many] replaced the replica; dropping a column frees
 * its copies. sgpu_index_device_bytes counts the copies of all replicas.
 * Columns are NOT part of the index file: sgpu_index_save does not write them, sgpu_index_load returns an index
 * without columns, and sgpu_index_convert does not carry them over. The file format is unchanged.
 * sgpu_index_set_column waits for the column calls running on every replica (it takes their mutex) before it frees or
 * replaces anything; like sgpu_index_set_knn it must not run beside a HOST call that reads the same column. */
enum { SGPU_COL_U32 = 0, SGPU_COL_I32 = 1, SGPU_COL_F32 = 2 };
#define SGPU_MAX_COLUMNS 16
sgpu_status sgpu_index_set_column(sgpu_index* idx, uint32_t slot, uint32_t type, const void* values, uint64_t n);
sgpu_status sgpu_index_get_column(const sgpu_index* idx, uint32_t slot, uint32_t* type, const void** values, uint64_t* n);

/* Column filter: the must / must-not / should shape of the term filter over column predicates.
 * A RANGE clause MATCHES document d iff lo <= v[d] && v[d] <= hi, in the order of the column's type: unsigned for U32,
 * two's complement for I32, the IEEE comparison of f32 for F32 (lo_bits / hi_bits are the bounds' bit patterns in that
 * type). An IN clause matches iff v[d] equals one of set_values[set_begin .. set_begin + set_count) under the same
 * comparison; the values need not be sorted or distinct, clauses may share them, and set_count == 0 matches nothing.
 *  - F32: a stored NaN matches no RANGE and no IN clause; -0.0 equals +0.0; +-INFINITY are valid bounds.
 *  - lo > hi gives a clause that matches nothing; it is not an error.
 * The set: A = { d < n_docs : every MUST clause matches d, no MUST_NOT clause matches d, and the number of SHOULD
 * clauses that match d is >= min_should }, intersected with `within`'s set when `within` is not NULL. The corner cases
 * are the term filter's: n_clauses == 0 gives all documents (of `within`); min_should above the number of SHOULD
 * clauses gives the empty set; SHOULD is counted per clause (two SHOULD clauses on one slot count on their own); with
 * no MUST clause and min_should == 0, A is the complement of the MUST_NOT matches.
 * The result is an ordinary sgpu_filter of `idx`: sgpu_filter_count is the number of matching documents, every filtered
 * call takes it, and it stays valid when the columns change later (it is a bitmap).
 * Checks, in this order: (1) NULL idx or out, NULL clauses with n_clauses > 0, NULL set_values with n_set_values > 0:
 * SGPU_EINVAL; (2) an occur outside 0..2, an op outside 0..1, a slot >= SGPU_MAX_COLUMNS or without a column, a NaN
 * bound (RANGE) or a NaN set value (IN) on an F32 column, set_begin + set_count > n_set_values (IN): SGPU_EINVAL, the
 * message names the first offending clause; (3) n_clauses > 64 or n_set_values > 8192: SGPU_ELIMIT; (4) a `within` of
 * another index: SGPU_EINVAL; (5, device call only) index not uploaded or replica out of range: SGPU_EDEVICE; device
 * memory: SGPU_ENOMEM, and the index stays usable.
 * sgpu_filter_create_columns_host needs no upload, scans the host columns with num_threads threads (0 = all) and
 * DEFINES the words; sgpu_filter_create_columns returns the same words, computed by one kernel on the device of
 * `replica` and copied (n_docs / 8 bytes) to the host. The column calls of a replica (this one and sgpu_facet_counts)
 * run on a stream of their own under one mutex: they take turns; searches and the other calls run beside them. */
enum { SGPU_COLOP_RANGE = 0, SGPU_COLOP_IN = 1 };
typedef struct sgpu_column_clause {
  uint32_t slot;      /* a set column */
  uint32_t occur;     /* SGPU_TERM_MUST / _MUST_NOT / _SHOULD */
  uint32_t op;        /* SGPU_COLOP_* */
  uint32_t lo_bits;   /* RANGE: lower bound, bit pattern of the column's type */
  uint32_t hi_bits;   /* RANGE: upper bound */
  uint32_t set_begin; /* IN: the clause's values are set_values[set_begin .. set_begin + set_count) */
  uint32_t set_count;
  uint32_t reserved;  /* 0 */
} sgpu_column_clause;
sgpu_status sgpu_filter_create_columns(sgpu_index* idx, uint32_t replica, const sgpu_column_clause* clauses,
                                       uint32_t n_clauses, uint32_t min_should, const uint32_t* set_values,
                                       uint32_t n_set_values, const sgpu_filter* within, sgpu_filter** out);
sgpu_status sgpu_filter_create_columns_host(sgpu_index* idx, const sgpu_column_clause* clauses, uint32_t n_clauses,
                                            uint32_t min_should, const uint32_t* set_values, uint32_t n_set_values,
                                            const sgpu_filter* within, uint32_t num_threads, sgpu_filter** out);

/* Facet counts: over the documents of `filter` (NULL: all documents), the t values of the U32 column `slot` held by
 * the most documents, by (count descending, value ascending). Only values with a non-zero count are listed.
 * *out_n = min(t, distinct); *out_distinct = the number of values with a non-zero count; *out_docs = the number of
 * documents counted (|filter|, or n_docs). out_values and out_counts have room for t entries; rows past *out_n are
 * written as zero.
 * Checks, in this order: (1) NULL idx or a NULL output, t outside 1..1024, slot >= SGPU_MAX_COLUMNS or empty, a column
 * that is not U32: SGPU_EINVAL; (2) a filter of another index: SGPU_EINVAL; (3) a column whose recorded maximum is
 * >= 1 << 22 = 4194304: SGPU_ELIMIT (the message names the limit); (4, device call only) index not uploaded or replica
 * out of range: SGPU_EDEVICE; device memory: SGPU_ENOMEM, and the index stays usable.
 * Counts are integers: the device result equals the host twin's exactly. sgpu_facet_counts_host needs no upload and
 * DEFINES the rows. The device call uploads the filter's host words for the call (n_docs / 8 bytes), counts in a
 * table of max + 1 u32 bins (at most 16 MiB, recycled) and selects on the device; it runs on the column calls' stream. */
sgpu_status sgpu_facet_counts(sgpu_index* idx, uint32_t replica, uint32_t slot, const sgpu_filter* filter, uint32_t t,
                              uint32_t* out_values, uint64_t* out_counts, uint32_t* out_n, uint64_t* out_distinct,
                              uint64_t* out_docs);
sgpu_status sgpu_facet_counts_host(const sgpu_index* idx, uint32_t slot, const sgpu_filter* filter, uint32_t t,
                                   uint32_t num_threads, uint32_t* out_values, uint64_t* out_counts, uint32_t* out_n,
                                   uint64_t* out_distinct, uint64_t* out_docs);

/* ---- column aggregations: statistics, histograms, sorted top-k ----------------
 * Three summaries of the column `slot` (any type) over the documents of `filter` (NULL: all documents), each as a
 * device call and a host twin that needs no upload, scans the host column with num_threads threads (0 = all) and
 * DEFINES the result; the device call returns the same bits. Every comparison is made on one unsigned key per type
 * (U32: the value; I32: the sign bit flipped; F32: the IEEE order of the numbers with -0.0 equal to +0.0), so the two
 * cannot disagree on one. A stored F32 NaN is not a value: it is counted apart and never ordered. Like the columns,
 * the results are NOT part of the index file. The device calls run on the column calls' stream under its mutex, read
 * the column as it is once they hold the mutex, and upload the filter's host words for the call (n_docs / 8 bytes).
 *
 * sgpu_column_stats[_host]: docs = |filter| (n_docs for NULL); valid = docs minus the NaNs of an F32 column; min_bits /
 * max_bits = the smallest / largest value as a bit pattern of the column's type (an f32 zero is reported as +0.0
 * whichever sign was stored; both 0 where valid == 0); sum_int = U32: the exact sum, I32: the exact i64 sum as two's
 * complement, F32: 0; sum = U32 / I32: sum_int converted once; F32: the binary64 sum in this canonical order. The
 * contribution of document d is x[d] = (double)v[d] where d is in the filter and v[d] is not NaN, +0.0 otherwise.
 *   1. documents are taken in tiles of 16384 consecutive ids;
 *   2. in tile t, 256 lane sums c[j], j = 0..255, start at +0.0 and add x[t * 16384 + r * 256 + j] for r = 0..63
 *      ascending (ids at or past n_docs contribute +0.0);
 *   3. c[j] += c[j + h] for j < h, with h = 128, 64, ..., 1; c[0] is the tile's sum;
 *   4. the tile sums are added in ascending tile order, starting at +0.0.
 * Binary64 adds, never contracted or reordered. A NaN result (both infinities among the values) is written as
 * 0x7ff8000000000000.
 * Checks, in this order: (1) NULL idx or out, slot >= SGPU_MAX_COLUMNS or empty: SGPU_EINVAL; (2) a filter of another
 * index: SGPU_EINVAL; (3, device call only) index not uploaded or replica out of range: SGPU_EDEVICE; device memory:
 * SGPU_ENOMEM, and the index stays usable.
 *
 * sgpu_column_histogram[_host]: `edges` holds n_edges bit patterns of the column's type whose values ascend strictly
 * (n_edges - 1 buckets, at most 4096). numpy.histogram's reading: bucket b counts the documents with
 * edges[b] <= v < edges[b + 1], and the last bucket also takes v == edges[n_edges - 1]. *out_below counts
 * v < edges[0], *out_above v > edges[n_edges - 1], *out_nan the NaNs of an F32 column, *out_docs the documents looked
 * at: sum(out_counts) + below + above + nan == docs always. out_counts has room for n_edges - 1 entries.
 * Checks, in this order: (1) NULL idx, edges or output, slot >= SGPU_MAX_COLUMNS or empty: SGPU_EINVAL; (2) n_edges
 * outside 2..4097: SGPU_ELIMIT; (3) an edge that is NaN (F32) or not above the edge before it in the type's order (the
 * pair -0.0, +0.0 is equal): SGPU_EINVAL, the message names the first offending edge; (4) a filter of another index:
 * SGPU_EINVAL; (5, device call only) as above.
 *
 * sgpu_column_top[_host]: the filter's documents ordered by the column. Rows are the first min(t, valid) documents by
 * (value ascending for order == 0, descending for order == 1; document id ascending among equal values - -0.0 and
 * +0.0 are equal). NaN documents never appear. out_doc_ids (native document ids, as sgpu_filter_create takes them)
 * and out_value_bits (the stored bit patterns) have room for t entries; rows past *out_n are written as zero.
 * *out_valid and *out_docs are those of the stats.
 * Checks, in this order: (1) NULL idx or a NULL output, t outside 1..1024, order outside 0..1, slot >=
 * SGPU_MAX_COLUMNS or empty: SGPU_EINVAL; (2) a filter of another index: SGPU_EINVAL; (3, device call only) as above. */
struct sgpu_column_stats { /* (a tag only: the call of the same name stands beside it) */
  uint64_t docs;
  uint64_t valid;
  uint32_t min_bits;
  uint32_t max_bits;
  uint64_t sum_int;
  double sum;
};
sgpu_status sgpu_column_stats(sgpu_index* idx, uint32_t replica, uint32_t slot, const sgpu_filter* filter,
                              struct sgpu_column_stats* out);
sgpu_status sgpu_column_stats_host(const sgpu_index* idx, uint32_t slot, const sgpu_filter* filter, uint32_t num_threads,
                                   struct sgpu_column_stats* out);
sgpu_status sgpu_column_histogram(sgpu_index* idx, uint32_t replica, uint32_t slot, const sgpu_filter* filter,
                                  const uint32_t* edges, uint32_t n_edges, uint64_t* out_counts, uint64_t* out_below,
                                  uint64_t* out_above, uint64_t* out_nan, uint64_t* out_docs);
sgpu_status sgpu_column_histogram_host(const sgpu_index* idx, uint32_t slot, const sgpu_filter* filter,
                                       const uint32_t* edges, uint32_t n_edges, uint32_t num_threads,
                                       uint64_t* out_counts, uint64_t* out_below, uint64_t* out_above, uint64_t* out_nan,
                                       uint64_t* out_docs);
sgpu_status sgpu_column_top(sgpu_index* idx, uint32_t replica, uint32_t slot, const sgpu_filter* filter, uint32_t t,
                            uint32_t order, uint32_t* out_doc_ids, uint32_t* out_value_bits, uint32_t* out_n,
                            uint64_t* out_valid, uint64_t* out_docs);
sgpu_status sgpu_column_top_host(const sgpu_index* idx, uint32_t slot, const sgpu_filter* filter, uint32_t t,
                                 uint32_t order, uint32_t num_threads, uint32_t* out_doc_ids, uint32_t* out_value_bits,
                                 uint32_t* out_n, uint64_t* out_valid, uint64_t* out_docs);

/* ---- scores of caller-given documents ----------------------------------------
 * "What does THIS document score for THIS query?": reranking the candidates of another retriever, fusing candidate
 * lists, explaining a hit, re-checking a stored result. The reference has no by-id entry point; its nearest item is
 * QueryEvaluator::compute_distance at its call site src/posting_list.rs:210-211, the score its search computes for
 * a document of a posting list.
 * Query q = [q_off[q], q_off[q+1]) as in sgpu_batch_search; its candidates are
 * cand_ids[cand_off[q] .. cand_off[q+1]) (native document ids, any order, repeats allowed, possibly none).
 * out_scores[i] is the score of cand_ids[i] for its query: one float per candidate, cand_off[nq] in all.
 * A score is, bit for bit, the score sgpu_search / sgpu_batch_search return for that document and query: the full query's
 * dot product over the document's stored values in the canonical order - 16 accumulators, element e of the document to
 * accumulator (e / 8) % 16 in increasing e, the partials combined by t[j] += t[j ^ s], s = 8, 4, 2, 1; f32 multiply then
 * add, never contracted; components the query does not carry, and query components of weight +-0, contribute nothing. A
 * document without components scores +0.0, as does every document for an empty query. Scores that are not finite (inf
 * query values) need not match. Every value type, component width and forward layout.
 * Checks, in this order: null arguments (SGPU_EINVAL; cand_ids and out_scores too, also when there is no candidate), the
 * queries (SGPU_EINVAL), cand_off[0] != 0 or cand_off decreasing (SGPU_EINVAL), a document id >= n_docs (SGPU_EINVAL; the
 * message names the first one and its query), a query of more than 8192 components (SGPU_ELIMIT), index not uploaded or
 * replica out of range (SGPU_EDEVICE), device memory (SGPU_ENOMEM; the index stays usable). nq == 0 or no candidate at
 * all is SGPU_OK.
 * Safe to call while other threads search the same replica: the call has a stream of its own; score calls on one replica
 * take turns. Its scratch on the device (the staged queries, ids and scores) is kept per replica and recycled, freed by
 * sgpu_index_destroy or a new upload, and not counted by sgpu_index_device_bytes; no index array is added. A call of more
 * candidates than a launch's budget (2^20; environment SGPU_SCORE_CHUNK overrides) runs as several launches. */
sgpu_status sgpu_score_documents(sgpu_index* idx, uint32_t replica,
    const uint64_t* q_off, const uint32_t* comps, const float* vals, uint32_t nq,
    const uint64_t* cand_off, const uint64_t* cand_ids, float* out_scores);
/* The same on the host cores (needs no upload), bit-identical; the same checks without the device ones.
 * num_threads == 0: all host cores (over the queries). */
sgpu_status sgpu_score_documents_host(const sgpu_index* idx,
    const uint64_t* q_off, const uint32_t* comps, const float* vals, uint32_t nq,
    const uint64_t* cand_off, const uint64_t* cand_ids, uint32_t num_threads, float* out_scores);

/* ---- rerank: the k best of each query's candidates ----------------------------
 * The second stage in one call: the candidates are scored as by sgpu_score_documents and the selection runs on the
 * device too, so only nq x k rows come back. Queries and candidates are given exactly as for sgpu_score_documents (any
 * order, repeats allowed, possibly none).
 * Row q of the nq x k row-major outputs holds the DISTINCT document ids among query q's candidates, ordered by score
 * descending, ties by document id ascending, cut to the first k; out_n[q] = min(k, distinct candidates of q). Slots past
 * out_n[q] are written as zero, as sgpu_batch_search does. A query without candidates gets out_n = 0 and a zeroed row.
 * Each returned score is, bit for bit, what sgpu_score_documents and sgpu_search return for that pair. A score is never
 * -0.0: every accumulator starts at +0.0 and is only added to, and x + y is -0.0 only if both are; so numeric order and
 * the order of the monotone integer image of the f32 bits agree on finite scores, and the device selects on that image.
 * The host twin places NaN scores after every number, by id ascending; device rows that contain a score that is not
 * finite need not match it (sgpu_score_documents makes the same reservation).
 * Checks, in this order: null arguments (SGPU_EINVAL; cand_ids, out_scores, out_doc_ids and out_n too, also when there is
 * nothing to do), everything sgpu_score_documents checks in its order, k == 0 (SGPU_EINVAL), k > 1024 (SGPU_ELIMIT), index
 * not uploaded or replica out of range (SGPU_EDEVICE), device memory (SGPU_ENOMEM; the index stays usable). nq == 0 is
 * SGPU_OK.
 * The call shares the score calls' per-replica stream and recycled scratch and takes turns with them; it is safe beside
 * searches, filtered and exact calls. It adds no index array; its scratch is freed by sgpu_index_destroy or a new upload.
 * A call of more candidates than a launch's budget (2^20; SGPU_SCORE_CHUNK overrides) runs as several launches, also
 * where the cut falls inside one query's candidates; the rows do not depend on where the cuts fall. */
sgpu_status sgpu_rerank_documents(sgpu_index* idx, uint32_t replica,
    const uint64_t* q_off, const uint32_t* comps, const float* vals, uint32_t nq,
    const uint64_t* cand_off, const uint64_t* cand_ids, uint32_t k,
    float* out_scores, uint64_t* out_doc_ids, uint32_t* out_n);
/* The same on the host cores (needs no upload): the same rows, bit for bit, wherever every score is finite; the same
 * checks without the device ones. num_threads == 0: all host cores (over the queries). */
sgpu_status sgpu_rerank_documents_host(const sgpu_index* idx,
    const uint64_t* q_off, const uint32_t* comps, const float* vals, uint32_t nq,
    const uint64_t* cand_off, const uint64_t* cand_ids, uint32_t k, uint32_t num_threads,
    float* out_scores, uint64_t* out_doc_ids, uint32_t* out_n);

/* ---- explain: the terms behind a document's score -----------------------------
 * A score is a sum of products over the vocabulary terms query and document share; this call returns, beside each
 * candidate's score, the m largest of those products with their components and both weights. Queries and candidates
 * are given exactly as for sgpu_score_documents (any order, repeats allowed, possibly none); candidate i is cand_ids[i]
 * with its query, rows are numbered like the candidates (cand_off[nq] in all).
 * Term: a stored element e < len(d) of the document whose component c the query carries with a weight w that is not
 * +-0. Padding elements of a record are never terms; a stored value of 0 still makes a term.
 * Product of a term: the f32 the score adds for that element, bit for bit - F16: fl(w * f32(value)); FIXEDU8 and
 * DOTVBYTE: fl(fl(w * val_scale) * (float)code), where the inner product is exact because val_scale is a power of two
 * (a w so small that fl(w * val_scale) underflows is outside this contract: a w whose scaled weight is +-0 counts as +-0).
 * out_scores[i]    the bits sgpu_score_documents returns for the pair (the canonical order above): the call takes the
 *                  score call's place when terms are wanted.
 * out_n_terms[i]   all terms of the pair, however many are returned.
 * Row i of the cand_off[nq] x m row-major out_comps, out_q_vals, out_d_vals, out_products holds the first
 * min(m, out_n_terms[i]) terms in this order: ordered(product bits) descending, then component ascending, where
 * ordered(b) is the monotone integer image of f32 bits (all bits of a negative flipped, the sign bit of the others
 * set): the numeric order on finite products with -0.0 below +0.0. A document's components are distinct, so the order
 * is total. Per term: the component, w as the caller gave it, the stored value as an f32 (binary16 widened, or
 * code * val_scale; both exact) and the product. Slots past the filled ones are zero in all four arrays.
 * Where m >= out_n_terms[i] the returned products, added at their elements' places in the canonical order, give
 * out_scores[i]. Pairs with a score or product that is not finite (inf query values) need not match the host twin.
 * Checks, in this order: null arguments (SGPU_EINVAL; every output pointer too, also when there is no candidate),
 * everything sgpu_score_documents checks in its order, m == 0 (SGPU_EINVAL), m > 32 (SGPU_ELIMIT), index not uploaded or
 * replica out of range (SGPU_EDEVICE), device memory (SGPU_ENOMEM; the index stays usable). nq == 0 or no candidate at
 * all is SGPU_OK.
 * The call shares the score calls' per-replica stream, mutex and recycled scratch and takes turns with them; it is safe
 * beside searches. It adds no index array. SGPU_SCORE_CHUNK cuts it into launches as it cuts the score call (without it
 * a launch takes as many candidates as 64 MiB of term rows hold, at most 2^20); the outputs do not depend on the cuts. */
sgpu_status sgpu_explain_documents(sgpu_index* idx, uint32_t replica,
    const uint64_t* q_off, const uint32_t* comps, const float* vals, uint32_t nq,
    const uint64_t* cand_off, const uint64_t* cand_ids, uint32_t m,
    float* out_scores, uint32_t* out_n_terms,
    uint32_t* out_comps, float* out_q_vals, float* out_d_vals, float* out_products);
/* The same on the host cores (needs no upload), bit-identical wherever scores and products are finite; the same checks
 * without the device ones. num_threads == 0: all host cores (over the queries). */
sgpu_status sgpu_explain_documents_host(const sgpu_index* idx,
    const uint64_t* q_off, const uint32_t* comps, const float* vals, uint32_t nq,
    const uint64_t* cand_off, const uint64_t* cand_ids, uint32_t m, uint32_t num_threads,
    float* out_scores, uint32_t* out_n_terms,
    uint32_t* out_comps, float* out_q_vals, float* out_d_vals, float* out_products);

/* ---- expand: Rocchio feedback queries ------------------------------------------
 * Pseudo-relevance feedback in one call: fold the vectors of a query's feedback documents (usually the best of a first
 * search) into the query, keep the heaviest terms, search again with the row that comes back. The reference has no
 * counterpart. Queries and candidates are given exactly as for sgpu_score_documents (any order, repeats allowed, possibly
 * none); cand_w[i] is the weight of feedback document cand_ids[i] - the caller forms beta / |R|, or a weight that depends
 * on the score; weights may be negative.
 * The table. For query q define the dense f32 vector W over the vocabulary: W starts at +0.0 everywhere. For each query
 * element (c, w), in the order given, W[c] = fl(alpha * w) (set, not added). Then for each candidate i of q IN THE ORDER
 * GIVEN, for each stored element e < len(d) of its document d with component c: W[c] = fl(W[c] + p), where p is the
 * product rule of sgpu_explain_documents with cand_w[i] in the place of the query weight - F16: fl(cand_w[i] * f32(value));
 * FIXEDU8 and DOTVBYTE: fl(fl(cand_w[i] * val_scale) * (float)code), with the same narrowing (a cand_w[i] * val_scale
 * that underflows is outside this contract). Multiply then add, never contracted. A document's components are distinct,
 * so the additions of one document do not depend on each other: the only order that matters is the order of the
 * documents, and it is fixed. A document listed twice is added twice. Padding elements of a record add nothing.
 * Which terms are returned. The terms of q are the components with W[c] > 0 (pairs whose W holds a NaN or an inf are
 * outside this contract). The t best are kept, by (W descending, component ascending); out_n[q] = min(t, terms of q).
 * Row q of the nq x t row-major out_comps / out_vals holds the kept terms in ASCENDING COMPONENT ORDER, slots past
 * out_n[q] are zero: the first out_n[q] entries of a row are a valid query for sgpu_batch_search as they stand.
 * Checks, in this order: null arguments (SGPU_EINVAL; cand_ids, cand_w and the three outputs too, also when there is
 * nothing to do), everything sgpu_score_documents checks in its order, an alpha or a cand_w[i] that is not finite
 * (SGPU_EINVAL; the message names the first such candidate and its query), a query of more than 65536 candidates
 * (SGPU_ELIMIT), t == 0 (SGPU_EINVAL), t > 1024 (SGPU_ELIMIT), index not uploaded or replica out of range (SGPU_EDEVICE),
 * device memory (SGPU_ENOMEM; the index stays usable). nq == 0 is SGPU_OK.
 * The call shares the score calls' per-replica stream, mutex and recycled scratch and takes turns with them; it is safe
 * beside searches, filtered and exact calls. It adds no index array; its scratch is freed by sgpu_index_destroy or a new
 * upload. A launch takes whole queries only: SGPU_SCORE_CHUNK (candidates per launch, default 2^20) cuts between
 * queries, a query of more candidates than that goes alone; the outputs do not depend on the cuts. */
sgpu_status sgpu_expand_queries(sgpu_index* idx, uint32_t replica,
    const uint64_t* q_off, const uint32_t* comps, const float* vals, uint32_t nq,
    const uint64_t* cand_off, const uint64_t* cand_ids, const float* cand_w,
    float alpha, uint32_t t,
    uint32_t* out_comps, float* out_vals, uint32_t* out_n);
/* The same on the host cores (needs no upload): the arbiter of the contract above, the device call returns its bits;
 * the same checks without the device ones. num_threads == 0: all host cores (over the queries). */
sgpu_status sgpu_expand_queries_host(const sgpu_index* idx,
    const uint64_t* q_off, const uint32_t* comps, const float* vals, uint32_t nq,
    const uint64_t* cand_off, const uint64_t* cand_ids, const float* cand_w,
    float alpha, uint32_t t, uint32_t num_threads,
    uint32_t* out_comps, float* out_vals, uint32_t* out_n);

/* ---- diversify: MMR selection of candidates -----------------------------------
 * A result list that does not repeat itself: Maximal Marginal Relevance over each query's candidates, greedy, round by
 * round, with document-against-document similarities computed on the device. The reference has no counterpart. Queries
 * and candidates are given exactly as for sgpu_score_documents (any order, repeats allowed, possibly none).
 * Relevance and similarity. rel(d) is the bits sgpu_score_documents returns for (query q, document d). sim(d, s), for a
 * candidate d and an already selected document s, is the bits sgpu_score_documents returns for document d and the QUERY
 * made of s's stored elements: one (component, weight) per stored element e < len(s), padding excluded, the weight the
 * stored value as an f32 (binary16 widened, or code * val_scale; both exact); a stored value of +-0 contributes nothing,
 * as a query weight of +-0 does. The streamed document is always the candidate d and the table always the selected s:
 * sim(d, s) and sim(s, d) may differ in their last bits, and only the first is used. For FIXEDU8 / DOTVBYTE the product
 * of an element is fl(fl((code_s * val_scale) * val_scale) * (float)code_d) (a val_scale^2 that underflows is outside
 * this contract, as in explain and expand).
 * Greedy selection, per query. Every candidate ENTRY (a place in the list) starts with pen = +0.0 and untaken. Round
 * r = 0, 1, ...: among the untaken entries the one with the largest key (ordered(mmr bits) descending, document id
 * ascending) is chosen, mmr = fl(fl(lambda * rel) - fl(mu * pen)): multiply, multiply, subtract, each rounded once,
 * never contracted; ordered() is the monotone integer image of f32 bits of sgpu_explain_documents (-0.0 below +0.0).
 * out_doc_ids[q, r] = its id, out_scores[q, r] = its rel, out_penalties[q, r] = its pen at the moment of selection (+0.0
 * in round 0). Every entry with that id is marked taken: a document listed twice is selected once, and both its entries
 * carry equal rel and pen throughout. Then, for every untaken entry d, pen(d) = max(pen(d), sim(d, selected)): pen is
 * max(0, largest similarity to anything selected) - a negative similarity (signed stored values exist) never lowers the
 * penalty below +0.0. The selection stops after k rounds or when no entry is untaken: out_n[q] = min(k, distinct
 * candidates of q). Slots past out_n[q] are zero in all three nq x k row-major arrays; a query without candidates gets
 * out_n = 0 and zeroed rows. Pairs whose rel, sim or mmr is not finite need not match the host twin.
 * Consequences. With lambda = 1 and mu = 0, ids, scores and out_n are exactly those of sgpu_rerank_documents. The rows
 * do not depend on the order in which the candidates are listed, nor on how the call is cut into launches.
 * Checks, in this order: null arguments (SGPU_EINVAL; cand_ids and the four outputs too, also when there is nothing to
 * do), everything sgpu_score_documents checks in its order, a lambda or mu that is not finite (SGPU_EINVAL), a query with
 * more than 2048 listed candidates (SGPU_ELIMIT; the message names the query), a candidate document of more than 8192
 * stored components (SGPU_ELIMIT: the most a half-full hash table in LDS holds, the bound the score call puts on a query;
 * the message names the first such document and its query), k == 0 (SGPU_EINVAL), k > 256 (SGPU_ELIMIT), index not
 * uploaded or replica out of range (SGPU_EDEVICE), device memory (SGPU_ENOMEM; the index stays usable). nq == 0 is
 * SGPU_OK.
 * The call shares the score calls' per-replica stream, mutex and recycled scratch and takes turns with them; it is safe
 * beside searches, filtered and exact calls. It adds no index array; its scratch is freed by sgpu_index_destroy or a new
 * upload. A launch takes whole queries only: SGPU_SCORE_CHUNK (candidates per launch, default 2^20) cuts between
 * queries, a query of more candidates than that goes alone, and a run of queries without any candidate is no launch. */
sgpu_status sgpu_diversify_documents(sgpu_index* idx, uint32_t replica,
    const uint64_t* q_off, const uint32_t* comps, const float* vals, uint32_t nq,
    const uint64_t* cand_off, const uint64_t* cand_ids,
    float lambda, float mu, uint32_t k,
    float* out_scores, float* out_penalties, uint64_t* out_doc_ids, uint32_t* out_n);
/* The same on the host cores (needs no upload): the arbiter of the contract above, the device call returns its bits;
 * the same checks without the device ones. num_threads == 0: all host cores (over the queries). */
sgpu_status sgpu_diversify_documents_host(const sgpu_index* idx,
    const uint64_t* q_off, const uint32_t* comps, const float* vals, uint32_t nq,
    const uint64_t* cand_off, const uint64_t* cand_ids,
    float lambda, float mu, uint32_t k, uint32_t num_threads,
    float* out_scores, float* out_penalties, uint64_t* out_doc_ids, uint32_t* out_n);

/* ---- collapse: the k best groups of a query's candidates ----------------------
 * Field collapsing on the device: the candidates carry a group key each (the document a passage belongs to, a site, an
 * author, a product), and what comes back per query is its k best GROUPS, each scored by its best member (m = 1: MaxP)
 * or by the sum of its m best members. The reference has no counterpart. Queries and candidates are given exactly as for
 * sgpu_score_documents (any order, repeats allowed, possibly none); cand_groups[i] is the group key of entry i: any u32,
 * 0 and 0xffffffff included. The caller owns its meaning: the library keeps no per-document state, and the call adds no
 * index array.
 * Members. The members of group g for query q are the DISTINCT pairs (g, document id) among q's entries: a pair listed
 * twice counts once, the same id listed under two keys is a member of both groups. No consistency check is made, and none
 * is needed. A member's score is, bit for bit, what sgpu_score_documents returns for (q, id). The members of a group are
 * ordered by score descending, then id ascending; the first is the group's BEST MEMBER.
 * Group score. The f32 sum of the group's first min(m, members) members, added in that order, starting from the best
 * member's score: s = score[0]; s = fl(s + score[1]); ... - never reassociated, never widened. m = 1 is MaxP; m >= the
 * group's size is the sum over all of them. A group score is never -0.0, because no member score is (sgpu_rerank_documents
 * says why, and x + y is -0.0 only if both are): the ordered integer image of the bits orders finite group scores
 * numerically, and the device selects on it.
 * Rows. Row q of the nq x k row-major outputs holds q's groups ordered by group score descending, then group key
 * ascending, cut to k: out_groups the key, out_scores the group score, out_best_ids and out_best_scores the best
 * member's id and score, out_members the number of members (all of them, not min(m, .)). out_n[q] = min(k, groups of q).
 * Slots past out_n[q] are zero in all five arrays; a query without candidates gets out_n = 0 and zeroed rows. An empty
 * query scores every member +0.0, so its groups come in key order.
 * Consequences. With m = 1 and every entry's key equal to its (u32) document id, out_best_ids, out_scores and out_n are
 * exactly the rows of sgpu_rerank_documents. The rows do not depend on the order in which the candidates are listed, nor
 * on how the call is cut into launches. Rows that contain a score that is not finite need not match the host twin
 * (sgpu_score_documents makes the same reservation).
 * Checks, in this order: null arguments (SGPU_EINVAL; cand_ids, cand_groups and the six outputs too, also when there is
 * nothing to do), everything sgpu_score_documents checks in its order, a query with more than 4096 listed candidates
 * (SGPU_ELIMIT; the message names the query), m == 0 (SGPU_EINVAL), m > 64 (SGPU_ELIMIT), k == 0 (SGPU_EINVAL), k > 1024
 * (SGPU_ELIMIT), index not uploaded or replica out of range (SGPU_EDEVICE), device memory (SGPU_ENOMEM; the index stays
 * usable). nq == 0 is SGPU_OK.
 * Limits. A query's entries are sorted three times by one workgroup without leaving LDS - by score, by group, and the
 * groups by their score -, 28 bytes per entry: 4096 entries are 112 KiB of a CU's 160. The sum of a group is sequential by
 * contract; m <= 64 keeps it a short loop of one thread.
 * The call shares the score calls' per-replica stream, mutex and recycled scratch and takes turns with them; it is safe
 * beside searches, filtered and exact calls. It adds no index array; its scratch is freed by sgpu_index_destroy or a new
 * upload. A launch takes whole queries only: SGPU_SCORE_CHUNK (candidates per launch, default 2^20) cuts between
 * queries, a query of more candidates than that goes alone, and a run of queries without any candidate is no launch. */
sgpu_status sgpu_collapse_documents(sgpu_index* idx, uint32_t replica,
    const uint64_t* q_off, const uint32_t* comps, const float* vals, uint32_t nq,
    const uint64_t* cand_off, const uint64_t* cand_ids, const uint32_t* cand_groups,
    uint32_t m, uint32_t k,
    uint32_t* out_groups, float* out_scores, uint64_t* out_best_ids, float* out_best_scores,
    uint32_t* out_members, uint32_t* out_n);
/* The same on the host cores (needs no upload): the arbiter of the contract above, the device call returns its bits;
 * the same checks without the device ones. num_threads == 0: all host cores (over the queries). */
sgpu_status sgpu_collapse_documents_host(const sgpu_index* idx,
    const uint64_t* q_off, const uint32_t* comps, const float* vals, uint32_t nq,
    const uint64_t* cand_off, const uint64_t* cand_ids, const uint32_t* cand_groups,
    uint32_t m, uint32_t k, uint32_t num_threads,
    uint32_t* out_groups, float* out_scores, uint64_t* out_best_ids, float* out_best_scores,
    uint32_t* out_members, uint32_t* out_n);

/* ---- fuse: hybrid fusion of a query's candidates with another retriever's scores ----
 * Hybrid retrieval on the device: this index's scores fused with the scores of another retriever (a dense ANN index,
 * BM25, a cross-encoder pass) over the union of both candidate lists; only nq x k rows come back. The reference has no
 * counterpart. Queries and candidates are given exactly as for sgpu_score_documents (any order, repeats allowed, possibly
 * none). cand_ext[i] is the other retriever's score of entry i; NaN of any payload means "not in the other list".
 * Documents. D_q is the set of distinct ids among q's entries. sparse(d) is the bits sgpu_score_documents returns for
 * (q, d). ext(d) is, over the entries of d whose cand_ext is not NaN, the one with the largest ordered() image; ordered()
 * is the monotone integer image of f32 bits of sgpu_explain_documents, -0.0 below +0.0. d is ABSENT if it has no such
 * entry; P_q is the set of documents of D_q that are present.
 * Ranks are ordinal; ties are broken by id and never shared. rank_s(d) = 1 + the number of d' in D_q with
 * ordered(sparse(d')) greater, or equal and a smaller id. rank_e(d) is the same over P_q on ordered(ext); it is 0 for an
 * absent document.
 * Fused score. All arithmetic is f32, every operation rounded once and never contracted; (float)rank is exact.
 *   SGPU_FUSE_RRF     fused = fl( fl(w_sparse / fl(rrf_c + (float)rank_s)) + t_e ),
 *                     t_e = fl(w_ext / fl(rrf_c + (float)rank_e)) if the document is present, else +0.0.
 *   SGPU_FUSE_MINMAX  lo_s, hi_s are the sparse scores of D_q with the smallest and the largest ordered() image;
 *                     n_s = (hi_s == lo_s as floats) ? 1.0f : fl( fl(sparse - lo_s) / fl(hi_s - lo_s) ); n_e the same over
 *                     P_q on ext; fused = fl( fl(w_sparse * n_s) + (present ? fl(w_ext * n_e) : +0.0) ).
 *   SGPU_FUSE_SUM     fused = fl( fl(w_sparse * sparse) + (present ? fl(w_ext * ext) : +0.0) ).
 * A document with an intermediate or a result that is not finite, or that is subnormal, is outside this contract and
 * need not match the host twin (explain and expand make the same kind of reservation).
 * Rows. Row q of the nq x k row-major outputs holds D_q ordered by ordered(fused bits) descending, then id ascending, cut
 * to k: out_doc_ids the id, out_scores fused, out_sparse sparse, out_ext ext (+0.0 where absent), out_rank_sparse rank_s,
 * out_rank_ext rank_e (0 where absent). out_n[q] = min(k, |D_q|). Slots past it are zero in all six arrays; a query
 * without candidates gets out_n = 0 and zeroed rows.
 * Consequences. SUM with w_sparse = 1 and w_ext = 0, any cand_ext: out_doc_ids, out_n and out_sparse are exactly the rows
 * of sgpu_rerank_documents, and out_scores == out_sparse bit for bit (a sparse score is never -0.0, so adding +-0 keeps
 * it). RRF with w_sparse = 1, w_ext = 0 and rrf_c = 60: the ids are rerank's and out_rank_sparse[q, j] = j + 1. The rows
 * depend neither on the order in which the entries are listed nor on how the call is cut into launches.
 * Checks, in this order: null arguments (SGPU_EINVAL; cand_ids, cand_ext and the seven outputs too, also when there is
 * nothing to do), everything sgpu_score_documents checks in its order, a cand_ext[i] that is +-inf (SGPU_EINVAL; the
 * message names the first such candidate and its query), an unknown method (SGPU_EINVAL), w_sparse or w_ext not finite
 * (SGPU_EINVAL), for RRF only an rrf_c that is not finite or < 0 (SGPU_EINVAL), a query with more than 4096 listed
 * candidates (SGPU_ELIMIT; the message names the query), k == 0 (SGPU_EINVAL), k > 1024 (SGPU_ELIMIT), index not uploaded
 * or replica out of range (SGPU_EDEVICE), device memory (SGPU_ENOMEM; the index stays usable). nq == 0 is SGPU_OK.
 * Limits. One team of threads owns a query and nothing leaves LDS between the score kernel and the row: the entries are
 * sorted by id, the documents by either score, then by the fused one - four sorts, 32 bytes per entry: 4096 entries are
 * 128 KiB of a CU's 160.
 * The call shares the score calls' per-replica stream, mutex and recycled scratch and takes turns with them; it is safe
 * beside searches, filtered and exact calls. It adds no index array; its scratch is freed by sgpu_index_destroy or a new
 * upload. A launch takes whole queries only: SGPU_SCORE_CHUNK (candidates per launch, default 2^20) cuts between
 * queries, a query of more candidates than that goes alone, and a run of queries without any candidate is no launch. */
enum { SGPU_FUSE_RRF = 0, SGPU_FUSE_MINMAX = 1, SGPU_FUSE_SUM = 2 };
sgpu_status sgpu_fuse_documents(sgpu_index* idx, uint32_t replica,
    const uint64_t* q_off, const uint32_t* comps, const float* vals, uint32_t nq,
    const uint64_t* cand_off, const uint64_t* cand_ids, const float* cand_ext,
    uint32_t method, float w_sparse, float w_ext, float rrf_c, uint32_t k,
    float* out_scores, uint64_t* out_doc_ids, float* out_sparse, float* out_ext,
    uint32_t* out_rank_sparse, uint32_t* out_rank_ext, uint32_t* out_n);
/* The same on the host cores (needs no upload): the arbiter of the contract above, the device call returns its bits;
 * the same checks without the device ones. num_threads == 0: all host cores (over the queries). */
sgpu_status sgpu_fuse_documents_host(const sgpu_index* idx,
    const uint64_t* q_off, const uint32_t* comps, const float* vals, uint32_t nq,
    const uint64_t* cand_off, const uint64_t* cand_ids, const float* cand_ext,
    uint32_t method, float w_sparse, float w_ext, float rrf_c, uint32_t k, uint32_t num_threads,
    float* out_scores, uint64_t* out_doc_ids, float* out_sparse, float* out_ext,
    uint32_t* out_rank_sparse, uint32_t* out_rank_ext, uint32_t* out_n);

/* Seismic's inner binary dataset format (documents.bin / queries.bin: written by the reference's
 * scripts/convert_json_to_inner_format.py:10-27, read by vectorium's read_seismic_format at
 * src/pylib/mod.rs:987,1127): u32 n_vecs; per vector u32 n, n x u32 components, n x f32 values.
 * read: call with offsets == NULL to size (*n_vecs, *nnz receive the counts), then with buffers of
 * n_vecs + 1 offsets and nnz components / values (*n_vecs, *nnz carry the capacities in). */
sgpu_status sgpu_dataset_read(const char* path, uint64_t* n_vecs, uint64_t* nnz, uint64_t* offsets,
                              uint32_t* comps, float* vals);
sgpu_status sgpu_dataset_write(const char* path, uint64_t n_vecs, const uint64_t* offsets,
                               const uint32_t* comps, const float* vals);
/* Replaces: the result dump of perf_inverted_index (src/bin/perf_inverted_index.rs:223-235), the file
 * scripts/run_experiments.py:287-309 compares with groundtruth.tsv:
 * query_index \t doc_id \t rank (from 1) \t score, one line per result (rows of nq x k slabs). */
sgpu_status sgpu_results_write_tsv(const char* path, uint32_t nq, uint32_t k, const float* scores,
                                   const uint64_t* doc_ids, const uint32_t* n);
/* Deterministic SPLADE-shaped synthetic data: writes a
 * CSR dataset into caller-provided buffers. Call with comps==NULL to size:
 * *out_nnz receives the number of entries. kind: 0 = documents, 1 = queries
 * (queries draw 60% of their tokens from a random source document of `docs_*`). */
typedef struct sgpu_synth_spec {
  uint64_t n_vecs;
  uint64_t dim;
  uint64_t seed;
  uint32_t kind;        /* 0 docs, 1 queries */
  uint32_t collection;  /* 0 = the SURVEY 8(d) law (the benchmark's headline collection); 1 = "clustered": documents drawn
                           around latent intents, queries carry their source document's weights (synth.cpp) */
} sgpu_synth_spec;
sgpu_status sgpu_synth_generate(const sgpu_synth_spec* spec,
                                const uint64_t* docs_offsets, const uint32_t* docs_comps,
                                const float* docs_vals, uint64_t n_docs,
                                uint64_t* out_offsets, uint32_t* out_comps, float* out_vals,
                                uint64_t* out_nnz);

#ifdef __cplusplus
}
#endif
#endif /* SEISMIC_HIP_H */
