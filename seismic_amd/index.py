"""Host-side mirror of the reference's Python API for the search path.

Same class names, argument names, defaults and result shapes as the PyO3 module
`seismic` (reference src/pylib/mod.rs), so code written against the reference
switches by changing the import:

    from seismic_amd import SeismicIndex, SeismicDataset, get_seismic_string

  SeismicIndex / SeismicIndexLV        string-keyed (u16 / u32 components)
      reference: src/pylib/mod.rs:46-661 (search 504-533, batch_search 587-655)
      wrapper semantics: src/inverted_index_wrapper.rs:58-91, 194-284
  SeismicIndexRaw / SeismicIndexRawLV  integer-keyed
      reference: src/pylib/mod.rs:663-1151 (search 1046-1076, batch_search 1111-1146)
  SeismicDataset / SeismicDatasetLV    in-memory dataset with exact search
      reference: src/pylib/dataset.rs, src/inverted_index_wrapper.rs:599-758

Search runs on the GPU through the C ABI (include/seismic_hip.h); everything
here is marshalling: token -> component id (unknown tokens dropped, sorted by
id), internal id -> document id string. There is no CPU search fallback.

Documented deviations (DESIGN.md "Boundary"):
  * token ids: tokens are numbered in SORTED order (the reference numbers them
    in HashMap iteration order, which changes from run to run;
    scripts/convert_json_to_inner_format.py:188-190 sorts too);
  * batch_search returns results in INPUT order (the reference's par_bridge
    does not guarantee any order, src/pylib/mod.rs:629-652);
  * num_threads is accepted and ignored on the GPU path (it is ineffective in
    the reference as well: the pool it builds is dropped, src/pylib/mod.rs:599-602);
  * the kNN graph (build_knn / nknn, n_knn at search time) is built ON THE GPU by searching every
    document through the same kernel; knn files are numpy .npy (the reference's *.knn.seismic
    uses vectorium's serializer).
"""
import ctypes as C
import gzip
import io
import json
import os
import tarfile

import numpy as np

from . import _native
from ._abi import SGPU_COLOP_IN, SGPU_COLOP_RANGE, SGPU_MAX_COLUMNS, BuildConfig

MAX_TOKEN_LEN = 30


def get_seismic_string():
    """numpy dtype string of token arrays (reference src/pylib/mod.rs:24-25, 41-44)."""
    return "U%d" % MAX_TOKEN_LEN


# ---------------------------------------------------------------------------
# ingestion (host side; reference src/json_utils.rs:10-78, wrapper 398-552)
# ---------------------------------------------------------------------------
def _iter_jsonl(path):
    if path.endswith(".tar.gz") or path.endswith(".tgz"):
        with tarfile.open(path, "r:gz") as tar:
            for member in tar:
                if not member.isfile():
                    continue
                f = tar.extractfile(member)
                for line in io.TextIOWrapper(f, encoding="utf-8"):
                    line = line.strip()
                    if line:
                        yield json.loads(line)
        return
    opener = gzip.open if path.endswith(".gz") else open
    with opener(path, "rt", encoding="utf-8") as f:
        for line in f:
            line = line.strip()
            if line:
                yield json.loads(line)


def read_jsonl(path):
    """rows {id: str|int, vector: {token: weight}, content?: str} -> (ids, [dict], [content])"""
    ids, vecs, contents = [], [], []
    try:
        for row in _iter_jsonl(path):
            ids.append(str(row["id"]))
            vecs.append(row["vector"])
            contents.append(row.get("content"))
    except (OSError, KeyError, ValueError, tarfile.TarError) as e:
        raise IOError("Failed to read %s: %s" % (path, e))
    return ids, vecs, contents


def read_inner_format(path, comp_dtype=np.uint32):
    """Seismic's inner binary format (scripts/convert_json_to_inner_format.py:10-27):
    u32 n_vecs; per vector: u32 n, n x u32 components (sorted), n x f32 values; little endian.
    Parsed by the native library (sgpu_dataset_read): an 8.8M-document file reads at disk speed."""
    try:
        return _native.read_inner_format(path)
    except _native.SeismicHipError as e:
        raise IOError(str(e))


def write_inner_format(path, off, comps, vals):
    try:
        _native.write_inner_format(path, off, comps, vals)
    except _native.SeismicHipError as e:
        raise IOError(str(e))


def write_results_tsv(path, scores, ids, n):
    """`query_index \\t doc_id \\t rank \\t score` per result, the dump of the reference's
    perf_inverted_index (src/bin/perf_inverted_index.rs:223-235)."""
    try:
        _native.write_results_tsv(path, scores, ids, n)
    except _native.SeismicHipError as e:
        raise IOError(str(e))


def read_results_tsv(path):
    """-> {query_id: [doc_id, ...]} of a results / groundtruth TSV (same four columns)."""
    out = {}
    try:
        with open(path, "r", encoding="utf-8") as f:
            for line in f:
                if line.strip():
                    q, d = line.split("\t")[:2]
                    out.setdefault(int(q), []).append(int(d))
    except (OSError, ValueError) as e:
        raise IOError("Failed to read %s: %s" % (path, e))
    return out


def accuracy(results, groundtruth):
    """compute_accuracy of the reference's scripts/run_experiments.py:287-309: per query the size of
    the intersection of the two doc-id sets, summed, over the number of ground-truth rows."""
    total = sum(len(v) for v in groundtruth.values())
    hit = sum(len(set(v) & set(results.get(q, ()))) for q, v in groundtruth.items())
    return hit / total if total else 0.0


def _token_map(vecs, given=None):
    if given is not None:
        return dict(given)
    toks = set()
    for v in vecs:
        toks.update(v.keys())
    return {t: i for i, t in enumerate(sorted(toks))}


def _to_csr(vecs, token_map):
    off = np.zeros(len(vecs) + 1, np.uint64)
    cs, vs = [], []
    for i, v in enumerate(vecs):
        items = sorted((token_map[t], w) for t, w in v.items() if t in token_map)
        off[i + 1] = off[i] + len(items)
        cs.extend(c for c, _ in items)
        vs.extend(w for _, w in items)
    return off, np.asarray(cs, np.uint32), np.asarray(vs, np.float32)


def _resolve(tokens, values, token_map):
    """resolve_query_tokens (reference src/inverted_index_wrapper.rs:75-91): unknown tokens are
    dropped silently, the rest is sorted by component id."""
    if isinstance(tokens, np.ndarray):
        tokens = tokens.ravel().tolist()   # python strings in one C-level pass
    if isinstance(values, np.ndarray):
        values = values.ravel().tolist()
    pairs = sorted((token_map[t], float(v)) for t, v in zip(tokens, values) if t in token_map)
    # a token repeated in the query would give a duplicate component; keep the first, as a
    # dict-built query (the documented way to make one) cannot contain duplicates
    comps, vals, last = [], [], None
    for c, v in pairs:
        if c != last:
            comps.append(c)
            vals.append(v)
            last = c
    return np.asarray(comps, np.uint32), np.asarray(vals, np.float32)


def _resolve_batch(query_components, query_values, token_map, tokens_of):
    """Queries resolved one by one (_resolve) into one CSR batch."""
    cs, vs = [], []
    off = np.zeros(len(query_components) + 1, np.uint64)
    for i, (qc, qv) in enumerate(zip(query_components, query_values)):
        c, v = _resolve(tokens_of(qc), np.asarray(qv, np.float32).ravel(), token_map)
        cs.append(c)
        vs.append(v)
        off[i + 1] = off[i] + len(c)
    comps = np.concatenate(cs) if cs else np.zeros(0, np.uint32)
    vals = np.concatenate(vs) if vs else np.zeros(0, np.float32)
    return off, comps, vals


def _cfg(n_postings, centroid_fraction, min_cluster_size, summary_energy, max_fraction, doc_cut, num_threads):
    # SGPU_BUILD_DEVICE=<n>: run the clustering step of the build on HIP device n (byte-identical index)
    dev = os.environ.get("SGPU_BUILD_DEVICE", "")
    return BuildConfig.defaults(n_postings=int(n_postings), centroid_fraction=float(centroid_fraction),
                                min_cluster_size=int(min_cluster_size), summary_energy=float(summary_energy),
                                max_fraction=float(max_fraction), doc_cut=int(doc_cut),
                                num_threads=int(num_threads), use_device=int(dev) + 1 if dev else 0)


def _no_knn_path(knn_path):
    if knn_path:
        raise ValueError("precomputed *.knn.seismic files use vectorium's serializer, which is not in the "
                         "reference tree; build the graph with nknn=... or load a .npy with load_knn()")


# ---------------------------------------------------------------------------
class SeismicFilter:
    """A set of allowed documents of one index (make_filter): search, batch_search and batch_exact_search with
    filter=this look at those documents only. Not in the reference. It keeps its index alive; on the GPU it holds,
    per device the index is on, the allowed documents' postings (built on first use, see include/seismic_hip.h)."""

    def __init__(self, index, native_filter):
        self.index = index
        self._f = native_filter

    @property
    def count(self):
        """Number of allowed documents."""
        return self._f.count

    def device_bytes(self):
        """HBM the filter holds on the devices (0 before its first GPU search)."""
        return self._f.device_bytes()

    def bits(self):
        """The allowed set over the index's internal document rows: u32 words, bit d of word d // 32."""
        return self._f.bits()

    def close(self):
        self._f.close()


def _native_filter(owner, filter):
    """filter= of a search call -> the NativeFilter to pass down (None: no filter). A SeismicFilter must be the
    owner's; anything else is an iterable of ids, made into a filter for this one call."""
    if filter is None:
        return None
    if isinstance(filter, SeismicFilter):
        if filter.index is not owner:
            raise ValueError("the filter was made on another index")
        return filter._f
    if isinstance(filter, (str, bytes)):
        raise TypeError("filter= takes a SeismicFilter or an iterable of document ids, not a single id")
    return owner.make_filter(filter)._f


def _term_filter(owner, component_of, must, must_not, should, min_should, min_weight, within, device):
    """make_term_filter of both class families. component_of(term) -> the component, or None for a term the index does
    not know. An entry of must / must_not / should is a bare term or a (term, min_weight) pair; min_weight= is the
    threshold of the bare ones (None: any stored entry). A MUST term the index does not know gives the empty filter; an
    unknown MUST_NOT or SHOULD term matches nothing and is dropped (min_should still counts against the given list's
    matches, so it may become unreachable). device None: on the GPU when the index is uploaded, else on the host
    cores; False: the host; an int or True: the GPU (uploaded first if need be)."""
    default = -np.inf if min_weight is None else float(min_weight)
    clauses, empty = [], False
    for occur, entries in ((0, must), (1, must_not), (2, should)):   # SGPU_TERM_MUST, _MUST_NOT, _SHOULD
        if isinstance(entries, (str, bytes)):
            raise TypeError("must / must_not / should take an iterable of terms, not a single term")
        for e in entries:
            term, w = (e[0], float(e[1])) if isinstance(e, tuple) else (e, default)
            c = component_of(term)
            if c is None:
                empty = empty or occur == 0
                continue
            clauses.append((c, occur, w))
    if within is not None and not isinstance(within, SeismicFilter):
        raise TypeError("within= takes a SeismicFilter")
    if within is not None and within.index is not owner:
        raise ValueError("the filter was made on another index")
    if empty:
        return SeismicFilter(owner, owner._ix.make_filter(np.zeros(0, np.int64)))
    host = device is False or (device is None and not owner._uploaded)
    if not host:
        owner._ensure_device()
    return SeismicFilter(owner, owner._ix.make_term_filter(clauses, min_should, None if within is None else within._f, host=host))


def _column_bounds(dt, lo, hi):
    """(lo, hi) of a range entry -> the bounds' bit patterns in the column's dtype; None: the type's lowest / highest
    value. A bound outside an integer type's range is moved to its nearest value, or the clause made one that matches
    nothing (lo > hi) where the range lies outside the type."""
    if dt == np.float32:
        lo = -np.inf if lo is None else lo
        hi = np.inf if hi is None else hi
    else:
        info = np.iinfo(dt)
        lo = info.min if lo is None or lo == -np.inf else lo
        hi = info.max if hi is None or hi == np.inf else hi
        if lo != lo or hi != hi:
            raise ValueError("a bound is NaN")
        if lo > info.max or hi < info.min:
            lo, hi = 1, 0
        lo, hi = max(int(np.ceil(lo)), info.min), min(int(np.floor(hi)), info.max)
    b = np.array([lo, hi], dt).view(np.uint32)
    return int(b[0]), int(b[1])


def _column_set(dt, values):
    """The values of a set entry -> their bit patterns in the column's dtype; a value the type cannot hold matches nothing
    and is dropped."""
    v = np.asarray(list(values) if not isinstance(values, np.ndarray) else values).ravel()
    if dt != np.float32 and v.size:
        info = np.iinfo(dt)
        if v.dtype.kind == "f":
            v = v[np.isfinite(v) & (v == np.floor(v))]
        v = np.asarray([int(x) for x in v if info.min <= int(x) <= info.max], np.int64)
    return v.astype(dt).view(np.uint32).tolist()


# ---------------------------------------------------------------------------
class _DatasetBase:
    """SeismicDataset (reference src/pylib/dataset.rs): add_document + exact search."""
    _CW = 2

    def __init__(self):
        self._ids, self._vecs, self._contents = [], [], []
        self._native = None
        self._tm = None
        self._on_device = None

    def add_document(self, doc_id, tokens, values, content=None):
        self._ids.append(str(doc_id))
        self._vecs.append({str(t): float(v) for t, v in zip(tokens, values)})
        self._contents.append(content)
        self._native = None
        self._on_device = None

    @property
    def len(self):
        return len(self._ids)

    def _freeze(self):
        if self._native is None:
            self._tm = _token_map(self._vecs)
            off, c, v = _to_csr(self._vecs, self._tm)
            # exact search only needs the forward index: build with the cheapest valid config
            self._native = _native.NativeIndex.build(self._CW, max(len(self._tm), 1), off, c, v,
                                                     _cfg(1, 1.0, 0, 1.0, 1.0, 1, 0))
            self._on_device = None
        return self._native

    def _exact(self, q_off, comps, vals, k, device, num_threads=0):
        """device None: the host cores; an int: that GPU (the frozen index is uploaded there once)."""
        ix = self._freeze()
        if device is None:
            return ix.exact_search(q_off, comps, vals, k, num_threads)
        if self._on_device != int(device):
            ix.upload(int(device))   # raises if there is no such device
            self._on_device = int(device)
        return ix.exact_search_device(q_off, comps, vals, k)

    def search(self, query_id, query_components, query_values, k, device=None):
        """Exact top-k (brute force; host cores, or the GPU `device`) -> [(query_id, score, doc_id)]."""
        ix = self._freeze()
        c, v = _resolve([str(t) for t in np.asarray(query_components).ravel()],
                        np.asarray(query_values, np.float32).ravel(), self._tm)
        sc, ids, n = self._exact(np.array([0, len(c)], np.uint64), c, v, k, device)
        return [(str(query_id), float(sc[0, i]), self._ids[int(ids[0, i])]) for i in range(int(n[0]))]

    def batch_search(self, queries_ids, query_components, query_values, k, num_threads=0, device=None):
        if device is None:
            return [self.search(q, c, v, k) for q, c, v in zip(np.asarray(queries_ids).ravel(), query_components,
                                                               query_values)]
        self._freeze()
        qids = [str(x) for x in np.asarray(queries_ids).ravel()]
        off, comps, vals = _resolve_batch(query_components, query_values, self._tm,
                                          lambda t: [str(x) for x in np.asarray(t).ravel()])
        sc, ids, n = self._exact(off, comps, vals, k, device)
        names = self._ids
        return [[(qids[i], float(sc[i, j]), names[int(ids[i, j])]) for j in range(int(n[i]))]
                for i in range(len(qids))]


class SeismicDataset(_DatasetBase):
    _CW = 2


class SeismicDatasetLV(_DatasetBase):
    _CW = 4



# ---------------------------------------------------------------------------
class _ScoreMixin:
    """score / batch_score / rerank / batch_rerank of the index classes: the scores of caller-given documents and the k
    best of them (sgpu_score_documents, sgpu_rerank_documents; no reference counterpart - the reference computes such a score only inside its search,
    QueryEvaluator::compute_distance at src/posting_list.rs:210-211). A score is what search returns for the document,
    bit for bit. The classes supply _score_queries (queries -> CSR, unknown tokens dropped as in search),
    _score_rows (document ids -> native ids, an unknown id raises KeyError) and _score_name (native id -> document id);
    explain / batch_explain (sgpu_explain_documents: the terms behind a score) and expand / batch_expand
    (sgpu_expand_queries: Rocchio feedback queries) also _score_token (component -> token); diversify / batch_diversify
    (sgpu_diversify_documents: MMR selection) need what rerank needs; collapse / batch_collapse (sgpu_collapse_documents:
    the k best groups) take group keys beside the ids, or look them up in the mapping set_groups keeps; fuse / batch_fuse
    (sgpu_fuse_documents: hybrid fusion) take another retriever's scores beside the ids."""

    def _score_csr(self, query_components, query_values, doc_ids_per_query):
        off, comps, vals = self._score_queries(query_components, query_values)
        rows = [self._score_rows(d) for d in doc_ids_per_query]
        if len(rows) != len(off) - 1:
            raise ValueError("%d queries but %d document id lists" % (len(off) - 1, len(rows)))
        cand_off = np.zeros(len(rows) + 1, np.uint64)
        if rows:
            cand_off[1:] = np.cumsum([len(r) for r in rows])
        cand = np.concatenate(rows).astype(np.uint64) if rows else np.zeros(0, np.uint64)
        return off, comps, vals, cand_off, cand, rows

    def _score_on_device(self, device):
        """False: the host twin. Else the GPU the index is on (uploading it if need be)."""
        if device is False:
            return False
        if device is not None and device is not True and int(device) != int(self._device):
            raise ValueError("the index is on device %d, not %d" % (self._device, int(device)))
        self._ensure_device()
        return True

    def _batch_score_native(self, query_components, query_values, doc_ids_per_query, device):
        off, comps, vals, cand_off, cand, rows = self._score_csr(query_components, query_values, doc_ids_per_query)
        if self._score_on_device(device):
            sc = self._ix.score_documents(off, comps, vals, cand_off, cand)
        else:
            sc = self._ix.score_documents_host(off, comps, vals, cand_off, cand)
        bounds = cand_off.astype(np.int64)
        return [sc[bounds[i]:bounds[i + 1]] for i in range(len(rows))], rows

    def batch_score(self, query_components, query_values, doc_ids_per_query, device=None):
        """Per query, the scores (float32 array) of its documents doc_ids_per_query[q], in the order given (any order,
        repeats allowed, possibly none). device None: the GPU the index is on; False: the host cores, bit-identical."""
        return self._batch_score_native(query_components, query_values, doc_ids_per_query, device)[0]

    def score(self, query_components, query_values, doc_ids, device=None):
        """The scores (float32 array) of the documents `doc_ids` for one query."""
        return self.batch_score([query_components], [query_values], [doc_ids], device)[0]

    def batch_rerank(self, query_components, query_values, doc_ids_per_query, k, device=None):
        """Per query the k best of its candidates -> [[(score, doc_id)]]: score descending, ties by native document id
        ascending, a candidate given more than once counted once. Scored and selected by sgpu_rerank_documents on the GPU
        the index is on (device None) or by its host twin (device False); a k the library does not take (0, above 1024)
        is selected here from batch_score's scores."""
        k = int(k)
        if not 1 <= k <= 1024:
            return self._batch_rerank_numpy(query_components, query_values, doc_ids_per_query, k, device)
        off, comps, vals, cand_off, cand, rows = self._score_csr(query_components, query_values, doc_ids_per_query)
        if self._score_on_device(device):
            sc, ids, n = self._ix.rerank_documents(off, comps, vals, cand_off, cand, k)
        else:
            sc, ids, n = self._ix.rerank_documents_host(off, comps, vals, cand_off, cand, k)
        sc, ids = sc.tolist(), ids.tolist()
        name = self._score_name
        return [[(s, name(d)) for s, d in zip(sc[q][:m], ids[q][:m])] for q, m in enumerate(n.tolist())]

    def rerank(self, query_components, query_values, doc_ids, k, device=None):
        """The k best of the documents `doc_ids` for one query -> [(score, doc_id)], best first."""
        return self.batch_rerank([query_components], [query_values], [doc_ids], k, device)[0]

    def batch_explain(self, query_components, query_values, doc_ids_per_query, m=10, device=None):
        """Per query and document of doc_ids_per_query[q] (as for batch_score) -> (score, n_terms, [(token, query weight,
        document weight, product)]): the score batch_score returns, the number of terms query and document share, and the
        m best of them (1 <= m <= 32), largest product first, ties by component ascending. The score is the sum of all
        n_terms products in the library's summation order. Tokens are mapped back through _score_token (the token string;
        the raw classes: the integer component). sgpu_explain_documents on the GPU the index is on (device None) or its
        host twin (device False)."""
        off, comps, vals, cand_off, cand, rows = self._score_csr(query_components, query_values, doc_ids_per_query)
        if self._score_on_device(device):
            out = self._ix.explain_documents(off, comps, vals, cand_off, cand, m)
        else:
            out = self._ix.explain_documents_host(off, comps, vals, cand_off, cand, m)
        sc, nt, tc, tq, td, tp = [a.tolist() for a in out]
        token = self._score_token
        docs = [(sc[i], nt[i], [(token(c), q, d, p) for c, q, d, p in list(zip(tc[i], tq[i], td[i], tp[i]))[:nt[i]]])
                for i in range(len(sc))]
        bounds = cand_off.astype(np.int64).tolist()
        return [docs[bounds[i]:bounds[i + 1]] for i in range(len(rows))]

    def explain(self, query_components, query_values, doc_ids, m=10, device=None):
        """(score, n_terms, [(token, query weight, document weight, product)]) of each of `doc_ids` for one query."""
        return self.batch_explain([query_components], [query_values], [doc_ids], m, device)[0]

    def batch_expand(self, query_components, query_values, doc_ids_per_query, doc_weights_per_query=None, alpha=1.0,
                     beta=0.75, terms=64, device=None):
        """Rocchio feedback queries -> one (tokens, values) pair per query: alpha * query + sum over the feedback documents
        doc_ids_per_query[q] of weight * document, the `terms` (1 .. 1024) heaviest positive components of it, in
        ascending component order (values: float32 array). doc_weights_per_query[q][i] is the weight of document i of
        query q; None: beta / len(doc_ids_per_query[q]) for each. Documents are added in the order given (f32 sums
        depend on it), one listed twice is added twice. Tokens are mapped back through _score_token (the raw classes:
        the integer component), so a pair can go to search / batch_search as it is. sgpu_expand_queries on the GPU the
        index is on (device None) or its host twin (device False)."""
        off, comps, vals, cand_off, cand, rows = self._score_csr(query_components, query_values, doc_ids_per_query)
        if doc_weights_per_query is None:
            w = [np.full(len(r), np.float32(beta) / np.float32(len(r)), np.float32) if len(r) else np.zeros(0, np.float32)
                 for r in rows]
        else:
            w = [np.asarray(x, np.float32).ravel() for x in doc_weights_per_query]
            if [len(x) for x in w] != [len(r) for r in rows]:
                raise ValueError("doc_weights_per_query does not match doc_ids_per_query")
        cand_w = np.concatenate(w) if w else np.zeros(0, np.float32)
        if self._score_on_device(device):
            oc, ov, n = self._ix.expand_queries(off, comps, vals, cand_off, cand, cand_w, alpha, terms)
        else:
            oc, ov, n = self._ix.expand_queries_host(off, comps, vals, cand_off, cand, cand_w, alpha, terms)
        token = self._score_token
        return [([token(c) for c in oc[q, :m].tolist()], ov[q, :m].copy()) for q, m in enumerate(n.tolist())]

    def expand(self, query_components, query_values, doc_ids, doc_weights=None, alpha=1.0, beta=0.75, terms=64, device=None):
        """(tokens, values) of one query's feedback query (batch_expand)."""
        return self.batch_expand([query_components], [query_values], [doc_ids], None if doc_weights is None else [doc_weights],
                                 alpha, beta, terms, device)[0]

    def batch_diversify(self, query_components, query_values, doc_ids_per_query, k, lam=0.5, mu=0.5, device=None):
        """Maximal Marginal Relevance over each query's candidates -> [[(score, penalty, doc_id)]] in selection order: round
        by round the candidate with the largest lam * score - mu * penalty, where penalty is its largest similarity (dot
        product of the stored vectors) to anything selected before, at least 0; ties by native document id ascending, a
        candidate given more than once counted once. k: 1 .. 256; at most 2048 candidates per query. lam = 1, mu = 0 is
        batch_rerank. sgpu_diversify_documents on the GPU the index is on (device None) or its host twin (device False)."""
        off, comps, vals, cand_off, cand, rows = self._score_csr(query_components, query_values, doc_ids_per_query)
        if self._score_on_device(device):
            sc, pen, ids, n = self._ix.diversify_documents(off, comps, vals, cand_off, cand, lam, mu, k)
        else:
            sc, pen, ids, n = self._ix.diversify_documents_host(off, comps, vals, cand_off, cand, lam, mu, k)
        sc, pen, ids = sc.tolist(), pen.tolist(), ids.tolist()
        name = self._score_name
        return [[(s, p, name(d)) for s, p, d in zip(sc[q][:m], pen[q][:m], ids[q][:m])] for q, m in enumerate(n.tolist())]

    def diversify(self, query_components, query_values, doc_ids, k, lam=0.5, mu=0.5, device=None):
        """The MMR selection among the documents `doc_ids` for one query -> [(score, penalty, doc_id)] (batch_diversify)."""
        return self.batch_diversify([query_components], [query_values], [doc_ids], k, lam, mu, device)[0]

    def set_groups(self, mapping):
        """The group keys (u32) of the documents, for batch_collapse and batch_search_collapsed without explicit keys: a
        dict document id -> key (a document id the index does not hold raises ValueError), or an array with one key per
        document in the index's order. None forgets them. Kept on this object only: not saved with the index, and the
        library never sees it."""
        if mapping is None:
            self._groups = None
            return
        known = np.ones(self.len, bool)
        if isinstance(mapping, dict):
            keys = np.zeros(self.len, np.int64)
            known[:] = False
            try:
                rows = self._score_rows(list(mapping.keys()))
            except KeyError as e:
                raise ValueError("set_groups: unknown document id %s" % (e,))
            keys[rows] = [int(g) for g in mapping.values()]
            known[rows] = True
        else:
            keys = np.asarray(mapping).astype(np.int64).ravel()
            if len(keys) != self.len:
                raise ValueError("%d group keys for %d documents" % (len(keys), self.len))
        if len(keys) and (keys.min() < 0 or keys.max() >= 2 ** 32):
            raise ValueError("a group key is a u32")
        self._groups = (keys.astype(np.uint32), known)

    # ---- document columns (sgpu_index_set_column, sgpu_filter_create_columns, sgpu_facet_counts) ----
    def set_column(self, name, values, dtype=None):
        """A per-document attribute of 32 bits, held with the index on host and device (not saved with it): an array with
        one value per document in the index's order, or a dict document id -> value (an id the index does not hold
        raises ValueError; documents that are not named get 0). The column's type follows `dtype`, or the values':
        unsigned -> u32, signed -> i32, floating -> f32; Python ints without a negative one are u32. Setting a name
        again replaces the column; None drops it. At most 16 names at a time (ValueError)."""
        slots = self.__dict__.setdefault("_columns", {})
        if values is None:
            if name in slots:
                self._ix.set_column(slots.pop(name)[0], None)
            return
        if name in slots:
            slot = slots[name][0]
        else:
            free = [s for s in range(SGPU_MAX_COLUMNS) if s not in {v[0] for v in slots.values()}]
            if not free:
                raise ValueError("set_column: %d columns are set already; drop one first" % SGPU_MAX_COLUMNS)
            slot = free[0]
        n = int(self.len)
        if isinstance(values, dict):
            try:
                rows = self._score_rows(list(values.keys()))
            except KeyError as e:
                raise ValueError("set_column: unknown document id %s" % (e,))
            given = _native.column_array(list(values.values()), dtype)
            col = np.zeros(n, given.dtype)
            col[rows] = given
        else:
            col = _native.column_array(values, dtype).ravel()
            if len(col) != n:
                raise ValueError("%d column values for %d documents" % (len(col), n))
        self._ix.set_column(slot, col)
        slots[name] = (slot, self._ix.get_column(slot).dtype)

    def _column(self, name):
        slots = getattr(self, "_columns", None) or {}
        if name not in slots:
            raise ValueError("no column %r: call set_column first" % (name,))
        return slots[name]

    def make_column_filter(self, must=(), must_not=(), should=(), min_should=0, within=None, device=None):
        """A SeismicFilter of the documents whose columns satisfy every `must` entry, no `must_not` entry and at least
        `min_should` of the `should` entries (sgpu_filter_create_columns). An entry is (name, lo, hi): lo <= value <= hi in
        the column's own order, None as a bound meaning the type's lowest or highest value (-inf / +inf for f32); or
        (name, [values]): the value is one of them. A stored NaN matches nothing; -0.0 equals +0.0. within: a
        SeismicFilter to intersect with. device None: the GPU when the index is uploaded, else the host cores; False:
        the host; an int: the GPU. count is the number of matching documents."""
        clauses, set_values = [], []
        for occur, entries in ((0, must), (1, must_not), (2, should)):   # SGPU_TERM_MUST, _MUST_NOT, _SHOULD
            if isinstance(entries, tuple) and entries and isinstance(entries[0], str):
                raise TypeError("must / must_not / should take an iterable of entries, not a single entry")
            for e in entries:
                e = tuple(e)
                slot, dt = self._column(e[0])
                if len(e) == 3:
                    lo, hi = _column_bounds(dt, e[1], e[2])
                    clauses.append((slot, occur, SGPU_COLOP_RANGE, lo, hi, 0, 0))
                elif len(e) == 2:
                    vals = _column_set(dt, e[1])
                    clauses.append((slot, occur, SGPU_COLOP_IN, 0, 0, len(set_values), len(vals)))
                    set_values.extend(vals)
                else:
                    raise ValueError("an entry is (name, lo, hi) or (name, [values]), got %r" % (e,))
        if within is not None and not isinstance(within, SeismicFilter):
            raise TypeError("within= takes a SeismicFilter")
        if within is not None and within.index is not self:
            raise ValueError("the filter was made on another index")
        host = device is False or (device is None and not self._uploaded)
        if not host:
            self._ensure_device()
        return SeismicFilter(self, self._ix.make_column_filter(clauses, min_should, np.asarray(set_values, np.uint32),
                                                               None if within is None else within._f, host=host))

    def facets(self, name, filter=None, top=10, device=None):
        """Facet counts -> ([(value, count)], distinct, docs): the `top` (1 .. 1024) most frequent values of the u32 column
        `name` among the filter's documents (None: all), by count descending, value ascending; `distinct` is the number
        of values that occur, `docs` the number of documents counted (sgpu_facet_counts). device as for
        make_column_filter."""
        slot, dt = self._column(name)
        host = device is False or (device is None and not self._uploaded)
        if not host:
            self._ensure_device()
        vals, cnts, distinct, docs = self._ix.facet_counts(slot, _native_filter(self, filter), top, host=host)
        return list(zip(vals.tolist(), cnts.tolist())), distinct, docs

    # ---- column aggregations (sgpu_column_stats, sgpu_column_histogram, sgpu_column_top) ----
    def _agg_call(self, name, filter, device):
        slot, dt = self._column(name)
        host = device is False or (device is None and not self._uploaded)
        if not host:
            self._ensure_device()
        return slot, dt, _native_filter(self, filter), host

    def stats(self, name, filter=None, device=None):
        """Summary of column `name` over the filter's documents (None: all) -> dict(docs, valid, min, max, sum, mean):
        `valid` leaves out the NaNs of an f32 column; min / max in the column's dtype (None where valid == 0; an f32 zero
        comes back as +0.0); sum an exact Python int for u32 / i32 and the canonical binary64 sum for f32; mean =
        sum / valid, None where valid == 0 (sgpu_column_stats). device as for make_column_filter."""
        slot, dt, f, host = self._agg_call(name, filter, device)
        s = self._ix.column_stats(slot, f, host=host)
        valid = s["valid"]
        lo, hi = np.array([s["min_bits"], s["max_bits"]], np.uint32).view(dt).tolist()
        if dt == np.float32:
            total = s["sum"]
        else:
            total = s["sum_int"] - (1 << 64) if dt == np.int32 and s["sum_int"] >> 63 else s["sum_int"]
        return dict(docs=s["docs"], valid=valid, min=lo if valid else None, max=hi if valid else None, sum=total,
                    mean=total / valid if valid else None)

    def histogram(self, name, edges, filter=None, device=None):
        """Counts of column `name` per range, numpy.histogram's reading -> dict(counts, below, above, nan, docs): `edges`
        (2 .. 4097 values of the column's dtype, strictly ascending) bound len(edges) - 1 buckets, bucket b holding
        edges[b] <= v < edges[b + 1] and the last one v == edges[-1] too; below / above count the values outside, nan the
        NaNs of an f32 column (sgpu_column_histogram). An edge the column's integer type cannot hold raises ValueError.
        device as for make_column_filter."""
        slot, dt, f, host = self._agg_call(name, filter, device)
        bits = []
        for e in (edges.tolist() if isinstance(edges, np.ndarray) else list(edges)):
            if e != e:
                raise ValueError("an edge is NaN")
            lo, hi = _column_bounds(dt, e, e)      # (an integer type: ceil and floor agree only on a value it holds)
            if lo != hi:
                raise ValueError("edge %r is not a value of the column's type %s" % (e, np.dtype(dt).name))
            bits.append(lo)
        counts, below, above, nan, docs = self._ix.column_histogram(slot, np.asarray(bits, np.uint32), f, host=host)
        return dict(counts=counts.astype(np.int64), below=below, above=above, nan=nan, docs=docs)

    def top_by(self, name, k=10, descending=False, filter=None, device=None):
        """The filter's documents (None: all) ordered by column `name` -> (ids, values): the first k (1 .. 1024) by value
        ascending (descending=True: descending), equal values by the index's document order; NaN documents never appear.
        ids as the results name them, values in the column's dtype (sgpu_column_top). device as for make_column_filter."""
        slot, dt, f, host = self._agg_call(name, filter, device)
        rows, bits, _, _ = self._ix.column_top(slot, k, 1 if descending else 0, f, host=host)
        return [self._score_name(r) for r in rows.tolist()], bits.view(dt)

    def batch_collapse(self, query_components, query_values, doc_ids_per_query, groups_per_query, k, m=1, device=None, groups=None):
        """Field collapsing -> [[(group, score, best_doc_id, best_score, members)]]: per query the k (1 .. 1024) best
        groups of its candidates (as for batch_score, at most 4096 per query). groups_per_query[q][i] is the u32 group
        key of candidate i of query q; None: the keys set_groups holds or, with groups="name", the values of that u32
        column (set_column). A group's members are its distinct documents,
        best first; its score is the f32 sum of its first m (1 .. 64) members in that order (m = 1: MaxP); groups come
        by score descending, key ascending. sgpu_collapse_documents on the GPU the index is on (device None) or its
        host twin (device False)."""
        off, comps, vals, cand_off, cand, rows = self._score_csr(query_components, query_values, doc_ids_per_query)
        if groups is not None:
            if groups_per_query is not None:
                raise ValueError("pass groups_per_query or groups=, not both")
            slot, dt = self._column(groups)
            if dt != np.uint32:
                raise ValueError("groups=%r: group keys come from a u32 column, this one is %s" % (groups, dt))
            grp = self._ix.get_column(slot)[cand.astype(np.int64)]
        elif groups_per_query is None:
            table = getattr(self, "_groups", None)
            if table is None:
                raise ValueError("no group keys: pass groups_per_query or call set_groups first")
            at = cand.astype(np.int64)
            if not table[1][at].all():
                raise ValueError("no group key for document %r" % (self._score_name(int(at[~table[1][at]][0])),))
            grp = table[0][at]
        else:
            g = [np.asarray(x).astype(np.int64).ravel() for x in groups_per_query]
            if [len(x) for x in g] != [len(r) for r in rows]:
                raise ValueError("groups_per_query does not match doc_ids_per_query")
            grp = np.concatenate(g) if g else np.zeros(0, np.int64)
            if len(grp) and (grp.min() < 0 or grp.max() >= 2 ** 32):
                raise ValueError("a group key is a u32")
            grp = grp.astype(np.uint32)
        if self._score_on_device(device):
            out = self._ix.collapse_documents(off, comps, vals, cand_off, cand, grp, m, k)
        else:
            out = self._ix.collapse_documents_host(off, comps, vals, cand_off, cand, grp, m, k)
        gk, sc, ids, bs, mem = [a.tolist() for a in out[:5]]
        name = self._score_name
        return [[(g, s, name(d), b, c) for g, s, d, b, c in zip(gk[q][:n], sc[q][:n], ids[q][:n], bs[q][:n], mem[q][:n])]
                for q, n in enumerate(out[5].tolist())]

    def collapse(self, query_components, query_values, doc_ids, groups, k, m=1, device=None):
        """The k best groups among the documents `doc_ids` for one query -> [(group, score, best_doc_id, best_score,
        members)] (batch_collapse)."""
        return self.batch_collapse([query_components], [query_values], [doc_ids], None if groups is None else [groups], k, m,
                                   device)[0]

    def batch_fuse(self, query_components, query_values, doc_ids_per_query, ext_scores_per_query, k, method="rrf", w_sparse=1.0,
                   w_ext=1.0, rrf_c=60.0, device=None):
        """Hybrid fusion -> [[(fused, doc_id, sparse, ext, rank_sparse, rank_ext)]], best first: per query the k (1 .. 1024)
        best of its candidates (as for batch_score, at most 4096 per query) under the fusion of this index's score with
        another retriever's. ext_scores_per_query[q][i] is that retriever's score of candidate i of query q, NaN (or None)
        where it does not list the document; of a document given more than once the largest counts. method "rrf": w_sparse /
        (rrf_c + rank_sparse) + w_ext / (rrf_c + rank_ext), ordinal ranks from 1; "minmax": the weighted sum of both
        scores normalised to [0, 1] over the query's documents; "sum": the weighted sum of the raw scores. A document the
        other list lacks gets no external term; its ext and rank_ext come back as 0.0 and 0. sgpu_fuse_documents on the
        GPU the index is on (device None) or its host twin (device False)."""
        off, comps, vals, cand_off, cand, rows = self._score_csr(query_components, query_values, doc_ids_per_query)
        e = [np.array([np.nan if x is None else x for x in row], np.float32).ravel() for row in ext_scores_per_query]
        if [len(x) for x in e] != [len(r) for r in rows]:
            raise ValueError("ext_scores_per_query does not match doc_ids_per_query")
        ext = np.concatenate(e) if e else np.zeros(0, np.float32)
        if self._score_on_device(device):
            out = self._ix.fuse_documents(off, comps, vals, cand_off, cand, ext, method, w_sparse, w_ext, rrf_c, k)
        else:
            out = self._ix.fuse_documents_host(off, comps, vals, cand_off, cand, ext, method, w_sparse, w_ext, rrf_c, k)
        fs, ids, sp, ex, rs, re = [a.tolist() for a in out[:6]]
        name = self._score_name
        return [[(f, name(d), s, x, a, b) for f, d, s, x, a, b in zip(fs[q][:n], ids[q][:n], sp[q][:n], ex[q][:n], rs[q][:n], re[q][:n])]
                for q, n in enumerate(out[6].tolist())]

    def fuse(self, query_components, query_values, doc_ids, ext_scores, k, method="rrf", w_sparse=1.0, w_ext=1.0, rrf_c=60.0,
             device=None):
        """The k best of the documents `doc_ids` for one query under the fusion with `ext_scores` -> [(fused, doc_id,
        sparse, ext, rank_sparse, rank_ext)] (batch_fuse)."""
        return self.batch_fuse([query_components], [query_values], [doc_ids], [ext_scores], k, method, w_sparse, w_ext, rrf_c,
                               device)[0]

    def _batch_rerank_numpy(self,query_components, query_values, doc_ids_per_query, k, device):
        scores, rows = self._batch_score_native(query_components, query_values, doc_ids_per_query, device)
        out = []
        for sc, r in zip(scores, rows):
            ids, first = np.unique(np.asarray(r, np.int64), return_index=True)   # (ascending native ids)
            s = sc[first]
            order = np.argsort(-s.astype(np.float64), kind="stable")[: int(k)]   # (stable: ties keep ascending ids)
            out.append([(float(s[i]), self._score_name(int(ids[i]))) for i in order])
        return out


# ---------------------------------------------------------------------------
class _IndexBase(_ScoreMixin):
    _CW = 2

    def __init__(self, native, token_map, doc_ids, contents=None, device=0, upload=True):
        self._ix = native
        self._tm = token_map
        self._doc_ids = doc_ids
        self._contents = contents
        self._doc_pos = None
        self._tokens = None   # component -> token (batch_explain)
        self._device = device
        self._uploaded = False
        if upload:
            self._ensure_device()

    def _ensure_device(self):
        if not self._uploaded:
            self._ix.upload(self._device)   # raises if no HIP device: no CPU fallback
            self._uploaded = True

    # ---- construction -------------------------------------------------
    @classmethod
    def build(cls, input_path, n_postings=3500, centroid_fraction=0.1, min_cluster_size=2, summary_energy=0.4,
              max_fraction=1.5, doc_cut=15, nknn=0, knn_path=None, batched_indexing=None,
              input_token_to_id_map=None, load_content=True, num_threads=0, device=0, upload=True):
        """Build from a .jsonl / .jsonl.gz / .tar.gz file (reference src/pylib/mod.rs:329-384)."""
        _no_knn_path(knn_path)
        ids, vecs, contents = read_jsonl(input_path)
        tm = _token_map(vecs, input_token_to_id_map)
        if cls._CW == 2 and len(tm) >= 2 ** 16:
            raise ValueError("The number of different tokens exceeds 2^16; use SeismicIndexLV")
        off, c, v = _to_csr(vecs, tm)
        ix = _native.NativeIndex.build(cls._CW, max(len(tm), 1), off, c, v,
                                       _cfg(n_postings, centroid_fraction, min_cluster_size, summary_energy,
                                            max_fraction, doc_cut, num_threads))
        return cls._finish_build(ix, nknn, device, upload, tm, ids, contents if load_content else None)

    @classmethod
    def _finish_build(cls, ix, nknn, device, upload, *meta):
        """The kNN graph is built on the index AS BUILT (u16/f16), before a class converts its forward index: the
        reference runs Index::from_file(..).knn(..) first and convert_dataset_into afterwards
        (src/pylib/dotvbyte.rs:193-209), so SeismicIndexDotVByte's graph is SeismicIndex's graph."""
        if nknn:
            ix.upload(device)      # Knn::new runs as batches through the GPU kernel
            ix.build_knn(nknn)
        self = cls(ix, *meta, device, False)
        if self._ix is ix and nknn:
            self._uploaded = True              # (not converted: the upload above is the index's)
        elif upload or nknn:
            self._ensure_device()
        return self

    @classmethod
    def build_from_dataset(cls, dataset, n_postings=3500, centroid_fraction=0.1, min_cluster_size=2,
                           summary_energy=0.4, max_fraction=1.5, doc_cut=15, nknn=0, knn_path=None,
                           batched_indexing=None, num_threads=0, device=0, upload=True):
        _no_knn_path(knn_path)
        tm = _token_map(dataset._vecs)
        off, c, v = _to_csr(dataset._vecs, tm)
        ix = _native.NativeIndex.build(cls._CW, max(len(tm), 1), off, c, v,
                                       _cfg(n_postings, centroid_fraction, min_cluster_size, summary_energy,
                                            max_fraction, doc_cut, num_threads))
        return cls._finish_build(ix, nknn, device, upload, tm, list(dataset._ids), list(dataset._contents))

    @classmethod
    def load(cls, index_path, device=0, upload=True):
        """Load `<index_path>.index.sgpu` + `.meta.json` (own format; reference files
        *.index.seismic use vectorium's serializer, which is not in the reference tree)."""
        base = index_path[:-len(".index.sgpu")] if index_path.endswith(".index.sgpu") else index_path
        try:
            ix = _native.NativeIndex.load(base + ".index.sgpu")
            with open(base + ".meta.json", "r", encoding="utf-8") as f:
                meta = json.load(f)
        except (_native.SeismicHipError, OSError, ValueError) as e:
            raise IOError("Failed to load index %s: %s" % (index_path, e))
        return cls(ix, meta["token_to_id_map"], meta["document_mapping"], meta.get("document_content"),
                   device, upload)

    def save(self, path):
        try:
            self._ix.save(path + ".index.sgpu")
            with open(path + ".meta.json", "w", encoding="utf-8") as f:
                json.dump({"token_to_id_map": self._tm, "document_mapping": self._doc_ids,
                           "document_content": self._contents}, f)
        except (_native.SeismicHipError, OSError) as e:
            raise IOError("Failed to save index %s: %s" % (path, e))

    # ---- accessors ----------------------------------------------------
    @property
    def dim(self):
        return int(self._ix.desc.dim)

    @property
    def len(self):
        return int(self._ix.desc.n_docs)

    @property
    def nnz(self):
        return int(self._ix.desc.nnz)

    @property
    def knn_len(self):
        return self._ix.get_knn()[1]

    def build_knn(self, nknn):
        """reference src/pylib/mod.rs:195-197 (build_knn). Runs on the GPU."""
        self._ensure_device()
        self._ix.build_knn(nknn)

    def save_knn(self, path):
        nb, dim = self._ix.get_knn()
        if dim == 0:
            raise ValueError("the index has no kNN graph")   # reference: PyValueError (src/pylib/mod.rs:217-221)
        np.save(path if path.endswith(".npy") else path + ".knn.npy", np.concatenate([[dim], nb]).astype(np.uint32))

    def load_knn(self, knn_path, nknn=None):
        try:
            a = np.load(knn_path if knn_path.endswith(".npy") else knn_path + ".knn.npy")
        except OSError as e:
            raise IOError(str(e))
        dim, nb = int(a[0]), a[1:].astype(np.uint32)
        if nknn is not None and nknn < dim and len(nb) == self.len * dim:   # keep the first nknn per document
            nb = nb.reshape(self.len, dim)[:, :nknn].reshape(-1)
            dim = nknn
        self._ix.set_knn(nb, dim)

    @property
    def is_empty(self):
        return self.len == 0

    def get(self, id):
        """Document `id` of the forward index -> (component ids, values as f32); reference
        src/pylib/mod.rs:157-165, 797-805 (`dataset().get(id)`, values widened with `to_f32`)."""
        d = self._ix.desc
        if not 0 <= id < d.n_docs:
            raise IndexError("document %d out of range (0..%d)" % (id, d.n_docs))   # the reference panics
        a, e = int(d.fwd_offsets[id]), int(d.fwd_offsets[id + 1])
        if e == a:
            return [], []
        cdt = np.uint16 if d.comp_width == 2 else np.uint32
        comps = np.ctypeslib.as_array((C.c_uint8 * ((e - a) * d.comp_width)).from_address(d.fwd_comps + a * d.comp_width))
        comps = comps.view(cdt)
        if d.value_type == 0:
            vals = np.ctypeslib.as_array((C.c_uint16 * (e - a)).from_address(d.fwd_vals + a * 2)).view(np.float16)
            vals = vals.astype(np.float32)
        else:
            codes = np.ctypeslib.as_array((C.c_uint8 * (e - a)).from_address(d.fwd_vals + a))
            vals = codes.astype(np.float32) * np.float32(d.val_scale)
        return [int(c) for c in comps], [float(v) for v in vals]

    def get_doc_ids_in_postings(self, list_id):
        d = self._ix.desc
        if not 0 <= list_id < d.dim:
            raise ValueError("Invalid list_id: %d" % list_id)
        b0, b1 = d.list_block_start[list_id], d.list_block_start[list_id + 1]
        p0, p1 = d.block_post_start[b0], d.block_post_start[b1]
        return [int(d.post_doc[p]) for p in range(p0, p1)]

    def print_space_usage_byte(self):
        d = self._ix.desc
        cw = d.comp_width
        fwd = d.nnz * (cw + 2) + (d.n_docs + 1) * 8
        packed = d.n_postings * 8
        boffs = (d.n_blocks + d.dim) * 8
        summ = d.n_entries * 3 + d.n_rows * (cw + 8) + d.n_blocks * 8
        print("Space Usage:")
        print("\tForward Index: %d Bytes" % fwd)
        print("\tPosting Lists: %d Bytes" % (packed + boffs + summ))
        print("\t  packed_postings: %d Bytes\n\t  block_offsets: %d Bytes\n\t  summaries: %d Bytes"
              % (packed, boffs, summ))
        knn = 4 * len(self._ix.get_knn()[0])
        print("\tKnn: %d Bytes" % knn)
        print("\tTotal: %d Bytes" % (fwd + packed + boffs + summ + knn))
        print("\tHBM resident: %d Bytes" % self._ix.device_bytes())

    def _positions(self):
        if self._doc_pos is None:   # built on first use: doc id -> position
            self._doc_pos = {d: i for i, d in enumerate(self._doc_ids)}
        return self._doc_pos

    def get_doc_text(self, doc_id):
        if self._contents is None:
            return None
        i = self._positions().get(doc_id)
        return None if i is None else self._contents[i]

    def make_filter(self, doc_ids):
        """A SeismicFilter of the documents `doc_ids` (external ids, as the results name them); an unknown id raises
        KeyError. Pass it as filter= to search, batch_search and batch_exact_search."""
        pos = self._positions()
        if isinstance(doc_ids, (str, bytes)):
            raise TypeError("make_filter takes an iterable of document ids, not a single id")
        rows = []
        for d in doc_ids:
            i = pos.get(str(d))
            if i is None:
                raise KeyError(d)
            rows.append(i)
        return SeismicFilter(self, self._ix.make_filter(np.asarray(rows, np.int64)))

    def make_term_filter(self, must=(), must_not=(), should=(), min_should=0, min_weight=None, within=None, device=None):
        """A SeismicFilter of the documents that store every `must` token, none of the `must_not` tokens and at least
        `min_should` of the `should` tokens (sgpu_filter_create_terms: evaluated against every stored component, not
        the pruned posting lists). An entry is a token or a (token, min_weight) pair: the token counts only where its
        stored weight is >= min_weight (min_weight= is the default of the bare tokens; None: any stored weight). A
        `must` token outside the vocabulary gives the empty filter; a `must_not` or `should` token outside it matches
        nothing. within: a SeismicFilter to intersect with. device None: the GPU when the index is uploaded, else the
        host cores; False: the host; an int: the GPU. count is the number of matching documents."""
        tm = self._tm
        return _term_filter(self, lambda t: tm.get(str(t)), must, must_not, should, min_should, min_weight, within, device)

    # ---- scores of given documents (_ScoreMixin) ----------------------
    def _score_queries(self, query_components, query_values):
        return _resolve_batch(query_components, query_values, self._tm, lambda t: np.asarray(t).astype(str))

    def _score_rows(self, doc_ids):
        if isinstance(doc_ids, (str, bytes)):
            raise TypeError("document ids come as an iterable, not a single id")
        pos, rows = self._positions(), []
        for d in doc_ids:
            i = pos.get(str(d))
            if i is None:
                raise KeyError(d)
            rows.append(i)
        return np.asarray(rows, np.int64)

    def _score_name(self, row):
        return self._doc_ids[row]

    def _score_token(self, component):
        if self._tokens is None:
            self._tokens = {i: t for t, i in self._tm.items()}
        return self._tokens[component]

    # ---- search -------------------------------------------------------
    def _remap(self, query_id, sc, ids, n):
        n, q, names = int(n), str(query_id), self._doc_ids
        return [(q, s, names[i]) for s, i in zip(sc[:n].tolist(), ids[:n].tolist())]

    def search(self, query_id, query_components, query_values, k, query_cut, heap_factor, n_knn=0, sorted=True,
               filter=None):
        """-> [(query_id, score, doc_id)], best first (reference src/pylib/mod.rs:490-533). filter: a SeismicFilter of
        this index or an iterable of document ids - only those documents can be returned."""
        self._ensure_device()
        f = _native_filter(self, filter)
        c, v = _resolve(np.asarray(query_components).astype(str), np.asarray(query_values, np.float32), self._tm)
        sc, ids = self._ix.search(c, v, k, query_cut, heap_factor, first_sorted=bool(sorted), n_knn=n_knn, filter=f)
        return self._remap(query_id, sc, ids, len(ids))

    def batch_search(self, queries_ids, query_components, query_values, k, query_cut, heap_factor, n_knn=0,
                     sorted=True, num_threads=0, filter=None):
        """-> [[(query_id, score, doc_id)]] in input order (reference src/pylib/mod.rs:572-655).
        One GPU pass over the whole batch. filter: as for search."""
        self._ensure_device()
        f = _native_filter(self, filter)
        qids = [str(x) for x in np.asarray(queries_ids).ravel()]
        off = np.zeros(len(qids) + 1, np.uint64)
        cs, vs = [], []
        for i, (qc, qv) in enumerate(zip(query_components, query_values)):
            c, v = _resolve(np.asarray(qc).astype(str), np.asarray(qv, np.float32), self._tm)
            cs.append(c)
            vs.append(v)
            off[i + 1] = off[i] + len(c)
        comps = np.concatenate(cs) if cs else np.zeros(0, np.uint32)
        vals = np.concatenate(vs) if vs else np.zeros(0, np.float32)
        sc, ids, n = self._ix.batch_search(off, comps, vals, k, query_cut, heap_factor, first_sorted=bool(sorted),
                                           n_knn=n_knn, filter=f)
        return [self._remap(qids[i], sc[i], ids[i], n[i]) for i in range(len(qids))]

    def batch_search_feedback(self, queries_ids, query_components, query_values, k, query_cut, heap_factor, fb_docs=10,
                              fb_terms=64, alpha=1.0, beta=0.75, n_knn=0, sorted=True, filter=None):
        """Pseudo-relevance feedback -> the rows of batch_search: search, batch_expand of every query with its first fb_docs
        results as feedback documents (weight beta / their number), search again with the expanded queries. Composition
        of the two calls, nothing else."""
        first = self.batch_search(queries_ids, query_components, query_values, k, query_cut, heap_factor, n_knn=n_knn,
                                  sorted=sorted, filter=filter)
        docs = [[d for _, _, d in row[:int(fb_docs)]] for row in first]
        expanded = self.batch_expand(query_components, query_values, docs, None, alpha, beta, fb_terms)
        return self.batch_search(queries_ids, [np.asarray(t, dtype=str) for t, _ in expanded], [v for _, v in expanded], k,
                                 query_cut, heap_factor, n_knn=n_knn, sorted=sorted, filter=filter)

    def batch_search_collapsed(self, queries_ids, query_components, query_values, k, query_cut, heap_factor, depth=100, m=1,
                               n_knn=0, sorted=True, filter=None, groups=None):
        """Search, then collapse -> [[(query_id, group, score, best_doc_id, best_score, members)]]: batch_search for `depth`
        hits per query, batch_collapse of every query's hits under the keys set_groups holds (or, with groups="name", the
        values of that u32 column), cut to k groups.
        Composition of the two calls, nothing else."""
        if groups is not None:
            self._column(groups)
        elif getattr(self, "_groups", None) is None:
            raise ValueError("no group keys: call set_groups first")
        hits = self.batch_search(queries_ids, query_components, query_values, depth, query_cut, heap_factor, n_knn=n_knn,
                                 sorted=sorted, filter=filter)
        docs = [[d for _, _, d in row] for row in hits]
        rows = self.batch_collapse(query_components, query_values, docs, None, k, m, groups=groups)
        qids = [str(x) for x in np.asarray(queries_ids).ravel()]
        return [[(qids[q],) + r for r in row] for q, row in enumerate(rows)]

    def batch_search_fused(self, queries_ids, query_components, query_values, external_hits, k, query_cut, heap_factor,
                           depth=100, method="rrf", w_sparse=1.0, w_ext=1.0, rrf_c=60.0, n_knn=0, sorted=True, filter=None):
        """Hybrid search -> [[(query_id, fused, doc_id, sparse, ext, rank_sparse, rank_ext)]]: batch_search for `depth` hits
        per query, their union with external_hits[q] - the other retriever's list of (doc_id, score) -, batch_fuse over
        it, cut to k. A document the search found and the external list lacks is absent there (ext = NaN); one the
        external list alone holds is scored by the fusion like any other. Composition of the two calls, nothing else."""
        hits = self.batch_search(queries_ids, query_components, query_values, depth, query_cut, heap_factor, n_knn=n_knn,
                                 sorted=sorted, filter=filter)
        if len(external_hits) != len(hits):
            raise ValueError("%d queries but %d external lists" % (len(hits), len(external_hits)))
        docs, ext = [], []
        for row, other in zip(hits, external_hits):
            other = [(str(d), float(s)) for d, s in other]
            listed = {d for d, _ in other}
            mine = [d for _, _, d in row if d not in listed]
            docs.append([d for d, _ in other] + mine)
            ext.append([s for _, s in other] + [np.nan] * len(mine))
        rows = self.batch_fuse(query_components, query_values, docs, ext, k, method, w_sparse, w_ext, rrf_c)
        qids = [str(x) for x in np.asarray(queries_ids).ravel()]
        return [[(qids[q],) + r for r in row] for q, row in enumerate(rows)]

    def batch_exact_search(self, queries_ids, query_components, query_values, k, device=None, filter=None):
        """Exact top-k over the index's own documents -> [[(query_id, score, doc_id)]] in input order, the rows of
        SeismicDataset.batch_search. device None: the host cores; an int: the GPU the index is on. filter: as for
        search (then the k best of the allowed documents, min(k, their number) of them)."""
        f = _native_filter(self, filter)
        qids = [str(x) for x in np.asarray(queries_ids).ravel()]
        off, comps, vals = _resolve_batch(query_components, query_values, self._tm, lambda t: np.asarray(t).astype(str))
        if device is None:
            sc, ids, n = self._ix.exact_search(off, comps, vals, k, filter=f)
        else:
            if int(device) != int(self._device):
                raise ValueError("the index is on device %d, not %d" % (self._device, int(device)))
            self._ensure_device()
            sc, ids, n = self._ix.exact_search_device(off, comps, vals, k, filter=f)
        return [self._remap(qids[i], sc[i], ids[i], n[i]) for i in range(len(qids))]


class SeismicIndex(_IndexBase):
    """u16 components (vocabulary < 65536)."""
    _CW = 2


class SeismicIndexLV(_IndexBase):
    """u32 components: large vocabularies."""
    _CW = 4


class SeismicIndexDotVByte(_IndexBase):
    """The reference's compressed index (src/pylib/dotvbyte.rs:20-36): the standard u16/f16 index is
    built first and its forward index is then converted (`convert_dataset_into`, :208-213) - here to
    SGPU_VAL_DOTVBYTE: fixed-u8 document values and a compressed component stream (12 bytes per
    8-element slice), 2.5 bytes per component in HBM instead of 4. Same query API and results type as
    SeismicIndex; scores differ by the 8-bit quantisation of the document values. u16 components only, as
    in the reference. (vectorium's DotVByteFixedU8Encoder is not in the reference tree: the fixed-point
    step and the layout of the lossless component stream are restated, see include/seismic_hip.h - parity
    unpinned; results are bit-identical to the fixed-u8 index, which the tests assert.)
    `component_stream=False` keeps the raw u16 components (SGPU_VAL_FIXEDU8, 3 bytes per component)."""
    _CW = 2

    def __init__(self, native, token_map, doc_ids, contents=None, device=0, upload=True, component_stream=True):
        from ._abi import SGPU_VAL_DOTVBYTE, SGPU_VAL_FIXEDU8
        want = SGPU_VAL_DOTVBYTE if component_stream else SGPU_VAL_FIXEDU8
        if native.desc.value_type != want:
            native = native.convert(want)
        super().__init__(native, token_map, doc_ids, contents, device, upload)


# ---------------------------------------------------------------------------
class _RawBase(_ScoreMixin):
    """Integer-keyed index over the inner binary format (reference src/pylib/mod.rs:663-1151)."""
    _CW = 2

    def __init__(self, native, device=0, upload=True):
        self._ix = native
        self._device = device
        self._uploaded = False
        if upload:
            self._ensure_device()

    _ensure_device = _IndexBase._ensure_device
    dim = _IndexBase.dim
    len = _IndexBase.len
    nnz = _IndexBase.nnz
    knn_len = _IndexBase.knn_len
    is_empty = _IndexBase.is_empty
    get = _IndexBase.get
    get_doc_ids_in_postings = _IndexBase.get_doc_ids_in_postings
    print_space_usage_byte = _IndexBase.print_space_usage_byte

    @classmethod
    def build(cls, input_file, n_postings=3500, centroid_fraction=0.1, min_cluster_size=2, summary_energy=0.4,
              max_fraction=1.5, doc_cut=15, nknn=0, knn_path=None, batched_indexing=None, num_threads=0,
              device=0, upload=True):
        _no_knn_path(knn_path)
        off, c, v = read_inner_format(input_file)
        dim = int(c.max()) + 1 if len(c) else 1
        if cls._CW == 2 and dim > 65536:
            raise ValueError("component ids do not fit u16; use SeismicIndexRawLV")
        ix = _native.NativeIndex.build(cls._CW, dim, off, c, v,
                                       _cfg(n_postings, centroid_fraction, min_cluster_size, summary_energy,
                                            max_fraction, doc_cut, num_threads))
        self = cls(ix, device, upload or bool(nknn))
        if nknn:
            self.build_knn(nknn)
        return self

    build_knn = _IndexBase.build_knn
    save_knn = _IndexBase.save_knn
    load_knn = _IndexBase.load_knn

    @classmethod
    def load(cls, index_path, device=0, upload=True):
        try:
            return cls(_native.NativeIndex.load(index_path), device, upload)
        except _native.SeismicHipError as e:
            raise IOError("Failed to load index %s: %s" % (index_path, e))

    def save(self, path):
        try:
            self._ix.save(path)
        except _native.SeismicHipError as e:
            raise IOError(str(e))

    def make_filter(self, doc_ids):
        """A SeismicFilter of the documents `doc_ids` (integer ids, or a boolean mask of length len). Pass it as
        filter= to search and batch_search."""
        return SeismicFilter(self, self._ix.make_filter(np.asarray(list(doc_ids) if not isinstance(doc_ids, np.ndarray)
                                                                   else doc_ids)))

    def make_term_filter(self, must=(), must_not=(), should=(), min_should=0, min_weight=None, within=None, device=None):
        """As SeismicIndex.make_term_filter, the terms being integer components; one >= dim is outside the vocabulary."""
        dim = int(self.dim)

        def component_of(t):
            return int(t) if 0 <= int(t) < dim else None
        return _term_filter(self, component_of, must, must_not, should, min_should, min_weight, within, device)

    def _score_queries(self, query_components, query_values):
        off = np.zeros(len(query_components) + 1, np.uint64)
        cs, vs = [], []
        for i, (qc, qv) in enumerate(zip(query_components, query_values)):
            c = np.asarray(qc).astype(np.uint32).ravel()
            v = np.asarray(qv, np.float32).ravel()
            order = np.argsort(c, kind="stable")
            cs.append(c[order])
            vs.append(v[order])
            off[i + 1] = off[i] + len(c)
        return (off, np.concatenate(cs) if cs else np.zeros(0, np.uint32),
                np.concatenate(vs) if vs else np.zeros(0, np.float32))

    def _score_rows(self, doc_ids):
        rows = np.asarray(list(doc_ids) if not isinstance(doc_ids, np.ndarray) else doc_ids).astype(np.int64).ravel()
        bad = rows[(rows < 0) | (rows >= self.len)]
        if len(bad):
            raise KeyError(int(bad[0]))
        return rows

    def _score_name(self, row):
        return row

    def _score_token(self, component):
        return component

    def search(self, query_components, query_values, k, query_cut, heap_factor, n_knn, sorted, filter=None):
        """-> [(score, doc_id)] (reference src/pylib/mod.rs:1033-1076). filter: a SeismicFilter of this index or an
        iterable of document ids - only those documents can be returned."""
        self._ensure_device()
        f = _native_filter(self, filter)
        sc, ids = self._ix.search(np.asarray(query_components).astype(np.uint32),
                                  np.asarray(query_values, np.float32), k, query_cut, heap_factor,
                                  first_sorted=bool(sorted), n_knn=n_knn, filter=f)
        return [(float(s), int(i)) for s, i in zip(sc, ids)]

    def batch_search(self, query_path, k, query_cut, heap_factor, n_knn, sorted, num_threads=0, filter=None):
        """queries.bin in the inner format -> [[(score, doc_id)]] in file order (src/pylib/mod.rs:1098-1146).
        filter: as for search."""
        self._ensure_device()
        f = _native_filter(self, filter)
        off, c, v = read_inner_format(query_path)
        sc, ids, n = self._ix.batch_search(off, c, v, k, query_cut, heap_factor, first_sorted=bool(sorted),
                                           n_knn=n_knn, filter=f)
        return [[(float(sc[q, i]), int(ids[q, i])) for i in range(int(n[q]))] for q in range(len(off) - 1)]


class SeismicIndexRaw(_RawBase):
    _CW = 2


class SeismicIndexRawLV(_RawBase):
    _CW = 4
