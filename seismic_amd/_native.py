"""ctypes binding of libseismic_hip.so (the C ABI in include/seismic_hip.h).

The library is built in-tree by seismic_amd/csrc/Makefile. There is no Python or
CPU fallback for the search path: if the shared object is missing, or no HIP
device is usable, the calls fail loudly.
"""
import ctypes as C
import os

import numpy as np

from ._abi import (ABI_VERSION, BuildConfig, ColumnStats, IndexDesc, LaunchStats, SearchParams, SynthSpec,
                   SGPU_COL_F32, SGPU_COL_I32, SGPU_COL_U32, SGPU_OK)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SGPU_LIB") or os.path.join(_HERE, "libseismic_hip.so")   # SGPU_LIB: experiment builds
_lib = None


class SeismicHipError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__("seismic_hip status %d: %s" % (status, msg))
        self.status = status


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                "%s not found: build it with `make -C seismic_amd/csrc` (needs hipcc); "
                "there is no CPU fallback for the search path" % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        L.sgpu_last_error.restype = C.c_char_p
        L.sgpu_build_info.restype = C.c_char_p
        L.sgpu_abi_version.restype = C.c_uint32
        L.sgpu_index_device_bytes.restype = C.c_uint64
        L.sgpu_index_device_bytes.argtypes = [C.c_void_p]
        L.sgpu_index_destroy.argtypes = [C.c_void_p]
        L.sgpu_index_destroy.restype = None
        L.sgpu_batch_destroy.argtypes = [C.c_void_p]
        L.sgpu_batch_destroy.restype = None
        vp = C.c_void_p
        L.sgpu_device_count.argtypes = [C.POINTER(C.c_int32)]
        L.sgpu_index_create.argtypes = [C.POINTER(IndexDesc), C.POINTER(vp)]
        L.sgpu_index_build.argtypes = [C.c_uint32, C.c_uint64, C.c_uint64, vp, vp, vp,
                                       C.POINTER(BuildConfig), C.POINTER(vp)]
        L.sgpu_index_get_desc.argtypes = [vp, C.POINTER(IndexDesc)]
        L.sgpu_index_save.argtypes = [vp, C.c_char_p]
        L.sgpu_index_load.argtypes = [C.c_char_p, C.POINTER(vp)]
        L.sgpu_index_convert.argtypes = [vp, C.c_uint32, C.POINTER(vp)]
        L.sgpu_index_upload.argtypes = [vp, C.c_int32]
        L.sgpu_index_upload_many.argtypes = [vp, vp, C.c_uint32]
        L.sgpu_index_replicas.argtypes = [vp]
        L.sgpu_index_replicas.restype = C.c_uint32
        L.sgpu_batch_create_on.argtypes = [vp, C.c_uint32, vp, vp, vp, C.c_uint32, C.c_uint32, C.POINTER(vp)]
        L.sgpu_index_build_knn.argtypes = [vp, C.c_uint32]
        L.sgpu_index_set_knn.argtypes = [vp, vp, C.c_uint64, C.c_uint32]
        L.sgpu_index_get_knn.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]
        L.sgpu_search.argtypes = [vp, vp, vp, C.c_uint32, C.POINTER(SearchParams), vp, vp,
                                  C.POINTER(C.c_uint32)]
        L.sgpu_batch_search.argtypes = [vp, vp, vp, vp, C.c_uint32, C.POINTER(SearchParams), vp, vp, vp]
        L.sgpu_search_sequential.argtypes = [vp, vp, vp, vp, C.c_uint32, C.POINTER(SearchParams), vp, vp, vp,
                                             C.POINTER(C.c_double), vp]
        L.sgpu_search_sequential_timed.argtypes = [vp, vp, vp, vp, C.c_uint32, C.POINTER(SearchParams), vp, vp, vp,
                                                   C.POINTER(C.c_double), vp, vp]
        L.sgpu_batch_create.argtypes = [vp, vp, vp, vp, C.c_uint32, C.c_uint32, C.POINTER(vp)]
        L.sgpu_batch_run.argtypes = [vp, vp, C.POINTER(SearchParams), C.c_int32, C.POINTER(LaunchStats)]
        L.sgpu_batch_run_counted.argtypes = [vp, vp, C.POINTER(SearchParams), C.POINTER(LaunchStats)]
        L.sgpu_batch_sync.argtypes = [vp, C.POINTER(LaunchStats)]
        L.sgpu_batch_fetch.argtypes = [vp, vp, C.c_uint32, vp, vp, vp]
        L.sgpu_batch_fetch_stats.argtypes = [vp, vp, vp]
        L.sgpu_summary_distances.argtypes = [vp, C.c_uint32, vp, vp, C.c_uint32, vp, C.POINTER(C.c_uint32)]
        L.sgpu_exact_search.argtypes = [vp, vp, vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp]
        L.sgpu_exact_search_device.argtypes = [vp, C.c_uint32, vp, vp, vp, C.c_uint32, C.c_uint32, vp, vp, vp]
        L.sgpu_filter_create.argtypes = [vp, vp, C.c_uint64, C.POINTER(vp)]
        L.sgpu_filter_create_terms.argtypes = [vp, C.c_uint32, vp, C.c_uint32, C.c_uint32, vp, C.POINTER(vp)]
        L.sgpu_filter_create_terms_host.argtypes = [vp, vp, C.c_uint32, C.c_uint32, vp, C.c_uint32, C.POINTER(vp)]
        L.sgpu_index_set_column.argtypes = [vp, C.c_uint32, C.c_uint32, vp, C.c_uint64]
        L.sgpu_index_get_column.argtypes = [vp, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(vp), C.POINTER(C.c_uint64)]
        L.sgpu_filter_create_columns.argtypes = [vp, C.c_uint32, vp, C.c_uint32, C.c_uint32, vp, C.c_uint32, vp, C.POINTER(vp)]
        L.sgpu_filter_create_columns_host.argtypes = [vp, vp, C.c_uint32, C.c_uint32, vp, C.c_uint32, vp, C.c_uint32, C.POINTER(vp)]
        L.sgpu_facet_counts.argtypes = [vp, C.c_uint32, C.c_uint32, vp, C.c_uint32, vp, vp, C.POINTER(C.c_uint32),
                                        C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.sgpu_facet_counts_host.argtypes = [vp, C.c_uint32, vp, C.c_uint32, C.c_uint32, vp, vp, C.POINTER(C.c_uint32),
                                             C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        u64p = C.POINTER(C.c_uint64)
        L.sgpu_column_stats.argtypes = [vp, C.c_uint32, C.c_uint32, vp, C.POINTER(ColumnStats)]
        L.sgpu_column_stats_host.argtypes = [vp, C.c_uint32, vp, C.c_uint32, C.POINTER(ColumnStats)]
        L.sgpu_column_histogram.argtypes = [vp, C.c_uint32, C.c_uint32, vp, vp, C.c_uint32, vp, u64p, u64p, u64p, u64p]
        L.sgpu_column_histogram_host.argtypes = [vp, C.c_uint32, vp, vp, C.c_uint32, C.c_uint32, vp, u64p, u64p, u64p, u64p]
        L.sgpu_column_top.argtypes = [vp, C.c_uint32, C.c_uint32, vp, C.c_uint32, C.c_uint32, vp, vp, C.POINTER(C.c_uint32), u64p, u64p]
        L.sgpu_column_top_host.argtypes = [vp, C.c_uint32, vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, C.POINTER(C.c_uint32), u64p,
                                           u64p]
        L.sgpu_filter_get_bits.argtypes = [vp, vp, C.c_uint64, C.POINTER(C.c_uint64)]
        L.sgpu_filter_count.argtypes = [vp]
        L.sgpu_filter_count.restype = C.c_uint64
        L.sgpu_filter_device_bytes.argtypes = [vp]
        L.sgpu_filter_device_bytes.restype = C.c_uint64
        L.sgpu_filter_destroy.argtypes = [vp]
        L.sgpu_filter_destroy.restype = None
        L.sgpu_search_filtered.argtypes = [vp, vp, vp, C.c_uint32, C.POINTER(SearchParams), vp, vp,
                                           C.POINTER(C.c_uint32), vp]
        L.sgpu_batch_search_filtered.argtypes = [vp, vp, vp, vp, C.c_uint32, C.POINTER(SearchParams), vp, vp, vp, vp]
        L.sgpu_exact_search_filtered.argtypes = [vp, vp, vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp, vp]
        L.sgpu_exact_search_device_filtered.argtypes = [vp, C.c_uint32, vp, vp, vp, C.c_uint32, C.c_uint32, vp, vp, vp,
                                                        vp]
        L.sgpu_score_documents.argtypes = [vp, C.c_uint32, vp, vp, vp, C.c_uint32, vp, vp, vp]
        L.sgpu_score_documents_host.argtypes = [vp, vp, vp, vp, C.c_uint32, vp, vp, C.c_uint32, vp]
        L.sgpu_rerank_documents.argtypes = [vp, C.c_uint32, vp, vp, vp, C.c_uint32, vp, vp, C.c_uint32, vp, vp, vp]
        L.sgpu_rerank_documents_host.argtypes = [vp, vp, vp, vp, C.c_uint32, vp, vp, C.c_uint32, C.c_uint32, vp, vp, vp]
        L.sgpu_explain_documents.argtypes = [vp, C.c_uint32, vp, vp, vp, C.c_uint32, vp, vp, C.c_uint32] + [vp] * 6
        L.sgpu_explain_documents_host.argtypes = [vp, vp, vp, vp, C.c_uint32, vp, vp, C.c_uint32, C.c_uint32] + [vp] * 6
        L.sgpu_expand_queries.argtypes = [vp, C.c_uint32, vp, vp, vp, C.c_uint32, vp, vp, vp, C.c_float, C.c_uint32, vp, vp, vp]
        L.sgpu_expand_queries_host.argtypes = [vp, vp, vp, vp, C.c_uint32, vp, vp, vp, C.c_float, C.c_uint32, C.c_uint32, vp, vp,
                                               vp]
        L.sgpu_diversify_documents.argtypes = [vp, C.c_uint32, vp, vp, vp, C.c_uint32, vp, vp, C.c_float, C.c_float, C.c_uint32,
                                               vp, vp, vp, vp]
        L.sgpu_diversify_documents_host.argtypes = [vp, vp, vp, vp, C.c_uint32, vp, vp, C.c_float, C.c_float, C.c_uint32,
                                                    C.c_uint32, vp, vp, vp, vp]
        L.sgpu_collapse_documents.argtypes = [vp, C.c_uint32, vp, vp, vp, C.c_uint32, vp, vp, vp, C.c_uint32, C.c_uint32] + [vp] * 6
        L.sgpu_collapse_documents_host.argtypes = [vp, vp, vp, vp, C.c_uint32, vp, vp, vp, C.c_uint32, C.c_uint32,
                                                   C.c_uint32] + [vp] * 6
        L.sgpu_fuse_documents.argtypes = [vp, C.c_uint32, vp, vp, vp, C.c_uint32, vp, vp, vp, C.c_uint32, C.c_float, C.c_float,
                                          C.c_float, C.c_uint32] + [vp] * 7
        L.sgpu_fuse_documents_host.argtypes = [vp, vp, vp, vp, C.c_uint32, vp, vp, vp, C.c_uint32, C.c_float, C.c_float, C.c_float,
                                               C.c_uint32, C.c_uint32] + [vp] * 7
        L.sgpu_synth_generate.argtypes = [C.POINTER(SynthSpec), vp, vp, vp, C.c_uint64, vp, vp, vp,
                                          C.POINTER(C.c_uint64)]
        L.sgpu_dataset_read.argtypes = [C.c_char_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), vp, vp, vp]
        L.sgpu_dataset_write.argtypes = [C.c_char_p, C.c_uint64, vp, vp, vp]
        L.sgpu_results_write_tsv.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, vp, vp, vp]
        if L.sgpu_abi_version() != ABI_VERSION:
            raise ImportError("libseismic_hip.so ABI version mismatch")
        _lib = L
    return _lib


def check(status):
    if status != SGPU_OK:
        raise SeismicHipError(status, lib().sgpu_last_error().decode("utf-8", "replace"))


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def build_info():
    """What the loaded library says it was built from (sgpu_build_info)."""
    return lib().sgpu_build_info().decode("utf-8", "replace")


def source_fingerprint(root=None):
    """The fingerprint sgpu_build_info() carries, recomputed from a source tree (default: the one this module lives in):
    first 64 bits of the SHA-256 of seismic_amd/csrc/{*.hip,*.cpp,*.hpp,*.inc} by name, the Makefile, include/*.h by name -
    the order of SOURCES in seismic_amd/csrc/Makefile."""
    import glob
    import hashlib
    pkg = os.path.join(root, "seismic_amd") if root else os.path.dirname(os.path.abspath(__file__))
    csrc = os.path.join(pkg, "csrc")
    files = sorted((p for ext in ("hip", "cpp", "hpp", "inc") for p in glob.glob(os.path.join(csrc, "*." + ext))), key=os.path.basename)
    files += [os.path.join(csrc, "Makefile")] + sorted(glob.glob(os.path.join(os.path.dirname(pkg), "include", "*.h")), key=os.path.basename)
    h = hashlib.sha256()
    for p in files:
        with open(p, "rb") as f:
            h.update(f.read())
    return h.hexdigest()[:16]


def device_count():
    n = C.c_int32(0)
    st = lib().sgpu_device_count(C.byref(n))
    return n.value if st == SGPU_OK else 0


# sgpu_debug_launch_config (include/seismic_hip_testing.h): the words it takes, with the values of an MI355X and of a
# launch nobody described further, and the words it returns
LAUNCH_CONFIG_IN = dict(n_cu=256, max_lds=160 * 1024, comp_width=2, value_type=0, dim=30522, val_scale_bits=0, coop_broken=0,
                        nq=1, max_nnz=32, k_max=1024, staged=0, has_plan=1, dots_cap=1, max_nb=0, max_list_nb=1, hash_ok=0,
                        target_list_nb=0, k=10, query_cut=4, n_knn=0, first_sorted=0, mode=0, occupancy_grid=0)
LAUNCH_CONFIG_OUT = ("q_comp q_val q_sc q_bits q_rank sel rt_start rt_mid rt_pre dots order uni part heap st qc qn qg dots_cap total "
                     "p_k p_query_cut p_heap_factor_bits p_first_sorted p_mode items_max items_init items_min rblocks_max p_n_knn "
                     "target_list p_val_scale_bits queue_base p_ring "
                     "lookup block lds_bytes counted streamed ring coop max_pos max_cand chunk chunk_min min_items first_reach "
                     "idle_min idle_ratio poll_sleep coop_grid grid grid_uncapped board_slots board_pos board_cand board_trace "
                     "board_total").split()


def debug_launch_config(heap_factor=1.0, **fields):
    """The launch configuration the library would choose (test hook, no device): fields override LAUNCH_CONFIG_IN, the
    SGPU_* knobs are read from the environment. Returns the output words by name; SeismicHipError where a launch fails."""
    unknown = set(fields) - set(LAUNCH_CONFIG_IN)
    if unknown:
        raise TypeError("unknown launch fact(s): %s" % ", ".join(sorted(unknown)))
    w = np.array([int(fields.get(name, dflt)) for name, dflt in LAUNCH_CONFIG_IN.items()], np.uint32)
    out = np.zeros(len(LAUNCH_CONFIG_OUT), np.uint32)
    fn = lib().sgpu_debug_launch_config
    fn.argtypes = [C.c_void_p, C.c_uint32, C.c_float, C.c_void_p, C.c_uint32]
    check(fn(_p(w), len(w), float(heap_factor), _p(out), len(out)))
    return dict(zip(LAUNCH_CONFIG_OUT, (int(x) for x in out)))


def debug_cut_rule(shared, device_plans):
    """(chunk_min, chunk_max) as this process cuts an entry-point call (test hook sgpu_debug_cut_rule, no device)."""
    out = np.zeros(2, np.uint32)
    fn = lib().sgpu_debug_cut_rule
    fn.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p]
    check(fn(int(shared), int(device_plans), _p(out)))
    return int(out[0]), int(out[1])


def debug_plan_seeds(index, q_off, comps, vals, query_cut):
    """(hash_ok, seeds [nq] u32) of the host's launch plan of a batch against `index` (test hook sgpu_debug_plan_seeds, no
    device): whether a launch may take the hashed query lookup, and every query's seed as the header describes the entries."""
    q_off, comps, vals = _csr(q_off, comps, vals)
    nq = len(q_off) - 1
    ok, seeds = C.c_uint32(0), np.zeros(max(nq, 1), np.uint32)
    fn = lib().sgpu_debug_plan_seeds
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.c_void_p]
    check(fn(index.h, _p(q_off), _p(comps), _p(vals), nq, int(query_cut), C.byref(ok), _p(seeds)))
    return int(ok.value), seeds[:nq]


def debug_lane_variant(index, lane=-1, replica=0):
    """dict(lookup, streamed, coop, counted) of the last search launch of a lane of `replica` - its main lane (lane < 0: what
    DeviceBatch.run / run_counted launch on) or chunk pool lane `lane` - or None where the lane has launched nothing (test
    hook sgpu_debug_lane_variant)."""
    out = np.zeros(4, np.uint32)
    fn = lib().sgpu_debug_lane_variant
    fn.restype = C.c_uint32
    fn.argtypes = [C.c_void_p, C.c_uint32, C.c_int32, C.c_void_p]
    if not fn(index.h, int(replica), int(lane), _p(out)):
        return None
    return dict(zip(("lookup", "streamed", "coop", "counted"), (int(x) for x in out)))


def debug_lane_chunk(index, lane):
    """dict(nq, q_base, planned_by, query_cut) of the last chunk pool lane `lane` of replica 0 served (planned_by: 0 the host,
    1 the device, 2 nobody), or None (test hook sgpu_debug_lane_chunk)."""
    info = np.zeros(4, np.uint32)
    fn = lib().sgpu_debug_lane_chunk
    fn.restype = C.c_uint32
    fn.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32]
    if not fn(index.h, int(lane), _p(info), None, 0):
        return None
    return dict(zip(("nq", "q_base", "planned_by", "query_cut"), (int(x) for x in info)))


def params(k, query_cut, heap_factor, first_sorted, n_knn=0):
    return SearchParams(k=int(k), query_cut=int(query_cut), heap_factor=float(heap_factor),
                        n_knn=int(n_knn), first_sorted=1 if first_sorted else 0)


def _csr(q_off, comps, vals):
    return (np.ascontiguousarray(q_off, np.uint64), np.ascontiguousarray(comps, np.uint32),
            np.ascontiguousarray(vals, np.float32))


class NativeIndex:
    """Owns an sgpu_index handle."""

    def __init__(self, handle):
        self.h = C.c_void_p(handle)
        self._desc = None

    @classmethod
    def build(cls, comp_width, dim, offsets, comps, vals, cfg=None):
        cfg = cfg or BuildConfig.defaults()
        offsets = np.ascontiguousarray(offsets, np.uint64)
        cdt = np.uint16 if comp_width == 2 else np.uint32
        comps = np.ascontiguousarray(comps, cdt)
        vals = np.ascontiguousarray(vals, np.float32)
        h = C.c_void_p()
        check(lib().sgpu_index_build(comp_width, len(offsets) - 1, dim, _p(offsets), _p(comps), _p(vals),
                                     C.byref(cfg), C.byref(h)))
        return cls(h.value)

    @classmethod
    def from_desc(cls, desc):
        h = C.c_void_p()
        check(lib().sgpu_index_create(C.byref(desc), C.byref(h)))
        return cls(h.value)

    @classmethod
    def load(cls, path):
        h = C.c_void_p()
        check(lib().sgpu_index_load(os.fsencode(path), C.byref(h)))
        return cls(h.value)

    def save(self, path):
        check(lib().sgpu_index_save(self.h, os.fsencode(path)))

    @property
    def desc(self):
        if self._desc is None:
            d = IndexDesc()
            check(lib().sgpu_index_get_desc(self.h, C.byref(d)))
            self._desc = d
        return self._desc

    def convert(self, value_type):
        """InvertedIndexBase::convert_dataset_into: a new index whose forward index stores the document
        values as `value_type` (0 = f16, 1 = fixed-u8, 2 = DotVByte: fixed-u8 + compressed component stream);
        lists, blocks and summaries are shared."""
        h = C.c_void_p()
        check(lib().sgpu_index_convert(self.h, int(value_type), C.byref(h)))
        return NativeIndex(h.value)

    def upload(self, device=0):
        check(lib().sgpu_index_upload(self.h, int(device)))
        return self

    def upload_many(self, devices):
        """Replicate on several devices (replica 0 from the host, the others GPU to GPU);
        batch_search then shards a batch over the replicas."""
        ids = np.ascontiguousarray(devices, np.int32)
        check(lib().sgpu_index_upload_many(self.h, _p(ids), len(ids)))
        return self

    @property
    def replicas(self):
        return int(lib().sgpu_index_replicas(self.h))

    # ---- kNN graph (reference Knn, src/inverted_index.rs:430-594) ----
    def build_knn(self, nknn):
        """Knn::new on the GPU: every document searched as a query, batched through the kernel."""
        check(lib().sgpu_index_build_knn(self.h, int(nknn)))

    def set_knn(self, neighbours, knn_dim):
        a = np.ascontiguousarray(neighbours, np.uint32)
        check(lib().sgpu_index_set_knn(self.h, _p(a), len(a), int(knn_dim)))

    def get_knn(self):
        ptr, n, dim = C.c_void_p(), C.c_uint64(0), C.c_uint32(0)
        check(lib().sgpu_index_get_knn(self.h, C.byref(ptr), C.byref(n), C.byref(dim)))
        if n.value == 0:
            return np.zeros(0, np.uint32), 0
        arr = np.ctypeslib.as_array((C.c_uint32 * n.value).from_address(ptr.value)).copy()
        return arr, int(dim.value)

    def device_bytes(self):
        return int(lib().sgpu_index_device_bytes(self.h))

    def make_filter(self, ids):
        """A document filter (sgpu_filter_create): `ids` are the allowed document ids (repeats allowed), or a boolean
        mask of length n_docs. Pass it as filter= to search, batch_search, exact_search and exact_search_device."""
        return NativeFilter(self, ids)

    def make_term_filter(self, clauses, min_should=0, within=None, replica=0, host=False, num_threads=0):
        """A term filter (sgpu_filter_create_terms[_host]): the documents that satisfy the must / must-not / should
        `clauses`, each a (component, occur, min_weight) triple (occur one of _abi.SGPU_TERM_*; min_weight -inf: any
        stored entry) or a numpy array of them with TERM_CLAUSE_DTYPE. within: a NativeFilter to intersect with.
        host=False: on the device of `replica`, from its exact file; host=True: the host twin that defines the bits."""
        cl = term_clauses(clauses)
        wh = None if within is None else _filter_handle(within)
        h = C.c_void_p()
        if host:
            check(lib().sgpu_filter_create_terms_host(self.h, _p(cl), len(cl), int(min_should), wh, int(num_threads), C.byref(h)))
        else:
            check(lib().sgpu_filter_create_terms(self.h, int(replica), _p(cl), len(cl), int(min_should), wh, C.byref(h)))
        return NativeFilter._adopt(self, h)

    # ---- document columns: range and set filters, facet counts ----
    def set_column(self, slot, values, dtype=None):
        """sgpu_index_set_column: one 32-bit value per document in slot `slot` (0..15), in the index's document order.
        The column's type follows `dtype`, or the array's: unsigned -> U32, signed -> I32, floating -> F32 (a bare list
        of Python ints is U32). values=None drops the column."""
        if values is None:
            check(lib().sgpu_index_set_column(self.h, int(slot), 0, None, 0))
            return
        a = column_array(values, dtype)
        check(lib().sgpu_index_set_column(self.h, int(slot), COLUMN_KINDS[a.dtype.kind][0], _p(a), len(a)))

    def get_column(self, slot):
        """sgpu_index_get_column: a copy of the column in `slot` with its type's dtype (uint32 / int32 / float32, the
        stored bits unchanged), or None for an empty slot."""
        t, ptr, n = C.c_uint32(0), C.c_void_p(), C.c_uint64(0)
        check(lib().sgpu_index_get_column(self.h, int(slot), C.byref(t), C.byref(ptr), C.byref(n)))
        if not ptr.value and n.value == 0:
            return None
        raw = np.ctypeslib.as_array((C.c_uint32 * n.value).from_address(ptr.value)).copy() if n.value else np.zeros(0, np.uint32)
        return raw.view(COLUMN_DTYPES[int(t.value)])

    def make_column_filter(self, clauses, min_should=0, set_values=(), within=None, replica=0, host=False, num_threads=0):
        """A column filter (sgpu_filter_create_columns[_host]): `clauses` are (slot, occur, op, lo_bits, hi_bits, set_begin,
        set_count) rows or an array of COLUMN_CLAUSE_DTYPE, `set_values` the u32 bit patterns the IN clauses point into.
        within: a NativeFilter to intersect with. host=False: one kernel on the device of `replica`; host=True: the host
        twin that defines the words."""
        cl = column_clauses(clauses)
        sv = np.ascontiguousarray(set_values, np.uint32)
        wh = None if within is None else _filter_handle(within)
        h = C.c_void_p()
        if host:
            check(lib().sgpu_filter_create_columns_host(self.h, _p(cl), len(cl), int(min_should), _p(sv), len(sv), wh,
                                                        int(num_threads), C.byref(h)))
        else:
            check(lib().sgpu_filter_create_columns(self.h, int(replica), _p(cl), len(cl), int(min_should), _p(sv), len(sv), wh,
                                                   C.byref(h)))
        return NativeFilter._adopt(self, h)

    def facet_counts(self, slot, filter=None, t=10, replica=0, host=False, num_threads=0):
        """sgpu_facet_counts[_host]: the t most frequent values of the U32 column `slot` among the filter's documents
        (None: all), by (count descending, value ascending). Returns (values u32 [n], counts u64 [n], distinct, docs)."""
        t = int(t)
        if not 0 <= t <= 0xffffffff:
            raise ValueError("t = %r out of range" % t)
        vals, cnts = np.zeros(max(t, 1), np.uint32), np.zeros(max(t, 1), np.uint64)
        n, distinct, docs = C.c_uint32(0), C.c_uint64(0), C.c_uint64(0)
        fh = None if filter is None else _filter_handle(filter)
        if host:
            check(lib().sgpu_facet_counts_host(self.h, int(slot), fh, t, int(num_threads), _p(vals), _p(cnts), C.byref(n),
                                               C.byref(distinct), C.byref(docs)))
        else:
            check(lib().sgpu_facet_counts(self.h, int(replica), int(slot), fh, t, _p(vals), _p(cnts), C.byref(n),
                                          C.byref(distinct), C.byref(docs)))
        if vals[n.value:t].any() or cnts[n.value:t].any():
            raise RuntimeError("facet rows past out_n are not zero")
        return vals[:n.value], cnts[:n.value], int(distinct.value), int(docs.value)

    # ---- column aggregations: statistics, histograms, sorted top-k ----
    def column_stats(self, slot, filter=None, replica=0, host=False, num_threads=0):
        """sgpu_column_stats[_host] over the filter's documents (None: all) -> dict(docs, valid, min_bits, max_bits, sum_int,
        sum, sum_bits): the struct's fields as Python ints, `sum` as a float and `sum_bits` its binary64 pattern."""
        out = ColumnStats()
        fh = None if filter is None else _filter_handle(filter)
        if host:
            check(lib().sgpu_column_stats_host(self.h, int(slot), fh, int(num_threads), C.byref(out)))
        else:
            check(lib().sgpu_column_stats(self.h, int(replica), int(slot), fh, C.byref(out)))
        return dict(docs=int(out.docs), valid=int(out.valid), min_bits=int(out.min_bits), max_bits=int(out.max_bits),
                    sum_int=int(out.sum_int), sum=float(out.sum), sum_bits=int(np.array([out.sum], np.float64).view(np.uint64)[0]))

    def column_histogram(self, slot, edges_bits, filter=None, replica=0, host=False, num_threads=0):
        """sgpu_column_histogram[_host]: `edges_bits` are the edges' u32 bit patterns in the column's type, strictly
        ascending in its order. Returns (counts u64 [n_edges - 1], below, above, nan, docs)."""
        e = np.ascontiguousarray(edges_bits, np.uint32).ravel()
        counts = np.zeros(max(len(e) - 1, 1), np.uint64)
        below, above, nan, docs = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        fh = None if filter is None else _filter_handle(filter)
        outs = (_p(counts), C.byref(below), C.byref(above), C.byref(nan), C.byref(docs))
        if host:
            check(lib().sgpu_column_histogram_host(self.h, int(slot), fh, _p(e), len(e), int(num_threads), *outs))
        else:
            check(lib().sgpu_column_histogram(self.h, int(replica), int(slot), fh, _p(e), len(e), *outs))
        return counts[:len(e) - 1], int(below.value), int(above.value), int(nan.value), int(docs.value)

    def column_top(self, slot, t=10, order=0, filter=None, replica=0, host=False, num_threads=0):
        """sgpu_column_top[_host]: the first min(t, valid) documents of the filter (None: all) by (value ascending for order
        0, descending for 1; id ascending). Returns (doc_ids u32 [n], value_bits u32 [n], valid, docs)."""
        t, order = int(t), int(order)
        if not 0 <= t <= 0xffffffff or not 0 <= order <= 0xffffffff:
            raise ValueError("t = %r / order = %r out of range" % (t, order))
        ids, vals = np.zeros(max(t, 1), np.uint32), np.zeros(max(t, 1), np.uint32)
        n, valid, docs = C.c_uint32(0), C.c_uint64(0), C.c_uint64(0)
        fh = None if filter is None else _filter_handle(filter)
        outs = (_p(ids), _p(vals), C.byref(n), C.byref(valid), C.byref(docs))
        if host:
            check(lib().sgpu_column_top_host(self.h, int(slot), fh, t, order, int(num_threads), *outs))
        else:
            check(lib().sgpu_column_top(self.h, int(replica), int(slot), fh, t, order, *outs))
        if ids[n.value:t].any() or vals[n.value:t].any():
            raise RuntimeError("top rows past out_n are not zero")
        return ids[:n.value], vals[:n.value], int(valid.value), int(docs.value)

    def debug_column_agg_stats(self, replica=0):
        """sgpu_debug_column_agg_stats (test hook): what the last column aggregations on `replica` measured."""
        out = np.zeros(10, np.float64)
        fn = lib().sgpu_debug_column_agg_stats
        fn.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
        check(fn(self.h, int(replica), _p(out)))
        return dict(stats_ms=float(out[0]), hist_ms=float(out[1]), top_ms=float(out[2]), stats_grid=int(out[3]), hist_grid=int(out[4]),
                    top_grid=int(out[5]), agg_tile=int(out[6]), top_passes=int(out[7]), hist_docs_per_wg=int(out[8]),
                    top_docs_per_wg=int(out[9]))

    def debug_column_stats(self, replica=0):
        """sgpu_debug_column_stats (test hook): what the last column calls on `replica` measured."""
        out = np.zeros(8, np.float64)
        fn = lib().sgpu_debug_column_stats
        fn.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
        check(fn(self.h, int(replica), _p(out)))
        return dict(filter_ms=float(out[0]), facet_ms=float(out[1]), filter_grid=int(out[2]), facet_grid=int(out[3]),
                    filter_docs_per_wg=int(out[4]), facet_docs_per_wg=int(out[5]), facet_path=int(out[6]), column_bytes=int(out[7]))

    def debug_posting_view(self, replica=0, filter=None):
        """sgpu_debug_posting_view (a test hook: needs SGPU_TEST_HOOKS=1): the posting arrays a search on `replica` walks,
        read back from the device, as a dict of numpy arrays - block_post_start u32 [n_blocks + 1], post_ref u64, post_doc u32,
        knn u32 (empty without a graph); with a filter, those of its view there plus bits u32 and count."""
        L = lib()
        L.sgpu_debug_posting_view.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p,
                                              C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p]
        fh = None if filter is None else _filter_handle(filter)
        sizes = np.zeros(5, np.uint64)
        check(L.sgpu_debug_posting_view(self.h, fh, int(replica), None, 0, None, None, 0, None, 0, None, 0, _p(sizes)))
        n_starts, n_post, n_knn, n_bits = (int(x) for x in sizes[:4])
        bps, ref, doc = np.zeros(n_starts, np.uint32), np.zeros(max(n_post, 1), np.uint64), np.zeros(max(n_post, 1), np.uint32)
        knn, bits = np.zeros(max(n_knn, 1), np.uint32), np.zeros(max(n_bits, 1), np.uint32)
        got = np.zeros(5, np.uint64)
        check(L.sgpu_debug_posting_view(self.h, fh, int(replica), _p(bps), n_starts, _p(ref), _p(doc), n_post, _p(knn), n_knn,
                                        _p(bits), n_bits, _p(got)))
        if not np.array_equal(got, sizes):
            raise RuntimeError("the view changed between the two calls: sizes %s, then %s" % (sizes, got))
        out = dict(block_post_start=bps, post_ref=ref[:n_post], post_doc=doc[:n_post], knn=knn[:n_knn])
        if filter is not None:
            out.update(bits=bits[:n_bits], count=int(sizes[4]))
        return out

    def stream_stats(self):
        """(documents, elements) a DotVByte index keeps in the raw record form; (0, 0) for the other value types."""
        a, b = C.c_uint64(0), C.c_uint64(0)
        lib().sgpu_index_stream_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        check(lib().sgpu_index_stream_stats(self.h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def close(self):
        if self.h:
            lib().sgpu_index_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- search ----
    def search(self, comps, vals, k, query_cut, heap_factor, first_sorted=False, n_knn=0, filter=None):
        comps = np.ascontiguousarray(comps, np.uint32)
        vals = np.ascontiguousarray(vals, np.float32)
        sc = np.zeros(max(k, 1), np.float32)
        ids = np.zeros(max(k, 1), np.uint64)
        n = C.c_uint32(0)
        p = params(k, query_cut, heap_factor, first_sorted, n_knn)
        if filter is None:
            check(lib().sgpu_search(self.h, _p(comps), _p(vals), len(comps), C.byref(p), _p(sc), _p(ids),
                                    C.byref(n)))
        else:
            check(lib().sgpu_search_filtered(self.h, _p(comps), _p(vals), len(comps), C.byref(p), _p(sc), _p(ids),
                                             C.byref(n), _filter_handle(filter)))
        return sc[: n.value].copy(), ids[: n.value].copy()

    def batch_search(self, q_off, comps, vals, k, query_cut, heap_factor, first_sorted=False, n_knn=0, out=None,
                     filter=None):
        """out: optional (scores f32 [nq, k], ids u64 [nq, k], n u32 [nq]) to receive the rows (no allocation per call)."""
        q_off, comps, vals = _csr(q_off, comps, vals)
        nq = len(q_off) - 1
        if out is not None:
            sc, ids, n = out
            assert sc.shape == (nq, k) and ids.shape == (nq, k) and len(n) >= nq
            assert sc.dtype == np.float32 and ids.dtype == np.uint64 and n.dtype == np.uint32
            assert sc.flags.c_contiguous and ids.flags.c_contiguous and n.flags.c_contiguous
        else:
            sc = np.zeros((nq, max(k, 1)), np.float32)
            ids = np.zeros((nq, max(k, 1)), np.uint64)
            n = np.zeros(max(nq, 1), np.uint32)
        p = params(k, query_cut, heap_factor, first_sorted, n_knn)
        if filter is None:
            check(lib().sgpu_batch_search(self.h, _p(q_off), _p(comps), _p(vals), nq, C.byref(p), _p(sc),
                                          _p(ids), _p(n)))
        else:
            check(lib().sgpu_batch_search_filtered(self.h, _p(q_off), _p(comps), _p(vals), nq, C.byref(p), _p(sc),
                                                   _p(ids), _p(n), _filter_handle(filter)))
        return sc, ids, n[:nq]

    def search_sequential(self, q_off, comps, vals, k, query_cut, heap_factor, first_sorted=False, n_knn=0, per_query=False):
        """The reference's AQT loop (src/bin/perf_inverted_index.rs:184-216) natively: one sgpu_search per
        query, timed around the loop. Returns (scores, ids, n, mean microseconds per query, the 8-entry
        host-side phase breakdown in microseconds per query); with per_query=True a sixth element, the wall
        time of every call in microseconds."""
        q_off, comps, vals = _csr(q_off, comps, vals)
        nq = len(q_off) - 1
        sc = np.zeros((nq, max(k, 1)), np.float32)
        ids = np.zeros((nq, max(k, 1)), np.uint64)
        n = np.zeros(max(nq, 1), np.uint32)
        mean = C.c_double(0.0)
        phases = np.zeros(8, np.float64)
        p = params(k, query_cut, heap_factor, first_sorted, n_knn)
        if per_query:
            each = np.zeros(max(nq, 1), np.float64)
            check(lib().sgpu_search_sequential_timed(self.h, _p(q_off), _p(comps), _p(vals), nq, C.byref(p), _p(sc), _p(ids),
                                                     _p(n), C.byref(mean), _p(phases), _p(each)))
            return sc, ids, n[:nq], mean.value, phases, each[:nq]
        check(lib().sgpu_search_sequential(self.h, _p(q_off), _p(comps), _p(vals), nq, C.byref(p), _p(sc), _p(ids),
                                           _p(n), C.byref(mean), _p(phases)))
        return sc, ids, n[:nq], mean.value, phases

    def summary_distances(self, list_id, comps, vals):
        comps = np.ascontiguousarray(comps, np.uint32)
        vals = np.ascontiguousarray(vals, np.float32)
        out = np.zeros(65536, np.float32)
        n = C.c_uint32(0)
        check(lib().sgpu_summary_distances(self.h, int(list_id), _p(comps), _p(vals), len(comps), _p(out),
                                           C.byref(n)))
        return out[: n.value].copy()

    def exact_search(self, q_off, comps, vals, k, num_threads=0, filter=None):
        q_off, comps, vals = _csr(q_off, comps, vals)
        nq = len(q_off) - 1
        sc = np.zeros((nq, k), np.float32)
        ids = np.zeros((nq, k), np.uint64)
        n = np.zeros(max(nq, 1), np.uint32)
        if filter is None:
            check(lib().sgpu_exact_search(self.h, _p(q_off), _p(comps), _p(vals), nq, k, num_threads, _p(sc),
                                          _p(ids), _p(n)))
        else:
            check(lib().sgpu_exact_search_filtered(self.h, _p(q_off), _p(comps), _p(vals), nq, k, num_threads, _p(sc),
                                                   _p(ids), _p(n), _filter_handle(filter)))
        return sc, ids, n[:nq]

    def exact_search_device(self, q_off, comps, vals, k, replica=0, filter=None):
        """exact_search on the device of an uploaded replica: the same results, bit for bit (the first call
        builds the replica's exact file, kept until the index is destroyed)."""
        q_off, comps, vals = _csr(q_off, comps, vals)
        nq = len(q_off) - 1
        sc = np.zeros((nq, k), np.float32)
        ids = np.zeros((nq, k), np.uint64)
        n = np.zeros(max(nq, 1), np.uint32)
        if filter is None:
            check(lib().sgpu_exact_search_device(self.h, int(replica), _p(q_off), _p(comps), _p(vals), nq, k, _p(sc),
                                                 _p(ids), _p(n)))
        else:
            check(lib().sgpu_exact_search_device_filtered(self.h, int(replica), _p(q_off), _p(comps), _p(vals), nq, k,
                                                          _p(sc), _p(ids), _p(n), _filter_handle(filter)))
        return sc, ids, n[:nq]

    # ---- scores of caller-given documents ----
    def score_documents(self, q_off, comps, vals, cand_off, cand_ids, replica=0):
        """sgpu_score_documents: query q's candidates are cand_ids[cand_off[q] : cand_off[q + 1]] (native document ids, any
        order, repeats allowed); returns one f32 per candidate - the score sgpu_search returns for that document, bit for
        bit. Runs on the device of `replica`."""
        q_off, comps, vals = _csr(q_off, comps, vals)
        cand_off = np.ascontiguousarray(cand_off, np.uint64)
        cand_ids = np.ascontiguousarray(cand_ids, np.uint64)
        out = np.zeros(max(len(cand_ids), 1), np.float32)
        ids = cand_ids if len(cand_ids) else np.zeros(1, np.uint64)
        check(lib().sgpu_score_documents(self.h, int(replica), _p(q_off), _p(comps), _p(vals), len(q_off) - 1,
                                         _p(cand_off), _p(ids), _p(out)))
        return out[: len(cand_ids)]

    def score_documents_host(self, q_off, comps, vals, cand_off, cand_ids, num_threads=0):
        """sgpu_score_documents_host: the same scores on the host cores (needs no upload), bit-identical."""
        q_off, comps, vals = _csr(q_off, comps, vals)
        cand_off = np.ascontiguousarray(cand_off, np.uint64)
        cand_ids = np.ascontiguousarray(cand_ids, np.uint64)
        out = np.zeros(max(len(cand_ids), 1), np.float32)
        ids = cand_ids if len(cand_ids) else np.zeros(1, np.uint64)
        check(lib().sgpu_score_documents_host(self.h, _p(q_off), _p(comps), _p(vals), len(q_off) - 1, _p(cand_off),
                                              _p(ids), int(num_threads), _p(out)))
        return out[: len(cand_ids)]

    # ---- the k best of each query's candidates ----
    @staticmethod
    def _rerank_buffers(q_off, comps, vals, cand_off, cand_ids, k):
        q_off, comps, vals = _csr(q_off, comps, vals)
        cand_off = np.ascontiguousarray(cand_off, np.uint64)
        cand_ids = np.ascontiguousarray(cand_ids, np.uint64)
        nq, k = len(q_off) - 1, int(k)
        if not 0 <= k < 2 ** 32:
            raise ValueError("k = %d" % k)
        rows = (max(nq, 1), k if 1 <= k <= 1024 else 1)   # (a k the library refuses: nothing is written)
        sc = np.zeros(rows, np.float32)
        ids = np.zeros(rows, np.uint64)
        n = np.zeros(max(nq, 1), np.uint32)
        cand = cand_ids if len(cand_ids) else np.zeros(1, np.uint64)
        return q_off, comps, vals, cand_off, cand, nq, k, sc, ids, n

    def rerank_documents(self, q_off, comps, vals, cand_off, cand_ids, k, replica=0):
        """sgpu_rerank_documents: per query the k best DISTINCT documents among its candidates (given as for
        score_documents), score descending, ties by id ascending, scored and selected on the device of `replica`.
        Returns (scores f32 [nq, k], ids u64 [nq, k], n u32 [nq]); slots past n[q] are zero."""
        q_off, comps, vals, cand_off, cand, nq, k, sc, ids, n = self._rerank_buffers(q_off, comps, vals, cand_off, cand_ids, k)
        check(lib().sgpu_rerank_documents(self.h, int(replica), _p(q_off), _p(comps), _p(vals), nq, _p(cand_off), _p(cand),
                                          k, _p(sc), _p(ids), _p(n)))
        return sc[:nq], ids[:nq], n[:nq]

    def rerank_documents_host(self, q_off, comps, vals, cand_off, cand_ids, k, num_threads=0):
        """sgpu_rerank_documents_host: the same rows on the host cores (needs no upload)."""
        q_off, comps, vals, cand_off, cand, nq, k, sc, ids, n = self._rerank_buffers(q_off, comps, vals, cand_off, cand_ids, k)
        check(lib().sgpu_rerank_documents_host(self.h, _p(q_off), _p(comps), _p(vals), nq, _p(cand_off), _p(cand), k,
                                               int(num_threads), _p(sc), _p(ids), _p(n)))
        return sc[:nq], ids[:nq], n[:nq]

    # ---- the terms behind each candidate's score ----
    @staticmethod
    def _explain_buffers(q_off, comps, vals, cand_off, cand_ids, m):
        q_off, comps, vals = _csr(q_off, comps, vals)
        cand_off = np.ascontiguousarray(cand_off, np.uint64)
        cand_ids = np.ascontiguousarray(cand_ids, np.uint64)
        m = int(m)
        if not 0 <= m < 2 ** 32:
            raise ValueError("m = %d" % m)
        n = len(cand_ids)
        rows = (max(n, 1), m if 1 <= m <= 32 else 1)   # (an m the library refuses: nothing is written)
        out = (np.zeros(max(n, 1), np.float32), np.zeros(max(n, 1), np.uint32), np.zeros(rows, np.uint32),
               np.zeros(rows, np.float32), np.zeros(rows, np.float32), np.zeros(rows, np.float32))
        cand = cand_ids if n else np.zeros(1, np.uint64)
        return q_off, comps, vals, cand_off, cand, n, m, out

    def explain_documents(self, q_off, comps, vals, cand_off, cand_ids, m, replica=0):
        """sgpu_explain_documents: per candidate (given as for score_documents) its score, the number of terms query and
        document share, and the m <= 32 best of them - product descending in the order of the f32 bits' integer image,
        then component ascending -, computed on the device of `replica`. Returns (scores f32 [n], n_terms u32 [n],
        components u32 [n, m], query weights f32 [n, m], document values f32 [n, m], products f32 [n, m]); slots past
        min(m, n_terms) are zero."""
        q_off, comps, vals, cand_off, cand, n, m, out = self._explain_buffers(q_off, comps, vals, cand_off, cand_ids, m)
        check(lib().sgpu_explain_documents(self.h, int(replica), _p(q_off), _p(comps), _p(vals), len(q_off) - 1, _p(cand_off),
                                           _p(cand), m, *[_p(a) for a in out]))
        return tuple(a[:n] for a in out)

    def explain_documents_host(self, q_off, comps, vals, cand_off, cand_ids, m, num_threads=0):
        """sgpu_explain_documents_host: the same on the host cores (needs no upload), bit-identical."""
        q_off, comps, vals, cand_off, cand, n, m, out = self._explain_buffers(q_off, comps, vals, cand_off, cand_ids, m)
        check(lib().sgpu_explain_documents_host(self.h, _p(q_off), _p(comps), _p(vals), len(q_off) - 1, _p(cand_off), _p(cand),
                                                m, int(num_threads), *[_p(a) for a in out]))
        return tuple(a[:n] for a in out)

    # ---- Rocchio feedback queries ----
    @staticmethod
    def _expand_buffers(q_off, comps, vals, cand_off, cand_ids, cand_w, t):
        q_off, comps, vals = _csr(q_off, comps, vals)
        cand_off = np.ascontiguousarray(cand_off, np.uint64)
        cand_ids = np.ascontiguousarray(cand_ids, np.uint64)
        cand_w = np.ascontiguousarray(cand_w, np.float32)
        if len(cand_w) != len(cand_ids):
            raise ValueError("%d candidates but %d weights" % (len(cand_ids), len(cand_w)))
        nq, t = len(q_off) - 1, int(t)
        if not 0 <= t < 2 ** 32:
            raise ValueError("t = %d" % t)
        rows = (max(nq, 1), t if 1 <= t <= 1024 else 1)   # (a t the library refuses: nothing is written)
        oc, ov, n = np.zeros(rows, np.uint32), np.zeros(rows, np.float32), np.zeros(max(nq, 1), np.uint32)
        if not len(cand_ids):
            cand_ids, cand_w = np.zeros(1, np.uint64), np.zeros(1, np.float32)
        return q_off, comps, vals, cand_off, cand_ids, cand_w, nq, t, oc, ov, n

    def expand_queries(self, q_off, comps, vals, cand_off, cand_ids, cand_w, alpha, t, replica=0):
        """sgpu_expand_queries: per query the Rocchio table W = alpha * query + sum of cand_w[i] * document cand_ids[i] (the
        documents added in the order given, f32, see include/seismic_hip.h), its t <= 1024 heaviest components with
        W > 0 (ties: the smaller component) in ascending component order, built on the device of `replica`. Returns
        (components u32 [nq, t], values f32 [nq, t], n u32 [nq]); slots past n[q] are zero."""
        q_off, comps, vals, cand_off, cand, w, nq, t, oc, ov, n = self._expand_buffers(q_off, comps, vals, cand_off, cand_ids,
                                                                                      cand_w, t)
        check(lib().sgpu_expand_queries(self.h, int(replica), _p(q_off), _p(comps), _p(vals), nq, _p(cand_off), _p(cand), _p(w),
                                        float(alpha), t, _p(oc), _p(ov), _p(n)))
        return oc[:nq], ov[:nq], n[:nq]

    def expand_queries_host(self, q_off, comps, vals, cand_off, cand_ids, cand_w, alpha, t, num_threads=0):
        """sgpu_expand_queries_host: the same rows on the host cores (needs no upload), bit-identical."""
        q_off, comps, vals, cand_off, cand, w, nq, t, oc, ov, n = self._expand_buffers(q_off, comps, vals, cand_off, cand_ids,
                                                                                      cand_w, t)
        check(lib().sgpu_expand_queries_host(self.h, _p(q_off), _p(comps), _p(vals), nq, _p(cand_off), _p(cand), _p(w),
                                             float(alpha), t, int(num_threads), _p(oc), _p(ov), _p(n)))
        return oc[:nq], ov[:nq], n[:nq]

    def debug_expand_stats(self, replica=0):
        """sgpu_debug_expand_stats (test hook): what the last expand_queries call on `replica` measured."""
        out = np.zeros(8, np.float64)
        fn = lib().sgpu_debug_expand_stats
        fn.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
        check(fn(self.h, int(replica), _p(out)))
        return dict(kernel_ms=float(out[0]), launches=int(out[1]), dense=int(out[2]), grid=int(out[3]), block=int(out[4]),
                    lds=int(out[5]), table_bytes=int(out[6]))

    # ---- MMR selection of candidates ----
    @staticmethod
    def _diversify_buffers(q_off, comps, vals, cand_off, cand_ids, k):
        q_off, comps, vals = _csr(q_off, comps, vals)
        cand_off = np.ascontiguousarray(cand_off, np.uint64)
        cand_ids = np.ascontiguousarray(cand_ids, np.uint64)
        nq, k = len(q_off) - 1, int(k)
        if not 0 <= k < 2 ** 32:
            raise ValueError("k = %d" % k)
        rows = (max(nq, 1), k if 1 <= k <= 256 else 1)   # (a k the library refuses: nothing is written)
        sc, pen, ids = np.zeros(rows, np.float32), np.zeros(rows, np.float32), np.zeros(rows, np.uint64)
        n = np.zeros(max(nq, 1), np.uint32)
        cand = cand_ids if len(cand_ids) else np.zeros(1, np.uint64)
        return q_off, comps, vals, cand_off, cand, nq, k, sc, pen, ids, n

    def diversify_documents(self, q_off, comps, vals, cand_off, cand_ids, lam, mu, k, replica=0):
        """sgpu_diversify_documents: per query the greedy MMR selection of at most k <= 256 DISTINCT documents among its
        candidates (given as for score_documents, at most 2048 per query): round by round the candidate with the largest
        lam * score - mu * (largest similarity to anything selected before, at least 0), ties by id ascending, scored and
        selected on the device of `replica` (f32, see include/seismic_hip.h). Returns (scores f32 [nq, k], penalties f32
        [nq, k], ids u64 [nq, k], n u32 [nq]); slots past n[q] are zero."""
        q_off, comps, vals, cand_off, cand, nq, k, sc, pen, ids, n = self._diversify_buffers(q_off, comps, vals, cand_off,
                                                                                             cand_ids, k)
        check(lib().sgpu_diversify_documents(self.h, int(replica), _p(q_off), _p(comps), _p(vals), nq, _p(cand_off), _p(cand),
                                             float(lam), float(mu), k, _p(sc), _p(pen), _p(ids), _p(n)))
        return sc[:nq], pen[:nq], ids[:nq], n[:nq]

    def diversify_documents_host(self, q_off, comps, vals, cand_off, cand_ids, lam, mu, k, num_threads=0):
        """sgpu_diversify_documents_host: the same rows on the host cores (needs no upload), bit-identical."""
        q_off, comps, vals, cand_off, cand, nq, k, sc, pen, ids, n = self._diversify_buffers(q_off, comps, vals, cand_off,
                                                                                             cand_ids, k)
        check(lib().sgpu_diversify_documents_host(self.h, _p(q_off), _p(comps), _p(vals), nq, _p(cand_off), _p(cand),
                                                  float(lam), float(mu), k, int(num_threads), _p(sc), _p(pen), _p(ids), _p(n)))
        return sc[:nq], pen[:nq], ids[:nq], n[:nq]

    def debug_diversify_stats(self, replica=0):
        """sgpu_debug_diversify_stats (test hook): what the last diversify_documents call on `replica` measured."""
        out = np.zeros(8, np.float64)
        fn = lib().sgpu_debug_diversify_stats
        fn.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
        check(fn(self.h, int(replica), _p(out)))
        return dict(kernel_ms=float(out[0]), launches=int(out[1]), grid=int(out[2]), block=int(out[3]), lds=int(out[4]),
                    dense=int(out[5]), rounds=int(out[6]))

    # ---- the k best groups of each query's candidates ----
    @staticmethod
    def _collapse_buffers(q_off, comps, vals, cand_off, cand_ids, cand_groups, m, k):
        q_off, comps, vals = _csr(q_off, comps, vals)
        cand_off = np.ascontiguousarray(cand_off, np.uint64)
        cand_ids = np.ascontiguousarray(cand_ids, np.uint64)
        cand_groups = np.ascontiguousarray(cand_groups, np.uint32)
        if len(cand_groups) != len(cand_ids):
            raise ValueError("%d candidates but %d group keys" % (len(cand_ids), len(cand_groups)))
        nq, m, k = len(q_off) - 1, int(m), int(k)
        if not (0 <= k < 2 ** 32 and 0 <= m < 2 ** 32):
            raise ValueError("m = %d, k = %d" % (m, k))
        rows = (max(nq, 1), k if 1 <= k <= 1024 else 1)   # (a k the library refuses: nothing is written)
        out = (np.zeros(rows, np.uint32), np.zeros(rows, np.float32), np.zeros(rows, np.uint64), np.zeros(rows, np.float32),
               np.zeros(rows, np.uint32), np.zeros(max(nq, 1), np.uint32))
        if not len(cand_ids):
            cand_ids, cand_groups = np.zeros(1, np.uint64), np.zeros(1, np.uint32)
        return q_off, comps, vals, cand_off, cand_ids, cand_groups, nq, m, k, out

    def collapse_documents(self, q_off, comps, vals, cand_off, cand_ids, cand_groups, m, k, replica=0):
        """sgpu_collapse_documents: per query the k <= 1024 best GROUPS of its candidates (given as for score_documents, at
        most 4096 per query; cand_groups[i] is the u32 group key of entry i). A group's members are its distinct
        documents, best first (score descending, id ascending); its score is the f32 sum of its first m <= 64 members in
        that order (m = 1: its best member's score); groups come by score descending, key ascending. Scored and selected
        on the device of `replica`. Returns (groups u32 [nq, k], scores f32 [nq, k], best ids u64 [nq, k], best scores
        f32 [nq, k], members u32 [nq, k], n u32 [nq]); slots past n[q] are zero."""
        q_off, comps, vals, cand_off, cand, grp, nq, m, k, out = self._collapse_buffers(q_off, comps, vals, cand_off, cand_ids,
                                                                                        cand_groups, m, k)
        check(lib().sgpu_collapse_documents(self.h, int(replica), _p(q_off), _p(comps), _p(vals), nq, _p(cand_off), _p(cand),
                                            _p(grp), m, k, *[_p(a) for a in out]))
        return tuple(a[:nq] for a in out)

    def collapse_documents_host(self, q_off, comps, vals, cand_off, cand_ids, cand_groups, m, k, num_threads=0):
        """sgpu_collapse_documents_host: the same rows on the host cores (needs no upload), bit-identical."""
        q_off, comps, vals, cand_off, cand, grp, nq, m, k, out = self._collapse_buffers(q_off, comps, vals, cand_off, cand_ids,
                                                                                        cand_groups, m, k)
        check(lib().sgpu_collapse_documents_host(self.h, _p(q_off), _p(comps), _p(vals), nq, _p(cand_off), _p(cand), _p(grp), m,
                                                 k, int(num_threads), *[_p(a) for a in out]))
        return tuple(a[:nq] for a in out)

    def debug_collapse_stats(self, replica=0):
        """sgpu_debug_collapse_stats (test hook): what the last collapse_documents call on `replica` measured."""
        out = np.zeros(8, np.float64)
        fn = lib().sgpu_debug_collapse_stats
        fn.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
        check(fn(self.h, int(replica), _p(out)))
        return dict(kernel_ms=float(out[0]), launches=int(out[1]), dense=int(out[2]), grid=int(out[3]), block=int(out[4]),
                    lds=int(out[5]), select_ms=float(out[6]), select_launches=int(out[7]))

    # ---- hybrid fusion of each query's candidates with another retriever's scores ----
    FUSE_METHODS = {"rrf": 0, "minmax": 1, "sum": 2}

    @classmethod
    def _fuse_buffers(cls, q_off, comps, vals, cand_off, cand_ids, cand_ext, method, k):
        q_off, comps, vals = _csr(q_off, comps, vals)
        cand_off = np.ascontiguousarray(cand_off, np.uint64)
        cand_ids = np.ascontiguousarray(cand_ids, np.uint64)
        cand_ext = np.ascontiguousarray(cand_ext, np.float32)
        if len(cand_ext) != len(cand_ids):
            raise ValueError("%d candidates but %d external scores" % (len(cand_ids), len(cand_ext)))
        method = cls.FUSE_METHODS.get(method, method)
        nq, k, method = len(q_off) - 1, int(k), int(method)
        if not (0 <= k < 2 ** 32 and 0 <= method < 2 ** 32):
            raise ValueError("method = %d, k = %d" % (method, k))
        rows = (max(nq, 1), k if 1 <= k <= 1024 else 1)   # (a k the library refuses: nothing is written)
        out = (np.zeros(rows, np.float32), np.zeros(rows, np.uint64), np.zeros(rows, np.float32), np.zeros(rows, np.float32),
               np.zeros(rows, np.uint32), np.zeros(rows, np.uint32), np.zeros(max(nq, 1), np.uint32))
        if not len(cand_ids):
            cand_ids, cand_ext = np.zeros(1, np.uint64), np.zeros(1, np.float32)
        return q_off, comps, vals, cand_off, cand_ids, cand_ext, nq, method, k, out

    def fuse_documents(self, q_off, comps, vals, cand_off, cand_ids, cand_ext, method, w_sparse, w_ext, rrf_c, k, replica=0):
        """sgpu_fuse_documents: per query the k <= 1024 best of its candidates (given as for score_documents, at most 4096
        per query) under the fusion of this index's score with another retriever's: cand_ext[i] is that retriever's score
        of entry i, NaN where it does not list the document. method: "rrf" (w_sparse / (rrf_c + rank) + w_ext / (rrf_c +
        rank), ordinal ranks from 1, ties by id), "minmax" (weighted sum of the scores normalised to [0, 1] over the
        query's documents) or "sum" (weighted sum of the raw scores), or its SGPU_FUSE_* number; a document the other list
        lacks gets no external term. All f32, see include/seismic_hip.h. Scored and selected on the device of `replica`.
        Returns (fused f32, ids u64, sparse scores f32, external scores f32, sparse ranks u32, external ranks u32 - all
        [nq, k] -, n u32 [nq]); slots past n[q] are zero, and so are the external score and rank of an absent document."""
        q_off, comps, vals, cand_off, cand, ext, nq, method, k, out = self._fuse_buffers(q_off, comps, vals, cand_off, cand_ids,
                                                                                         cand_ext, method, k)
        check(lib().sgpu_fuse_documents(self.h, int(replica), _p(q_off), _p(comps), _p(vals), nq, _p(cand_off), _p(cand), _p(ext),
                                        method, float(w_sparse), float(w_ext), float(rrf_c), k, *[_p(a) for a in out]))
        return tuple(a[:nq] for a in out)

    def fuse_documents_host(self, q_off, comps, vals, cand_off, cand_ids, cand_ext, method, w_sparse, w_ext, rrf_c, k,
                            num_threads=0):
        """sgpu_fuse_documents_host: the same rows on the host cores (needs no upload), bit-identical."""
        q_off, comps, vals, cand_off, cand, ext, nq, method, k, out = self._fuse_buffers(q_off, comps, vals, cand_off, cand_ids,
                                                                                         cand_ext, method, k)
        check(lib().sgpu_fuse_documents_host(self.h, _p(q_off), _p(comps), _p(vals), nq, _p(cand_off), _p(cand), _p(ext), method,
                                             float(w_sparse), float(w_ext), float(rrf_c), k, int(num_threads),
                                             *[_p(a) for a in out]))
        return tuple(a[:nq] for a in out)

    def debug_fuse_stats(self, replica=0):
        """sgpu_debug_fuse_stats (test hook): what the last fuse_documents call on `replica` measured."""
        out = np.zeros(8, np.float64)
        fn = lib().sgpu_debug_fuse_stats
        fn.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
        check(fn(self.h, int(replica), _p(out)))
        return dict(kernel_ms=float(out[0]), launches=int(out[1]), dense=int(out[2]), grid=int(out[3]), block=int(out[4]),
                    lds=int(out[5]), select_ms=float(out[6]), select_launches=int(out[7]))


TERM_CLAUSE_DTYPE = np.dtype([("component", np.uint32), ("occur", np.uint32), ("min_weight", np.float32),
                              ("reserved", np.uint32)])   # sgpu_term_clause


def term_clauses(clauses):
    """(component, occur, min_weight) triples, or an array of TERM_CLAUSE_DTYPE -> a contiguous array of sgpu_term_clause."""
    if isinstance(clauses, np.ndarray) and clauses.dtype == TERM_CLAUSE_DTYPE:
        return np.ascontiguousarray(clauses)
    rows = list(clauses)
    out = np.zeros(len(rows), TERM_CLAUSE_DTYPE)
    for i, (c, occur, w) in enumerate(rows):
        if not 0 <= int(c) <= 0xffffffff or not 0 <= int(occur) <= 0xffffffff:
            raise ValueError("clause %d: component %r / occur %r out of range" % (i, c, occur))
        out[i] = (int(c), int(occur), w, 0)
    return out


COLUMN_CLAUSE_DTYPE = np.dtype([("slot", np.uint32), ("occur", np.uint32), ("op", np.uint32), ("lo_bits", np.uint32),
                                ("hi_bits", np.uint32), ("set_begin", np.uint32), ("set_count", np.uint32),
                                ("reserved", np.uint32)])   # sgpu_column_clause
COLUMN_DTYPES = {SGPU_COL_U32: np.uint32, SGPU_COL_I32: np.int32, SGPU_COL_F32: np.float32}
COLUMN_KINDS = {"u": (SGPU_COL_U32, np.uint32), "b": (SGPU_COL_U32, np.uint32), "i": (SGPU_COL_I32, np.int32),
                "f": (SGPU_COL_F32, np.float32)}   # numpy dtype kind -> (column type, stored dtype)


def column_array(values, dtype=None):
    """The values of a column as a contiguous 1-d array of its stored dtype (uint32 / int32 / float32): the type follows
    `dtype`, or the values' - unsigned -> u32, signed -> i32, floating -> f32; Python ints without a negative one are u32.
    An integer that the stored dtype cannot hold raises ValueError."""
    a = np.asarray(values, dtype)
    kind = a.dtype.kind
    if dtype is None and not isinstance(values, np.ndarray) and kind == "i" and (a.size == 0 or int(a.min()) >= 0):
        kind = "u"
    if kind not in COLUMN_KINDS:
        raise TypeError("a column holds unsigned, signed or floating values, got dtype %s" % a.dtype)
    cdt = COLUMN_KINDS[kind][1]
    if kind != "f" and a.size and (int(a.min()) < np.iinfo(cdt).min or int(a.max()) > np.iinfo(cdt).max):
        raise ValueError("column values do not fit %s" % np.dtype(cdt).name)
    return np.ascontiguousarray(a.ravel(), cdt)


def column_clauses(clauses):
    """(slot, occur, op, lo_bits, hi_bits, set_begin, set_count) rows, or an array of COLUMN_CLAUSE_DTYPE -> a contiguous
    array of sgpu_column_clause."""
    if isinstance(clauses, np.ndarray) and clauses.dtype == COLUMN_CLAUSE_DTYPE:
        return np.ascontiguousarray(clauses)
    rows = list(clauses)
    out = np.zeros(len(rows), COLUMN_CLAUSE_DTYPE)
    for i, row in enumerate(rows):
        row = tuple(int(x) for x in row)
        if len(row) != 7 or any(not 0 <= x <= 0xffffffff for x in row):
            raise ValueError("clause %d: seven fields of 32 bits, got %r" % (i, row))
        out[i] = row + (0,)
    return out


def _filter_handle(f):
    if not isinstance(f, NativeFilter):
        raise TypeError("filter must be a NativeFilter (NativeIndex.make_filter), got %r" % type(f).__name__)
    if not f.h:
        raise ValueError("the filter has been closed")
    return f.h


class NativeFilter:
    """Owns an sgpu_filter handle: a set of allowed document ids of one index. It keeps that index alive (the C ABI
    wants every filter destroyed before its index)."""

    def __init__(self, index, ids):
        self.index = index
        a = np.asarray(ids)
        if a.dtype == np.bool_:
            n_docs = int(index.desc.n_docs)
            if a.ndim != 1 or len(a) != n_docs:
                raise ValueError("a boolean mask must have one entry per document (%d), got shape %s" % (n_docs, a.shape))
            a = np.flatnonzero(a)
        elif a.size and not np.issubdtype(a.dtype, np.integer):
            raise TypeError("document ids must be integers or a boolean mask, got dtype %s" % a.dtype)
        a = a.ravel()
        if a.size and (int(a.min()) < 0 or int(a.max()) > 0xffffffff):
            bad = a[(a < 0) | (a > 0xffffffff)][0]
            raise ValueError("document id %d out of range" % int(bad))
        self._ids = np.ascontiguousarray(a, np.uint32)
        self.h = C.c_void_p()
        h = C.c_void_p()
        check(lib().sgpu_filter_create(index.h, _p(self._ids), len(self._ids), C.byref(h)))
        self.h = h
        del self._ids

    @classmethod
    def _adopt(cls, index, handle):
        """The NativeFilter that owns an sgpu_filter the library has already made (make_term_filter)."""
        self = cls.__new__(cls)
        self.index = index
        self.h = handle
        return self

    @property
    def count(self):
        """Number of allowed documents."""
        return int(lib().sgpu_filter_count(self.h))

    def bits(self):
        """The allowed set as u32 words (sgpu_filter_get_bits): bit d of word d // 32, ceil(n_docs / 32) words (at least
        one), the bits past n_docs zero."""
        n = C.c_uint64(0)
        lib().sgpu_filter_get_bits(_filter_handle(self), None, 0, C.byref(n))   # (the size; SGPU_EINVAL by contract)
        out = np.zeros(int(n.value), np.uint32)
        check(lib().sgpu_filter_get_bits(self.h, _p(out), len(out), C.byref(n)))
        return out

    def ids(self):
        """The allowed document ids, ascending (int64)."""
        b = np.unpackbits(self.bits().view(np.uint8), bitorder="little")
        return np.flatnonzero(b).astype(np.int64)

    def device_bytes(self):
        return int(lib().sgpu_filter_device_bytes(self.h))

    def debug_view(self, replica=0):
        """The filter's view on `replica` read back from the device (NativeIndex.debug_posting_view with this filter): it
        is built there first if a search has not done so yet."""
        return self.index.debug_posting_view(replica, filter=self)

    def close(self):
        if self.h:
            lib().sgpu_filter_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceBatch:
    """A query batch resident in HBM (what bench.py times)."""

    def __init__(self, index, q_off, comps, vals, k_max, replica=0):
        self.index = index
        self.q_off, self.comps, self.vals = _csr(q_off, comps, vals)
        self.nq = len(self.q_off) - 1
        self.k_max = int(k_max)
        self.h = C.c_void_p()
        check(lib().sgpu_batch_create_on(index.h, int(replica), _p(self.q_off), _p(self.comps), _p(self.vals),
                                         self.nq, self.k_max, C.byref(self.h)))

    def run(self, k, query_cut, heap_factor, first_sorted=False, sync=True, n_knn=0):
        p = params(k, query_cut, heap_factor, first_sorted, n_knn)
        st = LaunchStats()
        check(lib().sgpu_batch_run(self.index.h, self.h, C.byref(p), 1 if sync else 0, C.byref(st)))
        return st

    def run_counted(self, k, query_cut, heap_factor, first_sorted=False, n_knn=0):
        """Synchronous pass with the visited bitmap: identical results, exact work counters."""
        p = params(k, query_cut, heap_factor, first_sorted, n_knn)
        st = LaunchStats()
        check(lib().sgpu_batch_run_counted(self.index.h, self.h, C.byref(p), C.byref(st)))
        return st

    def sync(self):
        st = LaunchStats()
        check(lib().sgpu_batch_sync(self.index.h, C.byref(st)))
        return st

    def fetch(self, k):
        sc = np.zeros((self.nq, k), np.float32)
        ids = np.zeros((self.nq, k), np.uint64)
        n = np.zeros(max(self.nq, 1), np.uint32)
        check(lib().sgpu_batch_fetch(self.index.h, self.h, k, _p(sc), _p(ids), _p(n)))
        return sc, ids, n[: self.nq]

    def fetch_stats(self):
        """nq x 24 counters of the last pass (see sgpu_batch_fetch_stats)."""
        st = np.zeros((max(self.nq, 1), 24), np.uint32)
        check(lib().sgpu_batch_fetch_stats(self.index.h, self.h, _p(st)))
        return st[: self.nq]

    def algorithmic_bytes(self, k, comp_width, val_bytes=2, doc_comp_bytes=None):
        """B_q of SURVEY.md 8(d), summed over the batch, from the kernel's own work counters
        (val_bytes: 2 for f16 document values, 1 for fixed-u8; doc_comp_bytes: bytes per document component as
        stored, comp_width unless the component stream is compressed - 1.5 for DotVByte's 12-byte slices of eight components)."""
        b, st = self.algorithmic_bytes_per_query(k, comp_width, val_bytes, doc_comp_bytes)
        return int(b.sum()), st

    def algorithmic_bytes_per_query(self, k, comp_width, val_bytes=2, doc_comp_bytes=None):
        """B_q of every query of the batch (int64 [nq]; float64 where doc_comp_bytes is fractional) and the counters it
        was computed from; algorithmic_bytes() is its sum."""
        st = self.fetch_stats().astype(np.int64)
        nnz_q = np.diff(self.q_off.astype(np.int64))
        per_elem = (comp_width if doc_comp_bytes is None else doc_comp_bytes) + val_bytes
        b = (nnz_q * (comp_width + 4) + 12 * k + 8 * st[:, 0] + 8 * st[:, 1] + 3 * st[:, 2]
             + 4 * (st[:, 4] + st[:, 3]) + 8 * st[:, 5] + st[:, 6] * per_elem)
        return b, st

    def close(self):
        if self.h:
            lib().sgpu_batch_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def synth(n_vecs, dim, seed, kind=0, docs=None, collection=0):
    """SPLADE-shaped synthetic CSR (offsets u64, comps u32, vals f32). kind 0 docs, 1 queries; collection 0 = the
    SURVEY 8(d) law, 1 = clustered (documents around latent intents; pass the same value for documents and queries)."""
    spec = SynthSpec(n_vecs=n_vecs, dim=dim, seed=seed, kind=kind, collection=collection)
    nnz = C.c_uint64(0)
    d_off = d_c = d_v = None
    nd = 0
    if kind == 1:
        d_off, d_c, d_v = _csr(*docs)
        nd = len(d_off) - 1
    check(lib().sgpu_synth_generate(C.byref(spec), _p(d_off), _p(d_c), _p(d_v), nd, None, None, None,
                                    C.byref(nnz)))
    off = np.zeros(n_vecs + 1, np.uint64)
    comps = np.zeros(max(nnz.value, 1), np.uint32)
    vals = np.zeros(max(nnz.value, 1), np.float32)
    check(lib().sgpu_synth_generate(C.byref(spec), _p(d_off), _p(d_c), _p(d_v), nd, _p(off), _p(comps),
                                    _p(vals), C.byref(nnz)))
    return off, comps[: nnz.value], vals[: nnz.value]


def read_inner_format(path):
    """documents.bin / queries.bin of the reference (scripts/convert_json_to_inner_format.py:10-27)
    -> (offsets u64, comps u32, vals f32)."""
    n, nnz = C.c_uint64(0), C.c_uint64(0)
    check(lib().sgpu_dataset_read(os.fsencode(path), C.byref(n), C.byref(nnz), None, None, None))
    off = np.zeros(n.value + 1, np.uint64)
    comps = np.zeros(max(nnz.value, 1), np.uint32)
    vals = np.zeros(max(nnz.value, 1), np.float32)
    check(lib().sgpu_dataset_read(os.fsencode(path), C.byref(n), C.byref(nnz), _p(off), _p(comps), _p(vals)))
    return off, comps[: nnz.value], vals[: nnz.value]


def write_inner_format(path, off, comps, vals):
    off, comps, vals = _csr(off, comps, vals)
    check(lib().sgpu_dataset_write(os.fsencode(path), len(off) - 1, _p(off), _p(comps), _p(vals)))


def write_results_tsv(path, scores, ids, n):
    """query_index\tdoc_id\trank\tscore (reference src/bin/perf_inverted_index.rs:223-235)."""
    scores = np.ascontiguousarray(scores, np.float32)
    ids = np.ascontiguousarray(ids, np.uint64)
    n = np.ascontiguousarray(n, np.uint32)
    nq, k = scores.shape if scores.ndim == 2 else (0, 1)
    check(lib().sgpu_results_write_tsv(os.fsencode(path), nq, k, _p(scores), _p(ids), _p(n)))
