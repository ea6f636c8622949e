"""Document filters on the GPU. Filtered search of an index I with a set A equals the UNCHANGED oracle searching I_A - the
descriptor with every posting of a document outside A deleted (built here in numpy from orc.desc_arrays), and, with a
kNN graph, the graph whose neighbours outside A are 0xffffffff - bit for bit: out_n, ids and their order, score bits.
Filtered exact search on the device equals filtered exact search on the host. Run with `-m gpu`."""
import ctypes as C
import threading

import numpy as np
import pytest

import orc
from seismic_amd import _native
from seismic_amd._abi import BuildConfig, IndexDesc
from util import random_dataset, random_queries

pytestmark = pytest.mark.gpu

DIM, N_DOCS = 600, 5000


def _same(g, c):
    gs, gi, gn = g
    cs, ci, cn = c
    assert np.array_equal(gn, cn), (np.flatnonzero(gn != cn)[:5], gn[gn != cn][:5], cn[gn != cn][:5])
    for q in range(len(gn)):
        n = int(gn[q])
        assert np.array_equal(gi[q, :n], ci[q, :n]), (q, gi[q, :n], ci[q, :n])
        assert np.array_equal(gs[q, :n].view(np.uint32), cs[q, :n].view(np.uint32)), q


class FilteredDesc:
    """I_A: the descriptor of `desc` with the postings of documents outside `allowed` deleted (blocks kept)."""

    def __init__(self, desc, allowed):
        a = orc.desc_arrays(desc)
        keep = allowed[a["post_doc"]]
        cum = np.concatenate([[0], np.cumsum(keep, dtype=np.uint64)]).astype(np.uint64)
        self.bps = np.ascontiguousarray(cum[a["block_post_start"].astype(np.int64)], np.uint64)
        self.post_doc = np.ascontiguousarray(a["post_doc"][keep], np.uint32)
        self.desc = IndexDesc()
        C.memmove(C.byref(self.desc), C.byref(desc), C.sizeof(IndexDesc))
        self.desc.n_postings = len(self.post_doc)
        self.desc.block_post_start = self.bps.ctypes.data_as(type(desc.block_post_start))
        self.desc.post_doc = (self.post_doc if len(self.post_doc) else np.zeros(1, np.uint32)).ctypes.data_as(
            type(desc.post_doc))


def _masked(graph, allowed):
    return np.where(allowed[graph], graph, np.uint32(0xffffffff)).astype(np.uint32)


def _oracle(fd, q, k, qc, hf, fs, n_knn=0):
    return orc.batch_search(fd.desc, *q, k, qc, hf, fs, n_knn=n_knn)[:3]


def _sets(desc, n_docs, seed):
    rng = np.random.default_rng(seed)
    a = orc.desc_arrays(desc)
    lbs, bps, pd = a["list_block_start"], a["block_post_start"], a["post_doc"]
    holes = np.ones(n_docs, bool)                  # empties whole lists and whole blocks
    for c in range(0, int(desc.dim), 7):           # every 7th list: all of it
        holes[pd[bps[lbs[c]]:bps[lbs[c + 1]]]] = False
    for c in range(3, int(desc.dim), 11):          # the first block of every 11th list
        if lbs[c + 1] > lbs[c]:
            holes[pd[bps[lbs[c]]:bps[lbs[c] + 1]]] = False
    return {"all": np.ones(n_docs, bool), "none": np.zeros(n_docs, bool), "one": np.arange(n_docs) == 77,
            "p1": rng.random(n_docs) < 0.01, "p50": rng.random(n_docs) < 0.5, "holes": holes}


@pytest.fixture(scope="module")
def base():
    off, comps, vals = random_dataset(81, N_DOCS, DIM, nnz_lo=6, nnz_hi=120, empty_every=313)
    ix = _native.NativeIndex.build(2, DIM, off, comps, vals,
                                   BuildConfig.defaults(n_postings=120, centroid_fraction=0.2, summary_energy=0.5,
                                                        max_fraction=4.0)).upload(0)
    graph = orc.knn_build(ix.desc, 5)
    ix.set_knn(graph, 5)
    return ix, graph, (off, comps, vals)


def test_parameter_sweep_against_the_oracle_on_i_a(base):
    ix, graph, _ = base
    q = random_queries(82, 64, DIM, 3, 60)
    q1 = (np.array([0, q[0][1]], np.uint64), q[1][:int(q[0][1])], q[2][:int(q[0][1])])
    combos = [(1, 4, 1.0, False, 0), (10, 4, 1.0, False, 0), (10, 3, 0.8, True, 5), (100, 6, 0.9, False, 5),
              (1000, 5, 1.0, False, 0), (10, 4, -0.5, False, 0), (10, 2, 1.0, True, 0)]
    for name, allowed in _sets(ix.desc, N_DOCS, 83).items():
        f = ix.make_filter(allowed)
        fd = FilteredDesc(ix.desc, allowed)
        orc.knn_attach(_masked(graph, allowed), 5)
        try:
            for k, qc, hf, fs, nk in combos:
                g = ix.batch_search(*q, k, qc, hf, fs, n_knn=nk, filter=f)
                _same(g, _oracle(fd, q, k, qc, hf, fs, nk))
                if name == "all":   # A = every document: the unfiltered search, bit for bit
                    _same(g, ix.batch_search(*q, k, qc, hf, fs, n_knn=nk))
                if name == "none":
                    assert (g[2] == 0).all()
                ids = g[1][np.arange(g[1].shape[1])[None, :] < g[2][:, None]]
                assert allowed[ids.astype(np.int64)].all()
            s, i = ix.search(q1[1], q1[2], 10, 4, 1.0, filter=f)   # sgpu_search_filtered
            _same((s[None, :], i[None, :], np.array([len(i)], np.uint32)), _oracle(fd, q1, 10, 4, 1.0, False))
        finally:
            orc.knn_attach(None, 0)
        assert f.device_bytes() > 0


@pytest.mark.parametrize("kind", ["u32", "fixedu8", "dotvbyte"])
def test_widths_and_value_types(base, kind):
    _, _, (off, comps, vals) = base
    if kind == "u32":
        dim = 70_000
        off, comps, vals = random_dataset(84, 3000, dim, nnz_lo=6, nnz_hi=120)
        ix = _native.NativeIndex.build(4, dim, off, comps, vals,
                                       BuildConfig.defaults(n_postings=40, centroid_fraction=0.2, summary_energy=0.5,
                                                            max_fraction=4.0)).upload(0)
    else:
        dim = DIM
        f16 = _native.NativeIndex.build(2, dim, off, comps, vals,
                                        BuildConfig.defaults(n_postings=120, centroid_fraction=0.2, summary_energy=0.5,
                                                             max_fraction=4.0))
        ix = f16.convert(1).upload(0)
    n_docs = int(ix.desc.n_docs)
    q = random_queries(85, 64, dim, 3, 60)
    # (DotVByte is lossless over the fixed-u8 index: its results are the fixed-u8 index's, which the oracle restates)
    dvb = f16.convert(2).upload(0) if kind == "dotvbyte" else None
    for name in ("p1", "p50", "holes"):
        allowed = _sets(ix.desc, n_docs, 86)[name]
        fd = FilteredDesc(ix.desc, allowed)
        for k, qc, hf, fs in ((10, 4, 1.0, False), (100, 5, 0.9, True)):
            want = _oracle(fd, q, k, qc, hf, fs)
            target = dvb if dvb is not None else ix
            _same(target.batch_search(*q, k, qc, hf, fs, filter=target.make_filter(allowed)), want)


def test_batch_sizes_reach_every_launch_path(base):
    ix, _, _ = base
    allowed = _sets(ix.desc, N_DOCS, 87)["p50"]
    f = ix.make_filter(allowed)
    fd = FilteredDesc(ix.desc, allowed)
    big = random_queries(88, 10_000, DIM, 3, 60)
    for nq in (1, 64, 1250, 10_000, 10_000):   # cooperative, chunked, streamed; the second 10 000: device-planned chunks
        off = big[0][:nq + 1].copy()
        q = (off, big[1][:int(off[nq])], big[2][:int(off[nq])])
        _same(ix.batch_search(*q, 10, 4, 1.0, False, filter=f), _oracle(fd, q, 10, 4, 1.0, False))


def test_cross_check_with_an_index_built_from_i_a(base):
    ix, _, _ = base
    allowed = _sets(ix.desc, N_DOCS, 89)["holes"]
    fd = FilteredDesc(ix.desc, allowed)
    ia = _native.NativeIndex.from_desc(fd.desc).upload(0)
    q = random_queries(90, 200, DIM, 3, 60)
    f = ix.make_filter(allowed)
    for k, qc, hf, fs in ((10, 4, 1.0, False), (50, 6, 0.8, True)):
        _same(ix.batch_search(*q, k, qc, hf, fs, filter=f), ia.batch_search(*q, k, qc, hf, fs))


def test_two_replicas_and_threads_and_rebuilt_views():
    off, comps, vals = random_dataset(91, 4000, DIM, nnz_lo=6, nnz_hi=120)
    ix = _native.NativeIndex.build(2, DIM, off, comps, vals,
                                   BuildConfig.defaults(n_postings=120, centroid_fraction=0.2, summary_energy=0.5,
                                                        max_fraction=4.0))
    allowed = _sets(ix.desc, 4000, 92)["p50"]
    fd = FilteredDesc(ix.desc, allowed)
    f = ix.make_filter(allowed)
    q = random_queries(93, 300, DIM, 3, 60)
    want_f = _oracle(fd, q, 10, 4, 1.0, False)
    want_u = orc.batch_search(ix.desc, *q, 10, 4, 1.0, False)[:3]
    ix.upload_many([0, 0])                     # two replicas on one device: the batch is sharded, each has its view
    _same(ix.batch_search(*q, 10, 4, 1.0, False, filter=f), want_f)
    for j in range(4):                         # single queries: the replicas take them in turn
        o = (np.array([0, q[0][j + 1] - q[0][j]], np.uint64), q[1][int(q[0][j]):int(q[0][j + 1])],
             q[2][int(q[0][j]):int(q[0][j + 1])])
        _same(ix.batch_search(*o, 10, 4, 1.0, False, filter=f), tuple(a[j:j + 1] for a in want_f))
    bytes2 = f.device_bytes()
    ix.upload(0)                               # a new upload: the views are rebuilt on their next use
    _same(ix.batch_search(*q, 10, 4, 1.0, False, filter=f), want_f)
    assert 0 < f.device_bytes() <= bytes2
    # filtered and unfiltered calls from two threads on one replica
    errors = []

    def serve(filtered):
        try:
            for _ in range(6):
                g = ix.batch_search(*q, 10, 4, 1.0, False, filter=f if filtered else None)
                _same(g, want_f if filtered else want_u)
        except Exception as e:   # (reported below)
            errors.append(e)
    ts = [threading.Thread(target=serve, args=(b,)) for b in (True, False)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors[0]
    # a new graph: the masked copy follows it
    for seed in (1, 2):
        graph = np.random.default_rng(seed).integers(0, 4000, 4000 * 6).astype(np.uint32)
        ix.set_knn(graph, 6)
        orc.knn_attach(_masked(graph, allowed), 6)
        try:
            _same(ix.batch_search(*q, 10, 4, 1.0, False, n_knn=6, filter=f), _oracle(fd, q, 10, 4, 1.0, False, 6))
        finally:
            orc.knn_attach(None, 0)


@pytest.mark.parametrize("value_type", [0, 1])
def test_device_filtered_exact_equals_host(value_type):
    dim, n_docs = 1000, 70_000                 # three ranges of 32768 documents, the last one partial
    off, comps, vals = random_dataset(94, n_docs, dim, nnz_lo=2, nnz_hi=40, empty_every=97)
    ix = _native.NativeIndex.build(2, dim, off, comps, vals, BuildConfig.defaults(n_postings=1, centroid_fraction=1.0,
                                                                                  min_cluster_size=0, summary_energy=1.0,
                                                                                  max_fraction=1.0, doc_cut=1))
    if value_type:
        ix = ix.convert(value_type)
    ix.upload(0)
    q_off, qc, qv = random_queries(95, 24, dim, 1, 30)
    qv = qv.copy()
    qv[::4] *= -1.0
    q = (q_off, qc, qv)
    rng = np.random.default_rng(96)
    sets = [np.ones(n_docs, bool), np.zeros(n_docs, bool), np.arange(n_docs) == 40_000, rng.random(n_docs) < 0.001,
            rng.random(n_docs) < 0.3, (np.arange(n_docs) >= 32_700) & (np.arange(n_docs) < 32_900)]
    for allowed in sets:
        f = ix.make_filter(allowed)
        for k in (1, 10, 100, 1024):
            d = ix.exact_search_device(*q, k, filter=f)
            h = ix.exact_search(*q, k, filter=f)
            assert (d[2] == min(k, int(allowed.sum()))).all()
            _same(d, h)
    u = ix.exact_search_device(*q, 10)
    _same(ix.exact_search_device(*q, 10, filter=ix.make_filter(np.ones(n_docs, bool))), u)
