"""Exact top-k on the device (sgpu_exact_search_device): for every query exactly what the host exact search returns,
and what the oracle's sequential brute force returns - n, ids and their order, score bits. Run with `-m gpu`."""
import threading

import numpy as np
import pytest

import orc
import seismic_amd
from seismic_amd import _native
from seismic_amd._abi import BuildConfig
from util import random_dataset, random_queries

pytestmark = pytest.mark.gpu

GOLD_TOY = __import__("os").path.join(__import__("os").path.dirname(__file__), "golden", "toy")


def _forward_only(cw, dim, off, comps, vals):
    # the config SeismicDataset._freeze uses: exact search only needs the forward index
    return _native.NativeIndex.build(cw, dim, off, comps, vals,
                                     BuildConfig.defaults(n_postings=1, centroid_fraction=1.0, min_cluster_size=0,
                                                          summary_energy=1.0, max_fraction=1.0, doc_cut=1))


def _same(dev, host):
    ds, di, dn = dev
    hs, hi, hn = host
    assert np.array_equal(dn, hn)
    for i in range(len(dn)):
        n = int(dn[i])
        assert np.array_equal(di[i, :n], hi[i, :n]), i
        assert np.array_equal(ds[i, :n].view(np.uint32), hs[i, :n].view(np.uint32)), i


def _check(ix, q_off, qc, qv, k, oracle=True):
    dev = ix.exact_search_device(q_off, qc, qv, k)
    host = ix.exact_search(q_off, qc, qv, k)
    _same(dev, host)
    assert (dev[2] == min(k, ix.desc.n_docs)).all()
    if oracle:
        for i in range(len(q_off) - 1):
            c, v = qc[q_off[i]:q_off[i + 1]], qv[q_off[i]:q_off[i + 1]]
            es, ei = orc.exact_search(ix.desc, c, v, k, orc.ORDER_SEQ)
            n = int(dev[2][i])
            assert np.array_equal(dev[1][i, :n], ei), i
            assert np.array_equal(dev[0][i, :n].view(np.uint32), es.view(np.uint32)), i
    return dev


def _with_empty_query(q_off, qc, qv):
    return np.concatenate([q_off, q_off[-1:]]), qc, qv


@pytest.mark.parametrize("cw,dim", [(2, 400), (4, 400), (4, 70_000)])
def test_widths_dims_empty_docs_and_k(cw, dim):
    off, comps, vals = random_dataset(21, 3000, dim, nnz_lo=3, nnz_hi=80, empty_every=7)
    ix = _forward_only(cw, dim, off, comps, vals).upload(0)
    q = _with_empty_query(*random_queries(22, 12, dim, 1, 60))
    for k in (1, 10, 100, 1024):
        _check(ix, *q, k, oracle=k <= 100)


def test_k_above_the_number_of_documents():
    dim = 50
    off, comps, vals = random_dataset(23, 7, dim, nnz_lo=2, nnz_hi=10)
    ix = _forward_only(2, dim, off, comps, vals).upload(0)
    q = _with_empty_query(*random_queries(24, 5, dim, 1, 8))
    for k in (7, 8, 100, 1024):
        dev = _check(ix, *q, k)
        assert (dev[2] == 7).all()
        assert (dev[1][:, 7:] == 0).all()


@pytest.mark.parametrize("value_type", [0, 1, 2])
def test_value_types_ties_and_negative_queries(value_type):
    """f16, fixed-u8 and DotVByte documents; values from 3 levels (many exact ties), query values of both signs."""
    dim, n_docs = 300, 5000
    rng = np.random.default_rng(25)
    off, comps, vals = random_dataset(26, n_docs, dim, nnz_lo=2, nnz_hi=40)
    vals = rng.choice(np.array([0.25, 0.5, 1.0], np.float32), len(vals))
    base = _forward_only(2, dim, off, comps, vals)
    ix = base if value_type == 0 else base.convert(value_type)
    ix.upload(0)
    q_off, qc, qv = random_queries(27, 16, dim, 1, 30)
    qv = rng.choice(np.array([-1.0, 0.5, 2.0], np.float32), len(qv))
    for k in (1, 10, 100):
        _check(ix, *_with_empty_query(q_off, qc, qv), k)


@pytest.mark.parametrize("n_docs", [32_767, 32_768, 32_769, 65_537])
def test_range_edges(n_docs):
    dim = 400
    off, comps, vals = random_dataset(28, n_docs, dim, nnz_lo=1, nnz_hi=6)
    ix = _forward_only(2, dim, off, comps, vals).upload(0)
    q_off, qc, qv = random_queries(29, 6, dim, 1, 20)
    qv[::3] = -qv[::3]
    for k in (10, 1024):
        _check(ix, *_with_empty_query(q_off, qc, qv), k, oracle=k == 10)


def test_large_vocabulary_1m_documents():
    dim, n_docs = 200_000, 1_000_000
    docs = _native.synth(n_docs, dim, 42, 0)
    ix = _forward_only(4, dim, *docs).upload(0)
    q = _native.synth(64, dim, 43, 1, docs)
    _check(ix, *q, 10, oracle=False)
    _check(ix, *q, 100, oracle=False)


def test_concurrent_searches_on_the_same_replica():
    """Two request threads run batch_search on the replica while exact calls run: every result is unchanged."""
    dim = 2000
    off, comps, vals = random_dataset(30, 60_000, dim, nnz_lo=5, nnz_hi=60)
    ix = _native.NativeIndex.build(2, dim, off, comps, vals,
                                   BuildConfig.defaults(n_postings=400, centroid_fraction=0.1)).upload(0)
    q = random_queries(31, 500, dim, 5, 40)
    want = ix.batch_search(*q, 10, 5, 0.9, False)
    want_exact = ix.exact_search(*q, 10)
    errors, stop = [], threading.Event()

    def serve():
        try:
            while not stop.is_set():
                got = ix.batch_search(*q, 10, 5, 0.9, False)
                for a, b in zip(got, want):
                    assert np.array_equal(a, b)
        except Exception as e:   # noqa: BLE001 - reported below
            errors.append(e)

    threads = [threading.Thread(target=serve) for _ in range(2)]
    for t in threads:
        t.start()
    try:
        for _ in range(3):
            _same(ix.exact_search_device(*q, 10), want_exact)
    finally:
        stop.set()
        for t in threads:
            t.join()
    assert not errors, errors


def test_dataset_on_the_device_equals_the_host():
    from seismic_amd.index import read_jsonl
    ids, vecs, _ = read_jsonl(__import__("os").path.join(GOLD_TOY, "documents.jsonl"))
    qids, qvecs, _ = read_jsonl(__import__("os").path.join(GOLD_TOY, "queries.jsonl"))
    for cls in (seismic_amd.SeismicDataset, seismic_amd.SeismicDatasetLV):
        ds = cls()
        for i, v in zip(ids, vecs):
            ds.add_document(i, list(v.keys()), list(v.values()))
        qc = [np.array(list(v.keys())) for v in qvecs]
        qv = [np.array(list(v.values()), np.float32) for v in qvecs]
        for k in (1, 10, 1024):
            host = ds.batch_search(qids, qc, qv, k)
            assert ds.batch_search(qids, qc, qv, k, device=0) == host
            assert [ds.search(q, c, v, k, device=0) for q, c, v in zip(qids, qc, qv)] == host


def test_index_batch_exact_search_equals_dataset():
    from seismic_amd.index import read_jsonl
    path = __import__("os").path.join(GOLD_TOY, "documents.jsonl")
    ids, vecs, _ = read_jsonl(path)
    qids, qvecs, _ = read_jsonl(__import__("os").path.join(GOLD_TOY, "queries.jsonl"))
    ds = seismic_amd.SeismicDataset()
    for i, v in zip(ids, vecs):
        ds.add_document(i, list(v.keys()), list(v.values()))
    qc = [np.array(list(v.keys())) for v in qvecs]
    qv = [np.array(list(v.values()), np.float32) for v in qvecs]
    want = ds.batch_search(qids, qc, qv, 10)
    ix = seismic_amd.SeismicIndex.build(path, n_postings=50, centroid_fraction=0.2)
    assert ix.batch_exact_search(qids, qc, qv, 10, device=0) == want
    assert ix.batch_exact_search(qids, qc, qv, 10) == want
