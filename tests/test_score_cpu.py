"""sgpu_score_documents / sgpu_score_documents_host without a device: the declarations, every argument check in the
header's order, the host twin against the oracle (bits) and the float64 model (derived bound), and the Python classes
with device=False. The cases are tests/score_cases.py."""
import ctypes as C
import os

import numpy as np
import pytest

import model64
import orc
import score_cases
import seismic_amd
from seismic_amd import _native
from seismic_amd._abi import BuildConfig
from seismic_amd.index import read_jsonl
from util import random_dataset, random_queries

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD_TOY = os.path.join(ROOT, "tests", "golden", "toy")
EINVAL, EDEVICE, ELIMIT = 1, 2, 5


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def test_header_declares_both_functions_and_the_abi_version_stays():
    text = open(os.path.join(ROOT, "include", "seismic_hip.h")).read()
    assert "sgpu_status sgpu_score_documents(sgpu_index* idx, uint32_t replica," in text
    assert "sgpu_status sgpu_score_documents_host(const sgpu_index* idx," in text
    L = _native.lib()
    assert hasattr(L, "sgpu_score_documents") and hasattr(L, "sgpu_score_documents_host")
    assert L.sgpu_abi_version() == 4


@pytest.fixture(scope="module")
def small():
    dim = 300
    off, comps, vals = random_dataset(3, 50, dim, 3, 20)
    ix = _native.NativeIndex.build(2, dim, off, comps, vals, BuildConfig.defaults(n_postings=10))
    q_off, qc, qv = random_queries(4, 3, dim, 2, 8)
    return ix, dim, q_off, qc, qv


def _calls(ix, q_off, qc, qv, cand_off, cand_ids, out):
    """(name, status, message) of the device call and of the host twin with the same arguments."""
    L = _native.lib()
    nq = len(q_off) - 1 if q_off is not None else 0
    got = []
    st = L.sgpu_score_documents(ix.h if ix else None, 0, _p(q_off), _p(qc), _p(qv), nq, _p(cand_off), _p(cand_ids), _p(out))
    got.append(("device", st, L.sgpu_last_error().decode()))
    st = L.sgpu_score_documents_host(ix.h if ix else None, _p(q_off), _p(qc), _p(qv), nq, _p(cand_off), _p(cand_ids), 0, _p(out))
    got.append(("host", st, L.sgpu_last_error().decode()))
    return got


def test_argument_checks_in_order_without_a_device(small):
    ix, dim, q_off, qc, qv = small
    cand_off = np.array([0, 2, 2, 3], np.uint64)
    cand_ids = np.array([1, 49, 7], np.uint64)
    out = np.zeros(3, np.float32)
    # 1. null arguments
    for args in ((None, q_off, qc, qv, cand_off, cand_ids, out), (ix, None, qc, qv, cand_off, cand_ids, out),
                 (ix, q_off, qc, qv, None, cand_ids, out), (ix, q_off, qc, qv, cand_off, None, out),
                 (ix, q_off, qc, qv, cand_off, cand_ids, None)):
        for name, st, _ in _calls(*args):
            assert st == EINVAL, name
    # 2. the queries - also when a later check would fail too (a bad id, a bad cand_off)
    bad_qc = qc.copy()
    bad_qc[0] = dim
    bad_ids = np.array([1, 50, 7], np.uint64)
    for name, st, msg in _calls(ix, q_off, bad_qc, qv, np.array([1, 2, 2, 3], np.uint64), bad_ids, out):
        assert st == EINVAL and "component >= dim" in msg, (name, msg)
    unsorted = qc.copy()
    unsorted[0], unsorted[1] = qc[1], qc[0]
    for name, st, msg in _calls(ix, q_off, unsorted, qv, cand_off, cand_ids, out):
        assert st == EINVAL and "ascending" in msg, (name, msg)
    # 3. cand_off
    for off in (np.array([1, 2, 2, 3], np.uint64), np.array([0, 2, 1, 3], np.uint64)):
        for name, st, msg in _calls(ix, q_off, qc, qv, off, bad_ids, out):
            assert st == EINVAL and "cand_off" in msg, (name, msg)
    # 4. an id >= n_docs: the first one and its query are named
    ids = np.array([1, 49, 50], np.uint64)
    for name, st, msg in _calls(ix, q_off, qc, qv, cand_off, ids, out):
        assert st == EINVAL and "query 2" in msg and "document id 50" in msg, (name, msg)
    ids = np.array([1, 77, 50], np.uint64)
    for name, st, msg in _calls(ix, q_off, qc, qv, cand_off, ids, out):
        assert st == EINVAL and "query 0" in msg and "document id 77" in msg, (name, msg)
    # 6. the device call on an index that is not uploaded: SGPU_EDEVICE, after the argument checks; the host twin runs
    (_, st, msg), (_, hst, _) = _calls(ix, q_off, qc, qv, cand_off, cand_ids, out)
    assert st == EDEVICE and "not uploaded" in msg and hst == 0
    # ... also with nothing to score
    zero = np.zeros(4, np.uint64)
    (_, st, _), (_, hst, _) = _calls(ix, q_off, qc, qv, zero, cand_ids, out)
    assert st == EDEVICE and hst == 0
    assert _native.lib().sgpu_score_documents_host(ix.h, _p(q_off), _p(qc), _p(qv), 0, _p(zero), _p(cand_ids), 0, _p(out)) == 0


def test_capacity_limit_is_checked_after_the_ids_and_before_the_device():
    dim = 9000
    off, comps, vals = random_dataset(5, 20, dim, 3, 20)
    ix = _native.NativeIndex.build(2, dim, off, comps, vals, BuildConfig.defaults(n_postings=10))
    cand_off = np.array([0, 1], np.uint64)
    out = np.zeros(1, np.float32)
    for n, want in ((8192, EDEVICE), (8193, ELIMIT)):
        q_off = np.array([0, n], np.uint64)
        qc = np.arange(n, dtype=np.uint32)
        qv = np.ones(n, np.float32)
        (_, st, msg), (_, hst, _) = _calls(ix, q_off, qc, qv, cand_off, np.array([3], np.uint64), out)
        assert st == want and hst == (0 if want == EDEVICE else ELIMIT), (n, st, hst, msg)
        (_, st, msg), (_, hst, _) = _calls(ix, q_off, qc, qv, cand_off, np.array([20], np.uint64), out)
        assert st == EINVAL and hst == EINVAL and "document id 20" in msg


@pytest.mark.parametrize("name", sorted(score_cases.CASES))
def test_host_twin_equals_the_oracle_and_meets_the_model_bound(name):
    case = score_cases.make(name)
    ix = case.index
    for cand_off, cand_ids in ((case.all_off, case.all_ids), (case.cand_off, case.cand_ids)):
        got = ix.score_documents_host(case.q_off, case.qc, case.qv, cand_off, cand_ids)
        assert np.array_equal(got.view(np.uint32), case.expected(cand_off, cand_ids))
    # one thread and many give the same bits
    one = ix.score_documents_host(case.q_off, case.qc, case.qv, case.all_off, case.all_ids, num_threads=1)
    assert np.array_equal(one.view(np.uint32), case.oracle_bits().ravel())
    # edge cases of the contract: +0.0 for the empty query and for documents without components
    bits = case.oracle_bits()
    assert not bits[0].any()
    assert not bits[:, np.diff(case.off.astype(np.int64)) == 0].any()
    # the float64 model: |score - s*| <= gamma(m + 1) * A for every pair
    d = ix.desc
    M = model64.Model(orc.desc_arrays(d), d.val_scale, d.value_type)
    host = one.reshape(score_cases.N_QUERIES, case.n_docs).astype(np.float64)
    for q, (c, v) in enumerate(case.queries):
        mq = M.query(c, v)
        err = np.abs(host[q] - mq.s)
        assert np.all(err <= mq.tol), (name, q, float((err - mq.tol).max()))


def _toy():
    ids, vecs, _ = read_jsonl(os.path.join(GOLD_TOY, "documents.jsonl"))
    qids, qvecs, _ = read_jsonl(os.path.join(GOLD_TOY, "queries.jsonl"))
    qc = [np.array(list(v.keys())) for v in qvecs]
    qv = [np.array(list(v.values()), np.float32) for v in qvecs]
    return ids, qids, qc, qv


@pytest.mark.parametrize("cls", ["SeismicIndex", "SeismicIndexLV", "SeismicIndexDotVByte"])
def test_python_batch_score_and_rerank_on_the_host(cls):
    ids, qids, qc, qv = _toy()
    ix = getattr(seismic_amd, cls).build(os.path.join(GOLD_TOY, "documents.jsonl"), n_postings=50, centroid_fraction=0.2,
                                          upload=False)
    every = [list(ids)] * len(qids)
    scores = ix.batch_score(qc, qv, every, device=False)
    assert len(scores) == len(qids) and all(s.dtype == np.float32 and len(s) == len(ids) for s in scores)
    # the oracle's bits, through the string ids
    d = ix._ix.desc
    for q in range(len(qids)):
        c, v = seismic_amd.index._resolve(qc[q].astype(str), qv[q], ix._tm)
        want = np.array([orc.score_doc(d, ix._positions()[i], c, v) for i in ids], np.float32)
        assert np.array_equal(scores[q].view(np.uint32), want.view(np.uint32))
    # order and repeats of the ids are the caller's; score() is one row of batch_score
    some = [ids[3], ids[0], ids[3], ids[-1]]
    s = ix.score(qc[0], qv[0], some, device=False)
    pos = [ids.index(x) for x in some]
    assert np.array_equal(s.view(np.uint32), scores[0][pos].view(np.uint32))
    assert len(ix.score(qc[0], qv[0], [], device=False)) == 0
    # unknown tokens are dropped as in search; unknown document ids raise KeyError
    s2 = ix.score(np.append(qc[0], "no-such-token"), np.append(qv[0], np.float32(3.0)), some, device=False)
    assert np.array_equal(s2.view(np.uint32), s.view(np.uint32))
    with pytest.raises(KeyError):
        ix.score(qc[0], qv[0], [ids[0], "no-such-document"], device=False)
    with pytest.raises(ValueError):
        ix.batch_score(qc, qv, every[:-1], device=False)
    # batch_rerank: k best, score descending, ties by native id ascending, duplicates dropped
    k = 5
    rr = ix.batch_rerank(qc, qv, [list(ids) + [ids[2], ids[2]]] * len(qids), k, device=False)
    for q, row in enumerate(rr):
        order = sorted(range(len(ids)), key=lambda i: (-float(scores[q][i]), i))[:k]
        assert row == [(float(scores[q][i]), ids[i]) for i in order]
    # the best candidate over ALL documents is exact search's top document wherever the float64 model separates the
    # top two by more than both tolerances
    exact = ix.batch_exact_search(qids, qc, qv, 1)
    M = model64.Model(orc.desc_arrays(d), d.val_scale, d.value_type)
    compared = 0
    for q in range(len(qids)):
        c, v = seismic_amd.index._resolve(qc[q].astype(str), qv[q], ix._tm)
        mq = M.query(c, v)
        top = np.argsort(-mq.s, kind="stable")[:2]
        if mq.s[top[0]] - mq.s[top[1]] > mq.tol[top[0]] + mq.tol[top[1]]:
            assert rr[q][0][1] == exact[q][0][2] == ids[int(top[0])]
            compared += 1
    assert compared >= len(qids) // 2


def test_raw_classes_score_by_integer_ids():
    dim = 300
    off, comps, vals = random_dataset(3, 50, dim, 3, 20)
    nat = _native.NativeIndex.build(2, dim, off, comps, vals, BuildConfig.defaults(n_postings=10))
    ix = seismic_amd.SeismicIndexRaw(nat, upload=False)
    q_off, qc, qv = random_queries(4, 3, dim, 2, 8)
    qcs = [qc[q_off[i]:q_off[i + 1]] for i in range(3)]
    qvs = [qv[q_off[i]:q_off[i + 1]] for i in range(3)]
    lists = [[4, 4, 0], [], list(range(49, -1, -1))]
    got = ix.batch_score(qcs, qvs, lists, device=False)
    for q in range(3):
        want = np.array([orc.score_doc(nat.desc, d, qcs[q], qvs[q]) for d in lists[q]], np.float32)
        assert np.array_equal(got[q].view(np.uint32), want.view(np.uint32))
    with pytest.raises(KeyError):
        ix.score(qcs[0], qvs[0], [50], device=False)
    top = ix.batch_rerank(qcs, qvs, lists, 2, device=False)
    assert [len(r) for r in top] == [2, 0, 2] and all(isinstance(d, int) for r in top for _, d in r)
