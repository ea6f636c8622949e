"""sgpu_diversify_documents on the device: every row equal, as bits, to its host twin (and so to the restatement) on the
calls of tests/diversify_cases.py, for every index form and both forward layouts, with the dense table at dim 32767 and
the hash table at dim 32768; independent of the table form and of the cuts into launches; no state left from a
workgroup's previous query; two replicas; safe beside a scoring and a searching thread; the device argument checks (no
fault is provoked: error paths are argument checks only); the Python classes."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

import diversify_cases
import seismic_amd
from diversify_cases import same
from seismic_amd import _native
from seismic_amd.index import read_jsonl

pytestmark = pytest.mark.gpu

GOLD_TOY = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "toy")
EDEVICE, ELIMIT = 2, 5


def _batch(case, names):
    """The queries of the named calls (all of lambda = mu = 0.5) as one call: (q_off, qc, qv, cand_off, cand_ids, 0.5, 0.5)."""
    import orc
    queries, lists = [], []
    for n in names:
        call = case.calls[n]
        assert call.lam == 0.5 and call.mu == 0.5
        queries += call.queries
        lists += call.lists
    q_off, qc, qv = orc.csr(queries)
    cand_off = np.zeros(len(queries) + 1, np.uint64)
    cand_off[1:] = np.cumsum([len(x) for x in lists])
    return q_off, qc, qv, cand_off, np.concatenate(lists).astype(np.uint64), 0.5, 0.5


@pytest.mark.parametrize("layout", ["block", "doc"])
@pytest.mark.parametrize("name", sorted(diversify_cases.CASES))
def test_device_equals_host_twin(name, layout, monkeypatch):
    case = diversify_cases.make(name)
    monkeypatch.setenv("SGPU_FWD_LAYOUT", layout)   # (read by the upload)
    ix = case.build().upload(0)
    for call in case.calls.values():
        for k in call.ks:
            dev = ix.diversify_documents(*call.args(), k)
            host = ix.diversify_documents_host(*call.args(), k)
            assert same(host, case.expected(call.name, k)) is None
            assert same(dev, host) is None, (name, call.name, k, same(dev, host))
            st = ix.debug_diversify_stats()
            # dim 32767: the last dense table; dim 32768: the first hash table
            assert st["dense"] == (1 if case.dim <= 32767 else 0) and st["launches"] == 1 and st["block"] == 1024
            assert 1 <= st["grid"] <= call.nq and st["rounds"] == host[3].max()
            assert st["lds"] % 16 == 0 and st["lds"] <= 160 * 1024
    # nothing to do: SGPU_OK
    sc, pen, ids, n = ix.diversify_documents(np.zeros(1, np.uint64), np.zeros(0, np.uint32), np.zeros(0, np.float32),
                                             np.zeros(1, np.uint64), np.zeros(0, np.uint64), 0.5, 0.5, 8)
    assert len(n) == 0
    ix.close()


@pytest.mark.parametrize("name", ["u16_f16_300", "u16_dvb_32767", "u16_u8_32767"])
def test_the_table_form_changes_no_row(name, monkeypatch):
    case = diversify_cases.make(name)
    ix = case.build().upload(0)
    monkeypatch.setenv("SGPU_SCORE_LOOKUP", "2")   # (test hook: the hash table although the dense one fits)
    for call_name, k in (("random", 10), ("ties", 7), ("lengths", 9), ("order", 3), ("counts", 4), ("empty_first", 4)):
        if call_name not in case.calls:
            continue
        call = case.calls[call_name]
        assert same(ix.diversify_documents(*call.args(), k), case.expected(call_name, k)) is None, (name, call_name)
        assert ix.debug_diversify_stats()["dense"] == 0
    ix.close()


def _launches(cand_off, chunk):
    """The launches the header promises: whole queries while their candidates fit the chunk, a larger query alone; a
    run of queries without any candidate is no launch."""
    n, q, nq = 0, 0, len(cand_off) - 1
    while q < nq:
        first = int(cand_off[q])
        q += 1
        while q < nq and int(cand_off[q + 1]) - first <= chunk:
            q += 1
        n += 1 if int(cand_off[q]) > first else 0
    return n


@pytest.mark.parametrize("name", ["u16_dvb_32767", "u32_f16_32768"])
def test_the_cuts_into_launches_change_no_row(name, monkeypatch):
    case = diversify_cases.make(name)
    ix = case.build().upload(0)
    args = _batch(case, ["lengths", "empty", "empty_first", "dups", "counts"])   # candidates: 9 9 0 3 0 5 8 1 2 63 ... 2048
    want = ix.diversify_documents(*args, 6)
    assert ix.debug_diversify_stats()["launches"] == 1
    assert same(want, ix.diversify_documents_host(*args, 6)) is None
    for chunk in (1, 5, 50):
        monkeypatch.setenv("SGPU_SCORE_CHUNK", str(chunk))
        got = ix.diversify_documents(*args, 6)
        monkeypatch.delenv("SGPU_SCORE_CHUNK")
        n = ix.debug_diversify_stats()["launches"]
        assert n == _launches(args[3], chunk) and n > 1, (chunk, n)
        assert same(got, want) is None, (chunk, same(got, want))
    ix.close()


@pytest.mark.parametrize("name", ["u16_f16_32767", "u16_f16_32768"])
def test_no_state_is_left_from_a_workgroups_previous_query(name, monkeypatch):
    """600 queries over 16 workgroups: each takes some 38 queries in turn, query i + 16 after query i. The pool's size is
    coprime to 16, so every pool query follows every other one in some workgroup - among them the one of 2048 candidates,
    one without candidates and one whose first pick is the empty document (it leaves an empty table behind)."""
    import math
    import orc
    case = diversify_cases.make(name)
    pool = _batch(case, ["counts", "empty", "empty_first", "lengths", "dups", "empty_first"])
    q_off, qc, qv, cand_off, cand_ids, lam, mu = pool
    n_pool = len(q_off) - 1
    assert n_pool == 17 and math.gcd(n_pool, 16) == 1 and int(np.diff(cand_off.astype(np.int64)).max()) == 2048
    pick = np.arange(600) % n_pool
    queries = [(qc[int(q_off[i]):int(q_off[i + 1])], qv[int(q_off[i]):int(q_off[i + 1])]) for i in pick]
    lists = [cand_ids[int(cand_off[i]):int(cand_off[i + 1])] for i in pick]
    Q_off, Qc, Qv = orc.csr(queries)
    C_off = np.zeros(601, np.uint64)
    C_off[1:] = np.cumsum([len(x) for x in lists])
    args = (Q_off, Qc, Qv, C_off, np.concatenate(lists), lam, mu)
    ix = case.build().upload(0)
    monkeypatch.setenv("SGPU_DIVERSIFY_GRID", "16")   # (test hook)
    dev = ix.diversify_documents(*args, 3)
    st = ix.debug_diversify_stats()
    assert st["grid"] == 16 and st["launches"] == 1
    first = ix.diversify_documents_host(*pool, 3)
    assert first[3].max() == 3 and first[3].min() == 0
    # every occurrence of a pool query has the row of its first one, which is the host twin's
    for a, b in zip(dev, first):
        assert all(np.array_equal(a[i], b[i % n_pool]) for i in range(600))
    assert same(tuple(a[:n_pool] for a in dev), first) is None
    ix.close()


def test_two_replicas():
    case = diversify_cases.make("u16_u8_32767")
    ix = case.build().upload_many([0, 0])
    assert ix.replicas == 2
    call = case.calls["random"]
    for replica in (0, 1):
        assert same(ix.diversify_documents(*call.args(), 10, replica=replica), case.expected("random", 10)) is None
        assert ix.debug_diversify_stats(replica)["launches"] == 1
    ix.close()


def test_diversifying_beside_a_scoring_and_a_searching_thread():
    case = diversify_cases.make("u16_f16_32767")
    ix = case.build().upload(0)
    call = case.calls["random"]
    want = case.expected("random", 10)
    score_args = (call.q_off, call.qc, call.qv, call.cand_off, call.cand_ids)
    want_scores = ix.score_documents(*score_args).view(np.uint32)
    want_rerank = ix.rerank_documents(*score_args, 10)
    want_search = ix.batch_search(call.q_off, call.qc, call.qv, 10, 4, 0.8)
    errors = []

    def diversify():
        for _ in range(10):
            if same(ix.diversify_documents(*call.args(), 10), want) is not None:
                errors.append("diversify")

    def score():   # (rerank shares the row buffers with diversify)
        for _ in range(10):
            if not np.array_equal(ix.score_documents(*score_args).view(np.uint32), want_scores):
                errors.append("score")
            if same(ix.rerank_documents(*score_args, 10), want_rerank, ("scores", "ids", "n")) is not None:
                errors.append("rerank")

    def search():
        for _ in range(10):
            sc, ids, n = ix.batch_search(call.q_off, call.qc, call.qv, 10, 4, 0.8)
            if not (np.array_equal(n, want_search[2]) and np.array_equal(ids, want_search[1])
                    and np.array_equal(sc.view(np.uint32), want_search[0].view(np.uint32))):
                errors.append("search")

    threads = [threading.Thread(target=f) for f in (diversify, score, search)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    ix.close()


def test_device_argument_checks():
    case = diversify_cases.make("u16_f16_300")
    call = case.calls["random"]
    L = _native.lib()

    def run(ix, replica, k=10, cand_off=None, cand_ids=None):
        cand_off = call.cand_off if cand_off is None else cand_off
        cand_ids = call.cand_ids if cand_ids is None else cand_ids
        rows = (call.nq, max(k, 1))
        outs = [np.zeros(rows, np.float32), np.zeros(rows, np.float32), np.zeros(rows, np.uint64), np.zeros(call.nq, np.uint32)]
        p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
        st = L.sgpu_diversify_documents(ix.h, replica, p(call.q_off), p(call.qc), p(call.qv), call.nq, p(cand_off), p(cand_ids),
                                        0.5, 0.5, k, *[p(a) for a in outs])
        return st, L.sgpu_last_error().decode()

    st, msg = run(case.index, 0)           # not uploaded
    assert st == EDEVICE and "not uploaded" in msg
    ix = case.build().upload(0)
    assert run(ix, 0)[0] == 0
    st, msg = run(ix, 1)                   # replica out of range
    assert st == EDEVICE and "replica" in msg
    assert run(ix, 1, 257)[0] == ELIMIT    # (the limits are checked before the device)
    off = np.zeros(call.nq + 1, np.uint64)
    off[1:] = 2049
    assert run(ix, 1, 10, off, np.zeros(2049, np.uint64))[0] == ELIMIT
    ix.close()


@pytest.mark.parametrize("cls", ["SeismicIndex", "SeismicIndexLV", "SeismicIndexDotVByte"])
def test_python_diversify(cls):
    ids, _, _ = read_jsonl(os.path.join(GOLD_TOY, "documents.jsonl"))
    _, qvecs, _ = read_jsonl(os.path.join(GOLD_TOY, "queries.jsonl"))
    qc = [np.array(list(v.keys())) for v in qvecs]
    qv = [np.array(list(v.values()), np.float32) for v in qvecs]
    ix = getattr(seismic_amd, cls).build(os.path.join(GOLD_TOY, "documents.jsonl"), n_postings=50, centroid_fraction=0.2)
    lists = [list(reversed(ids))[:40] if q % 2 else [ids[q % len(ids)]] * 3 + list(ids[:9]) for q in range(len(qc))]
    lists[1] = []
    dev = ix.batch_diversify(qc, qv, lists, 8)
    host = ix.batch_diversify(qc, qv, lists, 8, device=False)
    assert dev == host and any(len(r) == 8 for r in dev) and dev[1] == []
    assert ix.diversify(qc[0], qv[0], lists[0], 8) == dev[0]
    plain = ix.batch_diversify(qc, qv, lists, 8, lam=1.0, mu=0.0)
    assert [[(s, d) for s, _, d in row] for row in plain] == ix.batch_rerank(qc, qv, lists, 8)
