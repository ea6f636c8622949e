"""sgpu_expand_queries on the device: every row equal, as bits, to its host twin (and so to the restatement) on the calls
of tests/expand_cases.py, for every index form and both forward layouts, with the table in LDS at dim 32767 and in global
memory at dim 32768; independent of the cuts into launches; no state left from a workgroup's previous query; two replicas;
safe beside a scoring and a searching thread; its rows accepted by sgpu_batch_search; batch_search_feedback equal to its
three steps; the device argument checks (no fault is provoked: error paths are argument checks only)."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

import expand_cases
import seismic_amd
from expand_cases import same
from seismic_amd import _native
from seismic_amd.index import read_jsonl

pytestmark = pytest.mark.gpu

GOLD_TOY = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "toy")
EDEVICE, ELIMIT = 2, 5


def _batch(case, names):
    """The queries of the named calls (all of alpha = 1) as one call: (q_off, qc, qv, cand_off, cand_ids, cand_w, 1.0)."""
    import orc
    queries, lists, weights = [], [], []
    for n in names:
        call = case.calls[n]
        assert call.alpha == 1.0
        queries += call.queries
        lists += [np.asarray(x, np.uint64) for x in call.lists]
        weights += call.weights
    q_off, qc, qv = orc.csr(queries)
    cand_off = np.zeros(len(queries) + 1, np.uint64)
    cand_off[1:] = np.cumsum([len(x) for x in lists])
    return q_off, qc, qv, cand_off, np.concatenate(lists).astype(np.uint64), np.concatenate(weights).astype(np.float32), 1.0


@pytest.mark.parametrize("layout", ["block", "doc"])
@pytest.mark.parametrize("name", sorted(expand_cases.CASES))
def test_device_equals_host_twin(name, layout, monkeypatch):
    case = expand_cases.make(name)
    monkeypatch.setenv("SGPU_FWD_LAYOUT", layout)   # (read by the upload)
    ix = case.build().upload(0)
    for call in case.calls.values():
        for t in call.ts:
            dev = ix.expand_queries(*call.args(), t)
            host = ix.expand_queries_host(*call.args(), t)
            assert same(host, case.expected(call.name, t)) is None
            assert same(dev, host) is None, (name, call.name, t, same(dev, host))
            st = ix.debug_expand_stats()
            # dim 32767: the last table that fits LDS; dim 32768: the first in global memory
            assert st["dense"] == (1 if case.dim <= 32767 else 0) and st["launches"] == 1 and st["block"] == 1024
            assert st["grid"] == min(call.nq, st["grid"]) and (st["lds"] == 0) == (st["dense"] == 0)
            assert (st["table_bytes"] > 0) == (st["dense"] == 0)
    # nothing to do: SGPU_OK
    oc, ov, on = ix.expand_queries(np.zeros(1, np.uint64), np.zeros(0, np.uint32), np.zeros(0, np.float32), np.zeros(1, np.uint64),
                                   np.zeros(0, np.uint64), np.zeros(0, np.float32), 1.0, 8)
    assert len(on) == 0
    ix.close()


@pytest.mark.parametrize("name", ["u16_f16_300", "u16_dvb_32767"])
def test_the_table_form_changes_no_row(name, monkeypatch):
    case = expand_cases.make(name)
    ix = case.build().upload(0)
    monkeypatch.setenv("SGPU_SCORE_LOOKUP", "2")   # (test hook: the table in global memory although it fits LDS)
    for call_name, t in (("random", 10), ("ties", 30), ("lengths", 1024), ("order", 16)):
        call = case.calls[call_name]
        assert same(ix.expand_queries(*call.args(), t), case.expected(call_name, t)) is None
        assert ix.debug_expand_stats()["dense"] == 0
    ix.close()


def _launches(cand_off, chunk):
    """The launches the header promises: whole queries while their candidates fit the chunk, a larger query alone."""
    n, q, nq = 0, 0, len(cand_off) - 1
    while q < nq:
        first = int(cand_off[q])
        q += 1
        while q < nq and int(cand_off[q + 1]) - first <= chunk:
            q += 1
        n += 1
    return n


@pytest.mark.parametrize("name", ["u16_dvb_32767", "u32_f16_32768"])
def test_the_cuts_into_launches_change_no_row(name, monkeypatch):
    case = expand_cases.make(name)
    ix = case.build().upload(0)
    args = _batch(case, ["random", "empty", "lengths", "order", "ties", "many"])   # candidates per query: 10 x 8, 0, 3, 0, 9, 3, 0, 2
    want = ix.expand_queries(*args, 64)
    assert ix.debug_expand_stats()["launches"] == 1
    assert same(want, ix.expand_queries_host(*args, 64)) is None
    for chunk in (1, 5, 10, 25):   # (5: every query of 9 or 10 candidates is larger than the chunk and goes alone)
        monkeypatch.setenv("SGPU_SCORE_CHUNK", str(chunk))
        got = ix.expand_queries(*args, 64)
        monkeypatch.delenv("SGPU_SCORE_CHUNK")
        n = ix.debug_expand_stats()["launches"]
        assert n == _launches(args[3], chunk) and n > 1, (chunk, n)
        assert same(got, want) is None, (chunk, same(got, want))
    ix.close()


@pytest.mark.parametrize("name", ["u16_f16_32767", "u16_f16_32768"])
def test_no_state_is_left_from_a_workgroups_previous_query(name, monkeypatch):
    """600 queries over 16 workgroups: each takes some 38 queries in turn, query i + 16 after query i. The pool of 21 queries
    (21 and 16 are coprime) puts every query behind every other one in some workgroup - among them the one of more than
    1024 terms, followed by a query of two terms and by one without any."""
    case = expand_cases.make(name)
    pool = _batch(case, ["many", "order", "empty", "random", "negative", "lengths", "ties", "repeat", "empty", "order"])
    q_off, qc, qv, cand_off, cand_ids, cand_w, alpha = pool
    n_pool = len(q_off) - 1
    assert n_pool == 21
    pick = np.arange(600) % n_pool
    import orc
    queries = [(qc[int(q_off[i]):int(q_off[i + 1])], qv[int(q_off[i]):int(q_off[i + 1])]) for i in pick]
    lists = [cand_ids[int(cand_off[i]):int(cand_off[i + 1])] for i in pick]
    ws = [cand_w[int(cand_off[i]):int(cand_off[i + 1])] for i in pick]
    Q_off, Qc, Qv = orc.csr(queries)
    C_off = np.zeros(601, np.uint64)
    C_off[1:] = np.cumsum([len(x) for x in lists])
    args = (Q_off, Qc, Qv, C_off, np.concatenate(lists), np.concatenate(ws), alpha)
    ix = case.build().upload(0)
    monkeypatch.setenv("SGPU_EXPAND_GRID", "16")   # (test hook)
    dev = ix.expand_queries(*args, 1024)
    st = ix.debug_expand_stats()
    assert st["grid"] == 16 and st["launches"] == 1
    host = ix.expand_queries_host(*args, 1024)
    assert same(dev, host) is None, same(dev, host)
    assert host[2].max() == 1024 and host[2].min() == 0
    # every occurrence of a pool query has the row of its first one
    for a in dev:
        assert all(np.array_equal(a[i], a[i % n_pool]) for i in range(n_pool, 600))
    ix.close()


def test_two_replicas():
    case = expand_cases.make("u16_u8_32767")
    ix = case.build().upload_many([0, 0])
    assert ix.replicas == 2
    call = case.calls["random"]
    for replica in (0, 1):
        assert same(ix.expand_queries(*call.args(), 64, replica=replica), case.expected("random", 64)) is None
        assert ix.debug_expand_stats(replica)["launches"] == 1
    ix.close()


def test_expanding_beside_a_scoring_and_a_searching_thread():
    case = expand_cases.make("u16_f16_32767")
    ix = case.build().upload(0)
    call = case.calls["random"]
    want = case.expected("random", 64)
    score_args = (call.q_off, call.qc, call.qv, call.cand_off, call.cand_ids)
    want_scores = ix.score_documents(*score_args).view(np.uint32)
    want_search = ix.batch_search(call.q_off, call.qc, call.qv, 10, 4, 0.8)
    errors = []

    def expand():
        for _ in range(10):
            if same(ix.expand_queries(*call.args(), 64), want) is not None:
                errors.append("expand")

    def score():
        for _ in range(10):
            if not np.array_equal(ix.score_documents(*score_args).view(np.uint32), want_scores):
                errors.append("score")

    def search():
        for _ in range(10):
            sc, ids, n = ix.batch_search(call.q_off, call.qc, call.qv, 10, 4, 0.8)
            if not (np.array_equal(n, want_search[2]) and np.array_equal(ids, want_search[1])
                    and np.array_equal(sc.view(np.uint32), want_search[0].view(np.uint32))):
                errors.append("search")

    threads = [threading.Thread(target=f) for f in (expand, score, search)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    ix.close()


@pytest.mark.parametrize("name", ["u16_f16_32767", "u32_u8_32768"])
def test_the_rows_are_queries_for_batch_search(name):
    case = expand_cases.make(name)
    ix = case.build().upload(0)
    for call_name, t in (("random", 64), ("many", 1024), ("empty", 8)):
        call = case.calls[call_name]
        oc, ov, on = ix.expand_queries(*call.args(), t)
        off = np.zeros(call.nq + 1, np.uint64)
        off[1:] = np.cumsum(on)
        qc = np.concatenate([oc[q, :on[q]] for q in range(call.nq)])
        qv = np.concatenate([ov[q, :on[q]] for q in range(call.nq)])
        sc, ids, n = ix.batch_search(off, qc, qv, 10, 4, 0.8)   # (raises where the batch is refused)
        assert all(n[q] > 0 for q in range(call.nq) if on[q]) and all(n[q] == 0 for q in range(call.nq) if not on[q])
    ix.close()


def test_device_argument_checks():
    case = expand_cases.make("u16_f16_300")
    call = case.calls["random"]
    L = _native.lib()

    def run(ix, replica, t=10):
        outs = [np.zeros((call.nq, max(t, 1)), np.uint32), np.zeros((call.nq, max(t, 1)), np.float32), np.zeros(call.nq, np.uint32)]
        p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
        st = L.sgpu_expand_queries(ix.h, replica, p(call.q_off), p(call.qc), p(call.qv), call.nq, p(call.cand_off), p(call.cand_ids),
                                   p(call.cand_w), 1.0, t, *[p(a) for a in outs])
        return st, L.sgpu_last_error().decode()

    st, msg = run(case.index, 0)           # not uploaded
    assert st == EDEVICE and "not uploaded" in msg
    ix = case.build().upload(0)
    assert run(ix, 0)[0] == 0
    st, msg = run(ix, 1)                   # replica out of range
    assert st == EDEVICE and "replica" in msg
    assert run(ix, 1, 1025)[0] == ELIMIT   # (t is checked before the device)
    ix.close()


@pytest.mark.parametrize("cls", ["SeismicIndex", "SeismicIndexLV", "SeismicIndexDotVByte"])
def test_python_expand_and_feedback_search(cls):
    ids, _, _ = read_jsonl(os.path.join(GOLD_TOY, "documents.jsonl"))
    _, qvecs, _ = read_jsonl(os.path.join(GOLD_TOY, "queries.jsonl"))
    qids = list(range(len(qvecs)))
    qc = [np.array(list(v.keys())) for v in qvecs]
    qv = [np.array(list(v.values()), np.float32) for v in qvecs]
    ix = getattr(seismic_amd, cls).build(os.path.join(GOLD_TOY, "documents.jsonl"), n_postings=50, centroid_fraction=0.2)
    lists = [list(reversed(ids))[:7] if q % 2 else [ids[q % len(ids)]] * 3 for q in range(len(qc))]
    lists[1] = []
    dev = ix.batch_expand(qc, qv, lists, terms=32)
    host = ix.batch_expand(qc, qv, lists, terms=32, device=False)
    assert [t for t, _ in dev] == [t for t, _ in host]
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for (_, a), (_, b) in zip(dev, host))
    one = ix.expand(qc[0], qv[0], lists[0], terms=32)
    assert one[0] == dev[0][0] and np.array_equal(one[1], dev[0][1])
    # batch_search_feedback is its three steps
    got = ix.batch_search_feedback(qids, qc, qv, 5, 4, 0.8, fb_docs=3, fb_terms=16, alpha=1.0, beta=0.5)
    first = ix.batch_search(qids, qc, qv, 5, 4, 0.8)
    fb = [[d for _, _, d in row[:3]] for row in first]
    exp = ix.batch_expand(qc, qv, fb, None, 1.0, 0.5, 16)
    assert any(len(t) == 16 for t, _ in exp)
    want = ix.batch_search(qids, [np.asarray(t, dtype=str) for t, _ in exp], [v for _, v in exp], 5, 4, 0.8)
    assert got == want and len(got) == len(qids) and any(got)
