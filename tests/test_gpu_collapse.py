"""sgpu_collapse_documents on the device: every row equal, as bits, to its host twin (and so to the restatement) on the
calls of tests/collapse_cases.py, for every index form and both forward layouts, with the dense table at dim 32767 and
the hash table at dim 32768; independent of the table form and of the cuts into launches; no state left from a
workgroup's previous query; the rerank equality; two replicas; safe beside a scoring and a searching thread; the device
argument checks (no fault is provoked: error paths are argument checks only); the Python classes."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

import collapse_cases
import seismic_amd
from collapse_cases import same
from seismic_amd import _native
from seismic_amd.index import read_jsonl

pytestmark = pytest.mark.gpu

GOLD_TOY = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "toy")
EDEVICE, ELIMIT = 2, 5


def _batch(case, names):
    """The queries of the named calls as one call: (q_off, qc, qv, cand_off, cand_ids, cand_groups)."""
    import orc
    queries, lists, groups = [], [], []
    for n in names:
        call = case.calls[n]
        queries += call.queries
        lists += call.lists
        groups += call.groups
    q_off, qc, qv = orc.csr(queries)
    cand_off = np.zeros(len(queries) + 1, np.uint64)
    cand_off[1:] = np.cumsum([len(x) for x in lists])
    return q_off, qc, qv, cand_off, np.concatenate(lists).astype(np.uint64), np.concatenate(groups).astype(np.uint32)


def _tiers(cand_off):
    """The selection launches of one launch over these queries: one per tier of list lengths that has a query."""
    n = np.diff(cand_off.astype(np.int64))
    return sum(int(((n > lo) & (n <= hi)).any()) for lo, hi in ((0, 128), (128, 512), (512, 1024), (1024, 4096)))


@pytest.mark.parametrize("layout", ["block", "doc"])
@pytest.mark.parametrize("name", sorted(collapse_cases.CASES))
def test_device_equals_host_twin(name, layout, monkeypatch):
    case = collapse_cases.make(name)
    monkeypatch.setenv("SGPU_FWD_LAYOUT", layout)   # (read by the upload)
    ix = case.build().upload(0)
    for call in case.calls.values():
        for m in call.ms:
            for k in call.ks:
                dev = ix.collapse_documents(*call.args(), m, k)
                host = ix.collapse_documents_host(*call.args(), m, k)
                assert same(host, case.expected(call.name, m, k)) is None
                assert same(dev, host) is None, (name, call.name, m, k, same(dev, host))
                st = ix.debug_collapse_stats()
                # dim 32767: the last dense table; dim 32768: the first hash table
                assert st["dense"] == (1 if case.dim <= 32767 else 0) and st["launches"] == 1
                assert st["select_launches"] == _tiers(call.cand_off) and st["grid"] >= 1
    # nothing to do: SGPU_OK
    out = ix.collapse_documents(np.zeros(1, np.uint64), np.zeros(0, np.uint32), np.zeros(0, np.float32), np.zeros(1, np.uint64),
                                np.zeros(0, np.uint64), np.zeros(0, np.uint32), 1, 8)
    assert len(out[5]) == 0
    ix.close()


@pytest.mark.parametrize("name", ["u16_f16_300", "u16_dvb_32767", "u16_u8_32767"])
def test_the_table_form_changes_no_row(name, monkeypatch):
    case = collapse_cases.make(name)
    ix = case.build().upload(0)
    monkeypatch.setenv("SGPU_SCORE_LOOKUP", "2")   # (test hook: the hash table although the dense one fits)
    for call_name, m, k in (("random", 3, 10), ("ties", 2, 4), ("top_m", 64, 7), ("sum_order", 3, 1), ("counts", 3, 10), ("keys", 1, 7)):
        call = case.calls[call_name]
        assert same(ix.collapse_documents(*call.args(), m, k), case.expected(call_name, m, k)) is None, (name, call_name)
        assert ix.debug_collapse_stats()["dense"] == 0
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
    case = collapse_cases.make(name)
    ix = case.build().upload(0)
    args = _batch(case, ["keys", "empty", "negative", "dups", "counts"])
    want = ix.collapse_documents(*args, 3, 6)
    assert ix.debug_collapse_stats()["launches"] == 1
    assert same(want, ix.collapse_documents_host(*args, 3, 6)) is None
    for chunk in (1, 64, 4096):
        monkeypatch.setenv("SGPU_SCORE_CHUNK", str(chunk))
        got = ix.collapse_documents(*args, 3, 6)
        monkeypatch.delenv("SGPU_SCORE_CHUNK")
        n = ix.debug_collapse_stats()["launches"]
        assert n == _launches(args[3], chunk) and n > 1, (chunk, n)
        assert same(got, want) is None, (chunk, same(got, want))
    ix.close()


@pytest.mark.parametrize("name", ["u16_f16_32767", "u16_f16_32768"])
def test_no_state_is_left_from_a_workgroups_previous_query(name, monkeypatch):
    """Some 350 queries over 3 workgroups per tier: each takes many queries in turn, so every pool query follows others of
    other lengths and group counts - among them the 4096-entry single group, the all-distinct one and an empty query."""
    import orc
    case = collapse_cases.make(name)
    pool = _batch(case, ["counts", "empty", "keys", "dups", "ties", "negative"])
    q_off, qc, qv, cand_off, cand_ids, cand_groups = pool
    n_pool = len(q_off) - 1
    assert int(np.diff(cand_off.astype(np.int64)).max()) == 4096
    pick = (np.arange(13 * n_pool) * 7) % n_pool   # (7 is coprime to the pool's size: asserted below)
    assert len(set(pick.tolist())) == n_pool
    queries = [(qc[int(q_off[i]):int(q_off[i + 1])], qv[int(q_off[i]):int(q_off[i + 1])]) for i in pick]
    lists = [cand_ids[int(cand_off[i]):int(cand_off[i + 1])] for i in pick]
    groups = [cand_groups[int(cand_off[i]):int(cand_off[i + 1])] for i in pick]
    Q_off, Qc, Qv = orc.csr(queries)
    C_off = np.zeros(len(pick) + 1, np.uint64)
    C_off[1:] = np.cumsum([len(x) for x in lists])
    args = (Q_off, Qc, Qv, C_off, np.concatenate(lists), np.concatenate(groups))
    ix = case.build().upload(0)
    monkeypatch.setenv("SGPU_COLLAPSE_GRID", "3")   # (test hook)
    dev = ix.collapse_documents(*args, 3, 5)
    st = ix.debug_collapse_stats()
    assert st["launches"] == 1 and st["select_launches"] == 4
    first = ix.collapse_documents_host(*pool, 3, 5)
    assert first[5].max() == 5 and first[5].min() == 0
    # every occurrence of a pool query has the row of its first one, which is the host twin's
    for a, b in zip(dev, first):
        assert all(np.array_equal(a[i], b[pick[i]]) for i in range(len(pick)))
    ix.close()


@pytest.mark.parametrize("name", ["u16_dvb_32767", "u32_u8_32768"])
def test_key_equal_to_id_is_rerank_on_the_device(name):
    case = collapse_cases.make(name)
    ix = case.build().upload(0)
    for call_name, k in (("counts", 10), ("random", 40), ("ties", 4), ("empty", 8), ("ks", 13)):
        q_off, qc, qv, cand_off, cand_ids, _ = case.calls[call_name].args()
        g, s, ids, bs, mem, n = ix.collapse_documents(q_off, qc, qv, cand_off, cand_ids, cand_ids.astype(np.uint32), 1, k)
        want = ix.rerank_documents(q_off, qc, qv, cand_off, cand_ids, k)
        assert same((s, ids, n), want, ("out_scores", "out_best_ids", "out_n")) is None, (name, call_name)
        assert np.array_equal(g, ids.astype(np.uint32)) and np.array_equal(s.view(np.uint32), bs.view(np.uint32))
    ix.close()


def test_two_replicas():
    case = collapse_cases.make("u16_u8_32767")
    ix = case.build().upload_many([0, 0])
    assert ix.replicas == 2
    call = case.calls["random"]
    for replica in (0, 1):
        assert same(ix.collapse_documents(*call.args(), 3, 10, replica=replica), case.expected("random", 3, 10)) is None
        assert ix.debug_collapse_stats(replica)["launches"] == 1
    ix.close()


def test_collapsing_beside_a_scoring_and_a_searching_thread():
    case = collapse_cases.make("u16_f16_32767")
    ix = case.build().upload(0)
    call = case.calls["random"]
    want = case.expected("random", 3, 10)
    score_args = (call.q_off, call.qc, call.qv, call.cand_off, call.cand_ids)
    want_scores = ix.score_documents(*score_args).view(np.uint32)
    want_rerank = ix.rerank_documents(*score_args, 10)
    want_search = ix.batch_search(call.q_off, call.qc, call.qv, 10, 4, 0.8)
    errors = []

    def collapse():
        for _ in range(10):
            if same(ix.collapse_documents(*call.args(), 3, 10), want) is not None:
                errors.append("collapse")

    def score():   # (rerank shares row buffers with collapse)
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

    threads = [threading.Thread(target=f) for f in (collapse, score, search)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    ix.close()


def test_device_argument_checks():
    case = collapse_cases.make("u16_f16_300")
    call = case.calls["random"]
    L = _native.lib()

    def run(ix, replica, m=1, k=10, cand_off=None, cand_ids=None, cand_groups=None):
        cand_off = call.cand_off if cand_off is None else cand_off
        cand_ids = call.cand_ids if cand_ids is None else cand_ids
        cand_groups = call.cand_groups if cand_groups is None else cand_groups
        rows = (call.nq, max(k, 1))
        outs = [np.zeros(rows, np.uint32), np.zeros(rows, np.float32), np.zeros(rows, np.uint64), np.zeros(rows, np.float32),
                np.zeros(rows, np.uint32), np.zeros(call.nq, np.uint32)]
        p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
        st = L.sgpu_collapse_documents(ix.h, replica, p(call.q_off), p(call.qc), p(call.qv), call.nq, p(cand_off), p(cand_ids),
                                       p(cand_groups), m, k, *[p(a) for a in outs])
        return st, L.sgpu_last_error().decode()

    st, msg = run(case.index, 0)           # not uploaded
    assert st == EDEVICE and "not uploaded" in msg
    ix = case.build().upload(0)
    assert run(ix, 0)[0] == 0
    st, msg = run(ix, 1)                   # replica out of range
    assert st == EDEVICE and "replica" in msg
    assert run(ix, 1, 1, 1025)[0] == ELIMIT    # (the limits are checked before the device)
    assert run(ix, 1, 65, 10)[0] == ELIMIT
    off = np.zeros(call.nq + 1, np.uint64)
    off[1:] = 4097
    assert run(ix, 1, 1, 10, off, np.zeros(4097, np.uint64), np.zeros(4097, np.uint32))[0] == ELIMIT
    ix.close()


@pytest.mark.parametrize("cls", ["SeismicIndex", "SeismicIndexLV", "SeismicIndexDotVByte"])
def test_python_collapse(cls):
    ids, _, _ = read_jsonl(os.path.join(GOLD_TOY, "documents.jsonl"))
    qids, qvecs, _ = read_jsonl(os.path.join(GOLD_TOY, "queries.jsonl"))
    qc = [np.array(list(v.keys())) for v in qvecs]
    qv = [np.array(list(v.values()), np.float32) for v in qvecs]
    ix = getattr(seismic_amd, cls).build(os.path.join(GOLD_TOY, "documents.jsonl"), n_postings=50, centroid_fraction=0.2)
    key_of = {d: i // 3 for i, d in enumerate(ids)}
    lists = [list(reversed(ids))[:40] if q % 2 else [ids[q % len(ids)]] * 3 + list(ids[:9]) for q in range(len(qc))]
    lists[1] = []
    groups = [[key_of[d] for d in row] for row in lists]
    dev = ix.batch_collapse(qc, qv, lists, groups, 4, m=2)
    host = ix.batch_collapse(qc, qv, lists, groups, 4, m=2, device=False)
    assert dev == host and any(len(r) == 4 for r in dev) and dev[1] == []
    assert ix.collapse(qc[0], qv[0], lists[0], groups[0], 4, m=2) == dev[0]
    ix.set_groups(key_of)
    assert ix.batch_collapse(qc, qv, lists, None, 4, m=2) == dev
    # batch_search_collapsed: the search, then the host twin over its hits
    got = ix.batch_search_collapsed(qids, qc, qv, 2, 10, 0.9, depth=30, m=2)
    hits = ix.batch_search(qids, qc, qv, 30, 10, 0.9)
    docs = [[d for _, _, d in row] for row in hits]
    want = ix.batch_collapse(qc, qv, docs, None, 2, m=2, device=False)
    assert [[r[1:] for r in row] for row in got] == want
    assert [[r[0] for r in row] for row in got] == [[str(q)] * len(row) for q, row in zip(qids, want)]
    assert any(len(row) == 2 for row in got)
