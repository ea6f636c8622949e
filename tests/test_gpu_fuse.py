"""sgpu_fuse_documents on the device: every row equal, as bits, to its host twin (and so to the restatement) on the calls
of tests/fuse_cases.py, for every index form and both forward layouts, with the dense table at dim 32767 and the hash
table at dim 32768; independent of the table form and of the cuts into launches; no state left from a workgroup's
previous query; the rerank and rank consequences; two replicas; safe beside a scoring and a searching thread; the device
argument checks (no fault is provoked: error paths are argument checks only); the Python classes."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

import fuse_cases
import seismic_amd
from fuse_cases import MINMAX, RRF, SUM, same
from seismic_amd import _native
from seismic_amd.index import read_jsonl

pytestmark = pytest.mark.gpu

GOLD_TOY = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "toy")
EDEVICE, ELIMIT = 2, 5


def _batch(case, names):
    """The queries of the named calls as one call: (q_off, qc, qv, cand_off, cand_ids, cand_ext)."""
    import orc
    queries, lists, exts = [], [], []
    for n in names:
        call = case.calls[n]
        queries += call.queries
        lists += call.lists
        exts += call.exts
    q_off, qc, qv = orc.csr(queries)
    cand_off = np.zeros(len(queries) + 1, np.uint64)
    cand_off[1:] = np.cumsum([len(x) for x in lists])
    return q_off, qc, qv, cand_off, np.concatenate(lists).astype(np.uint64), np.concatenate(exts).astype(np.float32)


def _tiers(cand_off):
    """The selection launches of one launch over these queries: one per tier of list lengths that has a query."""
    n = np.diff(cand_off.astype(np.int64))
    return sum(int(((n > lo) & (n <= hi)).any()) for lo, hi in ((0, 128), (128, 512), (512, 1024), (1024, 4096)))


@pytest.mark.parametrize("layout", ["block", "doc"])
@pytest.mark.parametrize("name", sorted(fuse_cases.CASES))
def test_device_equals_host_twin(name, layout, monkeypatch):
    case = fuse_cases.make(name)
    monkeypatch.setenv("SGPU_FWD_LAYOUT", layout)   # (read by the upload)
    ix = case.build().upload(0)
    for call in case.calls.values():
        for config in call.configs:
            for k in call.ks:
                dev = ix.fuse_documents(*call.args(), *config, k)
                host = ix.fuse_documents_host(*call.args(), *config, k)
                assert same(host, case.expected(call.name, config, k)) is None
                assert same(dev, host) is None, (name, call.name, config, k, same(dev, host))
                st = ix.debug_fuse_stats()
                # dim 32767: the last dense table; dim 32768: the first hash table
                if call.cand_off[-1]:
                    assert st["dense"] == (1 if case.dim <= 32767 else 0) and st["launches"] == 1
                    assert st["select_launches"] == _tiers(call.cand_off) and st["grid"] >= 1
    # nothing to do: SGPU_OK
    out = ix.fuse_documents(np.zeros(1, np.uint64), np.zeros(0, np.uint32), np.zeros(0, np.float32), np.zeros(1, np.uint64),
                            np.zeros(0, np.uint64), np.zeros(0, np.float32), RRF, 1.0, 1.0, 60.0, 8)
    assert len(out[6]) == 0
    ix.close()


@pytest.mark.parametrize("name", ["u16_f16_300", "u16_dvb_32767", "u16_u8_32767"])
def test_the_table_form_changes_no_row(name, monkeypatch):
    case = fuse_cases.make(name)
    ix = case.build().upload(0)
    monkeypatch.setenv("SGPU_SCORE_LOOKUP", "2")   # (test hook: the hash table although the dense one fits)
    for call_name in ("random", "ties", "dups", "counts", "methods"):
        call = case.calls[call_name]
        for config in call.configs[:3]:
            k = call.ks[-1]
            assert same(ix.fuse_documents(*call.args(), *config, k), case.expected(call_name, config, k)) is None, (name, call_name)
            assert ix.debug_fuse_stats()["dense"] == 0
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
    case = fuse_cases.make(name)
    ix = case.build().upload(0)
    args = _batch(case, ["ties", "empty", "absent", "dups", "counts", "negzero"])
    for config in ((RRF, 1.0, 0.5, 60.0), (MINMAX, 0.5, -0.25, 0.0)):
        want = ix.fuse_documents(*args, *config, 6)
        assert ix.debug_fuse_stats()["launches"] == 1
        assert same(want, ix.fuse_documents_host(*args, *config, 6)) is None
        for chunk in (1, 7, 100, 5000):
            monkeypatch.setenv("SGPU_SCORE_CHUNK", str(chunk))
            got = ix.fuse_documents(*args, *config, 6)
            monkeypatch.delenv("SGPU_SCORE_CHUNK")
            n = ix.debug_fuse_stats()["launches"]
            assert n == _launches(args[3], chunk) and n > 1, (chunk, n)
            assert same(got, want) is None, (chunk, same(got, want))
    ix.close()


@pytest.mark.parametrize("name", ["u16_f16_32767", "u16_f16_32768"])
def test_no_state_is_left_from_a_workgroups_previous_query(name, monkeypatch):
    """One workgroup takes every query of a tier in turn: a 4096-entry query and a 1-entry one alternate, present and
    absent ones too - among them all entries one id, 4096 documents none present and 4096 all present -, then the pool of
    the other calls, every query following others of other lengths and document counts."""
    import orc
    case = fuse_cases.make(name)
    counts = case.calls["counts"]
    big = [len(counts.lists) - 4 + i for i in range(4)]   # one id / each id twice / none present / all present
    assert [len(counts.lists[i]) for i in big] == [4096] * 4 and len(counts.lists[0]) == 1
    one_absent = (counts.queries[0], counts.lists[0], fuse_cases._ext([None]))
    one_present = (counts.queries[0], counts.lists[0], fuse_cases._ext([1.5]))
    seq = []
    for i in big + big[::-1]:
        seq += [(counts.queries[i], counts.lists[i], counts.exts[i]), one_absent if len(seq) % 4 == 0 else one_present]
    pool = _batch(case, ["counts", "empty", "ties", "dups", "absent", "negzero"])
    q_off, qc, qv, cand_off, cand_ids, cand_ext = pool
    n_pool = len(q_off) - 1
    pick = (np.arange(3 * n_pool) * 7) % n_pool   # (7 is coprime to the pool's size: asserted below)
    assert len(set(pick.tolist())) == n_pool
    for i in pick:
        a, b = int(cand_off[i]), int(cand_off[i + 1])
        seq.append(((qc[int(q_off[i]):int(q_off[i + 1])], qv[int(q_off[i]):int(q_off[i + 1])]), cand_ids[a:b], cand_ext[a:b]))
    Q_off, Qc, Qv = orc.csr([s[0] for s in seq])
    C_off = np.zeros(len(seq) + 1, np.uint64)
    C_off[1:] = np.cumsum([len(s[1]) for s in seq])
    args = (Q_off, Qc, Qv, C_off, np.concatenate([s[1] for s in seq]).astype(np.uint64),
            np.concatenate([s[2] for s in seq]).astype(np.float32))
    ix = case.build().upload(0)
    monkeypatch.setenv("SGPU_FUSE_GRID", "1")   # (test hook)
    for config in ((RRF, 1.0, 1.0, 60.0), (MINMAX, 1.0, 1.0, 0.0)):
        dev = ix.fuse_documents(*args, *config, 5)
        st = ix.debug_fuse_stats()
        assert st["launches"] == 1 and st["select_launches"] == 4
        host = ix.fuse_documents_host(*args, *config, 5)
        assert host[6].max() == 5 and host[6].min() == 0
        assert same(dev, host) is None, (config, same(dev, host))
    ix.close()


@pytest.mark.parametrize("name", ["u16_dvb_32767", "u32_u8_32768"])
def test_the_consequences_against_rerank_on_the_device(name):
    case = fuse_cases.make(name)
    ix = case.build().upload(0)
    for call_name, k in (("counts", 10), ("random", 60), ("ties", 4), ("empty", 8), ("ks", 13)):
        q_off, qc, qv, cand_off, cand_ids, cand_ext = case.calls[call_name].args()
        want = ix.rerank_documents(q_off, qc, qv, cand_off, cand_ids, k)
        f, ids, sp, ex, rs, re, n = ix.fuse_documents(q_off, qc, qv, cand_off, cand_ids, cand_ext, SUM, 1.0, 0.0, 0.0, k)
        assert same((sp, ids, n), want, ("out_sparse", "out_doc_ids", "out_n")) is None, (name, call_name)
        assert np.array_equal(f.view(np.uint32), sp.view(np.uint32))
        f, ids, sp, ex, rs, re, n = ix.fuse_documents(q_off, qc, qv, cand_off, cand_ids, cand_ext, RRF, 1.0, 0.0, 60.0, k)
        assert same((ids, n), want[1:], ("out_doc_ids", "out_n")) is None, (name, call_name)
        filled = np.arange(k)[None, :] < n[:, None]
        assert np.array_equal(rs, np.where(filled, np.arange(k)[None, :] + 1, 0))
    ix.close()


def test_two_replicas():
    case = fuse_cases.make("u16_u8_32767")
    ix = case.build().upload_many([0, 0])
    assert ix.replicas == 2
    call = case.calls["random"]
    for replica in (0, 1):
        for config in call.configs[:3]:
            assert same(ix.fuse_documents(*call.args(), *config, 10, replica=replica), case.expected("random", config, 10)) is None
        assert ix.debug_fuse_stats(replica)["launches"] == 1
    ix.close()


def test_fusing_beside_a_scoring_and_a_searching_thread():
    case = fuse_cases.make("u16_f16_32767")
    ix = case.build().upload(0)
    call = case.calls["random"]
    config = call.configs[1]
    want = case.expected("random", config, 10)
    score_args = (call.q_off, call.qc, call.qv, call.cand_off, call.cand_ids)
    want_scores = ix.score_documents(*score_args).view(np.uint32)
    want_rerank = ix.rerank_documents(*score_args, 10)
    groups = (call.cand_ids % 7).astype(np.uint32)
    want_collapse = ix.collapse_documents(*score_args, groups, 2, 10)
    want_search = ix.batch_search(call.q_off, call.qc, call.qv, 10, 4, 0.8)
    errors = []

    def fuse():
        for _ in range(10):
            if same(ix.fuse_documents(*call.args(), *config, 10), want) is not None:
                errors.append("fuse")

    def score():   # (rerank and collapse share row buffers with fuse)
        for _ in range(10):
            if not np.array_equal(ix.score_documents(*score_args).view(np.uint32), want_scores):
                errors.append("score")
            if same(ix.rerank_documents(*score_args, 10), want_rerank, ("scores", "ids", "n")) is not None:
                errors.append("rerank")
            if same(ix.collapse_documents(*score_args, groups, 2, 10), want_collapse, ("g", "s", "ids", "bs", "mem", "n")) is not None:
                errors.append("collapse")

    def search():
        for _ in range(10):
            sc, ids, n = ix.batch_search(call.q_off, call.qc, call.qv, 10, 4, 0.8)
            if not (np.array_equal(n, want_search[2]) and np.array_equal(ids, want_search[1])
                    and np.array_equal(sc.view(np.uint32), want_search[0].view(np.uint32))):
                errors.append("search")

    threads = [threading.Thread(target=f) for f in (fuse, score, search)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    ix.close()


def test_device_argument_checks():
    case = fuse_cases.make("u16_f16_300")
    call = case.calls["random"]
    L = _native.lib()

    def run(ix, replica, method=RRF, k=10, cand_off=None, cand_ids=None, cand_ext=None):
        cand_off = call.cand_off if cand_off is None else cand_off
        cand_ids = call.cand_ids if cand_ids is None else cand_ids
        cand_ext = call.cand_ext if cand_ext is None else cand_ext
        rows = (call.nq, max(k, 1))
        outs = [np.zeros(rows, np.float32), np.zeros(rows, np.uint64), np.zeros(rows, np.float32), np.zeros(rows, np.float32),
                np.zeros(rows, np.uint32), np.zeros(rows, np.uint32), np.zeros(call.nq, np.uint32)]
        p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
        st = L.sgpu_fuse_documents(ix.h, replica, p(call.q_off), p(call.qc), p(call.qv), call.nq, p(cand_off), p(cand_ids),
                                   p(cand_ext), method, 1.0, 1.0, 60.0, k, *[p(a) for a in outs])
        return st, L.sgpu_last_error().decode()

    st, msg = run(case.index, 0)           # not uploaded
    assert st == EDEVICE and "not uploaded" in msg
    ix = case.build().upload(0)
    assert run(ix, 0)[0] == 0
    st, msg = run(ix, 1)                   # replica out of range
    assert st == EDEVICE and "replica" in msg
    assert run(ix, 1, RRF, 1025)[0] == ELIMIT    # (the limits are checked before the device)
    assert run(ix, 1, 3, 10)[0] == 1
    off = np.zeros(call.nq + 1, np.uint64)
    off[1:] = 4097
    assert run(ix, 1, RRF, 10, off, np.zeros(4097, np.uint64), np.zeros(4097, np.float32))[0] == ELIMIT
    ix.close()


@pytest.mark.parametrize("cls", ["SeismicIndex", "SeismicIndexLV", "SeismicIndexDotVByte"])
def test_python_fuse(cls):
    ids, _, _ = read_jsonl(os.path.join(GOLD_TOY, "documents.jsonl"))
    qids, qvecs, _ = read_jsonl(os.path.join(GOLD_TOY, "queries.jsonl"))
    qc = [np.array(list(v.keys())) for v in qvecs]
    qv = [np.array(list(v.values()), np.float32) for v in qvecs]
    ix = getattr(seismic_amd, cls).build(os.path.join(GOLD_TOY, "documents.jsonl"), n_postings=50, centroid_fraction=0.2)
    lists = [list(reversed(ids))[:40] if q % 2 else [ids[q % len(ids)]] * 3 + list(ids[:9]) for q in range(len(qc))]
    lists[1] = []
    ext = [[None if i % 3 == 1 else float((i * 5) % 7) - 2.0 for i in range(len(row))] for row in lists]
    for method in ("rrf", "minmax", "sum"):
        dev = ix.batch_fuse(qc, qv, lists, ext, 4, method=method, w_sparse=0.7, w_ext=0.3)
        host = ix.batch_fuse(qc, qv, lists, ext, 4, method=method, w_sparse=0.7, w_ext=0.3, device=False)
        assert dev == host and any(len(r) == 4 for r in dev) and dev[1] == []
    assert ix.fuse(qc[0], qv[0], lists[0], ext[0], 4, method="sum", w_sparse=0.7, w_ext=0.3) == dev[0]
    # batch_search_fused: the search, the union with the other list, then the host twin over it
    other = [[(ids[(3 * q + j) % len(ids)], 1.0 / (1 + j)) for j in range(8)] for q in range(len(qc))]
    other[2] = []
    got = ix.batch_search_fused(qids, qc, qv, other, 5, 10, 0.9, depth=30, w_ext=0.5)
    hits = ix.batch_search(qids, qc, qv, 30, 10, 0.9)
    docs, scores = [], []
    for row, lst in zip(hits, other):
        listed = {d for d, _ in lst}
        mine = [d for _, _, d in row if d not in listed]
        docs.append([d for d, _ in lst] + mine)
        scores.append([s for _, s in lst] + [None] * len(mine))
    want = ix.batch_fuse(qc, qv, docs, scores, 5, w_ext=0.5, device=False)
    assert [[r[1:] for r in row] for row in got] == want
    assert [[r[0] for r in row] for row in got] == [[str(q)] * len(row) for q, row in zip(qids, want)]
    assert any(len(row) == 5 for row in got)
    for q, row in enumerate(got):   # a document of the external list alone is fused too; one the search alone found is absent
        listed = {d for d, _ in other[q]}
        assert all((r[6] > 0) == (r[2] in listed) for r in row)
