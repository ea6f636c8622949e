"""sgpu_diversify_documents / sgpu_diversify_documents_host without a device: the host twin against the numpy
restatement of tests/diversify_cases.py (bit for bit, one thread and four), each wrong reading of the contract differing
from it on the call named for it, the returned scores and penalties rebuilt from sgpu_score_documents_host alone, the
rerank equality and the permutation property, the argument checks in the header's order, and the Python classes with
device=False."""
import ctypes as C
import os

import numpy as np
import pytest

import diversify_cases
import seismic_amd
from diversify_cases import same
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
    assert "sgpu_status sgpu_diversify_documents(sgpu_index* idx, uint32_t replica," in text
    assert "sgpu_status sgpu_diversify_documents_host(const sgpu_index* idx," in text
    assert text.index("---- expand:") < text.index("---- diversify:")
    assert "sgpu_debug_diversify_stats" in open(os.path.join(ROOT, "include", "seismic_hip_testing.h")).read()
    L = _native.lib()
    assert hasattr(L, "sgpu_diversify_documents") and hasattr(L, "sgpu_diversify_documents_host")
    assert hasattr(L, "sgpu_debug_diversify_stats")
    assert L.sgpu_abi_version() == 4


@pytest.mark.parametrize("name", sorted(diversify_cases.CASES))
def test_host_twin_equals_the_restatement(name):
    case = diversify_cases.make(name)
    ix = case.index
    for call in case.calls.values():
        for k in call.ks:
            for threads in (1, 4):   # (the thread count does not change a bit)
                got = ix.diversify_documents_host(*call.args(), k, num_threads=threads)
                diff = same(got, case.expected(call.name, k))
                assert diff is None, (name, call.name, k, threads, diff)
    # the named edges, read off the host twin's rows
    sc, pen, ids, n = ix.diversify_documents_host(*case.calls["empty"].args(), 8)
    assert n.tolist() == [0, len(set(case.calls["empty"].lists[1].tolist())), 0]
    for q in range(3):
        assert not sc[q, n[q]:].view(np.uint32).any() and not pen[q, n[q]:].view(np.uint32).any() and not ids[q, n[q]:].any()
    assert not sc[1].view(np.uint32).any()   # an empty query: every rel is +0.0
    for call in case.calls.values():   # a penalty is never below +0.0, and +0.0 in round 0
        sc, pen, ids, n = ix.diversify_documents_host(*call.args(), call.ks[0])
        assert not np.signbit(pen).any() and not pen[:, 0].view(np.uint32).any()


# the calls on which a wrong reading must differ from the host twin
WRONG = [("padding", "lengths", 9), ("symmetric", "order", 3), ("float64", "order", 3), ("pen_sum", "max_not_sum", 4),
         ("signed_pen", "negative", 3), ("no_refresh", "stale", 4), ("dup_twice", "dups", 8), ("dup_twice", "dups", 9),
         ("ties_high", "ties", 1), ("ties_high", "ties", 3), ("ties_high", "ties", 7), ("fused", "rounding", 3),
         ("fused", "rounding", 2)]


@pytest.mark.parametrize("name", ["u16_f16_32767", "u16_dvb_32767", "u32_u8_32768", "u16_f16_300"])
def test_each_wrong_reading_fails_on_its_named_call(name):
    case = diversify_cases.make(name)
    assert {r for r, _, _ in WRONG} == set(diversify_cases.READINGS)
    for reading, call_name, k in WRONG:
        if call_name not in case.calls:   # (signed and very large stored values: the binary16 forms)
            assert call_name in diversify_cases.F16_ONLY and case.value_type != 0
            continue
        call = case.calls[call_name]
        got = case.index.diversify_documents_host(*call.args(), k)
        wrong = diversify_cases.diversify_numpy(case, call, k, reading=reading)
        assert same(got, wrong) is not None, (name, reading, call_name, k)
        assert same(got, case.expected(call_name, k)) is None
    # dup_twice also counts entries where the contract counts documents
    call = case.calls["dups"]
    assert diversify_cases.diversify_numpy(case, call, 9, reading="dup_twice")[3][0] == len(call.lists[0]) == 8
    assert case.index.diversify_documents_host(*call.args(), 9)[3][0] == 6


def _stored_query(case, doc):
    """Document `doc` as a query for sgpu_score_documents_host: its stored components and values as f32."""
    off, comps, x, scale = case.stored()
    c, v = comps[off[doc]:off[doc + 1]], x[off[doc]:off[doc + 1]]
    return c.astype(np.uint32), (v if scale is None else v * scale).astype(np.float32)


@pytest.mark.parametrize("name", sorted(diversify_cases.CASES))
def test_scores_and_penalties_are_what_the_score_call_returns(name):
    """out_scores and out_penalties rebuilt through sgpu_score_documents_host, code that existed before the twin:
    out_penalties[q, r] = max(0, max over the earlier picks s of score(query = s's stored vector, document d))."""
    import orc
    case = diversify_cases.make(name)
    ix = case.index
    for call_name in ("lengths", "random", "dups", "order", "negative", "big", "empty_first"):
        if call_name not in case.calls:
            continue
        call = case.calls[call_name]
        k = call.ks[0]
        sc, pen, ids, n = ix.diversify_documents_host(*call.args(), k)
        off = np.zeros(call.nq + 1, np.uint64)
        off[1:] = np.cumsum(n)
        picked = np.concatenate([ids[q, :n[q]] for q in range(call.nq)])
        rel = ix.score_documents_host(call.q_off, call.qc, call.qv, off, picked)
        want = np.concatenate([sc[q, :n[q]] for q in range(call.nq)])
        assert np.array_equal(rel.view(np.uint32), want.view(np.uint32)), (name, call_name)
        for q in range(call.nq):
            row = ids[q, :n[q]].tolist()
            if len(row) < 2:
                continue
            # one "query" per pick s, its candidates the picks after it
            s_off, s_c, s_v = orc.csr([_stored_query(case, int(s)) for s in row[:-1]])
            later = [row[r + 1:] for r in range(len(row) - 1)]
            c_off = np.zeros(len(later) + 1, np.uint64)
            c_off[1:] = np.cumsum([len(x) for x in later])
            sims = ix.score_documents_host(s_off, s_c, s_v, c_off, np.concatenate(later).astype(np.uint64))
            best = np.zeros(len(row), np.float32)
            for r in range(len(row) - 1):
                seg = sims[int(c_off[r]):int(c_off[r + 1])]
                best[r + 1:] = np.maximum(best[r + 1:], seg)
            assert np.array_equal(best.view(np.uint32), pen[q, :len(row)].view(np.uint32)), (name, call_name, q)


@pytest.mark.parametrize("name", sorted(diversify_cases.CASES))
def test_rerank_equality_and_permutations(name):
    case = diversify_cases.make(name)
    ix = case.index
    for call in case.calls.values():
        q_off, qc, qv, cand_off, cand_ids, lam, mu = call.args()
        for k in call.ks:
            # lambda = 1, mu = 0: the rows of sgpu_rerank_documents_host
            sc, pen, ids, n = ix.diversify_documents_host(q_off, qc, qv, cand_off, cand_ids, 1.0, 0.0, k)
            want = ix.rerank_documents_host(q_off, qc, qv, cand_off, cand_ids, k)
            assert same((sc, ids, n), want, ("out_scores", "out_doc_ids", "out_n")) is None, (name, call.name, k)
            # ... and of the restatement
            one = diversify_cases.Call(call.name, call.queries, call.lists, 1.0, 0.0, call.ks)
            assert same(diversify_cases.diversify_numpy(case, one, k)[2:], (ids, n), ("out_doc_ids", "out_n")) is None
            # a permutation of the candidate list changes no row: the twin and the restatement
            lists = diversify_cases.permuted(call)
            got = ix.diversify_documents_host(*call.args(lists), k)
            assert same(got, case.expected(call.name, k)) is None, (name, call.name, k)
        k = call.ks[0]
        assert same(diversify_cases.diversify_numpy(case, call, k, lists=diversify_cases.permuted(call, 7)),
                    case.expected(call.name, k)) is None, (name, call.name)


@pytest.fixture(scope="module")
def small():
    dim = 300
    off, comps, vals = random_dataset(3, 50, dim, 3, 20)
    ix = _native.NativeIndex.build(2, dim, off, comps, vals, BuildConfig.defaults(n_postings=10))
    q_off, qc, qv = random_queries(4, 3, dim, 2, 8)
    return ix, dim, q_off, qc, qv


def _calls(ix, q_off, qc, qv, cand_off, cand_ids, lam, mu, k, outs):
    """(name, status, message) of the device call and of the host twin with the same arguments."""
    L = _native.lib()
    nq = len(q_off) - 1 if q_off is not None else 0
    o = [_p(a) for a in outs]
    got = []
    st = L.sgpu_diversify_documents(ix.h if ix else None, 0, _p(q_off), _p(qc), _p(qv), nq, _p(cand_off), _p(cand_ids), lam, mu, k, *o)
    got.append(("device", st, L.sgpu_last_error().decode()))
    st = L.sgpu_diversify_documents_host(ix.h if ix else None, _p(q_off), _p(qc), _p(qv), nq, _p(cand_off), _p(cand_ids), lam, mu,
                                         k, 0, *o)
    got.append(("host", st, L.sgpu_last_error().decode()))
    return got


def _outs(nq, k):
    return [np.zeros((nq, k), np.float32), np.zeros((nq, k), np.float32), np.zeros((nq, k), np.uint64), np.zeros(nq, np.uint32)]


def test_argument_checks_in_order_without_a_device(small):
    ix, dim, q_off, qc, qv = small
    cand_off = np.array([0, 2, 2, 3], np.uint64)
    cand_ids = np.array([1, 49, 7], np.uint64)
    outs = _outs(3, 4)
    zero = np.zeros(4, np.uint64)
    nan, inf = float("nan"), float("inf")
    # 1. null arguments: cand_ids and every output count, also with nothing to do and when later checks would fire
    for args in ((None, q_off, qc, qv, cand_off, cand_ids), (ix, None, qc, qv, cand_off, cand_ids),
                 (ix, q_off, qc, qv, None, cand_ids), (ix, q_off, qc, qv, cand_off, None)):
        for name, st, _ in _calls(*args, 0.5, 0.5, 4, outs):
            assert st == EINVAL, name
    for missing in range(4):
        o = list(outs)
        o[missing] = None
        for off in (cand_off, zero):
            for k, lam in ((4, 0.5), (257, nan)):
                for name, st, msg in _calls(ix, q_off, qc, qv, off, cand_ids, lam, 0.5, k, o):
                    assert st == EINVAL and "null" in msg, (name, missing, msg)
    # 2. what the score call checks, before lambda, mu and k: the queries, cand_off, the ids
    bad_qc = qc.copy()
    bad_qc[0] = dim
    bad_ids = np.array([1, 50, 7], np.uint64)
    for name, st, msg in _calls(ix, q_off, bad_qc, qv, np.array([1, 2, 2, 3], np.uint64), bad_ids, nan, nan, 0, outs):
        assert st == EINVAL and "component >= dim" in msg, (name, msg)
    for name, st, msg in _calls(ix, q_off, qc, qv, np.array([0, 2, 1, 3], np.uint64), bad_ids, nan, nan, 0, outs):
        assert st == EINVAL and "cand_off" in msg, (name, msg)
    for name, st, msg in _calls(ix, q_off, qc, qv, cand_off, bad_ids, nan, nan, 0, outs):
        assert st == EINVAL and "query 0" in msg and "document id 50" in msg, (name, msg)
    # 3. lambda or mu that is not finite, before the candidate count and k
    many_off = np.array([0, 0, 2049, 2049], np.uint64)
    many_ids = np.zeros(2049, np.uint64)
    for bad in (nan, inf, -inf):
        for name, st, msg in _calls(ix, q_off, qc, qv, many_off, many_ids, bad, 0.5, 0, outs):
            assert st == EINVAL and "lambda" in msg, (name, msg)
        for name, st, msg in _calls(ix, q_off, qc, qv, many_off, many_ids, 0.5, bad, 0, outs):
            assert st == EINVAL and "mu" in msg, (name, msg)
    # 4. more than 2048 listed candidates of one query, before k: the message names the query
    for name, st, msg in _calls(ix, q_off, qc, qv, many_off, many_ids, 0.5, 0.5, 0, outs):
        assert st == ELIMIT and "query 1" in msg and "2049" in msg, (name, msg)
    # 6. k == 0, 7. k > 256 - before the device checks (the index is not uploaded)
    for name, st, msg in _calls(ix, q_off, qc, qv, cand_off, cand_ids, 0.5, 0.5, 0, outs):
        assert st == EINVAL and "k must be" in msg, (name, msg)
    for name, st, msg in _calls(ix, q_off, qc, qv, cand_off, cand_ids, 0.5, 0.5, 257, outs):
        assert st == ELIMIT and "257" in msg, (name, msg)
    # 8. the device call on an index that is not uploaded: SGPU_EDEVICE; the host twin runs - also with nothing to do
    (_, st, msg), (_, hst, _) = _calls(ix, q_off, qc, qv, cand_off, cand_ids, 0.5, 0.5, 4, outs)
    assert st == EDEVICE and "not uploaded" in msg and hst == 0 and outs[3].tolist() == [2, 0, 1]
    (_, st, _), (_, hst, _) = _calls(ix, q_off, qc, qv, zero, cand_ids, 0.5, 0.5, 4, outs)
    assert st == EDEVICE and hst == 0 and not outs[3].any() and not outs[2].any()
    o = [_p(a) for a in outs]
    assert _native.lib().sgpu_diversify_documents_host(ix.h, _p(q_off), _p(qc), _p(qv), 0, _p(zero), _p(cand_ids), 0.5, 0.5, 4, 0,
                                                       *o) == 0
    # 2048 candidates of one query and k = 256 are taken
    full = _outs(3, 256)
    (_, st, _), (_, hst, msg) = _calls(ix, q_off, qc, qv, np.array([0, 0, 2048, 2048], np.uint64), many_ids[:2048], 0.5, 0.5, 256,
                                       full)
    assert st == EDEVICE and hst == 0 and full[3].tolist() == [0, 1, 0], msg


def test_the_document_length_limit():
    """5. a candidate document of more than 8192 stored components: after the candidate count, before k."""
    case = diversify_cases.make("u16_f16_32768")
    ix = case.index
    big, over = case.named["big_8192"], case.named["big_8193"]
    q_off, qc, qv = case.calls["big"].q_off, case.calls["big"].qc, case.calls["big"].qv
    outs = _outs(1, 4)
    ids = np.array([3, big, over, over], np.uint64)
    for name, st, msg in _calls(ix, q_off, qc, qv, np.array([0, 4], np.uint64), ids, 0.5, 0.5, 0, outs):
        assert st == ELIMIT and "8193" in msg and "document id %d" % over in msg and "query 0" in msg, (name, msg)
    many = np.full(2049, over, np.uint64)
    for name, st, msg in _calls(ix, q_off, qc, qv, np.array([0, 2049], np.uint64), many, 0.5, 0.5, 0, outs):
        assert st == ELIMIT and "2049" in msg, (name, msg)   # (the candidate count comes first)
    (_, st, _), (_, hst, msg) = _calls(ix, q_off, qc, qv, np.array([0, 2], np.uint64), ids[:2], 0.5, 0.5, 4, outs)
    assert st == EDEVICE and hst == 0 and outs[3][0] == 2, msg   # 8192 components are taken


def test_query_length_limit_comes_before_lambda_and_k():
    dim = 9000
    off, comps, vals = random_dataset(5, 20, dim, 3, 20)
    ix = _native.NativeIndex.build(2, dim, off, comps, vals, BuildConfig.defaults(n_postings=10))
    q_off = np.array([0, 8193], np.uint64)
    qc = np.arange(8193, dtype=np.uint32)
    qv = np.ones(8193, np.float32)
    for name, st, msg in _calls(ix, q_off, qc, qv, np.array([0, 1], np.uint64), np.array([3], np.uint64), float("nan"), 0.5, 0,
                                _outs(1, 1)):
        assert st == ELIMIT and "8193" in msg, (name, msg)


@pytest.mark.parametrize("cls", ["SeismicIndex", "SeismicIndexLV", "SeismicIndexDotVByte"])
def test_python_diversify_on_the_host(cls):
    ids, vecs, _ = read_jsonl(os.path.join(GOLD_TOY, "documents.jsonl"))
    _, qvecs, _ = read_jsonl(os.path.join(GOLD_TOY, "queries.jsonl"))
    qc = [np.array(list(v.keys())) for v in qvecs]
    qv = [np.array(list(v.values()), np.float32) for v in qvecs]
    ix = getattr(seismic_amd, cls).build(os.path.join(GOLD_TOY, "documents.jsonl"), n_postings=50, centroid_fraction=0.2,
                                          upload=False)
    lists = [list(ids[q % len(ids):q % len(ids) + 12]) + [ids[q % len(ids)]] for q in range(len(qc))]
    lists[1] = []
    rows = ix.batch_diversify(qc, qv, lists, 5, device=False)
    assert len(rows) == len(qc) and rows[1] == []
    for q, row in enumerate(rows):
        assert len(row) == min(5, len(set(lists[q]))) and len({d for _, _, d in row}) == len(row)
        assert all(d in lists[q] and p >= 0 for _, p, d in row) and (not row or row[0][1] == 0)
    # lam = 1, mu = 0 is batch_rerank
    plain = ix.batch_diversify(qc, qv, lists, 5, lam=1.0, mu=0.0, device=False)
    assert [[(s, d) for s, _, d in row] for row in plain] == ix.batch_rerank(qc, qv, lists, 5, device=False)
    assert ix.diversify(qc[0], qv[0], lists[0], 5, device=False) == rows[0]
    # a heavy mu changes some row: the selection is not the rerank
    heavy = ix.batch_diversify(qc, qv, lists, 5, lam=0.1, mu=1.0, device=False)
    assert any([d for _, _, d in a] != [d for _, _, d in b] for a, b in zip(heavy, plain))
    with pytest.raises(KeyError):
        ix.diversify(qc[0], qv[0], ["no-such-document"], 3, device=False)
    with pytest.raises(_native.SeismicHipError):
        ix.diversify(qc[0], qv[0], lists[0], 257, device=False)
