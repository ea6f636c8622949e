"""sgpu_collapse_documents / sgpu_collapse_documents_host without a device: the host twin against the numpy restatement of
tests/collapse_cases.py (bit for bit, one thread and four), each wrong reading of the contract differing from it on the
call named for it, the rerank equality and the permutation property, the argument checks in the header's order, and the
Python classes with device=False."""
import ctypes as C
import os

import numpy as np
import pytest

import collapse_cases
import seismic_amd
from collapse_cases import same
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
    assert "sgpu_status sgpu_collapse_documents(sgpu_index* idx, uint32_t replica," in text
    assert "sgpu_status sgpu_collapse_documents_host(const sgpu_index* idx," in text
    assert text.index("---- diversify:") < text.index("---- collapse:")
    assert "sgpu_debug_collapse_stats" in open(os.path.join(ROOT, "include", "seismic_hip_testing.h")).read()
    L = _native.lib()
    assert hasattr(L, "sgpu_collapse_documents") and hasattr(L, "sgpu_collapse_documents_host")
    assert hasattr(L, "sgpu_debug_collapse_stats")
    assert L.sgpu_abi_version() == 4


@pytest.mark.parametrize("name", sorted(collapse_cases.CASES))
def test_host_twin_equals_the_restatement(name):
    case = collapse_cases.make(name)
    ix = case.index
    for call in case.calls.values():
        for m in call.ms:
            for k in call.ks:
                for threads in (1, 4):   # (the thread count does not change a bit)
                    got = ix.collapse_documents_host(*call.args(), m, k, num_threads=threads)
                    diff = same(got, case.expected(call.name, m, k))
                    assert diff is None, (name, call.name, m, k, threads, diff)
    # the named edges, read off the host twin's rows
    out = ix.collapse_documents_host(*case.calls["empty"].args(), 1, 8)
    assert out[5].tolist() == [0, 2, 0]
    for q in range(3):
        for a in out[:5]:
            assert not a[q, out[5][q]:].view(np.uint32 if a.dtype.itemsize == 4 else np.uint64).any()
    assert not out[1][1].view(np.uint32).any() and not out[3][1].view(np.uint32).any()   # an empty query: every score is +0.0
    for call in case.calls.values():   # no score is -0.0
        out = ix.collapse_documents_host(*call.args(), call.ms[0], call.ks[0])
        assert not (out[1].view(np.uint32) == 0x80000000).any() and not (out[3].view(np.uint32) == 0x80000000).any()


# the calls (with m and k) on which a wrong reading must differ from the host twin
WRONG = [("ascending", "sum_order", 3, 1), ("float64", "sum_order", 3, 1), ("sum_all", "top_m", 1, 7), ("sum_all", "top_m", 2, 7),
         ("sum_all", "top_m", 3, 7), ("sum_all", "top_m", 64, 7), ("dup_twice", "dups", 2, 2), ("dup_twice", "dups", 1, 1),
         ("group_of_id", "two_keys", 1, 3), ("group_of_id", "two_keys", 2, 3), ("ties_high", "ties", 1, 1),
         ("ties_high", "ties", 2, 2), ("best_high", "ties", 1, 4), ("best_high", "ties", 1, 5)]


@pytest.mark.parametrize("name", ["u16_f16_32767", "u16_dvb_32767", "u32_u8_32768", "u16_f16_300"])
def test_each_wrong_reading_fails_on_its_named_call(name):
    case = collapse_cases.make(name)
    assert {r for r, _, _, _ in WRONG} == set(collapse_cases.READINGS)
    for reading, call_name, m, k in WRONG:
        call = case.calls[call_name]
        got = case.index.collapse_documents_host(*call.args(), m, k)
        wrong = collapse_cases.collapse_numpy(case, call, m, k, reading=reading)
        assert same(got, wrong) is not None, (name, reading, call_name, m, k)
        assert same(got, case.expected(call_name, m, k)) is None
    # sum_order: 2^24 against 2^24 + 2; dup_twice also counts listings where the contract counts documents
    call = case.calls["sum_order"]
    assert case.index.collapse_documents_host(*call.args(), 3, 1)[1][0, 0] == np.float32(16777216.0)
    for reading in ("ascending", "float64"):
        assert collapse_cases.collapse_numpy(case, call, 3, 1, reading=reading)[1][0, 0] == np.float32(16777218.0)
    call = case.calls["dups"]
    assert sorted(collapse_cases.collapse_numpy(case, call, 2, 2, reading="dup_twice")[4][0].tolist()) == [1, 4]
    assert sorted(case.index.collapse_documents_host(*call.args(), 2, 2)[4][0].tolist()) == [1, 2]


@pytest.mark.parametrize("name", sorted(collapse_cases.CASES))
def test_member_scores_are_what_the_score_call_returns(name):
    """m = 1: a group's score is its best member's, and that is the largest sgpu_score_documents_host score among the
    group's entries - code that existed before the twin."""
    case = collapse_cases.make(name)
    ix = case.index
    for call_name in ("random", "keys", "negative", "top_m"):
        call = case.calls[call_name]
        sc = ix.score_documents_host(call.q_off, call.qc, call.qv, call.cand_off, call.cand_ids)
        g, s, ids, bs, mem, n = ix.collapse_documents_host(*call.args(), 1, 1024)
        assert np.array_equal(s.view(np.uint32), bs.view(np.uint32))
        for q in range(call.nq):
            a, b = int(call.cand_off[q]), int(call.cand_off[q + 1])
            keys = call.cand_groups[a:b]
            assert n[q] == len(set(keys.tolist()))
            for j in range(n[q]):
                at = np.flatnonzero(keys == g[q, j]) + a
                assert s[q, j] == sc[at].max() and mem[q, j] == len(set(call.cand_ids[at].tolist()))
                assert ids[q, j] == call.cand_ids[at][sc[at] == s[q, j]].min()


@pytest.mark.parametrize("name", sorted(collapse_cases.CASES))
def test_rerank_equality_and_permutations(name):
    case = collapse_cases.make(name)
    ix = case.index
    for call in case.calls.values():
        q_off, qc, qv, cand_off, cand_ids, cand_groups = call.args()
        for k in call.ks:
            # m = 1 and key = id: the rows of sgpu_rerank_documents_host
            g, s, ids, bs, mem, n = ix.collapse_documents_host(q_off, qc, qv, cand_off, cand_ids, cand_ids.astype(np.uint32), 1, k)
            want = ix.rerank_documents_host(q_off, qc, qv, cand_off, cand_ids, k)
            assert same((s, ids, n), want, ("out_scores", "out_best_ids", "out_n")) is None, (name, call.name, k)
            filled = np.arange(k)[None, :] < n[:, None]
            assert np.array_equal(g, ids.astype(np.uint32)) and (mem[filled] == 1).all() and not mem[~filled].any()
            # a permutation of the entries changes no row: the twin ...
            for m in call.ms:
                got = ix.collapse_documents_host(*call.args(collapse_cases.permuted(call)), m, k)
                assert same(got, case.expected(call.name, m, k)) is None, (name, call.name, m, k)
        # ... and the restatement
        m, k = call.ms[-1], call.ks[0]
        assert same(collapse_cases.collapse_numpy(case, call, m, k, order=collapse_cases.permuted(call, 7)),
                    case.expected(call.name, m, k)) is None, (name, call.name)


@pytest.fixture(scope="module")
def small():
    dim = 300
    off, comps, vals = random_dataset(3, 50, dim, 3, 20)
    ix = _native.NativeIndex.build(2, dim, off, comps, vals, BuildConfig.defaults(n_postings=10))
    q_off, qc, qv = random_queries(4, 3, dim, 2, 8)
    return ix, dim, q_off, qc, qv


def _calls(ix, q_off, qc, qv, cand_off, cand_ids, cand_groups, m, k, outs):
    """(name, status, message) of the device call and of the host twin with the same arguments."""
    L = _native.lib()
    nq = len(q_off) - 1 if q_off is not None else 0
    o = [_p(a) for a in outs]
    got = []
    st = L.sgpu_collapse_documents(ix.h if ix else None, 0, _p(q_off), _p(qc), _p(qv), nq, _p(cand_off), _p(cand_ids), _p(cand_groups),
                                   m, k, *o)
    got.append(("device", st, L.sgpu_last_error().decode()))
    st = L.sgpu_collapse_documents_host(ix.h if ix else None, _p(q_off), _p(qc), _p(qv), nq, _p(cand_off), _p(cand_ids),
                                        _p(cand_groups), m, k, 0, *o)
    got.append(("host", st, L.sgpu_last_error().decode()))
    return got


def _outs(nq, k):
    return [np.zeros((nq, k), np.uint32), np.zeros((nq, k), np.float32), np.zeros((nq, k), np.uint64), np.zeros((nq, k), np.float32),
            np.zeros((nq, k), np.uint32), np.zeros(nq, np.uint32)]


def test_argument_checks_in_order_without_a_device(small):
    ix, dim, q_off, qc, qv = small
    cand_off = np.array([0, 2, 2, 3], np.uint64)
    cand_ids = np.array([1, 49, 7], np.uint64)
    grp = np.array([4, 4, 0xffffffff], np.uint32)
    outs = _outs(3, 4)
    zero = np.zeros(4, np.uint64)
    # 1. null arguments: cand_ids, cand_groups and every output count, also with nothing to do and when later checks would fire
    for args in ((None, q_off, qc, qv, cand_off, cand_ids, grp), (ix, None, qc, qv, cand_off, cand_ids, grp),
                 (ix, q_off, qc, qv, None, cand_ids, grp), (ix, q_off, qc, qv, cand_off, None, grp),
                 (ix, q_off, qc, qv, cand_off, cand_ids, None)):
        for name, st, _ in _calls(*args, 1, 4, outs):
            assert st == EINVAL, name
    for missing in range(6):
        o = list(outs)
        o[missing] = None
        for off in (cand_off, zero):
            for m, k in ((1, 4), (65, 1025)):
                for name, st, msg in _calls(ix, q_off, qc, qv, off, cand_ids, grp, m, k, o):
                    assert st == EINVAL and "null" in msg, (name, missing, msg)
    # 2. what the score call checks, before the candidate count, m and k: the queries, cand_off, the ids
    bad_qc = qc.copy()
    bad_qc[0] = dim
    bad_ids = np.array([1, 50, 7], np.uint64)
    for name, st, msg in _calls(ix, q_off, bad_qc, qv, np.array([1, 2, 2, 3], np.uint64), bad_ids, grp, 0, 0, outs):
        assert st == EINVAL and "component >= dim" in msg, (name, msg)
    for name, st, msg in _calls(ix, q_off, qc, qv, np.array([0, 2, 1, 3], np.uint64), bad_ids, grp, 0, 0, outs):
        assert st == EINVAL and "cand_off" in msg, (name, msg)
    for name, st, msg in _calls(ix, q_off, qc, qv, cand_off, bad_ids, grp, 0, 0, outs):
        assert st == EINVAL and "query 0" in msg and "document id 50" in msg, (name, msg)
    # 3. more than 4096 listed candidates of one query, before m and k: the message names the query
    many_off = np.array([0, 0, 4097, 4097], np.uint64)
    many_ids = np.zeros(4097, np.uint64)
    many_grp = np.zeros(4097, np.uint32)
    for name, st, msg in _calls(ix, q_off, qc, qv, many_off, many_ids, many_grp, 0, 0, outs):
        assert st == ELIMIT and "query 1" in msg and "4097" in msg, (name, msg)
    # 4. m == 0, 5. m > 64, before k
    for name, st, msg in _calls(ix, q_off, qc, qv, cand_off, cand_ids, grp, 0, 0, outs):
        assert st == EINVAL and "m must be" in msg, (name, msg)
    for name, st, msg in _calls(ix, q_off, qc, qv, cand_off, cand_ids, grp, 65, 0, outs):
        assert st == ELIMIT and "m = 65" in msg, (name, msg)
    # 6. k == 0, 7. k > 1024 - before the device checks (the index is not uploaded)
    for name, st, msg in _calls(ix, q_off, qc, qv, cand_off, cand_ids, grp, 64, 0, outs):
        assert st == EINVAL and "k must be" in msg, (name, msg)
    for name, st, msg in _calls(ix, q_off, qc, qv, cand_off, cand_ids, grp, 64, 1025, outs):
        assert st == ELIMIT and "1025" in msg, (name, msg)
    # 8. the device call on an index that is not uploaded: SGPU_EDEVICE; the host twin runs - also with nothing to do
    (_, st, msg), (_, hst, _) = _calls(ix, q_off, qc, qv, cand_off, cand_ids, grp, 1, 4, outs)
    assert st == EDEVICE and "not uploaded" in msg and hst == 0 and outs[5].tolist() == [1, 0, 1]
    assert outs[0][:, 0].tolist() == [4, 0, 0xffffffff] and outs[4][:, 0].tolist() == [2, 0, 1]
    (_, st, _), (_, hst, _) = _calls(ix, q_off, qc, qv, zero, cand_ids, grp, 1, 4, outs)
    assert st == EDEVICE and hst == 0 and not outs[5].any() and not outs[0].any() and not outs[2].any()
    o = [_p(a) for a in outs]
    assert _native.lib().sgpu_collapse_documents_host(ix.h, _p(q_off), _p(qc), _p(qv), 0, _p(zero), _p(cand_ids), _p(grp), 1, 4, 0,
                                                      *o) == 0
    # 4096 candidates of one query, m = 64 and k = 1024 are taken
    full = _outs(3, 1024)
    (_, st, _), (_, hst, msg) = _calls(ix, q_off, qc, qv, np.array([0, 0, 4096, 4096], np.uint64), many_ids[:4096], many_grp[:4096],
                                       64, 1024, full)
    assert st == EDEVICE and hst == 0 and full[5].tolist() == [0, 1, 0] and full[4][1, 0] == 1, msg


def test_query_length_limit_comes_before_m_and_k():
    dim = 9000
    off, comps, vals = random_dataset(5, 20, dim, 3, 20)
    ix = _native.NativeIndex.build(2, dim, off, comps, vals, BuildConfig.defaults(n_postings=10))
    q_off = np.array([0, 8193], np.uint64)
    qc = np.arange(8193, dtype=np.uint32)
    qv = np.ones(8193, np.float32)
    for name, st, msg in _calls(ix, q_off, qc, qv, np.array([0, 1], np.uint64), np.array([3], np.uint64), np.zeros(1, np.uint32), 0, 0,
                                _outs(1, 1)):
        assert st == ELIMIT and "8193" in msg, (name, msg)


@pytest.mark.parametrize("cls", ["SeismicIndex", "SeismicIndexLV", "SeismicIndexDotVByte"])
def test_python_collapse_on_the_host(cls):
    ids, vecs, _ = read_jsonl(os.path.join(GOLD_TOY, "documents.jsonl"))
    _, qvecs, _ = read_jsonl(os.path.join(GOLD_TOY, "queries.jsonl"))
    qc = [np.array(list(v.keys())) for v in qvecs]
    qv = [np.array(list(v.values()), np.float32) for v in qvecs]
    ix = getattr(seismic_amd, cls).build(os.path.join(GOLD_TOY, "documents.jsonl"), n_postings=50, centroid_fraction=0.2,
                                          upload=False)
    lists = [list(ids[q % len(ids):q % len(ids) + 12]) + [ids[q % len(ids)]] for q in range(len(qc))]
    lists[1] = []
    key_of = {d: i // 3 for i, d in enumerate(ids)}   # three passages per "document"
    groups = [[key_of[d] for d in row] for row in lists]
    rows = ix.batch_collapse(qc, qv, lists, groups, 3, device=False)
    assert len(rows) == len(qc) and rows[1] == []
    scores = ix.batch_score(qc, qv, lists, device=False)
    for q, row in enumerate(rows):
        keys = sorted(set(groups[q]))
        assert len(row) == min(3, len(keys)) and len({g for g, _, _, _, _ in row}) == len(row)
        for g, s, best, bs, members in row:
            mine = [(float(scores[q][i]), d) for i, d in enumerate(lists[q]) if groups[q][i] == g]
            assert s == bs == max(x for x, _ in mine) and key_of[best] == g and members == len({d for _, d in mine})
        assert [s for _, s, _, _, _ in row] == sorted((s for _, s, _, _, _ in row), reverse=True)
    # the mapping set_groups keeps gives the same rows; m = 2 sums two members
    with pytest.raises(ValueError):
        ix.batch_collapse(qc, qv, lists, None, 3, device=False)
    ix.set_groups(key_of)
    assert ix.batch_collapse(qc, qv, lists, None, 3, device=False) == rows
    ix.set_groups([key_of[d] for d in ids])
    assert ix.batch_collapse(qc, qv, lists, None, 3, device=False) == rows
    assert ix.collapse(qc[0], qv[0], lists[0], groups[0], 3, device=False) == rows[0]
    assert ix.collapse(qc[0], qv[0], lists[0], None, 3, device=False) == rows[0]
    two = ix.batch_collapse(qc, qv, lists, None, 3, m=2, device=False)
    assert any(a != b for a, b in zip(two, rows))
    # key = id and m = 1 is batch_rerank
    own = [[ix._score_rows([d])[0] for d in row] for row in lists]
    plain = ix.batch_collapse(qc, qv, lists, own, 5, device=False)
    assert [[(s, d) for _, s, d, _, _ in row] for row in plain] == ix.batch_rerank(qc, qv, lists, 5, device=False)
    # a partial mapping: a candidate without a key; an id the index does not hold; the limits are the library's
    ix.set_groups({ids[0]: 7})
    with pytest.raises(ValueError):
        ix.batch_collapse(qc, qv, lists, None, 3, device=False)
    with pytest.raises(ValueError):
        ix.set_groups({"no-such-document": 1})
    with pytest.raises(ValueError):
        ix.set_groups([1, 2, 3])
    ix.set_groups(None)
    with pytest.raises(ValueError):   # (no mapping: refused before anything is searched)
        ix.batch_search_collapsed(["q"], qc[:1], qv[:1], 3, 4, 0.8)
    with pytest.raises(KeyError):
        ix.collapse(qc[0], qv[0], ["no-such-document"], [1], 3, device=False)
    with pytest.raises(_native.SeismicHipError):
        ix.collapse(qc[0], qv[0], lists[0], groups[0], 1025, device=False)
    with pytest.raises(_native.SeismicHipError):
        ix.collapse(qc[0], qv[0], lists[0], groups[0], 3, m=65, device=False)
