"""sgpu_rerank_documents / sgpu_rerank_documents_host without a device: the declarations, every argument check in the
header's order, the host twin against rows taken from the oracle's bits alone (tests/rerank_cases.py), the NaN-last rule,
and the Python classes with device=False. The cases are tests/score_cases.py."""
import ctypes as C
import os

import numpy as np
import pytest

import orc
import rerank_cases
import score_cases
import seismic_amd
from rerank_cases import KS_CPU, assert_rows, expected_rows
from seismic_amd import _native
from seismic_amd._abi import BuildConfig
from util import random_dataset, random_queries

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EDEVICE, ELIMIT = 1, 2, 5


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def test_header_declares_both_functions_and_the_abi_version_stays():
    text = open(os.path.join(ROOT, "include", "seismic_hip.h")).read()
    assert "sgpu_status sgpu_rerank_documents(sgpu_index* idx, uint32_t replica," in text
    assert "sgpu_status sgpu_rerank_documents_host(const sgpu_index* idx," in text
    assert "never\n * -0.0" in text or "never -0.0" in text
    L = _native.lib()
    assert hasattr(L, "sgpu_rerank_documents") and hasattr(L, "sgpu_rerank_documents_host")
    assert L.sgpu_abi_version() == 4


def test_the_cases_can_discriminate():
    rerank_cases.assert_discriminates(KS_CPU)


@pytest.fixture(scope="module")
def small():
    dim = 300
    off, comps, vals = random_dataset(3, 50, dim, 3, 20)
    ix = _native.NativeIndex.build(2, dim, off, comps, vals, BuildConfig.defaults(n_postings=10))
    q_off, qc, qv = random_queries(4, 3, dim, 2, 8)
    return ix, dim, q_off, qc, qv


def _calls(ix, q_off, qc, qv, cand_off, cand_ids, k, out_s, out_i, out_n):
    """(name, status, message) of the device call and of the host twin with the same arguments."""
    L = _native.lib()
    nq = len(q_off) - 1 if q_off is not None else 0
    h = ix.h if ix else None
    got = []
    st = L.sgpu_rerank_documents(h, 0, _p(q_off), _p(qc), _p(qv), nq, _p(cand_off), _p(cand_ids), k, _p(out_s), _p(out_i), _p(out_n))
    got.append(("device", st, L.sgpu_last_error().decode()))
    st = L.sgpu_rerank_documents_host(h, _p(q_off), _p(qc), _p(qv), nq, _p(cand_off), _p(cand_ids), k, 0, _p(out_s), _p(out_i),
                                      _p(out_n))
    got.append(("host", st, L.sgpu_last_error().decode()))
    return got


def test_argument_checks_in_order_without_a_device(small):
    ix, dim, q_off, qc, qv = small
    cand_off = np.array([0, 2, 2, 3], np.uint64)
    cand_ids = np.array([1, 49, 7], np.uint64)
    zero = np.zeros(4, np.uint64)
    k = 2
    s, i, n = np.zeros((3, k), np.float32), np.zeros((3, k), np.uint64), np.zeros(3, np.uint32)
    ok = (ix, q_off, qc, qv, cand_off, cand_ids, k, s, i, n)
    # 1. null arguments - the outputs too, also when there is no candidate, and before every other check (k = 0, bad ids)
    for at in (0, 1, 4, 5, 7, 8, 9):
        for base in (ok, ok[:4] + (zero,) + ok[5:], ok[:6] + (0,) + ok[7:], ok[:5] + (np.array([1, 50, 7], np.uint64),) + ok[6:]):
            args = list(base)
            args[at] = None
            for name, st, msg in _calls(*args):
                assert st == EINVAL and "null" in msg, (name, at, msg)
    # 2. what sgpu_score_documents checks, in its order, each before k: the queries, cand_off, the ids
    bad_qc = qc.copy()
    bad_qc[0] = dim
    bad_ids = np.array([1, 50, 7], np.uint64)
    for kk in (k, 0, 1025):
        for name, st, msg in _calls(ix, q_off, bad_qc, qv, np.array([1, 2, 2, 3], np.uint64), bad_ids, kk, s, i, n):
            assert st == EINVAL and "component >= dim" in msg, (name, msg)
        for off in (np.array([1, 2, 2, 3], np.uint64), np.array([0, 2, 1, 3], np.uint64)):
            for name, st, msg in _calls(ix, q_off, qc, qv, off, bad_ids, kk, s, i, n):
                assert st == EINVAL and "cand_off" in msg, (name, msg)
        for name, st, msg in _calls(ix, q_off, qc, qv, cand_off, bad_ids, kk, s, i, n):
            assert st == EINVAL and "query 0" in msg and "document id 50" in msg, (name, msg)
    # 3. k == 0, 4. k > 1024 - both before the device is looked at, also with nothing to do
    for off in (cand_off, zero):
        for name, st, msg in _calls(ix, q_off, qc, qv, off, cand_ids, 0, s, i, n):
            assert st == EINVAL and "k must" in msg, (name, msg)
        for name, st, msg in _calls(ix, q_off, qc, qv, off, cand_ids, 1025, s, i, n):
            assert st == ELIMIT and "1025" in msg, (name, msg)
    assert _native.lib().sgpu_rerank_documents_host(ix.h, _p(q_off), _p(qc), _p(qv), 0, _p(zero), _p(cand_ids), 0, 0, _p(s), _p(i),
                                                    _p(n)) == EINVAL
    # 5. the device call on an index that is not uploaded: SGPU_EDEVICE after all of the above, the host twin runs -
    # k = 1024 is inside the limit
    for kk in (k, 1024):
        s2, i2 = np.zeros((3, kk), np.float32), np.zeros((3, kk), np.uint64)
        (_, st, msg), (_, hst, _) = _calls(ix, q_off, qc, qv, cand_off, cand_ids, kk, s2, i2, n)
        assert st == EDEVICE and "not uploaded" in msg and hst == 0
    (_, st, _), (_, hst, _) = _calls(ix, q_off, qc, qv, zero, cand_ids, k, s, i, n)
    assert st == EDEVICE and hst == 0
    # 6. nq == 0 is SGPU_OK and writes nothing
    s[:], i[:], n[:] = 7.0, 7, 7
    assert _native.lib().sgpu_rerank_documents_host(ix.h, _p(q_off), _p(qc), _p(qv), 0, _p(zero), _p(cand_ids), k, 0, _p(s), _p(i),
                                                    _p(n)) == 0
    assert (s == 7.0).all() and (i == 7).all() and (n == 7).all()


def test_capacity_limit_of_the_queries_comes_before_k():
    dim = 9000
    off, comps, vals = random_dataset(5, 20, dim, 3, 20)
    ix = _native.NativeIndex.build(2, dim, off, comps, vals, BuildConfig.defaults(n_postings=10))
    q_off = np.array([0, 8193], np.uint64)
    qc, qv = np.arange(8193, dtype=np.uint32), np.ones(8193, np.float32)
    s, i, n = np.zeros((1, 1), np.float32), np.zeros((1, 1), np.uint64), np.zeros(1, np.uint32)
    for name, st, msg in _calls(ix, q_off, qc, qv, np.array([0, 1], np.uint64), np.array([3], np.uint64), 0, s, i, n):
        assert st == ELIMIT and "8193 components" in msg, (name, msg)


def test_rows_past_out_n_are_written_as_zero(small):
    ix, dim, q_off, qc, qv = small
    cand_off = np.array([0, 2, 2, 6], np.uint64)
    cand_ids = np.array([1, 49, 7, 7, 7, 8], np.uint64)
    k = 4
    s, i, n = np.full((3, k), 7.0, np.float32), np.full((3, k), 7, np.uint64), np.full(3, 7, np.uint32)
    assert _native.lib().sgpu_rerank_documents_host(ix.h, _p(q_off), _p(qc), _p(qv), 3, _p(cand_off), _p(cand_ids), k, 0, _p(s),
                                                    _p(i), _p(n)) == 0
    assert n.tolist() == [2, 0, 2]
    for q in range(3):
        assert not s[q, n[q]:].view(np.uint32).any() and not i[q, n[q]:].any()
        assert sorted(i[q, :n[q]].tolist()) == sorted(set(cand_ids[int(cand_off[q]):int(cand_off[q + 1])].tolist()))
        want = [orc.score_doc(ix.desc, int(d), qc[int(q_off[q]):int(q_off[q + 1])], qv[int(q_off[q]):int(q_off[q + 1])])
                for d in i[q, :n[q]]]
        assert np.array_equal(np.array(want, np.float32).view(np.uint32), s[q, :n[q]].view(np.uint32))


@pytest.mark.parametrize("k", KS_CPU)
@pytest.mark.parametrize("name", sorted(score_cases.CASES))
def test_host_twin_equals_the_rows_of_the_oracle(name, k):
    rerank_cases.assert_discriminates(KS_CPU)   # (the oracle alone, before the library is looked at; cached)
    case = score_cases.make(name)
    ix = case.index
    want = expected_rows(case, case.cand_off, case.cand_ids, k)
    assert want[2].tolist()[3:8] == [0, 1, 1, min(2, k), 1]   # the empty list; one id; one id three times; two ids; the empty document
    assert_rows(ix.rerank_documents_host(case.q_off, case.qc, case.qv, case.cand_off, case.cand_ids, k), want, name)
    # one thread and many give identical rows
    assert_rows(ix.rerank_documents_host(case.q_off, case.qc, case.qv, case.cand_off, case.cand_ids, k, num_threads=1), want, name)


def test_the_tie_rule_decides_rows_of_every_value_type():
    """The rows whose cut falls between equal scores, named by the oracle, one per value type at least: the host twin
    keeps the lower ids."""
    seen = set()
    for name, (_, _, vt) in sorted(score_cases.CASES.items()):
        ties = rerank_cases.discrimination(name)["ties"]
        if vt in seen or not ties:
            continue
        seen.add(vt)
        case = score_cases.make(name)
        q, k = ties[0]
        off = np.array([0, len(case.lists[q])], np.uint64)
        got = case.index.rerank_documents_host(case.q_off[q:q + 2] - case.q_off[q], case.qc[int(case.q_off[q]):int(case.q_off[q + 1])],
                                               case.qv[int(case.q_off[q]):int(case.q_off[q + 1])], off, case.lists[q], k)
        assert_rows(got, expected_rows(case, off, case.lists[q], k, queries=[q]), "%s q%d k%d" % (name, q, k))
    assert seen == {0, 1, 2}


def test_nan_scores_come_last_by_id_on_the_host():
    """An inf weight on a component that some documents carry with code 0 (inf * 0 = NaN), others with a positive code
    (+inf) and most not at all (+0.0): numbers first - score descending, id ascending -, then the NaNs by id ascending, as
    np.argsort(-s, kind="stable") over the ascending distinct ids orders them."""
    case = score_cases.make("u16_u8")
    ix = case.index
    every = np.arange(case.n_docs, dtype=np.uint64)
    off = np.array([0, case.n_docs], np.uint64)
    df = np.bincount(case.comps.astype(np.int64), minlength=case.dim)
    for c in np.argsort(-df, kind="stable")[:50]:
        qc, qv, q_off = np.array([c], np.uint32), np.array([np.inf], np.float32), np.array([0, 1], np.uint64)
        s = ix.score_documents_host(q_off, qc, qv, off, every)
        if np.isnan(s).sum() >= 3 and np.isposinf(s).sum() >= 3:
            break
    else:
        raise AssertionError("no component with both zero and positive codes")
    want_s = np.array([orc.score_doc(ix.desc, d, qc, qv) for d in range(case.n_docs)], np.float32)
    assert np.array_equal(np.isnan(want_s), np.isnan(s)) and np.array_equal(want_s[~np.isnan(s)], s[~np.isnan(s)])
    nan_ids, inf_ids = np.flatnonzero(np.isnan(want_s))[:300], np.flatnonzero(np.isposinf(want_s))[:300]
    zero_ids = np.flatnonzero(want_s == 0)[:20]
    assert len(zero_ids) == 20
    rng = np.random.default_rng(5)
    cand = rng.permutation(np.concatenate([nan_ids, inf_ids, zero_ids, nan_ids[:2], zero_ids[:2]])).astype(np.uint64)
    want_ids = np.concatenate([inf_ids, zero_ids, nan_ids])   # numbers by score descending and id ascending, then the NaNs
    n_num = len(inf_ids) + len(zero_ids)
    off = np.array([0, len(cand)], np.uint64)
    for k in (n_num - 1, n_num, n_num + 2, 1024):
        gs, gi, gn = ix.rerank_documents_host(q_off, qc, qv, off, cand, k)
        m = min(k, len(want_ids))
        assert gn[0] == m and np.array_equal(gi[0, :m].astype(np.int64), want_ids[:m]), k
        assert np.array_equal(gs[0, :m].view(np.uint32)[:min(m, n_num)], want_s[want_ids[:min(m, n_num)]].view(np.uint32))
        assert np.isnan(gs[0, n_num:m]).all() and not gs[0, m:].view(np.uint32).any() and not gi[0, m:].any()


def test_python_rerank_and_batch_rerank_on_the_host():
    case = score_cases.make("u16_f16")
    ix = seismic_amd.SeismicIndexRaw(case.index, upload=False)
    qcs = [c for c, _ in case.queries]
    qvs = [v for _, v in case.queries]
    for k in (1, 10, 1000):
        wb, wi, wn = expected_rows(case, case.cand_off, case.cand_ids, k)
        want = [[(float(wb[q, j:j + 1].view(np.float32)[0]), int(wi[q, j])) for j in range(wn[q])] for q in range(len(wn))]
        got = ix.batch_rerank(qcs, qvs, case.lists, k, device=False)
        assert got == want
        assert all(isinstance(d, int) and isinstance(s, float) for row in got for s, d in row)
        for q in (2, 3, 5, 11):
            assert ix.rerank(qcs[q], qvs[q], case.lists[q], k, device=False) == want[q]
    with pytest.raises(KeyError):
        ix.rerank(qcs[1], qvs[1], [0, case.n_docs], 3, device=False)
    with pytest.raises(ValueError):
        ix.batch_rerank(qcs, qvs, case.lists[:-1], 3, device=False)
    # a k the native call does not take keeps working through the scores (as before the native call existed)
    assert ix.rerank(qcs[2], qvs[2], case.lists[2], 0, device=False) == []
    wb, wi, wn = expected_rows(case, np.array([0, case.n_docs], np.uint64), case.lists[2], 1500, queries=[2])
    got = ix.rerank(qcs[2], qvs[2], case.lists[2], 1500, device=False)
    assert [d for _, d in got] == wi[0].tolist() and np.array_equal(np.array([s for s, _ in got], np.float32).view(np.uint32), wb[0])
