"""sgpu_fuse_documents / sgpu_fuse_documents_host without a device: the host twin against the numpy restatement of
tests/fuse_cases.py (bit for bit, one thread and four), each wrong reading of the contract differing from it on the call
named for it, the rerank and the rank consequences, the permutation property, the argument checks in the header's order,
and the Python classes with device=False."""
import ctypes as C
import os

import numpy as np
import pytest

import fuse_cases
import seismic_amd
from fuse_cases import MINMAX, RRF, SUM, same
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
    assert "sgpu_status sgpu_fuse_documents(sgpu_index* idx, uint32_t replica," in text
    assert "sgpu_status sgpu_fuse_documents_host(const sgpu_index* idx," in text
    assert "enum { SGPU_FUSE_RRF = 0, SGPU_FUSE_MINMAX = 1, SGPU_FUSE_SUM = 2 };" in text
    assert text.index("---- collapse:") < text.index("---- fuse:")
    assert "sgpu_debug_fuse_stats" in open(os.path.join(ROOT, "include", "seismic_hip_testing.h")).read()
    L = _native.lib()
    assert hasattr(L, "sgpu_fuse_documents") and hasattr(L, "sgpu_fuse_documents_host") and hasattr(L, "sgpu_debug_fuse_stats")
    assert L.sgpu_abi_version() == 4


@pytest.mark.parametrize("name", sorted(fuse_cases.CASES))
def test_host_twin_equals_the_restatement(name):
    case = fuse_cases.make(name)
    ix = case.index
    for call in case.calls.values():
        for config in call.configs:
            for k in call.ks:
                for threads in (1, 4):   # (the thread count does not change a bit)
                    got = ix.fuse_documents_host(*call.args(), *config, k, num_threads=threads)
                    diff = same(got, case.expected(call.name, config, k))
                    assert diff is None, (name, call.name, config, k, threads, diff)
    # the named edges, read off the host twin's rows
    call = case.calls["empty"]
    out = ix.fuse_documents_host(*call.args(), *call.configs[0], 8)
    assert out[6].tolist() == [0, 2, 0]
    for q in range(3):
        for a in out[:6]:
            assert not a[q, out[6][q]:].view(np.uint32 if a.dtype.itemsize == 4 else np.uint64).any()
    assert not out[2][1].view(np.uint32).any()   # an empty query: every sparse score is +0.0
    for call in case.calls.values():   # an absent document: ext +0.0 and rank 0; a present one: a rank of its own
        f, ids, sp, ex, rs, re, n = ix.fuse_documents_host(*call.args(), *call.configs[0], 1024)
        for q in range(call.nq):
            listed = {}
            for i, x in zip(call.lists[q].tolist(), call.exts[q]):
                listed[i] = listed.get(i, False) or not np.isnan(x)
            assert n[q] == min(1024, len(listed))
            if len(listed) > 1024:   # (the ranks below are all of them only where the row holds every document)
                continue
            there = np.array([listed[i] for i in ids[q, :n[q]].tolist()], bool)
            assert not ex[q, :n[q]][~there].view(np.uint32).any() and not re[q, :n[q]][~there].any()
            assert sorted(re[q, :n[q]][there].tolist()) == list(range(1, int(there.sum()) + 1))
            assert sorted(rs[q, :n[q]].tolist()) == list(range(1, int(n[q]) + 1))


# the calls (with config and k) on which a wrong reading must differ from the host twin
WRONG = [("shared_ranks", "ties", (RRF, 1.0, 1.0, 60.0), 8), ("shared_ranks", "ties", (RRF, 1.0, 0.5, 0.0), 4),
         ("zero_based", "ties", (RRF, 1.0, 1.0, 60.0), 8), ("zero_based", "absent", (RRF, 1.0, 1.0, 60.0), 12),
         ("absent_is_zero", "absent", (RRF, 1.0, 1.0, 60.0), 12), ("absent_is_zero", "absent", (MINMAX, 0.5, 0.25, 0.0), 12),
         ("absent_is_zero", "absent", (SUM, 1.0, 0.5, 0.0), 5), ("dup_first", "dups", (RRF, 1.0, 1.0, 60.0), 6),
         ("dup_first", "dups", (SUM, 1.0, 0.5, 0.0), 5), ("dup_twice", "dups", (RRF, 1.0, 1.0, 60.0), 6),
         ("float64", "methods", (SUM, 0.3, -0.7, 0.0), 20), ("float64", "random", (RRF, 1.0, 1.0, 60.0), 60),
         ("float64", "random", (MINMAX, -0.3, 0.7, 0.0), 60), ("contracted", "methods", (SUM, 0.3, -0.7, 0.0), 20),
         ("contracted", "random", (MINMAX, -0.3, 0.7, 0.0), 60), ("contracted", "random", (SUM, 0.3, -0.7, 0.0), 60),
         ("flat_is_zero", "flat", (MINMAX, 1.0, 1.0, 0.0), 6), ("flat_is_zero", "flat", (MINMAX, 0.5, -2.0, 0.0), 3),
         ("ties_high", "ties", (SUM, 1.0, 1.0, 0.0), 8), ("ties_high", "ties", (MINMAX, 1.0, 1.0, 0.0), 4),
         ("neg_zero_equal", "negzero", (SUM, -1.0, 1.0, 0.0), 2), ("neg_zero_equal", "negzero", (SUM, -1.0, 1.0, 0.0), 1)]


@pytest.mark.parametrize("name", ["u16_f16_32767", "u16_dvb_32767", "u32_u8_32768", "u16_f16_300"])
def test_each_wrong_reading_fails_on_its_named_call(name):
    case = fuse_cases.make(name)
    assert {r for r, _, _, _ in WRONG} == set(fuse_cases.READINGS)
    for reading, call_name, config, k in WRONG:
        call = case.calls[call_name]
        config = (config[0],) + tuple(float(np.float32(x)) for x in config[1:])   # (the f32 the call holds)
        assert config in call.configs and k in call.ks, (call_name, config, k)
        got = case.index.fuse_documents_host(*call.args(), *config, k)
        wrong = fuse_cases.fuse_numpy(case, call, config, k, reading=reading)
        assert same(got, wrong) is not None, (name, reading, call_name, config, k)
        assert same(got, case.expected(call_name, config, k)) is None
    # negzero: +0.0 stands above -0.0, although the document that fuses to -0.0 has the smaller id
    call = case.calls["negzero"]
    f, ids, sp, ex, rs, re, n = case.index.fuse_documents_host(*call.args(), SUM, -1.0, 1.0, 0.0, 2)
    assert f[0].view(np.uint32).tolist() == [0, 0x80000000] and ids[0, 0] > ids[0, 1]
    wrong = fuse_cases.fuse_numpy(case, call, (SUM, -1.0, 1.0, 0.0), 2, reading="neg_zero_equal")
    assert wrong[1][0, 0] < wrong[1][0, 1]
    # dups: the largest external score of a document listed three times, not the first
    call = case.calls["dups"]
    f, ids, sp, ex, rs, re, n = case.index.fuse_documents_host(*call.args(), *call.configs[0], 6)
    assert ex[0, ids[0].tolist().index(case.named["len_127"])] == 3.0 and n[0] == 5


@pytest.mark.parametrize("name", sorted(fuse_cases.CASES))
def test_consequences_and_permutations(name):
    case = fuse_cases.make(name)
    ix = case.index
    for call in case.calls.values():
        q_off, qc, qv, cand_off, cand_ids, cand_ext = call.args()
        for k in call.ks:
            want = ix.rerank_documents_host(q_off, qc, qv, cand_off, cand_ids, k)
            filled = np.arange(k)[None, :] < want[2][:, None]
            # SUM, w_sparse = 1, w_ext = 0: the rows of sgpu_rerank_documents_host, whatever cand_ext holds
            f, ids, sp, ex, rs, re, n = ix.fuse_documents_host(q_off, qc, qv, cand_off, cand_ids, cand_ext, SUM, 1.0, 0.0, 0.0, k)
            assert same((sp, ids, n), want, ("out_sparse", "out_doc_ids", "out_n")) is None, (name, call.name, k)
            assert np.array_equal(f.view(np.uint32), sp.view(np.uint32))
            # RRF, w_sparse = 1, w_ext = 0, rrf_c = 60: rerank's ids, and the sparse rank is the slot
            f, ids, sp, ex, rs, re, n = ix.fuse_documents_host(q_off, qc, qv, cand_off, cand_ids, cand_ext, RRF, 1.0, 0.0, 60.0, k)
            assert same((ids, n), want[1:], ("out_doc_ids", "out_n")) is None, (name, call.name, k)
            assert np.array_equal(rs, np.where(filled, np.arange(k)[None, :] + 1, 0))
            # a permutation of the entries changes no row: the twin ...
            for seed in (3, 5):
                for config in call.configs[:4]:
                    got = ix.fuse_documents_host(*call.args(fuse_cases.permuted(call, seed)), *config, k)
                    assert same(got, case.expected(call.name, config, k)) is None, (name, call.name, config, k, seed)
        # ... and the restatement
        config, k = call.configs[-1], call.ks[0]
        assert same(fuse_cases.fuse_numpy(case, call, config, k, order=fuse_cases.permuted(call, 7)),
                    case.expected(call.name, config, k)) is None, (name, call.name)


@pytest.fixture(scope="module")
def small():
    dim = 300
    off, comps, vals = random_dataset(3, 50, dim, 3, 20)
    ix = _native.NativeIndex.build(2, dim, off, comps, vals, BuildConfig.defaults(n_postings=10))
    q_off, qc, qv = random_queries(4, 3, dim, 2, 8)
    return ix, dim, q_off, qc, qv


def _calls(ix, q_off, qc, qv, cand_off, cand_ids, cand_ext, method, ws, we, c, k, outs):
    """(name, status, message) of the device call and of the host twin with the same arguments."""
    L = _native.lib()
    nq = len(q_off) - 1 if q_off is not None else 0
    o = [_p(a) for a in outs]
    got = []
    st = L.sgpu_fuse_documents(ix.h if ix else None, 0, _p(q_off), _p(qc), _p(qv), nq, _p(cand_off), _p(cand_ids), _p(cand_ext),
                               method, ws, we, c, k, *o)
    got.append(("device", st, L.sgpu_last_error().decode()))
    st = L.sgpu_fuse_documents_host(ix.h if ix else None, _p(q_off), _p(qc), _p(qv), nq, _p(cand_off), _p(cand_ids), _p(cand_ext),
                                    method, ws, we, c, k, 0, *o)
    got.append(("host", st, L.sgpu_last_error().decode()))
    return got


def _outs(nq, k):
    return [np.zeros((nq, k), np.float32), np.zeros((nq, k), np.uint64), np.zeros((nq, k), np.float32), np.zeros((nq, k), np.float32),
            np.zeros((nq, k), np.uint32), np.zeros((nq, k), np.uint32), np.zeros(nq, np.uint32)]


def test_argument_checks_in_order_without_a_device(small):
    ix, dim, q_off, qc, qv = small
    cand_off = np.array([0, 2, 2, 3], np.uint64)
    cand_ids = np.array([1, 49, 7], np.uint64)
    ext = np.array([0.5, np.nan, -2.0], np.float32)
    outs = _outs(3, 4)
    zero = np.zeros(4, np.uint64)
    inf, nan = float("inf"), float("nan")
    bad = (7, nan, nan, nan, 0)   # method, weights, rrf_c and k that later checks refuse
    # 1. null arguments: cand_ids, cand_ext and every output count, also with nothing to do and when later checks would fire
    for args in ((None, q_off, qc, qv, cand_off, cand_ids, ext), (ix, None, qc, qv, cand_off, cand_ids, ext),
                 (ix, q_off, qc, qv, None, cand_ids, ext), (ix, q_off, qc, qv, cand_off, None, ext),
                 (ix, q_off, qc, qv, cand_off, cand_ids, None)):
        for name, st, _ in _calls(*args, RRF, 1.0, 1.0, 60.0, 4, outs):
            assert st == EINVAL, name
    for missing in range(7):
        o = list(outs)
        o[missing] = None
        for off in (cand_off, zero):
            for rest in ((RRF, 1.0, 1.0, 60.0, 4), bad):
                for name, st, msg in _calls(ix, q_off, qc, qv, off, cand_ids, ext, *rest, o):
                    assert st == EINVAL and "null" in msg, (name, missing, msg)
    # 2. what the score call checks, before everything of this call's own: the queries, cand_off, the ids
    bad_qc = qc.copy()
    bad_qc[0] = dim
    bad_ids = np.array([1, 50, 7], np.uint64)
    inf_ext = np.array([0.5, -inf, inf], np.float32)
    for name, st, msg in _calls(ix, q_off, bad_qc, qv, np.array([1, 2, 2, 3], np.uint64), bad_ids, inf_ext, *bad, outs):
        assert st == EINVAL and "component >= dim" in msg, (name, msg)
    for name, st, msg in _calls(ix, q_off, qc, qv, np.array([0, 2, 1, 3], np.uint64), bad_ids, inf_ext, *bad, outs):
        assert st == EINVAL and "cand_off" in msg, (name, msg)
    for name, st, msg in _calls(ix, q_off, qc, qv, cand_off, bad_ids, inf_ext, *bad, outs):
        assert st == EINVAL and "query 0" in msg and "document id 50" in msg, (name, msg)
    # 3. an infinite external score, before the method: the message names the first such candidate and its query
    for name, st, msg in _calls(ix, q_off, qc, qv, cand_off, cand_ids, inf_ext, *bad, outs):
        assert st == EINVAL and "query 0" in msg and "candidate 1" in msg and "document id 49" in msg and "infinite" in msg, (name, msg)
    for name, st, msg in _calls(ix, q_off, qc, qv, cand_off, cand_ids, np.array([nan, 1.0, inf], np.float32), *bad, outs):
        assert st == EINVAL and "query 2" in msg and "candidate 0" in msg and "document id 7" in msg, (name, msg)
    # 4. an unknown method, before the weights
    for name, st, msg in _calls(ix, q_off, qc, qv, cand_off, cand_ids, ext, 3, nan, nan, nan, 0, outs):
        assert st == EINVAL and "method 3" in msg, (name, msg)
    # 5. weights that are not finite, before rrf_c
    for ws, we, word in ((nan, inf, "w_sparse"), (inf, 1.0, "w_sparse"), (1.0, nan, "w_ext"), (0.0, -inf, "w_ext")):
        for name, st, msg in _calls(ix, q_off, qc, qv, cand_off, cand_ids, ext, RRF, ws, we, -1.0, 0, outs):
            assert st == EINVAL and word in msg, (name, msg)
    # 6. RRF only: rrf_c not finite or below 0, before the candidate count
    many_off = np.array([0, 0, 4097, 4097], np.uint64)
    many_ids = np.zeros(4097, np.uint64)
    many_ext = np.zeros(4097, np.float32)
    for c in (nan, inf, -1.0, -1e-30):
        for name, st, msg in _calls(ix, q_off, qc, qv, many_off, many_ids, many_ext, RRF, 1.0, 1.0, c, 0, outs):
            assert st == EINVAL and "rrf_c" in msg, (name, msg)
    # 7. more than 4096 listed candidates of one query, before k: the message names the query; rrf_c is RRF's alone
    for method, c in ((RRF, 0.0), (MINMAX, nan), (SUM, -1.0)):
        for name, st, msg in _calls(ix, q_off, qc, qv, many_off, many_ids, many_ext, method, 1.0, 1.0, c, 0, outs):
            assert st == ELIMIT and "query 1" in msg and "4097" in msg, (name, msg)
    # 8. k == 0, 9. k > 1024 - before the device checks (the index is not uploaded)
    for name, st, msg in _calls(ix, q_off, qc, qv, cand_off, cand_ids, ext, SUM, 1.0, 1.0, nan, 0, outs):
        assert st == EINVAL and "k must be" in msg, (name, msg)
    for name, st, msg in _calls(ix, q_off, qc, qv, cand_off, cand_ids, ext, SUM, 1.0, 1.0, nan, 1025, outs):
        assert st == ELIMIT and "1025" in msg, (name, msg)
    # 10. the device call on an index that is not uploaded: SGPU_EDEVICE; the host twin runs - also with nothing to do
    (_, st, msg), (_, hst, _) = _calls(ix, q_off, qc, qv, cand_off, cand_ids, ext, RRF, 1.0, 1.0, 0.0, 4, outs)
    assert st == EDEVICE and "not uploaded" in msg and hst == 0 and outs[6].tolist() == [2, 0, 1]
    assert sorted(outs[1][0, :2].tolist()) == [1, 49] and outs[5][:, 0].tolist() in ([1, 0, 1], [0, 0, 1]) and outs[3][2, 0] == -2.0
    (_, st, _), (_, hst, _) = _calls(ix, q_off, qc, qv, zero, cand_ids, ext, RRF, 1.0, 1.0, 0.0, 4, outs)
    assert st == EDEVICE and hst == 0 and not outs[6].any() and not outs[0].any() and not outs[1].any() and not outs[4].any()
    o = [_p(a) for a in outs]
    assert _native.lib().sgpu_fuse_documents_host(ix.h, _p(q_off), _p(qc), _p(qv), 0, _p(zero), _p(cand_ids), _p(ext), RRF, 1.0, 1.0,
                                                  60.0, 4, 0, *o) == 0
    # 4096 candidates of one query and k = 1024 are taken
    full = _outs(3, 1024)
    (_, st, _), (_, hst, msg) = _calls(ix, q_off, qc, qv, np.array([0, 0, 4096, 4096], np.uint64), many_ids[:4096], many_ext[:4096],
                                       MINMAX, 1.0, 1.0, 0.0, 1024, full)
    assert st == EDEVICE and hst == 0 and full[6].tolist() == [0, 1, 0] and full[4][1, 0] == 1 and full[5][1, 0] == 1, msg
    assert full[0][1, 0] == 2.0   # (one document: both orders are flat, both normalised scores 1)


def test_query_length_limit_comes_before_the_fusion_checks():
    dim = 9000
    off, comps, vals = random_dataset(5, 20, dim, 3, 20)
    ix = _native.NativeIndex.build(2, dim, off, comps, vals, BuildConfig.defaults(n_postings=10))
    q_off = np.array([0, 8193], np.uint64)
    qc = np.arange(8193, dtype=np.uint32)
    qv = np.ones(8193, np.float32)
    for name, st, msg in _calls(ix, q_off, qc, qv, np.array([0, 1], np.uint64), np.array([3], np.uint64),
                                np.array([float("inf")], np.float32), 9, float("nan"), 1.0, -1.0, 0, _outs(1, 1)):
        assert st == ELIMIT and "8193" in msg, (name, msg)


@pytest.mark.parametrize("cls", ["SeismicIndex", "SeismicIndexLV", "SeismicIndexDotVByte"])
def test_python_fuse_on_the_host(cls):
    ids, vecs, _ = read_jsonl(os.path.join(GOLD_TOY, "documents.jsonl"))
    _, qvecs, _ = read_jsonl(os.path.join(GOLD_TOY, "queries.jsonl"))
    qc = [np.array(list(v.keys())) for v in qvecs]
    qv = [np.array(list(v.values()), np.float32) for v in qvecs]
    ix = getattr(seismic_amd, cls).build(os.path.join(GOLD_TOY, "documents.jsonl"), n_postings=50, centroid_fraction=0.2,
                                          upload=False)
    lists = [list(ids[q % len(ids):q % len(ids) + 12]) + [ids[q % len(ids)]] for q in range(len(qc))]
    lists[1] = []
    ext = [[None if i % 3 == 0 else float((i * 7) % 5) - 1.5 for i in range(len(row))] for row in lists]
    rows = ix.batch_fuse(qc, qv, lists, ext, 5, device=False)
    assert len(rows) == len(qc) and rows[1] == []
    scores = ix.batch_score(qc, qv, lists, device=False)
    for q, row in enumerate(rows):
        docs = sorted(set(lists[q]))
        assert len(row) == min(5, len(docs)) and len({d for _, d, _, _, _, _ in row}) == len(row)
        best = {}
        for i, d in enumerate(lists[q]):
            if ext[q][i] is not None:
                best[d] = max(best.get(d, -np.inf), ext[q][i])
        by_sparse = sorted(docs, key=lambda d: -float(scores[q][lists[q].index(d)]))
        for f, d, s, x, a, b in row:
            assert s == float(scores[q][lists[q].index(d)]) and x == best.get(d, 0.0) and (b > 0) == (d in best)
            assert s == float(scores[q][lists[q].index(by_sparse[a - 1])])   # (the rank's document has this score)
            want = np.float32(1.0) / np.float32(60.0 + a) + (np.float32(1.0) / np.float32(60.0 + b) if b else np.float32(0.0))
            assert f == float(np.float32(want))
        assert [f for f, _, _, _, _, _ in row] == sorted((f for f, _, _, _, _, _ in row), reverse=True)
    assert ix.fuse(qc[0], qv[0], lists[0], ext[0], 5, device=False) == rows[0]
    # the other methods by name and by number; SUM with w_ext = 0 is batch_rerank
    assert ix.batch_fuse(qc, qv, lists, ext, 5, method="minmax", device=False) == ix.batch_fuse(qc, qv, lists, ext, 5, method=1, device=False)
    plain = ix.batch_fuse(qc, qv, lists, ext, 5, method="sum", w_sparse=1.0, w_ext=0.0, device=False)
    assert [[(f, d) for f, d, _, _, _, _ in row] for row in plain] == ix.batch_rerank(qc, qv, lists, 5, device=False)
    with pytest.raises(ValueError):
        ix.batch_fuse(qc, qv, lists, ext[:-1], 5, device=False)
    with pytest.raises(KeyError):
        ix.fuse(qc[0], qv[0], ["no-such-document"], [1.0], 3, device=False)
    with pytest.raises(_native.SeismicHipError):
        ix.fuse(qc[0], qv[0], lists[0], ext[0], 1025, device=False)
    with pytest.raises(_native.SeismicHipError):
        ix.fuse(qc[0], qv[0], lists[0], [float("inf")] * len(lists[0]), 3, device=False)
    with pytest.raises(_native.SeismicHipError):
        ix.fuse(qc[0], qv[0], lists[0], ext[0], 3, method=3, device=False)
