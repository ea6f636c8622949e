"""sgpu_score_documents on the device: equal, as bits, to its host twin and to the oracle on tests/score_cases.py, for
every value type, component width, forward layout and lookup form; several launches per call; consistent with what the
searches return; safe beside searching threads; the Python classes."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

import score_cases
import seismic_amd
from seismic_amd import _native
from seismic_amd._abi import BuildConfig
from seismic_amd.index import read_jsonl
from util import random_dataset, random_queries

pytestmark = pytest.mark.gpu

GOLD_TOY = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "toy")


def _stats(ix):
    """sgpu_debug_score_stats of replica 0: kernel ms, launches, dense, grid, block, LDS bytes."""
    out = np.zeros(8, np.float64)
    L = _native.lib()
    L.sgpu_debug_score_stats.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    _native.check(L.sgpu_debug_score_stats(ix.h, 0, out.ctypes.data_as(C.c_void_p)))
    return dict(ms=out[0], launches=int(out[1]), dense=int(out[2]), grid=int(out[3]), block=int(out[4]), lds=int(out[5]))


def _check_case(case, ix):
    for cand_off, cand_ids in ((case.cand_off, case.cand_ids), (case.all_off, case.all_ids)):
        dev = ix.score_documents(case.q_off, case.qc, case.qv, cand_off, cand_ids)
        host = ix.score_documents_host(case.q_off, case.qc, case.qv, cand_off, cand_ids)
        want = case.expected(cand_off, cand_ids)
        assert np.array_equal(host.view(np.uint32), want)
        bad = np.flatnonzero(dev.view(np.uint32) != want)
        assert len(bad) == 0, "%s: %d of %d scores differ, first at %d: %r != %r" % (
            case.name, len(bad), len(want), bad[0], dev[bad[0]], want[bad[0]:bad[0] + 1].view(np.float32)[0])


@pytest.mark.parametrize("layout", ["block", "doc"])
@pytest.mark.parametrize("name", sorted(score_cases.CASES))
def test_device_equals_host_twin_equals_oracle(name, layout, monkeypatch):
    case = score_cases.make(name)
    monkeypatch.setenv("SGPU_FWD_LAYOUT", layout)   # (read by the upload)
    ix = case.build().upload(0)
    _check_case(case, ix)
    st = _stats(ix)
    assert st["dense"] == (1 if case.dim <= 32767 else 0) and st["launches"] == 1
    # nothing to score: SGPU_OK, nothing written
    zero = np.zeros(score_cases.N_QUERIES + 1, np.uint64)
    assert len(ix.score_documents(case.q_off, case.qc, case.qv, zero, np.zeros(0, np.uint64))) == 0
    assert len(ix.score_documents(np.zeros(1, np.uint64), case.qc, case.qv, np.zeros(1, np.uint64), np.zeros(0, np.uint64))) == 0
    ix.close()


@pytest.mark.parametrize("name", ["u16_f16_small", "u16_dvb_small", "u32_u8_small"])
def test_the_lookup_form_changes_no_score(name, monkeypatch):
    case = score_cases.make(name)
    ix = case.build().upload(0)
    monkeypatch.setenv("SGPU_SCORE_LOOKUP", "2")   # (test hook: the hash table although the dense one fits)
    _check_case(case, ix)
    assert _stats(ix)["dense"] == 0
    monkeypatch.delenv("SGPU_SCORE_LOOKUP")
    _check_case(case, ix)
    assert _stats(ix)["dense"] == 1
    ix.close()


@pytest.mark.parametrize("name", ["u16_dvb", "u32_f16", "u16_f16_small"])
def test_several_launches_give_the_same_scores(name, monkeypatch):
    case = score_cases.make(name)
    ix = case.build().upload(0)
    one = ix.score_documents(case.q_off, case.qc, case.qv, case.cand_off, case.cand_ids)
    assert _stats(ix)["launches"] == 1
    for chunk in (64, 1, 1000):   # (below, far below and above the tile of 128 candidates)
        if chunk == 1:
            off, ids = case.cand_off[:9], case.cand_ids[:int(case.cand_off[8])][-7:]   # queries 3 .. 7: seven candidates
            off = np.concatenate([np.zeros(4, np.uint64), off[4:] - off[3]])
            q_off, want = case.q_off[:9], one[int(case.cand_off[3]):int(case.cand_off[8])]
        else:
            off, ids, q_off, want = case.cand_off, case.cand_ids, case.q_off, one
        monkeypatch.setenv("SGPU_SCORE_CHUNK", str(chunk))
        got = ix.score_documents(q_off, case.qc, case.qv, off, ids)
        monkeypatch.delenv("SGPU_SCORE_CHUNK")
        assert _stats(ix)["launches"] == -(-len(ids) // chunk)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    ix.close()


@pytest.fixture(scope="module")
def searched():
    dim = 4000
    off, comps, vals = random_dataset(21, 5000, dim, 8, 150)
    ix = _native.NativeIndex.build(2, dim, off, comps, vals, BuildConfig.defaults())
    ix.upload(0)
    q_off, qc, qv = random_queries(22, 64, dim, 5, 40)
    yield ix, q_off, qc, qv
    ix.close()


def _rescore(ix, q_off, qc, qv, ids, n):
    cand_off = np.zeros(len(n) + 1, np.uint64)
    cand_off[1:] = np.cumsum(n)
    cand = np.concatenate([ids[q, :n[q]] for q in range(len(n))]).astype(np.uint64)
    return ix.score_documents(q_off, qc, qv, cand_off, cand), cand_off.astype(np.int64)


def test_scores_are_the_bits_the_searches_return(searched):
    ix, q_off, qc, qv = searched
    for n_knn in (0, 3):
        if n_knn:
            ix.build_knn(5)
        sc, ids, n = ix.batch_search(q_off, qc, qv, 10, 4, 0.8, n_knn=n_knn)
        assert n.sum() > 5 * len(n)
        got, off = _rescore(ix, q_off, qc, qv, ids, n)
        for q in range(len(n)):
            assert np.array_equal(got[off[q]:off[q + 1]].view(np.uint32), sc[q, :n[q]].view(np.uint32)), (n_knn, q)
    for vt in (1, 2):   # the other value types: the converted index's own searches
        cx = ix.convert(vt).upload(0)
        sc, ids, n = cx.batch_search(q_off, qc, qv, 10, 4, 0.8)
        got, off = _rescore(cx, q_off, qc, qv, ids, n)
        for q in range(len(n)):
            assert np.array_equal(got[off[q]:off[q + 1]].view(np.uint32), sc[q, :n[q]].view(np.uint32)), (vt, q)
        cx.close()


def test_scoring_beside_two_searching_threads():
    case = score_cases.make("u16_f16")
    ix = case.build().upload(0)
    want_scores = case.expected(case.cand_off, case.cand_ids)
    want_search = ix.batch_search(case.q_off, case.qc, case.qv, 10, 4, 0.8)
    errors = []

    def score():
        for _ in range(20):
            got = ix.score_documents(case.q_off, case.qc, case.qv, case.cand_off, case.cand_ids)
            if not np.array_equal(got.view(np.uint32), want_scores):
                errors.append("score")

    def search():
        for _ in range(20):
            sc, ids, n = ix.batch_search(case.q_off, case.qc, case.qv, 10, 4, 0.8)
            if not (np.array_equal(n, want_search[2]) and np.array_equal(ids, want_search[1])
                    and np.array_equal(sc.view(np.uint32), want_search[0].view(np.uint32))):
                errors.append("search")

    threads = [threading.Thread(target=score)] + [threading.Thread(target=search) for _ in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    ix.close()


@pytest.mark.parametrize("cls", ["SeismicIndex", "SeismicIndexLV", "SeismicIndexDotVByte"])
def test_python_batch_score_on_the_device_equals_the_host(cls):
    ids, _, _ = read_jsonl(os.path.join(GOLD_TOY, "documents.jsonl"))
    _, qvecs, _ = read_jsonl(os.path.join(GOLD_TOY, "queries.jsonl"))
    qc = [np.array(list(v.keys())) for v in qvecs]
    qv = [np.array(list(v.values()), np.float32) for v in qvecs]
    ix = getattr(seismic_amd, cls).build(os.path.join(GOLD_TOY, "documents.jsonl"), n_postings=50, centroid_fraction=0.2)
    lists = [list(reversed(ids)) if q % 2 else [ids[q % len(ids)]] * 3 for q in range(len(qc))]
    lists[1] = []
    dev = ix.batch_score(qc, qv, lists)
    host = ix.batch_score(qc, qv, lists, device=False)
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(dev, host))
    assert ix.batch_rerank(qc, qv, lists, 3) == ix.batch_rerank(qc, qv, lists, 3, device=False)
    assert ix.batch_score(qc, qv, lists, device=0)[0].tolist() == dev[0].tolist()
    with pytest.raises(ValueError):
        ix.batch_score(qc, qv, lists, device=1)
