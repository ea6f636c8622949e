"""sgpu_explain_documents on the device: every output equal, as bits, to its host twin (and so to the restatement) on
tests/explain_cases.py, for every value type, component width, forward layout and lookup form; its scores the score call's;
independent of the cuts into launches; two replicas; safe beside a searching and a scoring thread; the device argument
checks; the Python classes."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

import explain_cases
import seismic_amd
from explain_cases import MS, same
from seismic_amd import _native
from seismic_amd.index import read_jsonl

pytestmark = pytest.mark.gpu

GOLD_TOY = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "toy")
EDEVICE = 2


def _stats(ix, replica=0):
    out = np.zeros(8, np.float64)
    L = _native.lib()
    L.sgpu_debug_score_stats.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    _native.check(L.sgpu_debug_score_stats(ix.h, replica, out.ctypes.data_as(C.c_void_p)))
    return dict(launches=int(out[1]), dense=int(out[2]))


def _explain(ix, case, m, replica=0):
    return ix.explain_documents(case.q_off, case.qc, case.qv, case.cand_off, case.cand_ids, m, replica=replica)


@pytest.mark.parametrize("layout", ["block", "doc"])
@pytest.mark.parametrize("name", sorted(explain_cases.CASES))
def test_device_equals_host_twin(name, layout, monkeypatch):
    case = explain_cases.make(name)
    monkeypatch.setenv("SGPU_FWD_LAYOUT", layout)   # (read by the upload)
    ix = case.build().upload(0)
    for m in MS:
        dev = _explain(ix, case, m)
        host = ix.explain_documents_host(case.q_off, case.qc, case.qv, case.cand_off, case.cand_ids, m)
        assert same(host, case.expected(m)) is None
        assert same(dev, host) is None, (name, m, same(dev, host))
        st = _stats(ix)
        assert st["dense"] == (1 if case.dim < 32768 else 0) and st["launches"] == 1
    # the scores are the score call's bits
    sc = ix.score_documents(case.q_off, case.qc, case.qv, case.cand_off, case.cand_ids)
    assert np.array_equal(dev[0].view(np.uint32), sc.view(np.uint32))
    # nothing to explain: SGPU_OK
    zero = np.zeros(explain_cases.N_QUERIES + 1, np.uint64)
    assert all(len(a) == 0 for a in ix.explain_documents(case.q_off, case.qc, case.qv, zero, np.zeros(0, np.uint64), 10))
    assert all(len(a) == 0 for a in ix.explain_documents(np.zeros(1, np.uint64), case.qc, case.qv, np.zeros(1, np.uint64),
                                                          np.zeros(0, np.uint64), 10))
    ix.close()


@pytest.mark.parametrize("name", ["u16_f16", "u16_dvb"])
def test_the_lookup_form_changes_no_output(name, monkeypatch):
    case = explain_cases.make(name)
    ix = case.build().upload(0)
    monkeypatch.setenv("SGPU_SCORE_LOOKUP", "2")   # (test hook: the hash table although the dense one fits)
    for m in (1, 32):
        assert same(_explain(ix, case, m), case.expected(m)) is None
        assert _stats(ix)["dense"] == 0
    ix.close()


@pytest.mark.parametrize("name", ["u16_dvb", "u32_f16"])
def test_the_cuts_into_launches_change_no_output(name, monkeypatch):
    case = explain_cases.make(name)
    ix = case.build().upload(0)
    # queries 1 .. 5: lists of 127, 128, 129, 0 and 1 ids (385 candidates: chunk 1 stays at a few hundred launches)
    lo, hi = int(case.cand_off[1]), int(case.cand_off[6])
    q_off = case.q_off[:7]
    off = np.concatenate([np.zeros(2, np.uint64), case.cand_off[2:7] - case.cand_off[1]])
    ids = case.cand_ids[lo:hi]
    want = tuple(a[lo:hi] for a in case.expected(10))
    for chunk in (1, 127, 128, 129):
        monkeypatch.setenv("SGPU_SCORE_CHUNK", str(chunk))
        got = ix.explain_documents(q_off, case.qc, case.qv, off, ids, 10)
        monkeypatch.delenv("SGPU_SCORE_CHUNK")
        assert _stats(ix)["launches"] == -(-len(ids) // chunk)
        assert same(got, want) is None, (chunk, same(got, want))
    ix.close()


@pytest.mark.parametrize("name", ["u16_f16", "u16_u8", "u16_dvb"])
def test_subnormal_weights_as_on_the_host(name):
    """Weights of 2^-149 and 2^-100: the device multiplies subnormals as the host does, and a fixed-u8 weight whose product
    with val_scale is +0.0 makes no term on either."""
    case = explain_cases.make(name)
    q_off, qc, qv, cand_off, cand, want = case.tiny_weight_call()
    ix = case.build().upload(0)
    dev = ix.explain_documents(q_off, qc, qv, cand_off, cand, 4)
    host = ix.explain_documents_host(q_off, qc, qv, cand_off, cand, 4)
    assert dev[1].tolist() == want and same(dev, host) is None, same(dev, host)
    ix.close()


def test_two_replicas():
    case = explain_cases.make("u16_u8")
    ix = case.build().upload_many([0, 0])
    assert ix.replicas == 2
    for replica in (0, 1):
        assert same(_explain(ix, case, 10, replica), case.expected(10)) is None
        assert _stats(ix, replica)["launches"] == 1
    ix.close()


def test_explaining_beside_a_searching_and_a_scoring_thread():
    case = explain_cases.make("u16_f16")
    ix = case.build().upload(0)
    want = case.expected(10)
    want_scores = want[0].view(np.uint32)
    want_search = ix.batch_search(case.q_off, case.qc, case.qv, 10, 4, 0.8)
    errors = []

    def explain():
        for _ in range(10):
            if same(_explain(ix, case, 10), want) is not None:
                errors.append("explain")

    def score():
        for _ in range(10):
            got = ix.score_documents(case.q_off, case.qc, case.qv, case.cand_off, case.cand_ids)
            if not np.array_equal(got.view(np.uint32), want_scores):
                errors.append("score")

    def search():
        for _ in range(10):
            sc, ids, n = ix.batch_search(case.q_off, case.qc, case.qv, 10, 4, 0.8)
            if not (np.array_equal(n, want_search[2]) and np.array_equal(ids, want_search[1])
                    and np.array_equal(sc.view(np.uint32), want_search[0].view(np.uint32))):
                errors.append("search")

    threads = [threading.Thread(target=f) for f in (explain, score, search)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    ix.close()


def test_device_argument_checks():
    case = explain_cases.make("u16_f16")
    L = _native.lib()

    def call(ix, replica, m=10):
        n = len(case.cand_ids)
        outs = [np.zeros(n, np.float32), np.zeros(n, np.uint32)] + [np.zeros((n, m), np.uint32) for _ in range(4)]
        p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
        st = L.sgpu_explain_documents(ix.h, replica, p(case.q_off), p(case.qc), p(case.qv), explain_cases.N_QUERIES, p(case.cand_off),
                                      p(case.cand_ids), m, *[p(a) for a in outs])
        return st, L.sgpu_last_error().decode()

    st, msg = call(case.index, 0)           # not uploaded
    assert st == EDEVICE and "not uploaded" in msg
    ix = case.build().upload(0)
    assert call(ix, 0)[0] == 0
    st, msg = call(ix, 1)                   # replica out of range
    assert st == EDEVICE and "replica" in msg
    assert call(ix, 1, 33)[0] == 5          # (m is checked before the device)
    ix.close()


@pytest.mark.parametrize("cls", ["SeismicIndex", "SeismicIndexLV", "SeismicIndexDotVByte"])
def test_python_batch_explain_on_the_device_equals_the_host(cls):
    ids, _, _ = read_jsonl(os.path.join(GOLD_TOY, "documents.jsonl"))
    _, qvecs, _ = read_jsonl(os.path.join(GOLD_TOY, "queries.jsonl"))
    qc = [np.array(list(v.keys())) for v in qvecs]
    qv = [np.array(list(v.values()), np.float32) for v in qvecs]
    ix = getattr(seismic_amd, cls).build(os.path.join(GOLD_TOY, "documents.jsonl"), n_postings=50, centroid_fraction=0.2)
    lists = [list(reversed(ids)) if q % 2 else [ids[q % len(ids)]] * 3 for q in range(len(qc))]
    lists[1] = []
    dev = ix.batch_explain(qc, qv, lists, m=5)
    assert dev == ix.batch_explain(qc, qv, lists, m=5, device=False)
    assert any(terms and isinstance(terms[0][0], str) for row in dev for _, _, terms in row)
    assert ix.explain(qc[0], qv[0], lists[0], m=5) == dev[0]
