"""sgpu_explain_documents / sgpu_explain_documents_host without a device: the host twin against the numpy restatement of
tests/explain_cases.py (every output array, bit for bit), its scores against sgpu_score_documents_host, the products
re-summed to the score, each wrong reading of the contract failing on the case named for it, the argument checks in the
header's order, and the Python classes with device=False.

Two of the wrong readings are narrower than their names. "Ties by position" is modelled as the later element first: the
components of a document ascend with the position, so ties broken by the earlier element cannot be told from the
contract's rule by any case. The u8 product taken as w * (code * scale) cannot differ with a power-of-two scale; the test
asserts that it does not."""
import ctypes as C
import os

import numpy as np
import pytest

import explain_cases
import seismic_amd
from explain_cases import MS, same
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
    assert "sgpu_status sgpu_explain_documents(sgpu_index* idx, uint32_t replica," in text
    assert "sgpu_status sgpu_explain_documents_host(const sgpu_index* idx," in text
    L = _native.lib()
    assert hasattr(L, "sgpu_explain_documents") and hasattr(L, "sgpu_explain_documents_host")
    assert L.sgpu_abi_version() == 4


@pytest.mark.parametrize("name", sorted(explain_cases.CASES))
def test_host_twin_equals_the_restatement(name):
    case = explain_cases.make(name)
    ix = case.index
    for m in MS:
        got = ix.explain_documents_host(case.q_off, case.qc, case.qv, case.cand_off, case.cand_ids, m)
        assert same(got, case.expected(m)) is None, (name, m, same(got, case.expected(m)))
    # one thread and many give the same bits
    one = ix.explain_documents_host(case.q_off, case.qc, case.qv, case.cand_off, case.cand_ids, 10, num_threads=1)
    assert same(one, case.expected(10)) is None
    # the scores are the score call's
    sc = ix.score_documents_host(case.q_off, case.qc, case.qv, case.cand_off, case.cand_ids)
    assert np.array_equal(one[0].view(np.uint32), sc.view(np.uint32))
    # an empty query and an empty document: +0.0, no terms, zeroed rows
    lo, hi = int(case.cand_off[2]), int(case.cand_off[3])
    assert not any(a[lo:hi].view(np.uint32).any() for a in one)
    row = case.row_of(0, "len_0")
    assert not any(a[row].view(np.uint32).any() for a in one)


@pytest.mark.parametrize("name", sorted(explain_cases.CASES))
def test_products_resummed_at_their_elements_give_the_score(name):
    case = explain_cases.make(name)
    sc, nt, tc, _, _, tp = case.index.explain_documents_host(case.q_off, case.qc, case.qv, case.cand_off, case.cand_ids, 32)
    off, comps, _, _ = case.stored()
    xor = np.arange(16)
    done = 0
    for i, d in enumerate(case.cand_ids.astype(np.int64).tolist()):
        if nt[i] > 32:
            continue
        at = np.searchsorted(comps[off[d]:off[d + 1]], tc[i, :nt[i]].astype(np.int64))   # the elements of the terms
        order = np.argsort(at)
        t = np.zeros(16, np.float32)
        for e, p in zip(at[order].tolist(), tp[i, :nt[i]][order]):   # (elements that are no terms add +-0.0: nothing)
            t[(e // 8) % 16] = t[(e // 8) % 16] + p
        for s in (8, 4, 2, 1):
            t = t + t[xor ^ s]
        assert t[:1].view(np.uint32)[0] == sc[i:i + 1].view(np.uint32)[0], (name, i, d)
        done += 1
    assert done > len(case.cand_ids) // 2


def _variant(case, change):
    """pairs() with every pair's terms passed through change(components, w, values, products, positions) -> the same."""
    out = []
    for s, c, w, v, p, e in case.pairs():
        c, w, v, p, e = change(c, w, v, p, e)
        out.append((s, c, w, v, p, e))
    return out


def _differs_at(case, m, pairs, query, label):
    """The wrong reading `pairs` gives other outputs than the host twin, and does so on the row of document `label`."""
    got = case.index.explain_documents_host(case.q_off, case.qc, case.qv, case.cand_off, case.cand_ids, m)
    wrong = case.expected(m, pairs)
    row = case.row_of(query, label)
    return any(not np.array_equal(a[row].view(np.uint32), b[row].view(np.uint32)) for a, b in zip(got, wrong))


@pytest.mark.parametrize("name", sorted(explain_cases.CASES))
def test_each_wrong_reading_fails_on_its_named_case(name):
    case = explain_cases.make(name)
    off, comps, x, scale = case.stored()

    # ties broken by a REVERSED position: a key that carries the element's position where the contract has the
    # complemented component puts the LATER element of equal products first. This is the only position rule the case can
    # tell from the contract: a document's components ascend with the position, so "earlier element first" IS "smaller
    # component first" and no case could separate the two.
    def by_position(c, w, v, p, e):
        o = np.lexsort((-e, -explain_cases.ordered(p).astype(np.int64)))
        return c[o], w[o], v[o], p[o], e[o]
    assert _differs_at(case, 10, _variant(case, by_position), 0, "ties")
    assert _differs_at(case, 1, _variant(case, by_position), 0, "ties")

    # -0.0 ordered with +0.0 (numeric comparison): then the component alone orders the two zero products
    def numeric(c, w, v, p, e):
        o = np.lexsort((c, -p.astype(np.float64)))
        return c[o], w[o], v[o], p[o], e[o]
    # (the -0.0 term of `zeros` has the smaller component - ExplainCase.check asserts it -, so the readings differ there)
    assert _differs_at(case, 10, _variant(case, numeric), 0, "zeros")

    # zero-weight query components counted, and padding counted: both add terms of product +-0.0
    def with_extra(extra_of):
        out, i = [], 0
        for q in range(explain_cases.N_QUERIES):
            for d in case.lists[q].astype(np.int64).tolist():
                s, c, w, v, p, e = case.pairs()[i]
                i += 1
                xc, xw, xv, xp = extra_of(q, d, c)
                c2, w2, v2, p2 = np.concatenate([c, xc]), np.concatenate([w, xw]), np.concatenate([v, xv]), np.concatenate([p, xp])
                key = (explain_cases.ordered(p2).astype(np.uint64) << np.uint64(32)) | (~c2.astype(np.uint32)).astype(np.uint64)
                o = np.argsort(key, kind="stable")[::-1]
                out.append((s, c2[o].astype(np.uint32), w2[o].astype(np.float32), v2[o].astype(np.float32),
                            p2[o].astype(np.float32), np.zeros(len(o), np.int64)))
        return out

    def zero_weights(q, d, c):
        qc, qw = case.queries[q]
        dc, dv = comps[off[d]:off[d + 1]], x[off[d]:off[d + 1]]
        hit = np.isin(dc, qc[qw == 0].astype(np.int64))
        w = qw[qw == 0][np.searchsorted(qc[qw == 0].astype(np.int64), dc[hit])]
        return dc[hit].astype(np.uint32), w, (dv[hit] * scale).astype(np.float32), (w * dv[hit]).astype(np.float32)
    assert _differs_at(case, 10, with_extra(zero_weights), 0, "zeros")

    def padding(q, d, c):   # a record pads its last slice of 8 by repeating the last component with the value 0
        n = int(off[d + 1] - off[d])
        pad = (-n) % 8
        if n == 0 or pad == 0 or len(c) == 0 or comps[off[d + 1] - 1] not in c.astype(np.int64):
            return np.zeros(0, np.uint32), np.zeros(0, np.float32), np.zeros(0, np.float32), np.zeros(0, np.float32)
        return (np.full(pad, comps[off[d + 1] - 1], np.uint32), np.full(pad, 1.0, np.float32), np.zeros(pad, np.float32),
                np.zeros(pad, np.float32))
    assert _differs_at(case, 32, with_extra(padding), 1, "big")   # (257 elements: 7 padding elements behind a term)

    # rows not zeroed past the terms
    got = case.index.explain_documents_host(case.q_off, case.qc, case.qv, case.cand_off, case.cand_ids, 32)
    row = case.row_of(0, "terms_2")
    assert got[1][row] == 2 and not any(a[row, 2:].view(np.uint32).any() for a in got[2:])

    # the u8 product taken as w * (code * scale): with a power-of-two scale both are the one rounding of the same real
    # number, so this reading cannot differ - asserted, not assumed
    if case.value_type:
        assert np.log2(float(scale)) == int(np.log2(float(scale)))
        for q, (qc, qw) in enumerate(case.queries):
            for d in case.lists[q].astype(np.int64).tolist()[:40]:
                dc, dv = comps[off[d]:off[d + 1]], x[off[d]:off[d + 1]]
                given = np.zeros(case.dim, np.float32)
                given[qc.astype(np.int64)] = qw
                a = (given[dc] * scale) * dv
                b = given[dc] * (dv * scale)
                assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("name", sorted(explain_cases.CASES))
def test_a_weight_whose_scaled_product_is_zero_makes_no_term(name):
    case = explain_cases.make(name)
    q_off, qc, qv, cand_off, cand, want = case.tiny_weight_call()
    if case.value_type:
        assert case.stored()[3] < 1 and want == [0, 1]   # (the narrowing applies: the case can show it)
    else:
        assert want == [1, 1]                            # (binary16 values: every weight that is not +-0 makes a term)
    sc, nt, tc, tq, td, tp = case.index.explain_documents_host(q_off, qc, qv, cand_off, cand, 4)
    assert nt.tolist() == want
    assert tq[1, 0] == qv[1] and tc[1, 0] == qc[1] and tp[1, 0] == sc[1]
    if not want[0]:
        assert not any(a[0].view(np.uint32).any() for a in (sc, tc, tq, td, tp))
    else:
        assert tq[0, 0].view(np.uint32) == qv[:1].view(np.uint32)[0] and tc[0, 0] == qc[0]


@pytest.fixture(scope="module")
def small():
    dim = 300
    off, comps, vals = random_dataset(3, 50, dim, 3, 20)
    ix = _native.NativeIndex.build(2, dim, off, comps, vals, BuildConfig.defaults(n_postings=10))
    q_off, qc, qv = random_queries(4, 3, dim, 2, 8)
    return ix, dim, q_off, qc, qv


def _outs(n, m):
    return [np.zeros(n, np.float32), np.zeros(n, np.uint32), np.zeros((n, m), np.uint32), np.zeros((n, m), np.float32),
            np.zeros((n, m), np.float32), np.zeros((n, m), np.float32)]


def _calls(ix, q_off, qc, qv, cand_off, cand_ids, m, outs):
    """(name, status, message) of the device call and of the host twin with the same arguments."""
    L = _native.lib()
    nq = len(q_off) - 1 if q_off is not None else 0
    o = [_p(a) for a in outs]
    got = []
    st = L.sgpu_explain_documents(ix.h if ix else None, 0, _p(q_off), _p(qc), _p(qv), nq, _p(cand_off), _p(cand_ids), m, *o)
    got.append(("device", st, L.sgpu_last_error().decode()))
    st = L.sgpu_explain_documents_host(ix.h if ix else None, _p(q_off), _p(qc), _p(qv), nq, _p(cand_off), _p(cand_ids), m, 0, *o)
    got.append(("host", st, L.sgpu_last_error().decode()))
    return got


def test_argument_checks_in_order_without_a_device(small):
    ix, dim, q_off, qc, qv = small
    cand_off = np.array([0, 2, 2, 3], np.uint64)
    cand_ids = np.array([1, 49, 7], np.uint64)
    outs = _outs(3, 4)
    zero = np.zeros(4, np.uint64)
    # 1. null arguments: every output pointer counts, also when there is no candidate and when m is bad too
    for args in ((None, q_off, qc, qv, cand_off, cand_ids), (ix, None, qc, qv, cand_off, cand_ids),
                 (ix, q_off, qc, qv, None, cand_ids), (ix, q_off, qc, qv, cand_off, None)):
        for name, st, _ in _calls(*args, 4, outs):
            assert st == EINVAL, name
    for missing in range(6):
        o = list(outs)
        o[missing] = None
        for off in (cand_off, zero):
            for m in (4, 33):
                for name, st, msg in _calls(ix, q_off, qc, qv, off, cand_ids, m, o):
                    assert st == EINVAL and "null" in msg, (name, missing, msg)
    # 2. what the score call checks, before m: the queries, cand_off, the ids
    bad_qc = qc.copy()
    bad_qc[0] = dim
    bad_ids = np.array([1, 50, 7], np.uint64)
    for name, st, msg in _calls(ix, q_off, bad_qc, qv, np.array([1, 2, 2, 3], np.uint64), bad_ids, 0, outs):
        assert st == EINVAL and "component >= dim" in msg, (name, msg)
    for name, st, msg in _calls(ix, q_off, qc, qv, np.array([0, 2, 1, 3], np.uint64), bad_ids, 0, outs):
        assert st == EINVAL and "cand_off" in msg, (name, msg)
    for name, st, msg in _calls(ix, q_off, qc, qv, cand_off, bad_ids, 33, outs):
        assert st == EINVAL and "query 0" in msg and "document id 50" in msg, (name, msg)
    # 3. m == 0, 4. m > 32 - before the device checks (the index is not uploaded)
    for name, st, msg in _calls(ix, q_off, qc, qv, cand_off, cand_ids, 0, outs):
        assert st == EINVAL and "m must be" in msg, (name, msg)
    for name, st, msg in _calls(ix, q_off, qc, qv, cand_off, cand_ids, 33, outs):
        assert st == ELIMIT, (name, msg)
    # 5. the device call on an index that is not uploaded: SGPU_EDEVICE; the host twin runs - also with nothing to do
    (_, st, msg), (_, hst, _) = _calls(ix, q_off, qc, qv, cand_off, cand_ids, 32, _outs(3, 32))
    assert st == EDEVICE and "not uploaded" in msg and hst == 0
    (_, st, _), (_, hst, _) = _calls(ix, q_off, qc, qv, zero, cand_ids, 4, outs)
    assert st == EDEVICE and hst == 0
    o = [_p(a) for a in outs]
    assert _native.lib().sgpu_explain_documents_host(ix.h, _p(q_off), _p(qc), _p(qv), 0, _p(zero), _p(cand_ids), 4, 0, *o) == 0


def test_query_length_limit_comes_before_m():
    dim = 9000
    off, comps, vals = random_dataset(5, 20, dim, 3, 20)
    ix = _native.NativeIndex.build(2, dim, off, comps, vals, BuildConfig.defaults(n_postings=10))
    q_off = np.array([0, 8193], np.uint64)
    qc = np.arange(8193, dtype=np.uint32)
    qv = np.ones(8193, np.float32)
    for name, st, msg in _calls(ix, q_off, qc, qv, np.array([0, 1], np.uint64), np.array([3], np.uint64), 0, _outs(1, 1)):
        assert st == ELIMIT and "8193" in msg, (name, msg)


@pytest.mark.parametrize("cls", ["SeismicIndex", "SeismicIndexLV", "SeismicIndexDotVByte"])
def test_python_explain_on_the_host(cls):
    ids, vecs, _ = read_jsonl(os.path.join(GOLD_TOY, "documents.jsonl"))
    _, qvecs, _ = read_jsonl(os.path.join(GOLD_TOY, "queries.jsonl"))
    qc = [np.array(list(v.keys())) for v in qvecs]
    qv = [np.array(list(v.values()), np.float32) for v in qvecs]
    ix = getattr(seismic_amd, cls).build(os.path.join(GOLD_TOY, "documents.jsonl"), n_postings=50, centroid_fraction=0.2,
                                          upload=False)
    lists = [list(ids)] * len(qc)
    lists[1] = []
    rows = ix.batch_explain(qc, qv, lists, m=32, device=False)
    scores = ix.batch_score(qc, qv, lists, device=False)
    assert [len(r) for r in rows] == [len(x) for x in lists]
    checked = 0
    for q in range(len(qc)):
        for (score, n_terms, terms), want, doc in zip(rows[q], scores[q].tolist(), lists[q]):
            assert score == want and len(terms) == min(n_terms, 32)
            shared = set(vecs[ids.index(doc)]) & {t for t, w in qvecs[q].items() if w != 0 and t in ix._tm}
            assert n_terms == len(shared) and {t for t, _, _, _ in terms} <= shared
            assert all(isinstance(t, str) and w == np.float32(qvecs[q][t]) for t, w, _, _ in terms)
            assert [p for _, _, _, p in terms] == sorted((p for _, _, _, p in terms), reverse=True)
            if cls != "SeismicIndexDotVByte" and n_terms:
                # binary16 values: the best term of a known pair, recomputed from the two vectors
                best = max(shared, key=lambda t: (float(np.float32(qvecs[q][t]) * np.float32(np.float16(vecs[ids.index(doc)][t]))),
                                                  -ix._tm[t]))
                assert terms[0][0] == best
                checked += 1
    assert checked > 10 or cls == "SeismicIndexDotVByte"
    # explain() is one row of batch_explain; m defaults to 10
    one = ix.explain(qc[0], qv[0], [ids[3], ids[0]], device=False)
    assert [r[:2] for r in one] == [rows[0][3][:2], rows[0][0][:2]] and all(len(r[2]) <= 10 for r in one)
    assert one[0][2] == rows[0][3][2][:10]
    with pytest.raises(KeyError):
        ix.explain(qc[0], qv[0], ["no-such-document"], device=False)


def test_raw_classes_explain_with_integer_components():
    dim = 300
    off, comps, vals = random_dataset(3, 50, dim, 3, 20)
    nat = _native.NativeIndex.build(2, dim, off, comps, vals, BuildConfig.defaults(n_postings=10))
    ix = seismic_amd.SeismicIndexRaw(nat, upload=False)
    q_off, qc, qv = random_queries(4, 3, dim, 2, 8)
    qcs = [qc[q_off[i]:q_off[i + 1]] for i in range(3)]
    qvs = [qv[q_off[i]:q_off[i + 1]] for i in range(3)]
    rows = ix.batch_explain(qcs, qvs, [[4, 4, 0], [], list(range(50))], m=5, device=False)
    assert [len(r) for r in rows] == [3, 0, 50] and rows[0][0] == rows[0][1]
    assert all(isinstance(t, int) and t in qcs[2].tolist() for _, _, terms in rows[2] for t, _, _, _ in terms)
    assert any(n for _, n, _ in rows[2])
