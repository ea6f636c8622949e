"""sgpu_expand_queries / sgpu_expand_queries_host without a device: the host twin against the numpy restatement of
tests/expand_cases.py (bit for bit, one thread and four), each wrong reading of the contract differing from it on the call
named for it, the argument checks in the header's order, every row accepted as a query, and the Python classes with
device=False.

The fixed-u8 rounding case: the issue behind this call asked for a cand_w at which fl(fl(w * val_scale) * code) differs
from fl(w * fl(code * val_scale)). val_scale is a power of two, so outside underflow (which the contract excludes) both
are the one rounding of the same real number: no such weight exists. Both products are restated and the test asserts what
holds - that they agree on every stored element for ordinary weights, and that the one weight range where they do differ
is the excluded underflow."""
import ctypes as C
import os

import numpy as np
import pytest

import expand_cases
import seismic_amd
from expand_cases import same
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
    assert "sgpu_status sgpu_expand_queries(sgpu_index* idx, uint32_t replica," in text
    assert "sgpu_status sgpu_expand_queries_host(const sgpu_index* idx," in text
    assert "sgpu_debug_expand_stats" in open(os.path.join(ROOT, "include", "seismic_hip_testing.h")).read()
    L = _native.lib()
    assert hasattr(L, "sgpu_expand_queries") and hasattr(L, "sgpu_expand_queries_host") and hasattr(L, "sgpu_debug_expand_stats")
    assert L.sgpu_abi_version() == 4


@pytest.mark.parametrize("name", sorted(expand_cases.CASES))
def test_host_twin_equals_the_restatement(name):
    case = expand_cases.make(name)
    ix = case.index
    for call in case.calls.values():
        for t in call.ts:
            for threads in (1, 4):
                got = ix.expand_queries_host(*call.args(), t, num_threads=threads)
                diff = same(got, case.expected(call.name, t))
                assert diff is None, (name, call.name, t, threads, diff)
    # the named edges, read off the host twin's rows
    oc, ov, on = ix.expand_queries_host(*case.calls["empty"].args(), 64)
    q0c, q0w = case.calls["empty"].queries[0]
    assert (q0w < 0).any() and oc[0, :on[0]].tolist() == q0c[q0w > 0].tolist()   # no candidates: the query's positive terms
    assert np.array_equal(ov[0, :on[0]], q0w[q0w > 0])
    assert on[1] > 0 and on[2] == 0 and not oc[2].any() and not ov[2].view(np.uint32).any()
    assert all(not oc[q, on[q]:].any() and not ov[q, on[q]:].view(np.uint32).any() for q in range(3))
    for call in case.calls.values():   # rows ascend by component
        oc, ov, on = ix.expand_queries_host(*call.args(), call.ts[-1])
        assert all((np.diff(oc[q, :on[q]].astype(np.int64)) > 0).all() and (ov[q, :on[q]] > 0).all() for q in range(call.nq))


# the calls on which a wrong reading must differ from the host twin
WRONG = [("reversed", "order", 16), ("float64", "order", 16), ("dedupe", "repeat", 16), ("presum", "repeat", 16),
         ("abs", "negative", 16), ("abs", "ties", 30), ("unrounded", "unrounded", 4), ("ties_high", "ties", 30),
         ("ties_high", "ties", 59), ("ties_high", "ties", 1), ("weight_order", "ties", 60), ("weight_order", "ties", 1024)]


@pytest.mark.parametrize("name", ["u16_f16_32767", "u16_dvb_32767", "u32_u8_32768", "u16_f16_300"])
def test_each_wrong_reading_fails_on_its_named_call(name):
    case = expand_cases.make(name)
    assert {r for r, _, _ in WRONG} == set(expand_cases.READINGS)
    for reading, call_name, t in WRONG:
        call = case.calls[call_name]
        got = case.index.expand_queries_host(*call.args(), t)
        wrong = expand_cases.expand_numpy(case, call, t, reading=reading)
        assert same(got, wrong) is not None, (name, reading, call_name, t)
        assert same(got, case.expected(call_name, t)) is None


@pytest.mark.parametrize("name", ["u16_u8_32767", "u16_dvb_32767", "u32_u8_32768"])
def test_the_fixed_u8_product_both_ways(name):
    case = expand_cases.make(name)
    for w in (0.075, 1.0 / 3.0, -0.3, 3.0e-5, 1.0e5):
        a, b = expand_cases.u8_products_both_ways(case, w)
        assert a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32)), w
    # where they do differ: fl(w * val_scale) underflows - the range the contract excludes
    a, b = expand_cases.u8_products_both_ways(case, 2.0 ** -149)
    assert not np.array_equal(a.view(np.uint32), b.view(np.uint32)) and np.float32(2.0 ** -149) * case.stored()[3] == 0


@pytest.mark.parametrize("name", ["u16_f16_32767", "u32_u8_32768"])
def test_every_row_is_a_valid_query(name):
    case = expand_cases.make(name)
    ix = case.index
    for call_name, t in (("random", 64), ("many", 1024), ("ties", 1024), ("empty", 8)):
        call = case.calls[call_name]
        oc, ov, on = ix.expand_queries_host(*call.args(), t)
        off = np.zeros(call.nq + 1, np.uint64)
        off[1:] = np.cumsum(on)
        qc = np.concatenate([oc[q, :on[q]] for q in range(call.nq)])
        qv = np.concatenate([ov[q, :on[q]] for q in range(call.nq)])
        sc, ids, n = ix.exact_search(off, qc, qv, 5)   # (raises where validate_queries refuses the batch)
        assert len(n) == call.nq and all(n[q] > 0 for q in range(call.nq) if on[q])


@pytest.fixture(scope="module")
def small():
    dim = 300
    off, comps, vals = random_dataset(3, 50, dim, 3, 20)
    ix = _native.NativeIndex.build(2, dim, off, comps, vals, BuildConfig.defaults(n_postings=10))
    q_off, qc, qv = random_queries(4, 3, dim, 2, 8)
    return ix, dim, q_off, qc, qv


def _calls(ix, q_off, qc, qv, cand_off, cand_ids, cand_w, alpha, t, outs):
    """(name, status, message) of the device call and of the host twin with the same arguments."""
    L = _native.lib()
    nq = len(q_off) - 1 if q_off is not None else 0
    o = [_p(a) for a in outs]
    got = []
    st = L.sgpu_expand_queries(ix.h if ix else None, 0, _p(q_off), _p(qc), _p(qv), nq, _p(cand_off), _p(cand_ids), _p(cand_w),
                               alpha, t, *o)
    got.append(("device", st, L.sgpu_last_error().decode()))
    st = L.sgpu_expand_queries_host(ix.h if ix else None, _p(q_off), _p(qc), _p(qv), nq, _p(cand_off), _p(cand_ids), _p(cand_w),
                                    alpha, t, 0, *o)
    got.append(("host", st, L.sgpu_last_error().decode()))
    return got


def test_argument_checks_in_order_without_a_device(small):
    ix, dim, q_off, qc, qv = small
    cand_off = np.array([0, 2, 2, 3], np.uint64)
    cand_ids = np.array([1, 49, 7], np.uint64)
    cand_w = np.array([0.5, 0.25, 1.0], np.float32)
    outs = [np.zeros((3, 4), np.uint32), np.zeros((3, 4), np.float32), np.zeros(3, np.uint32)]
    zero = np.zeros(4, np.uint64)
    nan, inf = float("nan"), float("inf")
    # 1. null arguments: cand_ids, cand_w and every output count, also with nothing to do and when later checks would fire
    for args in ((None, q_off, qc, qv, cand_off, cand_ids, cand_w), (ix, None, qc, qv, cand_off, cand_ids, cand_w),
                 (ix, q_off, qc, qv, None, cand_ids, cand_w), (ix, q_off, qc, qv, cand_off, None, cand_w),
                 (ix, q_off, qc, qv, cand_off, cand_ids, None)):
        for name, st, _ in _calls(*args, 1.0, 4, outs):
            assert st == EINVAL, name
    for missing in range(3):
        o = list(outs)
        o[missing] = None
        for off in (cand_off, zero):
            for t, alpha in ((4, 1.0), (1025, nan)):
                for name, st, msg in _calls(ix, q_off, qc, qv, off, cand_ids, cand_w, alpha, t, o):
                    assert st == EINVAL and "null" in msg, (name, missing, msg)
    # 2. what the score call checks, before the weights and t: the queries, cand_off, the ids
    bad_qc = qc.copy()
    bad_qc[0] = dim
    bad_ids = np.array([1, 50, 7], np.uint64)
    bad_w = np.array([0.5, inf, nan], np.float32)
    for name, st, msg in _calls(ix, q_off, bad_qc, qv, np.array([1, 2, 2, 3], np.uint64), bad_ids, bad_w, nan, 0, outs):
        assert st == EINVAL and "component >= dim" in msg, (name, msg)
    for name, st, msg in _calls(ix, q_off, qc, qv, np.array([0, 2, 1, 3], np.uint64), bad_ids, bad_w, nan, 0, outs):
        assert st == EINVAL and "cand_off" in msg, (name, msg)
    for name, st, msg in _calls(ix, q_off, qc, qv, cand_off, bad_ids, bad_w, nan, 0, outs):
        assert st == EINVAL and "query 0" in msg and "document id 50" in msg, (name, msg)
    # 3. alpha or a weight that is not finite, before t: the message names the first candidate and its query
    for alpha in (nan, inf, -inf):
        for name, st, msg in _calls(ix, q_off, qc, qv, cand_off, cand_ids, bad_w, alpha, 0, outs):
            assert st == EINVAL and "alpha" in msg, (name, msg)
    for name, st, msg in _calls(ix, q_off, qc, qv, cand_off, cand_ids, bad_w, 1.0, 0, outs):
        assert st == EINVAL and "query 0" in msg and "candidate 1" in msg and "not finite" in msg, (name, msg)
    for name, st, msg in _calls(ix, q_off, qc, qv, cand_off, cand_ids, np.array([0.5, 1.0, nan], np.float32), 1.0, 1025, outs):
        assert st == EINVAL and "query 2" in msg and "candidate 0" in msg, (name, msg)
    # 4. more than 65536 candidates of one query, before t
    many_off = np.array([0, 0, 65537, 65537], np.uint64)
    many_ids = np.zeros(65537, np.uint64)
    many_w = np.ones(65537, np.float32)
    for name, st, msg in _calls(ix, q_off, qc, qv, many_off, many_ids, many_w, 1.0, 0, outs):
        assert st == ELIMIT and "query 1" in msg and "65537" in msg, (name, msg)
    # 5. t == 0, 6. t > 1024 - before the device checks (the index is not uploaded)
    for name, st, msg in _calls(ix, q_off, qc, qv, cand_off, cand_ids, cand_w, 1.0, 0, outs):
        assert st == EINVAL and "t must be" in msg, (name, msg)
    for name, st, msg in _calls(ix, q_off, qc, qv, cand_off, cand_ids, cand_w, 1.0, 1025, outs):
        assert st == ELIMIT and "1025" in msg, (name, msg)
    # 7. the device call on an index that is not uploaded: SGPU_EDEVICE; the host twin runs - also with nothing to do
    (_, st, msg), (_, hst, _) = _calls(ix, q_off, qc, qv, cand_off, cand_ids, cand_w, 1.0, 4, outs)
    assert st == EDEVICE and "not uploaded" in msg and hst == 0 and outs[2].any()
    (_, st, _), (_, hst, _) = _calls(ix, q_off, qc, qv, zero, cand_ids, cand_w, 1.0, 4, outs)
    assert st == EDEVICE and hst == 0
    o = [_p(a) for a in outs]
    assert _native.lib().sgpu_expand_queries_host(ix.h, _p(q_off), _p(qc), _p(qv), 0, _p(zero), _p(cand_ids), _p(cand_w),
                                                  1.0, 4, 0, *o) == 0
    # 65536 candidates of one query are taken
    full = [np.zeros((3, 4), np.uint32), np.zeros((3, 4), np.float32), np.zeros(3, np.uint32)]
    (_, st, _), (_, hst, msg) = _calls(ix, q_off, qc, qv, np.array([0, 0, 65536, 65536], np.uint64), many_ids[:65536],
                                       many_w[:65536], 1.0, 4, full)
    assert st == EDEVICE and hst == 0, msg


def test_query_length_limit_comes_before_the_weights_and_t():
    dim = 9000
    off, comps, vals = random_dataset(5, 20, dim, 3, 20)
    ix = _native.NativeIndex.build(2, dim, off, comps, vals, BuildConfig.defaults(n_postings=10))
    q_off = np.array([0, 8193], np.uint64)
    qc = np.arange(8193, dtype=np.uint32)
    qv = np.ones(8193, np.float32)
    outs = [np.zeros((1, 1), np.uint32), np.zeros((1, 1), np.float32), np.zeros(1, np.uint32)]
    for name, st, msg in _calls(ix, q_off, qc, qv, np.array([0, 1], np.uint64), np.array([3], np.uint64),
                                np.array([float("nan")], np.float32), 1.0, 0, outs):
        assert st == ELIMIT and "8193" in msg, (name, msg)


@pytest.mark.parametrize("cls", ["SeismicIndex", "SeismicIndexLV", "SeismicIndexDotVByte"])
def test_python_expand_on_the_host(cls):
    ids, vecs, _ = read_jsonl(os.path.join(GOLD_TOY, "documents.jsonl"))
    _, qvecs, _ = read_jsonl(os.path.join(GOLD_TOY, "queries.jsonl"))
    qc = [np.array(list(v.keys())) for v in qvecs]
    qv = [np.array(list(v.values()), np.float32) for v in qvecs]
    ix = getattr(seismic_amd, cls).build(os.path.join(GOLD_TOY, "documents.jsonl"), n_postings=50, centroid_fraction=0.2,
                                          upload=False)
    lists = [list(ids[q % len(ids):q % len(ids) + 4]) for q in range(len(qc))]
    lists[1] = []
    rows = ix.batch_expand(qc, qv, lists, terms=1024, device=False)
    assert len(rows) == len(qc)
    for q, (tokens, values) in enumerate(rows):
        assert values.dtype == np.float32 and len(tokens) == len(values) and all(isinstance(t, str) for t in tokens)
        comps = [ix._tm[t] for t in tokens]
        assert comps == sorted(comps) and (values > 0).all()   # ascending components: a query as it stands
        # default weights beta / |R| with alpha = 1: every positive query token and every token of a feedback document
        want = {t for t, w in qvecs[q].items() if w > 0 and t in ix._tm}
        if cls != "SeismicIndexDotVByte":   # (binary16 keeps every stored weight of the toy set positive)
            for d in lists[q]:
                want |= {t for t, w in vecs[ids.index(d)].items() if np.float16(w) > 0}
            assert set(tokens) == want, q
            # a token only the query carries keeps alpha * w; one only a single document carries gets (beta / |R|) * value
            only_q = [t for t in qvecs[q] if t in ix._tm and qvecs[q][t] > 0 and not any(t in vecs[ids.index(d)] for d in lists[q])]
            for t in only_q:
                assert values[tokens.index(t)] == np.float32(qvecs[q][t])
            for t in set(tokens) - set(qvecs[q]):
                holders = [d for d in lists[q] if t in vecs[ids.index(d)]]
                if len(holders) == 1:
                    w = np.float32(0.75) / np.float32(len(lists[q]))
                    assert values[tokens.index(t)] == w * np.float32(np.float16(vecs[ids.index(holders[0])][t]))
        else:
            assert want <= set(tokens)
    # no documents: the query's own positive terms, values alpha * w
    tokens, values = rows[1]
    assert set(tokens) == {t for t, w in qvecs[1].items() if w > 0 and t in ix._tm}
    # terms cuts to the heaviest; explicit weights and alpha; expand() is one row of batch_expand
    cut = ix.batch_expand(qc, qv, lists, terms=5, device=False)
    for (tokens, values), (ft, fv) in zip(cut, rows):
        assert len(tokens) == min(5, len(ft)) and set(tokens) <= set(ft)
        assert min(values) >= sorted(fv.tolist(), reverse=True)[len(tokens) - 1] if len(tokens) else True
    w4 = [0.5, 0.25, 0.125, 0.0625]
    one = ix.expand(qc[0], qv[0], lists[0], doc_weights=w4, alpha=0.5, terms=1024, device=False)
    again = ix.batch_expand([qc[0]], [qv[0]], [lists[0]], [w4], alpha=0.5, terms=1024, device=False)[0]
    assert one[0] == again[0] and np.array_equal(one[1], again[1]) and not np.array_equal(one[1], rows[0][1])
    # the pair goes back into the query path as it is
    assert len(ix.batch_score([np.array(one[0])], [one[1]], [lists[0]], device=False)[0]) == 4
    with pytest.raises(KeyError):
        ix.expand(qc[0], qv[0], ["no-such-document"], device=False)
    with pytest.raises(ValueError):
        ix.batch_expand(qc[:1], qv[:1], lists[:1], [[1.0]], device=False)


def test_raw_classes_expand_with_integer_components():
    dim = 300
    off, comps, vals = random_dataset(3, 50, dim, 3, 20)
    nat = _native.NativeIndex.build(2, dim, off, comps, vals, BuildConfig.defaults(n_postings=10))
    ix = seismic_amd.SeismicIndexRaw(nat, upload=False)
    q_off, qc, qv = random_queries(4, 3, dim, 2, 8)
    qcs = [qc[q_off[i]:q_off[i + 1]] for i in range(3)]
    qvs = [qv[q_off[i]:q_off[i + 1]] for i in range(3)]
    rows = ix.batch_expand(qcs, qvs, [[4, 4, 0], [], list(range(10))], terms=16, device=False)
    assert 0 < len(rows[0][0]) <= 16 and len(rows[2][0]) == 16
    assert all(isinstance(t, int) for tokens, _ in rows for t in tokens)
    assert rows[1][0] == qcs[1].tolist() and np.array_equal(rows[1][1], qvs[1])
    assert not hasattr(ix, "batch_search_feedback") and hasattr(seismic_amd.SeismicIndex, "batch_search_feedback")
