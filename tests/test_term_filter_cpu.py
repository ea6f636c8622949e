"""Term filters without a GPU: the entry points are exported and declared, the host twin's bits equal the numpy restatement
of the header text (term_filter_cases.expected_bits) word for word on every case, each wrong reading of the text differs
from it on a named case, the argument checks come in the stated order, a term filter drives filtered exact search as the id
filter of the same set does, sgpu_filter_get_bits, and the Python layer."""
import ctypes
import os
import re

import numpy as np
import pytest

import filter_cases
import seismic_amd
import term_filter_cases as tc
from seismic_amd import _native
from seismic_amd._abi import SGPU_TERM_MUST, SGPU_TERM_MUST_NOT, SGPU_TERM_SHOULD, TermClause
from util import random_queries

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
SGPU_OK, SGPU_EINVAL, SGPU_EDEVICE, SGPU_ELIMIT = 0, 1, 2, 5
NEW = ("sgpu_filter_create_terms", "sgpu_filter_create_terms_host", "sgpu_filter_get_bits")
p = _native._p
NINF = float("-inf")


def _err():
    return _native.lib().sgpu_last_error().decode()


def test_entry_points_exported_and_declared():
    hdr = open(os.path.join(ROOT, "include", "seismic_hip.h")).read()
    so = ctypes.CDLL(_native.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(so, name), name
    assert re.search(r"SGPU_TERM_MUST = 0, SGPU_TERM_MUST_NOT = 1, SGPU_TERM_SHOULD = 2", hdr)
    assert (SGPU_TERM_MUST, SGPU_TERM_MUST_NOT, SGPU_TERM_SHOULD) == (tc.MUST, tc.MUST_NOT, tc.SHOULD) == (0, 1, 2)
    assert ctypes.sizeof(TermClause) == 16 == _native.TERM_CLAUSE_DTYPE.itemsize
    assert _native.lib().sgpu_abi_version() == 4
    assert "take turns" in hdr and "sgpu_debug_term_filter_stats" not in hdr
    assert "sgpu_debug_term_filter_stats" in open(os.path.join(ROOT, "include", "seismic_hip_testing.h")).read()


@pytest.mark.parametrize("variant", tc.VARIANTS)
@pytest.mark.parametrize("n_docs", tc.N_DOCS)
def test_host_twin_equals_the_restated_contract(n_docs, variant):
    t = tc.make(n_docs, variant)
    assert t.fwd["n_docs"] == n_docs and t.fwd["f16"] == variant.endswith("f16")
    if n_docs > 1:
        assert (np.diff(t.fwd["off"]) == 0).any()                       # empty documents
    sets = tc.clause_sets(t)
    counts = {}
    for name, (clauses, ms) in sets.items():
        for threads in ((1, 3) if name in ("mixed", "c1024") else (2,)):
            f = t.ix.make_term_filter(clauses, ms, host=True, num_threads=threads)
            want = tc.expected_bits(t.fwd, clauses, ms)
            assert tc.bits_diff(f.bits(), want) is None, (name, tc.bits_diff(f.bits(), want))
            assert f.count == tc.popcount(want), name
            counts[name] = f.count
    w = tc.within_sets(n_docs)
    for wname, allowed in w.items():
        wf = t.ix.make_filter(allowed)
        for name in tc.WITHIN_CLAUSES:
            clauses, ms = sets[name]
            f = t.ix.make_term_filter(clauses, ms, within=wf, host=True)
            want = tc.expected_bits(t.fwd, clauses, ms, allowed)
            assert tc.bits_diff(f.bits(), want) is None, (name, wname)
            assert f.count == tc.popcount(want)
    # what the cases are meant to hold
    assert counts["none"] == n_docs and counts["should3_min4"] == 0 and counts["c1024_all_should"] == 0
    assert counts["must_not"] == n_docs - counts["must_frequent"]
    for L in tc.LS:
        held = int((t.fwd["comps"] == tc.L_COMP[L]).sum())
        assert counts["L%d" % L] == held and counts["notL%d" % L] == n_docs - held
        if n_docs >= 32767:
            assert held == L
    if n_docs == 65541:
        assert 0 < counts["c1024"] < n_docs and counts["at_value"] > counts["above_value"] > 0
        if variant.endswith("f16"):
            assert counts["plus_zero"] == counts["minus_zero"] > counts["subnormal"] > 0 and counts["huge"] > 0
            raw = t.fwd["raw"]
            assert (raw == 0x8000).any() and (raw == 0x0001).any() and (raw == 0x7bff).any() and (raw > 0x8000).any()
        last = tc.expected_bits(t.fwd, *sets["last_range"])
        assert not last[:2 * tc.RANGE // 32].any() and last[2 * tc.RANGE // 32:].any()
    if variant.startswith("u32"):
        assert t.dim - 1 > 65535 and counts["last_component"] == int((t.fwd["comps"] == t.dim - 1).sum())


def test_dotvbyte_answers_as_its_fixed_u8_twin():
    for n_docs in (33, 32769):
        a, b = tc.make(n_docs, "u16_u8"), tc.make(n_docs, "u16_dvb")
        assert int(a.ix.desc.value_type) == 1 and int(b.ix.desc.value_type) == 2
        for name, (clauses, ms) in tc.clause_sets(a).items():
            fa, fb = a.ix.make_term_filter(clauses, ms, host=True), b.ix.make_term_filter(clauses, ms, host=True)
            assert np.array_equal(fa.bits(), fb.bits()), name


@pytest.mark.parametrize("wrong", tc.WRONG)
def test_each_wrong_reading_differs_on_its_case(wrong):
    n_docs, variant, name, wname = tc.WRONG_CASES[wrong]
    t = tc.make(n_docs, variant)
    clauses, ms = tc.clause_sets(t)[name]
    allowed = None if wname is None else tc.within_sets(n_docs)[wname]
    wf = None if wname is None else t.ix.make_filter(allowed)
    got = t.ix.make_term_filter(clauses, ms, within=wf, host=True).bits()
    assert tc.bits_diff(got, tc.expected_bits(t.fwd, clauses, ms, allowed)) is None
    assert tc.bits_diff(got, tc.expected_bits(t.fwd, clauses, ms, allowed, wrong=wrong)) is not None


def _raw(ix, clauses, n=None, ms=0, within=None, host=True, out=True, replica=0):
    cl = _native.term_clauses(clauses) if clauses is not None else None
    n = len(cl) if n is None else n
    h = ctypes.c_void_p(123)
    L = _native.lib()
    ixh = ix.h if ix is not None else None
    ref = ctypes.byref(h) if out else None
    if host:
        st = L.sgpu_filter_create_terms_host(ixh, p(cl), n, ms, within, 1, ref)
    else:
        st = L.sgpu_filter_create_terms(ixh, replica, p(cl), n, ms, within, ref)
    return st, _err(), h


@pytest.mark.parametrize("host", [True, False])
def test_checks_in_the_stated_order(host):
    t, other = tc.make(33, "u16_f16"), tc.make(32, "u16_f16")
    ix, dim = t.ix, t.dim
    foreign = other.ix.make_filter([1])
    good = [(0, 0, NINF)]
    nan = float("nan")
    many = np.zeros(1025, _native.TERM_CLAUSE_DTYPE)
    many["min_weight"] = NINF
    # 1: null arguments, before anything else (a bad clause and a foreign filter are there too)
    assert _raw(None, [(dim, 7, nan)], within=foreign.h, host=host)[0] == SGPU_EINVAL and "null" in _err()
    assert _raw(ix, [(dim, 7, nan)], within=foreign.h, host=host, out=False)[0] == SGPU_EINVAL and "null" in _err()
    st, msg, _ = _raw(ix, None, n=3, within=foreign.h, host=host)
    assert st == SGPU_EINVAL and "null" in msg
    # 2: the first offending clause is named; before the limit (1025 clauses) and the foreign filter
    bad = many.copy()
    bad[7]["occur"], bad[9]["component"], bad[11]["min_weight"] = 3, dim, nan
    st, msg, h = _raw(ix, bad, within=foreign.h, host=host)
    assert st == SGPU_EINVAL and "clause 7" in msg and "occur" in msg and h.value is None
    bad[7]["occur"] = 2
    st, msg, _ = _raw(ix, bad, within=foreign.h, host=host)
    assert st == SGPU_EINVAL and "clause 9" in msg and str(dim) in msg
    bad[9]["component"] = dim - 1
    st, msg, _ = _raw(ix, bad, within=foreign.h, host=host)
    assert st == SGPU_EINVAL and "clause 11" in msg and "NaN" in msg
    # 3: the limit, before the foreign filter
    st, msg, _ = _raw(ix, many, within=foreign.h, host=host)
    assert st == SGPU_ELIMIT and "1024" in msg
    # 4: the foreign filter, before the device
    st, msg, _ = _raw(ix, good, within=foreign.h, host=host)
    assert st == SGPU_EINVAL and "another index" in msg
    # 5: the device call on an index that is on no device; the host twin needs none
    st, msg, h = _raw(ix, good, host=host)
    if host:
        assert st == SGPU_OK and _native.lib().sgpu_filter_count(h) > 0
        _native.lib().sgpu_filter_destroy(h)
        st, msg, h = _raw(ix, many[:1024], host=True)                  # exactly the limit; no clause with n_clauses == 0
        assert st == SGPU_OK
        _native.lib().sgpu_filter_destroy(h)
        st, msg, h = _raw(ix, None, n=0, host=True)
        assert st == SGPU_OK and _native.lib().sgpu_filter_count(h) == 33
        _native.lib().sgpu_filter_destroy(h)
    else:
        assert st == SGPU_EDEVICE and "upload" in msg and h.value is None
        assert _raw(ix, good, host=False, replica=5)[0] == SGPU_EDEVICE
    # min_should above the SHOULD clauses: the empty set, not an error
    f = ix.make_term_filter([(0, 2, NINF)], 2, host=True)
    assert f.count == 0 and not f.bits().any()


def test_get_bits_and_the_id_filter():
    t = tc.make(33, "u16_f16")
    L = _native.lib()
    for name, allowed in tc.within_sets(33).items():
        f = t.ix.make_filter(allowed)
        assert np.array_equal(f.bits(), filter_cases.bitmap(allowed)) and f.bits().dtype == np.uint32, name
        assert np.array_equal(f.ids(), np.flatnonzero(allowed)) and f.count == int(allowed.sum())
    f = t.ix.make_filter([0, 32])
    n = ctypes.c_uint64(0)
    out = np.full(4, 77, np.uint32)
    assert L.sgpu_filter_get_bits(f.h, p(out), 1, ctypes.byref(n)) == SGPU_EINVAL and n.value == 2 and (out == 77).all()
    assert L.sgpu_filter_get_bits(f.h, None, 0, ctypes.byref(n)) == SGPU_EINVAL and n.value == 2
    assert L.sgpu_filter_get_bits(None, p(out), 4, ctypes.byref(n)) == SGPU_EINVAL
    assert L.sgpu_filter_get_bits(f.h, p(out), 4, None) == SGPU_OK and out.tolist() == [1, 1, 77, 77]
    one = tc.make(1, "u16_f16").ix.make_filter([])
    assert one.bits().tolist() == [0]


@pytest.mark.parametrize("variant", ["u16_f16", "u32_u8"])
def test_exact_search_with_a_term_filter_equals_the_id_filter(variant):
    t = tc.make(32769, variant)
    sets = tc.clause_sets(t)
    q = random_queries(5, 6, 12)
    for name in ("mixed", "L65", "must_not", "last_range"):
        clauses, ms = sets[name]
        tf = t.ix.make_term_filter(clauses, ms, host=True)
        idf = t.ix.make_filter(tf.ids())
        assert idf.count == tf.count
        a, b = t.ix.exact_search(*q, 20, filter=tf), t.ix.exact_search(*q, 20, filter=idf)
        assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b)), name


def test_python_layer_tokens_unknown_tokens_and_pairs():
    ix = seismic_amd.SeismicIndex.build(os.path.join(GOLD, "toy", "documents.jsonl"), upload=False)
    _, vecs, _ = seismic_amd.index.read_jsonl(os.path.join(GOLD, "toy", "documents.jsonl"))
    names, n = ix._doc_ids, ix.len
    fwd = tc.forward(ix._ix.desc)
    stored = [dict() for _ in range(n)]                                   # row -> {component: stored value}
    vals = tc.decoded(fwd, fwd["raw"])
    for d, c, v in zip(fwd["doc"].tolist(), fwd["comps"].tolist(), vals.tolist()):
        stored[d][c] = v
    tm = ix._tm
    by_freq = sorted(tm, key=lambda tok: -sum(tm[tok] in s for s in stored))
    a, b, c = by_freq[0], by_freq[1], by_freq[2]

    def rows(pred):
        return [d for d in range(n) if pred(stored[d])]

    f = ix.make_term_filter(must=[a])
    assert isinstance(f, seismic_amd.SeismicFilter) and f._f.ids().tolist() == rows(lambda s: tm[a] in s) and f.count > 0
    f = ix.make_term_filter(must=[a], must_not=[b])
    assert f._f.ids().tolist() == rows(lambda s: tm[a] in s and tm[b] not in s)
    f = ix.make_term_filter(should=[a, b, c], min_should=2)
    assert f._f.ids().tolist() == rows(lambda s: sum(tm[x] in s for x in (a, b, c)) >= 2)
    w = sorted(s[tm[a]] for s in stored if tm[a] in s)[len(rows(lambda s: tm[a] in s)) // 2]   # a stored weight of a
    f = ix.make_term_filter(must=[(a, w)], should=[b])
    assert f._f.ids().tolist() == rows(lambda s: s.get(tm[a], -np.inf) >= w) and 0 < f.count
    g = ix.make_term_filter(must=[a], min_weight=w)                         # the default threshold of bare tokens
    assert np.array_equal(g.bits(), f.bits())
    # tokens outside the vocabulary
    assert "no such token" not in tm
    assert ix.make_term_filter(must=[a, "no such token"]).count == 0
    assert ix.make_term_filter(must=[a], must_not=["no such token"]).count == ix.make_term_filter(must=[a]).count
    f = ix.make_term_filter(should=[a, "no such token"], min_should=1)
    assert f._f.ids().tolist() == rows(lambda s: tm[a] in s)
    assert ix.make_term_filter(should=[a, "no such token"], min_should=2).count == 0
    assert ix.make_term_filter().count == n
    # within, and a term filter in a filtered call
    half = ix.make_filter(names[::2])
    f = ix.make_term_filter(must=[a], within=half)
    assert f._f.ids().tolist() == [d for d in rows(lambda s: tm[a] in s) if d % 2 == 0]
    other = seismic_amd.SeismicIndex.build(os.path.join(GOLD, "toy", "documents.jsonl"), upload=False)
    with pytest.raises(ValueError):
        ix.make_term_filter(must=[a], within=other.make_filter(names[::2]))
    with pytest.raises(TypeError):
        ix.make_term_filter(must=a)
    qids, qv, _ = seismic_amd.index.read_jsonl(os.path.join(GOLD, "toy", "queries.jsonl"))
    comps = [np.array(list(v.keys()), dtype="U30") for v in qv]
    qvals = [np.array(list(v.values()), np.float32) for v in qv]
    tf = ix.make_term_filter(must=[a])
    same = ix.make_filter([names[d] for d in tf._f.ids().tolist()])
    assert ix.batch_exact_search(qids, comps, qvals, 5, filter=tf) == ix.batch_exact_search(qids, comps, qvals, 5, filter=same)
    assert vecs and not ix._uploaded                                       # all of it on the host: nothing was uploaded
