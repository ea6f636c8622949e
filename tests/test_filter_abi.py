"""Document filters without a GPU: the entry points are exported and declared, their argument checks (and their order),
filter construction, a NULL filter is the unfiltered call, and filtered exact search on the host equals two
independent references bit for bit - the unfiltered host exact search restricted to A, and the oracle's brute force."""
import ctypes
import os
import re

import numpy as np
import pytest

import orc
import seismic_amd
from seismic_amd import _native
from seismic_amd._abi import BuildConfig
from util import random_dataset, random_queries

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
SGPU_OK, SGPU_EINVAL, SGPU_EDEVICE, SGPU_ELIMIT = 0, 1, 2, 5
NEW = ("sgpu_filter_create", "sgpu_filter_count", "sgpu_filter_device_bytes", "sgpu_filter_destroy",
       "sgpu_search_filtered", "sgpu_batch_search_filtered", "sgpu_exact_search_filtered",
       "sgpu_exact_search_device_filtered")
p = _native._p


def _index(seed=11, n_docs=300, dim=200, value_type=0, **kw):
    off, comps, vals = random_dataset(seed, n_docs, dim, **kw)
    ix = _native.NativeIndex.build(2, dim, off, comps, vals, BuildConfig.defaults(n_postings=10))
    return ix.convert(value_type) if value_type else ix


def _err():
    return _native.lib().sgpu_last_error().decode()


def _create(ix, ids):
    a = np.ascontiguousarray(ids, np.uint32)
    h = ctypes.c_void_p()
    st = _native.lib().sgpu_filter_create(ix.h if ix is not None else None, p(a), len(a), ctypes.byref(h))
    return st, h


def _out(nq, k):
    return (np.zeros((max(nq, 1), max(k, 1)), np.float32), np.zeros((max(nq, 1), max(k, 1)), np.uint64),
            np.zeros(max(nq, 1), np.uint32))


def _batch(ix, q, k, filt):
    q_off, comps, vals = (np.ascontiguousarray(q[0], np.uint64), np.ascontiguousarray(q[1], np.uint32),
                          np.ascontiguousarray(q[2], np.float32))
    nq = len(q_off) - 1
    sc, ids, n = _out(nq, k)
    prm = _native.params(k, 4, 1.0, False)
    st = _native.lib().sgpu_batch_search_filtered(ix.h, p(q_off), p(comps), p(vals), nq, ctypes.byref(prm), p(sc),
                                                   p(ids), p(n), filt)
    return st, _err()


def _single(ix, q, k, filt):
    comps, vals = np.ascontiguousarray(q[1], np.uint32), np.ascontiguousarray(q[2], np.float32)
    sc, ids, n = _out(1, k)
    prm = _native.params(k, 4, 1.0, False)
    nn = ctypes.c_uint32(0)
    st = _native.lib().sgpu_search_filtered(ix.h, p(comps), p(vals), len(comps), ctypes.byref(prm), p(sc), p(ids),
                                             ctypes.byref(nn), filt)
    return st, _err()


def _exact_dev(ix, q, k, filt):
    q_off, comps, vals = (np.ascontiguousarray(q[0], np.uint64), np.ascontiguousarray(q[1], np.uint32),
                          np.ascontiguousarray(q[2], np.float32))
    nq = len(q_off) - 1
    sc, ids, n = _out(nq, k)
    st = _native.lib().sgpu_exact_search_device_filtered(ix.h, 0, p(q_off), p(comps), p(vals), nq, k, p(sc), p(ids),
                                                          p(n), filt)
    return st, _err()


def _exact_host(ix, q, k, filt):
    q_off, comps, vals = (np.ascontiguousarray(q[0], np.uint64), np.ascontiguousarray(q[1], np.uint32),
                          np.ascontiguousarray(q[2], np.float32))
    nq = len(q_off) - 1
    sc, ids, n = _out(nq, k)
    st = _native.lib().sgpu_exact_search_filtered(ix.h, p(q_off), p(comps), p(vals), nq, k, 2, p(sc), p(ids), p(n),
                                                   filt)
    return st, _err(), (sc, ids, n)


def test_entry_points_exported_and_declared():
    hdr = open(os.path.join(ROOT, "include", "seismic_hip.h")).read()
    so = ctypes.CDLL(_native.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(so, name), name
    assert "destroy every filter before its index" in hdr.lower()
    assert _native.lib().sgpu_abi_version() == 4
    assert "SeismicFilter" in seismic_amd.__all__ and seismic_amd.SeismicFilter is seismic_amd.index.SeismicFilter


def test_create_checks_count_and_no_device():
    ix = _index()
    L = _native.lib()
    st, h = _create(None, [1, 2])
    assert st == SGPU_EINVAL
    st, h = _create(ix, [3, 299, 300, 7, 1000])
    assert st == SGPU_EINVAL and "300" in _err() and "1000" not in _err()   # the first bad id is named
    st, h = _create(ix, [])                                                  # the empty set
    assert st == SGPU_OK and L.sgpu_filter_count(h) == 0 and L.sgpu_filter_device_bytes(h) == 0
    L.sgpu_filter_destroy(h)
    st, h = _create(ix, [5, 5, 9, 5, 0, 299])                                # repeats count once
    assert st == SGPU_OK and L.sgpu_filter_count(h) == 4 and L.sgpu_filter_device_bytes(h) == 0
    L.sgpu_filter_destroy(h)
    L.sgpu_filter_destroy(None)
    assert L.sgpu_filter_count(None) == 0
    f = ix.make_filter(np.arange(300) % 3 == 0)                              # a boolean mask
    assert f.count == 100 and f.device_bytes() == 0
    with pytest.raises(ValueError):
        ix.make_filter(np.ones(299, bool))
    with pytest.raises(ValueError):
        ix.make_filter([-1])
    with pytest.raises(_native.SeismicHipError):
        ix.make_filter([300])


def test_argument_order_of_every_filtered_entry_point():
    ix, other = _index(), _index(seed=12)
    q = ([0, 2], [1, 5], [1.0, 2.0])
    fo = other.make_filter([1, 2, 3])
    f = ix.make_filter([1, 2, 3])
    # a filter of another index: EINVAL before anything else, even before a bad k
    for call in (_batch, _single, _exact_dev):
        for k in (0, 10):
            st, msg = call(ix, q, k, fo.h)
            assert st == SGPU_EINVAL and "another index" in msg, call
    st, msg, _ = _exact_host(ix, q, 0, fo.h)
    assert st == SGPU_EINVAL and "another index" in msg
    # the filter's own index: the unfiltered call's checks in their order
    for call in (_batch, _single):
        st, msg = call(ix, q, 0, f.h)
        assert st == SGPU_EINVAL and "k" in msg
        st, msg = call(ix, q, 10, f.h)
        assert st == SGPU_EDEVICE and "upload" in msg
    st, msg = _exact_dev(ix, q, 0, f.h)
    assert st == SGPU_EINVAL and "k" in msg
    st, msg = _exact_dev(ix, q, 1025, f.h)
    assert st == SGPU_ELIMIT and "1024" in msg
    st, msg = _exact_dev(ix, ([0, 2], [5, 1], [1.0, 2.0]), 10, f.h)          # components not ascending
    assert st == SGPU_EINVAL and msg
    st, msg = _exact_dev(ix, ([0, 1], [200], [1.0]), 10, f.h)                # component out of range
    assert st == SGPU_EINVAL and msg
    st, msg = _exact_dev(ix, q, 10, f.h)                                     # valid, but the index is on no device
    assert st == SGPU_EDEVICE and "upload" in msg
    st, msg, _ = _exact_host(ix, q, 0, f.h)
    assert st == SGPU_EINVAL
    st, msg, _ = _exact_host(ix, ([0, 1], [200], [1.0]), 10, f.h)
    assert st == SGPU_EINVAL


def test_null_filter_is_the_unfiltered_call():
    ix = _index()
    q = ([0, 2], [1, 5], [1.0, 2.0])
    L = _native.lib()
    for k, want in ((0, SGPU_EINVAL), (10, SGPU_EDEVICE)):
        assert _batch(ix, q, k, None)[0] == want and _single(ix, q, k, None)[0] == want
    for k, want in ((0, SGPU_EINVAL), (1025, SGPU_ELIMIT), (10, SGPU_EDEVICE)):
        assert _exact_dev(ix, q, k, None)[0] == want
    qq = random_queries(3, 7, 200)
    st, _, got = _exact_host(ix, qq, 12, None)
    want = ix.exact_search(*qq, 12)
    assert st == SGPU_OK
    assert np.array_equal(got[2][:7], want[2]) and np.array_equal(got[1][:7], want[1])
    assert np.array_equal(got[0][:7].view(np.uint32), want[0].view(np.uint32))
    assert L.sgpu_exact_search_filtered(None, None, None, None, 0, 1, 0, None, None, None, None) == SGPU_EINVAL


def _restricted(sc, ids, n, allowed, k):
    keep = [(s, i) for s, i in zip(sc[:n], ids[:n]) if allowed[int(i)]][:k]
    return (np.array([s for s, _ in keep], np.float32), np.array([i for _, i in keep], np.uint64))


@pytest.mark.parametrize("value_type", [0, 1])
def test_host_filtered_exact_equals_two_references(value_type):
    n_docs, dim = 300, 200
    ix = _index(n_docs=n_docs, dim=dim, value_type=value_type, empty_every=17)
    q_off, qc, qv = random_queries(4, 12, dim)
    qv = qv.copy()
    qv[::5] *= -1.0                              # negative weights: documents sharing nothing (0.0) win some slots
    q = (q_off, qc, qv)
    rng = np.random.default_rng(9)
    sets = {"half": rng.random(n_docs) < 0.5, "one": np.arange(n_docs) == 123, "none": np.zeros(n_docs, bool),
            "all": np.ones(n_docs, bool), "tail": np.arange(n_docs) >= 290}
    full = ix.exact_search(*q, n_docs)           # reference 1: every document ranked
    for name, allowed in sets.items():
        f = ix.make_filter(allowed)
        for k in (1, 10, 50):
            sc, ids, n = ix.exact_search(*q, k, filter=f)
            assert (n == min(k, int(allowed.sum()))).all(), name
            for j in range(len(q_off) - 1):
                a, b = int(q_off[j]), int(q_off[j + 1])
                r1 = _restricted(full[0][j], full[1][j], int(full[2][j]), allowed, k)
                os_, oi = orc.exact_search(ix.desc, qc[a:b], qv[a:b], n_docs, orc.ORDER_SEQ)   # reference 2: the oracle
                r2 = _restricted(os_, oi, len(oi), allowed, k)
                got = (sc[j, :n[j]], ids[j, :n[j]])
                for ref in (r1, r2):
                    assert np.array_equal(got[1], ref[1]), (name, k, j)
                    assert np.array_equal(got[0].view(np.uint32), ref[0].view(np.uint32)), (name, k, j)
        if name == "all":
            u = ix.exact_search(*q, 10)
            g = ix.exact_search(*q, 10, filter=f)
            assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(u, g))


def test_python_surface_on_the_toy_dataset():
    ix = seismic_amd.SeismicIndex.build(os.path.join(GOLD, "toy", "documents.jsonl"), upload=False)
    qids, vecs, _ = seismic_amd.index.read_jsonl(os.path.join(GOLD, "toy", "queries.jsonl"))
    comps = [np.array(list(v.keys()), dtype="U30") for v in vecs]
    vals = [np.array(list(v.values()), np.float32) for v in vecs]
    names = ix._doc_ids
    n = len(names)
    allowed = names[1::3]
    f = ix.make_filter(allowed)
    assert isinstance(f, seismic_amd.SeismicFilter) and f.count == len(set(allowed))
    full = ix.batch_exact_search(qids, comps, vals, n)
    for k in (1, 5):
        got = ix.batch_exact_search(qids, comps, vals, k, filter=f)
        want = [[r for r in row if r[2] in set(allowed)][:k] for row in full]
        assert got == want
        assert ix.batch_exact_search(qids, comps, vals, k, filter=allowed) == want   # an iterable, for this call
    assert ix.batch_exact_search(qids, comps, vals, 3, filter=[]) == [[] for _ in qids]
    with pytest.raises(KeyError):
        ix.make_filter([names[0], "no such document"])
    with pytest.raises(KeyError):
        ix.batch_exact_search(qids, comps, vals, 3, filter=["no such document"])
    other = seismic_amd.SeismicIndex.build(os.path.join(GOLD, "toy", "documents.jsonl"), upload=False)
    with pytest.raises(ValueError):
        ix.batch_exact_search(qids, comps, vals, 3, filter=other.make_filter(allowed))
    with pytest.raises(TypeError):
        ix.make_filter(names[0])
    # a filter keeps its index alive
    g = seismic_amd.SeismicIndex.build(os.path.join(GOLD, "toy", "documents.jsonl"), upload=False).make_filter(allowed)
    assert g.count == f.count and g.index.len == n


def test_the_posting_view_hook_is_a_test_hook(monkeypatch):
    """sgpu_debug_posting_view: declared in the testing header only, SGPU_EINVAL without SGPU_TEST_HOOKS=1 (and nothing
    written), SGPU_EDEVICE with it while the index is on no device, SGPU_EINVAL for a filter of another index."""
    name = "sgpu_debug_posting_view"
    assert re.search(r"\b%s\s*\(" % name, open(os.path.join(ROOT, "include", "seismic_hip_testing.h")).read())
    assert name not in open(os.path.join(ROOT, "include", "seismic_hip.h")).read()
    ix, other = _index(), _index(seed=12)
    f, fo = ix.make_filter([1, 2, 3]), other.make_filter([1, 2, 3])
    L = _native.lib()
    vp = ctypes.c_void_p
    L.sgpu_debug_posting_view.argtypes = [vp, vp, ctypes.c_uint32, vp, ctypes.c_uint64, vp, vp, ctypes.c_uint64, vp,
                                          ctypes.c_uint64, vp, ctypes.c_uint64, vp]

    def call(filt):
        sizes = np.full(5, 77, np.uint64)
        return L.sgpu_debug_posting_view(ix.h, filt, 0, None, 0, None, None, 0, None, 0, None, 0, p(sizes)), sizes

    for off in (None, "0", ""):
        if off is None:
            monkeypatch.delenv("SGPU_TEST_HOOKS")
        else:
            monkeypatch.setenv("SGPU_TEST_HOOKS", off)
        for filt in (None, f.h, fo.h):
            st, sizes = call(filt)
            assert st == SGPU_EINVAL and "test hook" in _err() and (sizes == 77).all()
        # (sgpu_debug_launch_config, the other hook that needs no device, obeys the same switch)
        words, cfg = np.array(list(_native.LAUNCH_CONFIG_IN.values()), np.uint32), np.full(len(_native.LAUNCH_CONFIG_OUT), 77, np.uint32)
        L.sgpu_debug_launch_config.argtypes = [vp, ctypes.c_uint32, ctypes.c_float, vp, ctypes.c_uint32]
        assert L.sgpu_debug_launch_config(p(words), len(words), 1.0, p(cfg), len(cfg)) == SGPU_EINVAL
        assert "sgpu_debug_launch_config is a test hook" in _err() and (cfg == 77).all()
    monkeypatch.setenv("SGPU_TEST_HOOKS", "1")
    assert L.sgpu_debug_launch_config(p(words), len(words), 1.0, p(cfg), len(cfg)) == 0 and cfg[35] in (512, 1024)
    header = open(os.path.join(ROOT, "include", "seismic_hip_testing.h")).read()
    assert re.search(r"\bsgpu_debug_launch_config\s*\(", header)
    assert "sgpu_debug_launch_config" not in open(os.path.join(ROOT, "include", "seismic_hip.h")).read()
    for filt in (None, f.h):
        st, _ = call(filt)
        assert st == SGPU_EDEVICE and "upload" in _err()
    st, _ = call(fo.h)
    assert st == SGPU_EINVAL and "another index" in _err()
    with pytest.raises(_native.SeismicHipError) as e:
        ix.debug_posting_view()
    assert e.value.status == SGPU_EDEVICE
    with pytest.raises(_native.SeismicHipError):
        f.debug_view()
    assert f.device_bytes() == 0 and _native.lib().sgpu_abi_version() == 4
