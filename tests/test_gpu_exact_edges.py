"""Device exact search (exact_device.hip) at the structural edges of its kernels, on the cases of tests/exact_cases.py:
segments longer than one step of 8 x 1024 entries, queries of more than 256 components, the offset scan at its tile
edges, documents at the count and scatter kernels' lane strides, one tie group spanning ranges, filtered ranges with 0,
1, k - 1, k, k + 1 allowed documents, and more than one chunk of queries per call (test hook SGPU_EXACT_CAND_BYTES, launches
counted by sgpu_debug_exact_launches; the shipped 256 MiB once). Every device row is the host's bit for bit - n, ids in
order, score bits, zeros past n - and the oracle's sequential brute force for k <= 100; test_exact_cases_cpu.py checks the
host side, the cases' properties and that the inputs see each class of bug. Lines starting "model64:" report the float64
model's verdicts (run with -s). Run with `-m gpu`."""
import ctypes as C
import functools

import numpy as np
import pytest

import exact_cases as EC
import model64 as M64
import orc
from seismic_amd import _native
from seismic_amd._abi import BuildConfig

pytestmark = pytest.mark.gpu

KS = (1, 10, 1024)


def _launches(ix, replica=0):
    """sgpu_debug_exact_launches: the accumulate launches of the last exact call on the replica."""
    L = _native.lib()
    L.sgpu_debug_exact_launches.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
    n = C.c_uint32(0xffffffff)
    _native.check(L.sgpu_debug_exact_launches(ix.h, replica, C.byref(n)))
    return int(n.value)


@functools.lru_cache(maxsize=None)
def _built(name, vt):
    """(case, uploaded index) of a variant, shared by the tests of this file."""
    case = EC.make(name)
    return case, case.build(vt).upload(0)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _assert_rows(dev, host, want_n, what):
    """Device rows = host rows bit for bit: n, ids in order, score bits; device slots past n are zero."""
    (ds, di, dn), (hs, hi, hn) = dev, host
    assert (dn == want_n).all() and np.array_equal(dn, hn), (what, dn[:8], hn[:8], want_n)
    bad = np.flatnonzero((di[:, :want_n] != hi[:, :want_n]).any(axis=1) | (_bits(ds)[:, :want_n] != _bits(hs)[:, :want_n]).any(axis=1))
    if len(bad):
        q = int(bad[0])
        at = int(np.flatnonzero((di[q, :want_n] != hi[q, :want_n]) | (_bits(ds)[q, :want_n] != _bits(hs)[q, :want_n]))[0])
        raise AssertionError("%s: query %d differs first at rank %d: device (%r, %d), host (%r, %d); %d of %d rows differ" % (
            what, q, at, ds[q, at], di[q, at], hs[q, at], hi[q, at], len(bad), len(dn)))
    assert not di[:, want_n:].any() and not _bits(ds)[:, want_n:].any(), "%s: slots past n were written" % what


@pytest.mark.parametrize("variant", EC.VARIANTS, ids=EC.VARIANT_IDS)
def test_device_rows_are_the_hosts_and_the_oracles(variant):
    case, ix = _built(*variant)
    Q = (case.q_off, case.qc, case.qv)
    for k in KS:
        dev = ix.exact_search_device(*Q, k)
        assert _launches(ix) == 1
        _assert_rows(dev, ix.exact_search(*Q, k), min(k, case.n_docs), "%s-vt%d k=%d" % (variant + (k,)))
        if k <= 100:
            for i, (c, v) in enumerate(case.queries):
                es, ei = orc.exact_search(ix.desc, c, v, k, orc.ORDER_SEQ)
                assert np.array_equal(dev[1][i, :len(ei)], ei) and np.array_equal(_bits(dev[0][i, :len(es)]), _bits(es)), (k, i)


@pytest.mark.parametrize("variant", EC.VARIANTS, ids=EC.VARIANT_IDS)
def test_device_rows_pass_the_models_checkers(variant):
    case, ix = _built(*variant)
    d = ix.desc
    model = M64.Model(orc.desc_arrays(d), d.val_scale, d.value_type)
    nq = len(case.queries)
    sample = sorted(set(range(0, nq, 3)) | {nq - 1})
    tally, worst = M64.Tally(), 0.0
    for k in (10, 1024):
        sc, ids, n = ix.exact_search_device(case.q_off, case.qc, case.qv, k)
        for i in sample:
            q = model.query(*case.queries[i], index=i)
            m = int(n[i])
            model.check_rows(sc[i], ids[i], m, k, i)
            worst = max(worst, model.check_scores(q, ids[i, :m], sc[i, :m]))
            tally.add(model.check_topk(q, ids[i, :m], sc[i, :m], None, k))
    print("model64: %-34s unambiguous=%s score_ratio=%.4g" % ("device exact edges %s-vt%d" % variant, tally, worst))


# ---- more than one chunk of queries per call ----
def _chunk_queries():
    case = EC.make("long_u16")
    picked = [case.queries[i] for i in EC.LONG_CHUNK_QUERIES]
    assert len(picked) == 9 and len(picked[0][0]) == 0 and len(picked[1][0]) == 1000
    return case, orc.csr(picked)


@pytest.mark.parametrize("filtered", [False, True], ids=["all", "filtered"])
def test_chunks_of_a_call_with_the_hook(filtered, monkeypatch):
    """SGPU_EXACT_CAND_BYTES = chunk x (n_ranges x k x 8): chunks of 1, 2, nq - 1, nq, nq + 1 queries. The q0 > 0 turns of
    exact_run - q_off indexed by a.q0 + ql, the candidate buffer reused, the merge's q0 + blockIdx.x rows - return the rows
    of the one-launch call. A fresh index: its candidate buffer is first allocated by the smallest chunk."""
    case, Q = _chunk_queries()
    nq = len(Q[0]) - 1
    shared = _built("long_u16", 0)[1]
    ix = case.build(0).upload(0)
    n_ranges = (case.n_docs + EC.RANGE - 1) // EC.RANGE
    rng = np.random.default_rng(7)
    allowed = np.union1d(np.flatnonzero(rng.random(case.n_docs) < 0.3), [0, EC.RANGE - 1, EC.RANGE, case.n_docs - 1]) if filtered else None
    f, fs = (ix.make_filter(allowed), shared.make_filter(allowed)) if filtered else (None, None)
    seen = {}
    for k in (10, 1024):
        want_n = min(k, case.n_docs if allowed is None else len(allowed))
        monkeypatch.delenv("SGPU_EXACT_CAND_BYTES", raising=False)
        plain = shared.exact_search_device(*Q, k, filter=fs)
        assert _launches(shared) == 1
        host = shared.exact_search(*Q, k, filter=fs)
        _assert_rows(plain, host, want_n, "one launch, k=%d" % k)
        for chunk in (1, 2, nq - 1, nq, nq + 1):
            monkeypatch.setenv("SGPU_EXACT_CAND_BYTES", str(chunk * n_ranges * k * 8))
            got = ix.exact_search_device(*Q, k, filter=f)
            seen[(k, chunk)] = _launches(ix)
            assert seen[(k, chunk)] == -(-nq // min(chunk, nq)), (k, chunk, seen)
            _assert_rows(got, host, want_n, "chunks of %d, k=%d" % (chunk, k))
            for a, b in zip(got, plain):
                assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)
    print("exact chunks (%s): launches %s" % ("filtered" if filtered else "all", seen))
    # a byte count below one query's candidates still serves one query per launch
    monkeypatch.setenv("SGPU_EXACT_CAND_BYTES", "1")
    _assert_rows(ix.exact_search_device(*Q, 10, filter=f), shared.exact_search(*Q, 10, filter=fs),
                 min(10, case.n_docs if allowed is None else len(allowed)), "1 byte")
    assert _launches(ix) == nq


def test_the_hook_is_inert_without_the_switch(monkeypatch):
    case, Q = _chunk_queries()
    ix = _built("long_u16", 0)[1]
    monkeypatch.setenv("SGPU_EXACT_CAND_BYTES", str(2 * 10 * 8))     # one query per launch, were it honoured
    for off in (None, "0"):
        if off is None:
            monkeypatch.delenv("SGPU_TEST_HOOKS")
        else:
            monkeypatch.setenv("SGPU_TEST_HOOKS", off)
        got = ix.exact_search_device(*Q, 10)
        L = _native.lib()
        L.sgpu_debug_exact_launches.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
        n = C.c_uint32(77)
        assert L.sgpu_debug_exact_launches(ix.h, 0, C.byref(n)) == 1 and n.value == 77     # SGPU_EINVAL: "is a test hook"
        monkeypatch.setenv("SGPU_TEST_HOOKS", "1")
        assert _launches(ix) == 1
        _assert_rows(got, ix.exact_search(*Q, 10), 10, "hook without the switch")
    assert len(ix.exact_search_device(*Q, 10)[2]) == 9 and _launches(ix) == 9      # (the same call with the switch: nine)


def test_the_shipped_candidate_buffer_cuts_a_call_in_two():
    """No hook: 163 841 documents are 6 ranges, so 256 MiB hold the candidates of 5461 queries at k = 1024; 5464 queries
    are two launches (5461 + 3)."""
    cw, dim, D, Q = EC.default_chunk_case()
    nq = len(Q[0]) - 1
    assert nq == 5464 and len(D[0]) - 1 == 163841 and nq > (256 << 20) // (6 * 1024 * 8) >= nq - 3
    lens = np.diff(D[0].astype(np.int64))
    assert lens.min() >= 1 and lens.max() <= 4
    ix = _native.NativeIndex.build(cw, dim, *D, BuildConfig.defaults(**EC.FORWARD_ONLY)).upload(0)
    dev = ix.exact_search_device(*Q, 1024)
    assert _launches(ix) == 2
    _assert_rows(dev, ix.exact_search(*Q, 1024), 1024, "default chunking")
    # the rows of the second launch's queries against the oracle, at a k it can afford
    dev = ix.exact_search_device(*Q, 10)
    assert _launches(ix) == 1
    for i in (0, nq - 3, nq - 2, nq - 1):
        c, v = Q[1][int(Q[0][i]): int(Q[0][i + 1])], Q[2][int(Q[0][i]): int(Q[0][i + 1])]
        es, ei = orc.exact_search(ix.desc, c, v, 10, orc.ORDER_SEQ)
        assert np.array_equal(dev[1][i], ei) and np.array_equal(_bits(dev[0][i]), _bits(es)), i


# ---- one tie group spanning ranges, filtered ranges around k ----
@pytest.mark.parametrize("kf", EC.TIES_KS)
def test_ties_under_filters(kf):
    """Every score ties inside a range and across ranges; the filters leave range 0 (or range 1 alone) exactly 0, 1, kf - 1,
    kf, kf + 1 allowed documents: at k = kf the task's `n_ok <= k` branch on both sides of the select."""
    case, ix = _built("ties", 0)
    Q = (case.q_off, case.qc, case.qv)
    filters = EC.tie_filters(kf)
    EC.check_tie_filters(kf, filters)
    for name, allowed in [("none", None)] + list(filters.items()):
        f = None if allowed is None else ix.make_filter(allowed)
        for k in (1, 64, 1024):
            want_n = min(k, case.n_docs if allowed is None else len(allowed))
            dev = ix.exact_search_device(*Q, k, filter=f)
            _assert_rows(dev, ix.exact_search(*Q, k, filter=f), want_n, "ties %s k=%d" % (name, k))
            for i in range(3):      # and what reasoning alone says
                es, ei = EC.ties_expected(i, k, allowed)
                assert np.array_equal(dev[1][i, :want_n], ei) and np.array_equal(_bits(dev[0][i, :want_n]), _bits(es)), (name, k, i)
