"""Term filters on the GPU: the words sgpu_filter_create_terms computes on the device from the replica's exact file equal
the host twin's word for word (and the counts) on every case of term_filter_cases, on replica 1 as on replica 0; the first
call on a fresh upload builds the exact file and exact search still returns the host's rows afterwards; a term filter
drives filtered approximate and exact search exactly as the id filter of the same set; the device-only errors leave the
index searchable. Run with `-m gpu`."""
import ctypes as C

import numpy as np
import pytest

import term_filter_cases as tc
from seismic_amd import _native
from seismic_amd._abi import BuildConfig
from util import random_dataset, random_queries

pytestmark = pytest.mark.gpu

SGPU_OK, SGPU_EINVAL, SGPU_EDEVICE = 0, 1, 2
NINF = float("-inf")


def _exact_launches(ix, replica=0):
    L = _native.lib()
    L.sgpu_debug_exact_launches.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
    n = C.c_uint32(77)
    return L.sgpu_debug_exact_launches(ix.h, replica, C.byref(n)), n.value


def _stats(ix, replica=0):
    L = _native.lib()
    L.sgpu_debug_term_filter_stats.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    out = np.zeros(4, np.float64)
    _native.check(L.sgpu_debug_term_filter_stats(ix.h, replica, _native._p(out)))
    return dict(kernel_ms=out[0], build_wall_ms=out[1], file_bytes=int(out[2]), ranges=int(out[3]))


def _compare_all(t, replica=0):
    sets = tc.clause_sets(t)
    for name, (clauses, ms) in sets.items():
        dev = t.ix.make_term_filter(clauses, ms, replica=replica)
        host = t.ix.make_term_filter(clauses, ms, host=True)
        assert tc.bits_diff(dev.bits(), host.bits()) is None, (name, tc.bits_diff(dev.bits(), host.bits()))
        assert dev.count == host.count == tc.popcount(host.bits()), name
    for wname, allowed in tc.within_sets(t.n_docs).items():
        wf = t.ix.make_filter(allowed)
        for name in tc.WITHIN_CLAUSES:
            clauses, ms = sets[name]
            dev = t.ix.make_term_filter(clauses, ms, within=wf, replica=replica)
            host = t.ix.make_term_filter(clauses, ms, within=wf, host=True)
            assert tc.bits_diff(dev.bits(), host.bits()) is None, (name, wname)
            assert dev.count == host.count


@pytest.mark.parametrize("variant", tc.VARIANTS)
@pytest.mark.parametrize("n_docs", tc.N_DOCS)
def test_device_bits_equal_the_host_twin(n_docs, variant):
    t = tc.fresh(n_docs, variant)
    t.ix.upload(0)
    _compare_all(t)
    assert _stats(t.ix)["ranges"] == t.n_ranges
    t.ix.close()


@pytest.mark.parametrize("n_docs,variant", [(65541, "u16_f16"), (33, "u16_dvb"), (32769, "u32_u8")])
def test_replica_one_of_an_index_uploaded_twice(n_docs, variant):
    t = tc.fresh(n_docs, variant)
    t.ix.upload_many([0, 0])
    assert t.ix.replicas == 2
    _compare_all(t, replica=1)
    assert _exact_launches(t.ix, 1)[0] == SGPU_OK and _exact_launches(t.ix, 0)[0] == SGPU_EINVAL   # replica 1's file alone
    t.ix.close()


def test_first_call_builds_the_exact_file_and_exact_search_still_agrees():
    t = tc.fresh(32769, "u16_f16")
    ix = t.ix.upload(0)
    assert _exact_launches(ix)[0] == SGPU_EINVAL                       # no exact file yet
    clauses, ms = tc.clause_sets(t)["mixed"]
    f = ix.make_term_filter(clauses, ms)
    st, launches = _exact_launches(ix)
    assert st == SGPU_OK and launches == 0                             # the file is there; no exact call has run
    s = _stats(ix)
    assert s["ranges"] == 2 and s["file_bytes"] >= 4 * int(t.fwd["off"][-1]) and s["kernel_ms"] > 0
    q = random_queries(7, 9, 12)
    dev, host = ix.exact_search_device(*q, 25), ix.exact_search(*q, 25)
    assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(dev, host))
    assert _exact_launches(ix) == (SGPU_OK, 1) and _stats(ix)["build_wall_ms"] == s["build_wall_ms"]   # one file, built once
    g = ix.make_term_filter(clauses, ms)                               # and a term filter after an exact call
    assert np.array_equal(g.bits(), f.bits())
    devf, hostf = ix.exact_search_device(*q, 25, filter=g), ix.exact_search(*q, 25, filter=f)
    assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(devf, hostf))
    ix.close()


@pytest.fixture(scope="module")
def small():
    dim, n_docs = 300, 3000
    off, comps, vals = random_dataset(61, n_docs, dim, nnz_lo=6, nnz_hi=60, empty_every=97)
    ix = _native.NativeIndex.build(2, dim, off, comps, vals,
                                   BuildConfig.defaults(n_postings=100, centroid_fraction=0.2, summary_energy=0.5,
                                                        max_fraction=4.0)).upload(0)
    return ix, dim, n_docs


def _frequent(ix, n):
    fwd = tc.forward(ix.desc)
    return np.argsort(-np.bincount(fwd["comps"], minlength=fwd["dim"]), kind="stable")[:n].tolist(), fwd


@pytest.mark.parametrize("nq", [4, 1250])                              # a cooperative launch; plain chunks
def test_filtered_search_with_a_term_filter_equals_the_id_filter(small, nq):
    ix, dim, n_docs = small
    (a, b, c, d), fwd = _frequent(ix, 4)
    q = random_queries(62, nq, dim, 3, 40)
    for clauses, ms in (([(a, tc.MUST, NINF)], 0), ([(a, tc.MUST_NOT, NINF), (b, tc.SHOULD, 0.3), (c, tc.SHOULD, NINF),
                                                      (d, tc.SHOULD, NINF)], 2)):
        tf = ix.make_term_filter(clauses, ms)
        assert tc.bits_diff(tf.bits(), tc.expected_bits(fwd, clauses, ms)) is None and 0 < tf.count < n_docs
        idf = ix.make_filter(tf.ids())
        got, want = ix.batch_search(*q, 10, 4, 1.0, False, filter=tf), ix.batch_search(*q, 10, 4, 1.0, False, filter=idf)
        assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(got, want))
        assert (got[2] > 0).any()
        if nq == 4:
            got, want = ix.exact_search_device(*q, 10, filter=tf), ix.exact_search_device(*q, 10, filter=idf)
            assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(got, want))
            host = ix.exact_search(*q, 10, filter=tf)
            assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(got, host))
        assert tf.device_bytes() > 0


def test_device_only_errors_leave_the_index_searchable(small):
    ix, dim, _ = small
    q = random_queries(63, 16, dim, 3, 40)
    before = ix.batch_search(*q, 10, 4, 1.0, False)
    with pytest.raises(_native.SeismicHipError) as e:
        ix.make_term_filter([(0, tc.MUST, NINF)], replica=1)           # replica out of range
    assert e.value.status == SGPU_EDEVICE
    cold = tc.fresh(33, "u16_f16").ix                                  # not uploaded
    with pytest.raises(_native.SeismicHipError) as e:
        cold.make_term_filter([(0, tc.MUST, NINF)])
    assert e.value.status == SGPU_EDEVICE and "upload" in str(e.value)
    assert cold.make_term_filter([(0, tc.MUST, NINF)], host=True).count > 0
    cold.upload(0)
    assert cold.make_term_filter([(0, tc.MUST, NINF)]).count == cold.make_term_filter([(0, tc.MUST, NINF)], host=True).count
    after = ix.batch_search(*q, 10, 4, 1.0, False)
    assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(before, after))
    f = ix.make_term_filter([(0, tc.MUST_NOT, NINF)])
    assert f.count > 0 and ix.batch_search(*q, 10, 4, 1.0, False, filter=f)[2].max() > 0
