"""Document columns on the GPU: the words sgpu_filter_create_columns computes on the device equal the host twin's word for
word (and the counts) on every case of column_cases, on replica 1 as on replica 0; the rows of sgpu_facet_counts equal the
host twin's on every facet column, on the path (LDS histograms or global atomics) the column's maximum asks for; a
replaced column, a new upload and a dropped column are seen by the next device call; a column filter drives filtered
approximate and exact search exactly as the id filter of the same set; term and column filters nest as `within`; the
device-only errors leave the index searchable. Run with `-m gpu`."""
import numpy as np
import pytest

import column_cases as cc
import term_filter_cases as tc
from seismic_amd import _native
from seismic_amd._abi import BuildConfig
from util import random_dataset, random_queries

pytestmark = pytest.mark.gpu

SGPU_EINVAL, SGPU_EDEVICE, SGPU_ELIMIT = 1, 2, 5


def _compare_all(t, replica=0):
    sets = cc.clause_sets(t)
    for name, (clauses, ms, sv) in sets.items():
        dev = t.ix.make_column_filter(clauses, ms, sv, replica=replica)
        host = t.ix.make_column_filter(clauses, ms, sv, host=True)
        assert cc.bits_diff(dev.bits(), host.bits()) is None, (name, cc.bits_diff(dev.bits(), host.bits()))
        assert dev.count == host.count == cc.popcount(host.bits()), name
    for wname, allowed in cc.within_sets(t.n_docs).items():
        wf = t.ix.make_filter(allowed)
        for name, (clauses, ms, sv) in sets.items():              # every clause set with every `within` set
            dev = t.ix.make_column_filter(clauses, ms, sv, within=wf, replica=replica)
            host = t.ix.make_column_filter(clauses, ms, sv, within=wf, host=True)
            assert cc.bits_diff(dev.bits(), host.bits()) is None, (name, wname)
            assert dev.count == host.count


@pytest.mark.parametrize("n_docs,variant", cc.SHAPES)
def test_device_words_equal_the_host_twin(n_docs, variant):
    t = cc.fresh(n_docs, variant)
    t.ix.upload(0)
    _compare_all(t)
    s = t.ix.debug_column_stats()
    assert s["filter_docs_per_wg"] == cc.W and s["filter_grid"] == -(-n_docs // cc.W)
    assert s["column_bytes"] >= 3 * 4 * n_docs
    t.ix.close()


@pytest.mark.parametrize("n_docs,variant", [(2 * cc.W + 5, "u16_f16"), (65, "u32_u8")])
def test_replica_one_of_an_index_uploaded_twice(n_docs, variant):
    t = cc.fresh(n_docs, variant)
    t.ix.upload_many([0, 0])
    assert t.ix.replicas == 2
    _compare_all(t, replica=1)
    col = cc.facet_columns(n_docs)["ties"]
    t.ix.set_column(cc.FACET_SLOT, col)
    assert _same(t.ix.facet_counts(cc.FACET_SLOT, None, 2, replica=1), t.ix.facet_counts(cc.FACET_SLOT, None, 2, host=True))
    assert t.ix.debug_column_stats(1)["column_bytes"] > 0
    with pytest.raises(_native.SeismicHipError):
        t.ix.debug_column_stats(0)                                      # replica 0 has run no column call
    t.ix.close()


def _same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2:] == want[2:]


def _facet_filters(t):
    out = {"all": None}
    for wname, allowed in cc.within_sets(t.n_docs).items():
        out[wname] = t.ix.make_filter(allowed)
    clauses, ms, sv = cc.clause_sets(t)["three_slots"]
    out["column_filter"] = t.ix.make_column_filter(clauses, ms, sv)
    return out


@pytest.mark.parametrize("n_docs", cc.FACET_N_DOCS)
def test_facet_rows_equal_the_host_twin(n_docs):
    t = cc.fresh(n_docs, "u16_f16")
    t.ix.upload(0)
    filters = _facet_filters(t)
    for cname, col in cc.facet_columns(n_docs).items():
        t.ix.set_column(cc.FACET_SLOT, col)
        for fname, f in filters.items():
            for top in cc.FACET_T:
                dev = t.ix.facet_counts(cc.FACET_SLOT, f, top)
                host = t.ix.facet_counts(cc.FACET_SLOT, f, top, host=True)
                assert _same(dev, host), (cname, fname, top, dev, host)
                if cname in cc.FACET_PATH:
                    assert t.ix.debug_column_stats()["facet_path"] == cc.FACET_PATH[cname], cname
        assert _same(t.ix.facet_counts(cc.FACET_SLOT, None, 2), cc.expected_facets(col, None, 2)), cname   # and the restatement itself
    s = t.ix.debug_column_stats()
    assert s["facet_docs_per_wg"] % 64 == 0 and s["facet_grid"] == -(-n_docs // s["facet_docs_per_wg"])
    t.ix.close()


def test_set_column_upload_and_drop_are_seen_by_the_next_device_call():
    t = cc.fresh(cc.W + 1, "u16_f16")
    ix, n = t.ix, cc.W + 1
    ix.upload(0)
    base = ix.device_bytes()
    a = np.arange(n, dtype=np.uint32)
    ix.set_column(9, a)
    assert ix.device_bytes() == base                                    # no copy before a device call needs one
    rng = [cc.rng_clause(9, cc.MUST, cc.U32, 10, 19)]
    assert ix.make_column_filter(rng).ids().tolist() == list(range(10, 20))
    one = ix.device_bytes()
    assert one >= base + 4 * n
    ix.set_column(9, a[::-1].copy())                                    # replaced after a device call
    assert ix.make_column_filter(rng).ids().tolist() == list(range(n - 20, n - 10))
    assert ix.device_bytes() == one                                     # the copy's memory is reused
    ix.set_column(9, (a % 50).astype(np.uint32))
    assert _same(ix.facet_counts(9, None, 3), ix.facet_counts(9, None, 3, host=True))
    ix.set_column(9, np.linspace(-1, 1, n).astype(np.float32))          # retyped
    f = [cc.rng_clause(9, cc.MUST, cc.F32, -0.5, 0.5)]
    assert np.array_equal(ix.make_column_filter(f).bits(), ix.make_column_filter(f, host=True).bits())
    ix.upload(0)                                                        # a new upload: the columns still answer
    assert ix.device_bytes() == base
    assert np.array_equal(ix.make_column_filter(f).bits(), ix.make_column_filter(f, host=True).bits())
    sets = cc.clause_sets(t)["three_slots"]
    assert np.array_equal(ix.make_column_filter(*sets).bits(), ix.make_column_filter(*sets, host=True).bits())
    four = ix.device_bytes()
    assert four >= base + 4 * 4 * n
    ix.set_column(9, None)                                              # dropped: its copy goes
    assert base + 3 * 4 * n <= ix.device_bytes() <= four - 4 * n
    with pytest.raises(_native.SeismicHipError) as e:
        ix.make_column_filter(f)
    assert e.value.status == SGPU_EINVAL
    for slot in (cc.U, cc.I, cc.F):
        ix.set_column(slot, None)
    assert ix.device_bytes() == base
    ix.close()


@pytest.fixture(scope="module")
def small():
    dim, n_docs = 300, 3000
    off, comps, vals = random_dataset(61, n_docs, dim, nnz_lo=6, nnz_hi=60, empty_every=97)
    ix = _native.NativeIndex.build(2, dim, off, comps, vals,
                                   BuildConfig.defaults(n_postings=100, centroid_fraction=0.2, summary_energy=0.5,
                                                        max_fraction=4.0)).upload(0)
    rng = np.random.default_rng(8)
    cols = {0: rng.integers(0, 20, n_docs).astype(np.uint32), 1: rng.integers(-1000, 1000, n_docs).astype(np.int32),
            2: rng.random(n_docs).astype(np.float32) * 100}
    for slot, col in cols.items():
        ix.set_column(slot, col)
    return ix, dim, n_docs, cols


@pytest.mark.parametrize("nq", [4, 1250])                              # a cooperative launch; plain chunks
def test_filtered_search_with_a_column_filter_equals_the_id_filter(small, nq):
    ix, dim, n_docs, cols = small
    q = random_queries(62, nq, dim, 3, 40)
    price = cc.bits_of([0.0, 60.0], cc.F32)
    clauses = [(0, cc.MUST, cc.IN, 0, 0, 0, 4), cc.rng_clause(1, cc.MUST, cc.I32, -500, 800), (2, cc.MUST, cc.RANGE, int(price[0]), int(price[1]), 0, 0)]
    cf = ix.make_column_filter(clauses, 0, [3, 7, 11, 3])
    want = np.isin(cols[0], [3, 7, 11]) & (cols[1] >= -500) & (cols[1] <= 800) & (cols[2] <= 60.0)
    assert np.array_equal(cf.ids(), np.flatnonzero(want)) and 0 < cf.count < n_docs
    idf = ix.make_filter(cf.ids())
    got, ref = ix.batch_search(*q, 10, 4, 1.0, False, filter=cf), ix.batch_search(*q, 10, 4, 1.0, False, filter=idf)
    assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(got, ref))
    assert (got[2] > 0).any()
    if nq == 4:
        got, ref = ix.exact_search_device(*q, 10, filter=cf), ix.exact_search_device(*q, 10, filter=idf)
        assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(got, ref))
        host = ix.exact_search(*q, 10, filter=cf)
        assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(got, host))
    assert cf.device_bytes() > 0


def test_term_and_column_filters_nest(small):
    ix, dim, n_docs, cols = small
    fwd = tc.forward(ix.desc)
    a = int(np.argmax(np.bincount(fwd["comps"], minlength=fwd["dim"])))
    term = [(a, tc.MUST, float("-inf"))]
    col = [cc.rng_clause(0, cc.MUST, cc.U32, 0, 9)]
    tf, cf = ix.make_term_filter(term), ix.make_column_filter(col)
    both = np.unpackbits((tf.bits() & cf.bits()).view(np.uint8), bitorder="little")[:n_docs].sum()
    inner = ix.make_column_filter(col, within=tf)                     # a term filter as `within` of a column filter
    outer = ix.make_term_filter(term, within=cf)                      # and the reverse
    assert np.array_equal(inner.bits(), tf.bits() & cf.bits()) and np.array_equal(outer.bits(), inner.bits())
    assert inner.count == outer.count == int(both) and 0 < inner.count < min(tf.count, cf.count)
    assert np.array_equal(ix.make_column_filter(col, within=tf, host=True).bits(), inner.bits())
    rows = ix.facet_counts(0, inner, 20)
    assert _same(rows, ix.facet_counts(0, inner, 20, host=True)) and rows[3] == inner.count and set(rows[0].tolist()) <= set(range(10))


def test_device_only_errors_leave_the_index_searchable(small):
    ix, dim, n_docs, cols = small
    q = random_queries(63, 16, dim, 3, 40)
    before = ix.batch_search(*q, 10, 4, 1.0, False)
    col = [cc.rng_clause(0, cc.MUST, cc.U32, 0, 9)]
    for call in (lambda r: ix.make_column_filter(col, replica=r), lambda r: ix.facet_counts(0, None, 5, replica=r)):
        with pytest.raises(_native.SeismicHipError) as e:
            call(1)                                                     # replica out of range
        assert e.value.status == SGPU_EDEVICE
    cold = cc.fresh(33, "u16_f16").ix                                   # not uploaded
    for call in (lambda: cold.make_column_filter(col), lambda: cold.facet_counts(cc.I + 4, None, 5)):
        cold.set_column(cc.I + 4, np.zeros(33, np.uint32))
        with pytest.raises(_native.SeismicHipError) as e:
            call()
        assert e.value.status == SGPU_EDEVICE and "upload" in str(e.value)
    assert cold.make_column_filter(col, host=True).count > 0
    cold.upload(0)
    assert cold.make_column_filter(col).count == cold.make_column_filter(col, host=True).count
    after = ix.batch_search(*q, 10, 4, 1.0, False)
    assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(before, after))


def test_a_column_at_the_limit_is_refused_on_device_and_host_alike(small):
    ix, dim, n_docs, cols = small
    over = cols[0].copy()
    over[n_docs - 1] = cc.MAX_BINS
    ix.set_column(7, over)
    for host in (False, True):
        with pytest.raises(_native.SeismicHipError) as e:
            ix.facet_counts(7, None, 5, host=host)
        assert e.value.status == SGPU_ELIMIT and "4194304" in str(e.value)
    over[n_docs - 1] = cc.MAX_BINS - 1
    ix.set_column(7, over)
    assert _same(ix.facet_counts(7, None, 5), ix.facet_counts(7, None, 5, host=True))
    assert ix.debug_column_stats()["facet_path"] == 1
    ix.set_column(7, None)


def test_python_classes_on_the_gpu():
    import os

    import seismic_amd
    from seismic_amd.index import read_jsonl
    toy = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "toy")
    ids, _, _ = read_jsonl(os.path.join(toy, "documents.jsonl"))
    _, qvecs, _ = read_jsonl(os.path.join(toy, "queries.jsonl"))
    qc = [np.array(list(v.keys())) for v in qvecs]
    qv = [np.array(list(v.values()), np.float32) for v in qvecs]
    ix = seismic_amd.SeismicIndex.build(os.path.join(toy, "documents.jsonl"), n_postings=50, centroid_fraction=0.2)
    n = len(ids)
    tenant = {d: i % 3 for i, d in enumerate(ids)}
    ix.set_column("tenant", tenant)
    ix.set_column("price", np.arange(n, dtype=np.float32) * 0.5)
    entries = dict(must=[("tenant", [1, 2]), ("price", None, 4.0)])
    dev, host = ix.make_column_filter(**entries), ix.make_column_filter(device=False, **entries)   # device=None: the GPU
    assert np.array_equal(dev.bits(), host.bits()) and dev.count == host.count > 0
    assert ix._ix.debug_column_stats()["filter_grid"] == 1                                         # the kernel ran
    assert ix.facets("tenant", filter=dev, top=2) == ix.facets("tenant", filter=host, top=2, device=False)
    assert ix._ix.debug_column_stats()["facet_grid"] == 1
    # batch_search_collapsed(groups="name") is the search and batch_collapse under the column's keys
    qids = ["q%d" % i for i in range(len(qc))]
    rows = ix.batch_search_collapsed(qids, qc, qv, 3, 4, 0.8, depth=10, groups="tenant")
    ix.set_groups(tenant)
    assert rows == ix.batch_search_collapsed(qids, qc, qv, 3, 4, 0.8, depth=10) and any(rows)
    ix.set_groups(None)
    with pytest.raises(ValueError):
        ix.batch_search_collapsed(qids, qc, qv, 3, 4, 0.8, depth=10, groups="no-such-column")
