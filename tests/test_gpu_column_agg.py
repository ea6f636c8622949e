"""Column aggregations on the GPU: sgpu_column_stats, sgpu_column_histogram and sgpu_column_top equal their host twins bit
for bit (and the numpy restatement of column_agg_cases) on every size, both index variants, every filter form and all three
column types; the hook shows the grids (more than one workgroup from 16385 documents on) and the select passes of the top
call; a replaced column and a new upload are seen by the next call; calls from two threads on one replica beside a running
batch_search return the same. Run with `-m gpu`."""
import threading

import numpy as np
import pytest

import column_agg_cases as ca
import column_cases as cc
from seismic_amd import _native
from seismic_amd._abi import BuildConfig
from column_agg_cases import native_filters, same_hist, same_top, stats_of
from util import random_dataset, random_queries

pytestmark = pytest.mark.gpu

SGPU_EDEVICE = 2


def _ceil(a, b):
    return -(-a // b)


@pytest.mark.parametrize("n_docs,variant", ca.SHAPES)
def test_device_calls_equal_the_host_twins(n_docs, variant):
    t, cols = ca.fresh(n_docs, variant)
    t.ix.upload(0)
    for fname, (f, mask) in native_filters(t, cols).items():
        docs = n_docs if mask is None else int(mask.sum())
        for slot in ca.SLOTS:
            dev = stats_of(t.ix, slot, f)
            assert dev == stats_of(t.ix, slot, f, host=True), (fname, slot)
            assert dev == ca.expected_stats(cols[slot], mask), (fname, slot)
            for ename, edges in ca.edge_sets(cc.F if slot == ca.MIXED else slot, cols[slot]).items():
                if slot == ca.CONST or (ename.endswith("4096") and fname not in ("null", "third")):
                    continue
                dev = t.ix.column_histogram(slot, edges.view(np.uint32), f)
                assert same_hist(dev, t.ix.column_histogram(slot, edges.view(np.uint32), f, host=True)), (fname, slot, ename)
                assert same_hist(dev, ca.expected_histogram(cols[slot], mask, edges)), (fname, slot, ename)
            for top in ca.TOP_T:
                for order in (0, 1):
                    dev = t.ix.column_top(slot, top, order, f)
                    assert same_top(dev, t.ix.column_top(slot, top, order, f, host=True)), (fname, slot, top, order)
                    assert same_top(dev, ca.expected_top(cols[slot], mask, top, order)), (fname, slot, top, order)
                    assert t.ix.debug_column_agg_stats()["top_passes"] == (0 if docs <= top else 4), (fname, top)
    s = t.ix.debug_column_agg_stats()
    assert s["agg_tile"] == ca.TILE and s["stats_grid"] == _ceil(n_docs, ca.TILE)
    assert s["hist_docs_per_wg"] % 64 == 0 and s["hist_docs_per_wg"] >= 4096 and s["hist_grid"] == _ceil(n_docs, s["hist_docs_per_wg"])
    assert s["top_docs_per_wg"] % 256 == 0 and s["top_docs_per_wg"] >= 2048 and s["top_grid"] == _ceil(n_docs, s["top_docs_per_wg"])
    if n_docs > ca.TILE:
        assert min(s["stats_grid"], s["hist_grid"], s["top_grid"]) > 1
    assert s["stats_ms"] > 0 and s["hist_ms"] > 0 and s["top_ms"] > 0
    t.ix.close()


def test_ties_across_workgroups_come_in_id_order():
    n = 2 * ca.TILE + 5
    t, cols = ca.fresh(n, "u16_f16")
    t.ix.upload(0)
    third = t.ix.make_filter(np.arange(n) % 3 == 0)
    for order in (0, 1):
        for top in ca.TOP_T:
            ids, bits, valid, docs = t.ix.column_top(ca.CONST, top, order, None)
            assert ids.tolist() == list(range(top)) and (bits.view(np.int32) == -7).all() and valid == docs == n
            ids, _, valid, docs = t.ix.column_top(ca.CONST, top, order, third)
            assert ids.tolist() == list(range(0, 3 * top, 3)) and valid == docs == _ceil(n, 3)
    # a column whose threshold value spans every workgroup: half the documents hold the maximum
    col = (np.arange(n, dtype=np.uint32) % 2) * np.uint32(5)
    t.ix.set_column(9, col)
    assert t.ix.debug_column_agg_stats()["top_grid"] > 4
    for top in (1, 1000, 1024):
        assert same_top(t.ix.column_top(9, top, 1, None), ca.expected_top(col, None, top, 1))
        assert same_top(t.ix.column_top(9, top, 0, third), ca.expected_top(col, np.arange(n) % 3 == 0, top, 0))
    t.ix.close()


def test_fewer_values_than_t_among_more_documents_than_t():
    """docs > t, so the select is launched; the first pick finds valid <= t and the rest of the select returns at once."""
    n = ca.TILE + 1
    t, cols = ca.fresh(n, "u16_f16")
    t.ix.upload(0)
    col = np.full(n, np.nan, np.float32)
    keep = [0, 63, 64, 2047, 2048, ca.TILE - 1, ca.TILE]               # values on both sides of slice and tile borders
    col[keep] = np.array([3.0, -0.0, 0.0, np.inf, -np.inf, 3.0, -2.5], np.float32)
    t.ix.set_column(9, col)
    for top in (7, 8, 1024):
        for order in (0, 1):
            dev = t.ix.column_top(9, top, order, None)
            assert same_top(dev, t.ix.column_top(9, top, order, None, host=True)) and same_top(dev, ca.expected_top(col, None, top, order))
            assert len(dev[0]) == 7 and dev[2] == 7 and dev[3] == n and t.ix.debug_column_agg_stats()["top_passes"] == 4
    dev = t.ix.column_top(9, 6, 0, None)                                # t just below valid: the full select
    assert same_top(dev, ca.expected_top(col, None, 6, 0)) and len(dev[0]) == 6
    s = stats_of(t.ix, 9, None)
    assert s == ca.expected_stats(col, None) and s["valid"] == 7
    t.ix.close()


def _all_calls(ix, slot, f, edges):
    return (stats_of(ix, slot, f), ix.column_histogram(slot, edges, f), ix.column_top(slot, 100, 1, f), ix.column_top(slot, 3, 0, f))


def _all_host(ix, slot, f, edges):
    return (stats_of(ix, slot, f, host=True), ix.column_histogram(slot, edges, f, host=True), ix.column_top(slot, 100, 1, f, host=True),
            ix.column_top(slot, 3, 0, f, host=True))


def _same_all(got, want):
    return got[0] == want[0] and same_hist(got[1], want[1]) and same_top(got[2], want[2]) and same_top(got[3], want[3])


def test_a_replaced_column_and_a_new_upload_are_seen_by_the_next_call():
    n = ca.TILE + 1
    t, cols = ca.fresh(n, "u16_f16")
    ix = t.ix
    ix.upload(0)
    rng = np.random.default_rng(3)
    f = ix.make_filter(np.arange(n) % 3 == 0)
    a = rng.integers(0, 1000, n).astype(np.uint32)
    edges_u = np.array([0, 10, 500, 999], np.uint32)
    ix.set_column(9, a)
    first = _all_calls(ix, 9, f, edges_u)
    assert _same_all(first, _all_host(ix, 9, f, edges_u)) and first[0]["max_bits"] <= 999
    ix.set_column(9, a + np.uint32(5000))                                # replaced after a device call (a new generation)
    second = _all_calls(ix, 9, f, edges_u)
    assert _same_all(second, _all_host(ix, 9, f, edges_u)) and second[0]["min_bits"] >= 5000 and second[1][2] == second[1][4]
    b = (rng.random(n).astype(np.float32) - np.float32(0.5)) * np.float32(1e6)
    b[5] = np.nan
    ix.set_column(9, b)                                                  # retyped
    edges_f = cc.bits_of([-1e6, -10.0, 0.0, 1e6], cc.F32)
    third = _all_calls(ix, 9, None, edges_f)
    assert _same_all(third, _all_host(ix, 9, None, edges_f)) and third[0]["valid"] == n - 1 and third[1][3] == 1
    ix.upload(0)                                                        # the replica replaced: the copies are made again
    assert _same_all(_all_calls(ix, 9, None, edges_f), third)
    assert _same_all(_all_calls(ix, cc.I, f, cc.bits_of([-30, 0, 30], cc.I32)), _all_host(ix, cc.I, f, cc.bits_of([-30, 0, 30], cc.I32)))
    ix.set_column(9, None)                                              # dropped
    with pytest.raises(_native.SeismicHipError):
        ix.column_stats(9)
    cold, _ = ca.fresh(33, "u16_f16")                                   # not uploaded; replica out of range
    for call in (lambda ix_, r: ix_.column_stats(cc.U, replica=r), lambda ix_, r: ix_.column_histogram(cc.U, edges_u, replica=r),
                 lambda ix_, r: ix_.column_top(cc.U, 5, replica=r)):
        for ix_, r in ((cold.ix, 0), (ix, 1)):
            with pytest.raises(_native.SeismicHipError) as e:
                call(ix_, r)
            assert e.value.status == SGPU_EDEVICE
    ix.close()


def test_calls_from_two_threads_beside_a_running_batch_search():
    dim, n_docs = 300, 3000
    off, comps, vals = random_dataset(71, n_docs, dim, nnz_lo=6, nnz_hi=60, empty_every=97)
    ix = _native.NativeIndex.build(2, dim, off, comps, vals,
                                   BuildConfig.defaults(n_postings=100, centroid_fraction=0.2, summary_energy=0.5, max_fraction=4.0)).upload(0)
    rng = np.random.default_rng(9)
    price = (rng.random(n_docs).astype(np.float32) * 100).astype(np.float32)
    price[::501] = np.nan
    ts = rng.integers(-10 ** 9, 10 ** 9, n_docs).astype(np.int32)
    ix.set_column(0, price)
    ix.set_column(1, ts)
    f = ix.make_filter(np.arange(n_docs) % 2 == 0)
    cases = {0: cc.bits_of(np.linspace(0, 100, 21), cc.F32), 1: cc.bits_of(np.linspace(-10 ** 9, 10 ** 9, 4097).astype(np.int64), cc.I32)}
    want = {slot: _all_host(ix, slot, f, e) for slot, e in cases.items()}
    q = random_queries(72, 1250, dim, 3, 40)
    ref = ix.batch_search(*q, 10, 4, 1.0, False)
    errors, found = [], []

    def searcher():
        try:
            for _ in range(3):
                found.append(ix.batch_search(*q, 10, 4, 1.0, False))
        except Exception as e:   # noqa: BLE001
            errors.append(e)

    def caller(slot):
        try:
            for _ in range(10):
                if not _same_all(_all_calls(ix, slot, f, cases[slot]), want[slot]):
                    errors.append((slot, "differs"))
        except Exception as e:   # noqa: BLE001
            errors.append(e)
    threads = [threading.Thread(target=searcher)] + [threading.Thread(target=caller, args=(slot,)) for slot in (0, 1)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    assert len(found) == 3 and all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for got in found for x, y in zip(got, ref))
    ix.close()


def test_python_classes_on_the_gpu():
    import os

    import seismic_amd
    from seismic_amd.index import read_jsonl
    toy = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "toy")
    ids, _, _ = read_jsonl(os.path.join(toy, "documents.jsonl"))
    ix = seismic_amd.SeismicIndex.build(os.path.join(toy, "documents.jsonl"), n_postings=50, centroid_fraction=0.2)
    n = len(ids)
    ix.set_column("tenant", np.arange(n, dtype=np.uint32) % 3)
    ix.set_column("price", (np.arange(n, dtype=np.float32) * 0.5) % 7)
    f = ix.make_column_filter(must=[("tenant", [1, 2])])
    for flt in (None, f):                                                # device=None: the GPU
        assert ix.stats("price", filter=flt) == ix.stats("price", filter=flt, device=False)
        dev, host = ix.histogram("price", [0.0, 1.0, 6.5], filter=flt), ix.histogram("price", [0.0, 1.0, 6.5], filter=flt, device=False)
        assert dev["counts"].tolist() == host["counts"].tolist() and {k: dev[k] for k in ("below", "above", "nan", "docs")} == {
            k: host[k] for k in ("below", "above", "nan", "docs")}
        dev, host = ix.top_by("price", k=5, descending=True, filter=flt), ix.top_by("price", k=5, descending=True, filter=flt, device=False)
        assert dev[0] == host[0] and dev[1].tolist() == host[1].tolist()
    s = ix._ix.debug_column_agg_stats()
    assert s["stats_grid"] == s["hist_grid"] == s["top_grid"] == 1      # the kernels ran
