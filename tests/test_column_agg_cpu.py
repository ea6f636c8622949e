"""Column aggregations without a device: the three host twins (sgpu_column_stats_host, sgpu_column_histogram_host,
sgpu_column_top_host) against the numpy restatement of tests/column_agg_cases.py - stats as bits (`sum` as the u64 pattern
of the double, sum_int exact), histogram counts exact with sum(counts) + below + above + nan == docs, top rows exact - on
every size, column and filter; each wrong reading differing from the host twin on the case named for it; the argument
checks in the header's order; 1 thread against 16; the histogram's and the top's edges; the Python classes with
device=False."""
import ctypes as C
import os

import numpy as np
import pytest

import column_agg_cases as ca
import column_cases as cc
import seismic_amd
from seismic_amd import _native
from seismic_amd._abi import ColumnStats
from seismic_amd.index import read_jsonl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD_TOY = os.path.join(ROOT, "tests", "golden", "toy")
OK, EINVAL, EDEVICE, ELIMIT = 0, 1, 2, 5
from column_agg_cases import native_filters, same_hist, same_top, stats_of


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def test_header_declares_the_six_calls_and_the_abi_version_stays():
    text = open(os.path.join(ROOT, "include", "seismic_hip.h")).read()
    for decl in ("struct sgpu_column_stats {",
                 "sgpu_status sgpu_column_stats(sgpu_index* idx, uint32_t replica, uint32_t slot, const sgpu_filter* filter,",
                 "sgpu_status sgpu_column_stats_host(const sgpu_index* idx, uint32_t slot, const sgpu_filter* filter, uint32_t num_threads,",
                 "sgpu_status sgpu_column_histogram(sgpu_index* idx, uint32_t replica, uint32_t slot, const sgpu_filter* filter,",
                 "sgpu_status sgpu_column_histogram_host(const sgpu_index* idx, uint32_t slot, const sgpu_filter* filter,",
                 "sgpu_status sgpu_column_top(sgpu_index* idx, uint32_t replica, uint32_t slot, const sgpu_filter* filter, uint32_t t,",
                 "sgpu_status sgpu_column_top_host(const sgpu_index* idx, uint32_t slot, const sgpu_filter* filter, uint32_t t,"):
        assert decl in text, decl
    assert text.index("---- document columns:") < text.index("---- column aggregations:")
    section = text[text.index("---- column aggregations:"):]
    assert "NOT part of the index file" in section and "0x7ff8000000000000" in section and "16384" in section
    assert "sgpu_debug_column_agg_stats" in open(os.path.join(ROOT, "include", "seismic_hip_testing.h")).read()
    L = _native.lib()
    for name in ("sgpu_column_stats", "sgpu_column_stats_host", "sgpu_column_histogram", "sgpu_column_histogram_host", "sgpu_column_top",
                 "sgpu_column_top_host", "sgpu_debug_column_agg_stats"):
        assert hasattr(L, name), name
    assert L.sgpu_abi_version() == 4
    assert C.sizeof(ColumnStats) == 40


def test_every_wrong_reading_changes_its_case():
    ca.check()


def test_the_canonical_sum_is_not_the_left_to_right_sum():
    x = np.array([1e30, 1.0, -1e30, 1e-30], np.float32).astype(np.float64)
    assert ((x[0] + x[1]) + x[2]) + x[3] == x[3]                           # left to right: the 1 is lost in 1e30
    assert ca.canonical_sum(x) == 1.0                                      # four lanes, folded as (x0 + x2) + (x1 + x3)
    y = np.concatenate([x, np.zeros(252), [-1e-30]]).astype(np.float32).astype(np.float64)
    assert ca.canonical_sum(y) == 1.0                                      # document 256 joins lane 0 BEFORE the fold: 1e30 - 1e-30 = 1e30
    z = np.zeros(ca.TILE + 1)
    z[0], z[ca.TILE] = 1e30, 1.0                                           # the second tile's sum is added last
    assert ca.canonical_sum(z) == 1e30


# ---------------------------------------------------------------------------------------------------------------------
# the host twins against the restatement
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_docs,variant", ca.SHAPES)
def test_host_stats_equal_the_restatement(n_docs, variant):
    t, cols = ca.make(n_docs, variant)
    for fname, (f, mask) in native_filters(t, cols).items():
        for slot in ca.SLOTS:
            want = ca.expected_stats(cols[slot], mask)
            for threads in (1, 16):                                     # 1 thread against 16: the same bits
                assert stats_of(t.ix, slot, f, host=True, num_threads=threads) == want, (fname, slot, threads)


@pytest.mark.parametrize("n_docs,variant", ca.SHAPES)
def test_host_histograms_equal_the_restatement(n_docs, variant):
    t, cols = ca.make(n_docs, variant)
    for fname, (f, mask) in native_filters(t, cols).items():
        for slot in (cc.U, cc.I, cc.F, ca.MIXED, ca.BIG):
            sets = ca.edge_sets(cc.F if slot == ca.MIXED else slot, cols[slot])
            for ename, edges in sets.items():
                if ename.endswith("4096") and fname not in ("null", "third"):
                    continue
                want = ca.expected_histogram(cols[slot], mask, edges)
                for threads in (1, 16):
                    got = t.ix.column_histogram(slot, edges.view(np.uint32), f, host=True, num_threads=threads)
                    assert same_hist(got, want), (fname, slot, ename, threads)
                    assert int(got[0].sum()) + got[1] + got[2] + got[3] == got[4] == (n_docs if mask is None else int(mask.sum()))
                assert len(got[0]) == len(edges) - 1


@pytest.mark.parametrize("n_docs,variant", ca.SHAPES)
def test_host_top_rows_equal_the_restatement(n_docs, variant):
    t, cols = ca.make(n_docs, variant)
    for fname, (f, mask) in native_filters(t, cols).items():
        for slot in ca.SLOTS:
            for top in ca.TOP_T:
                for order in (0, 1):
                    want = ca.expected_top(cols[slot], mask, top, order)
                    for threads in (1, 16):
                        got = t.ix.column_top(slot, top, order, f, host=True, num_threads=threads)
                        assert same_top(got, want), (fname, slot, top, order, threads)


def test_the_constant_column_ties_by_id_in_both_orders():
    n = 2 * ca.TILE + 5                                                 # n_docs > t: the rows are the first t ids
    t, cols = ca.make(n, "u16_f16")
    for order in (0, 1):
        for top in ca.TOP_T:
            ids, bits, valid, docs = t.ix.column_top(ca.CONST, top, order, None, host=True)
            assert ids.tolist() == list(range(top)) and (bits.view(np.int32) == -7).all() and valid == docs == n
    f = t.ix.make_filter(np.arange(n) % 3 == 0)
    ids, _, valid, docs = t.ix.column_top(ca.CONST, 1024, 1, f, host=True)
    assert ids.tolist() == list(range(0, 3 * 1024, 3)) and valid == docs == -(-n // 3)


def test_fewer_values_than_t():
    t, cols = ca.make(65, "u16_f16")
    nan = np.isnan(cols[cc.F])
    ids, bits, valid, docs = t.ix.column_top(cc.F, 1024, 0, None, host=True)
    assert valid == len(ids) == 65 - int(nan.sum()) < docs == 65 and not nan[ids].any()
    assert ids[0] == 0 and bits[0] == 0xff800000                       # -inf first
    only_nan = t.ix.make_filter(nan)
    ids, bits, valid, docs = t.ix.column_top(cc.F, 5, 1, only_nan, host=True)
    assert len(ids) == 0 and valid == 0 and docs == int(nan.sum()) > 0
    s = t.ix.column_stats(cc.F, only_nan, host=True)
    assert (s["valid"], s["min_bits"], s["max_bits"], s["sum_bits"]) == (0, 0, 0, 0) and s["docs"] == docs
    s = t.ix.column_stats(cc.F, None, host=True)                       # both infinities: the sum is THE quiet NaN
    assert s["sum_bits"] == ca.QUIET_NAN_BITS and s["min_bits"] == 0xff800000 and s["max_bits"] == 0x7f800000
    keep = ca.filters(65, cols[cc.F])["plus_inf_only"]
    s = t.ix.column_stats(cc.F, t.ix.make_filter(keep), host=True)
    assert s["sum_bits"] == 0x7ff0000000000000                         # +inf without -inf: +inf


@pytest.mark.parametrize("wrong", ca.STATS_WRONG)
def test_a_wrong_stats_reading_differs_from_the_host_twin(wrong):
    n_docs, slot, fname = ca.STATS_WRONG_CASES[wrong]
    t, cols = ca.make(n_docs, "u16_f16")
    f, mask = native_filters(t, cols)[fname]
    got = stats_of(t.ix, slot, f, host=True)
    assert got == ca.expected_stats(cols[slot], mask)
    assert got != ca.expected_stats(cols[slot], mask, wrong=wrong)


@pytest.mark.parametrize("wrong", ca.HIST_WRONG)
def test_a_wrong_histogram_reading_differs_from_the_host_twin(wrong):
    n_docs, slot, fname, ename = ca.HIST_WRONG_CASES[wrong]
    t, cols = ca.make(n_docs, "u16_f16")
    f, mask = native_filters(t, cols)[fname]
    edges = ca.edge_sets(slot, cols[slot])[ename]
    got = t.ix.column_histogram(slot, edges.view(np.uint32), f, host=True)
    assert same_hist(got, ca.expected_histogram(cols[slot], mask, edges))
    assert not same_hist(got, ca.expected_histogram(cols[slot], mask, edges, wrong=wrong))


@pytest.mark.parametrize("wrong", ca.TOP_WRONG)
def test_a_wrong_top_reading_differs_from_the_host_twin(wrong):
    n_docs, slot, fname, top, order = ca.TOP_WRONG_CASES[wrong]
    t, cols = ca.make(n_docs, "u16_f16")
    f, mask = native_filters(t, cols)[fname]
    got = t.ix.column_top(slot, top, order, f, host=True)
    assert same_top(got, ca.expected_top(cols[slot], mask, top, order))
    assert not same_top(got, ca.expected_top(cols[slot], mask, top, order, wrong=wrong))


# ---------------------------------------------------------------------------------------------------------------------
# the order of checks and each status
# ---------------------------------------------------------------------------------------------------------------------
def _raw_stats(ix, slot, flt, device, idx=True, out=True):
    L = _native.lib()
    s = ColumnStats()
    fh = None if flt is None else flt.h
    if device is None:
        st = L.sgpu_column_stats_host(ix.h if idx else None, slot, fh, 1, C.byref(s) if out else None)
    else:
        st = L.sgpu_column_stats(ix.h if idx else None, int(device), slot, fh, C.byref(s) if out else None)
    return st, L.sgpu_last_error().decode()


def _raw_hist(ix, slot, flt, edges, n_edges, device, null=None):
    L = _native.lib()
    counts = np.zeros(4100, np.uint64)
    outs = [_p(counts)] + [C.pointer(C.c_uint64(0)) for _ in range(4)]
    args = [ix.h, slot, None if flt is None else flt.h, _p(edges), n_edges]
    if null == "idx":
        args[0] = None
    elif null == "edges":
        args[3] = None
    elif null is not None:
        outs[null] = None
    if device is None:
        st = L.sgpu_column_histogram_host(*args, 1, *outs)
    else:
        st = L.sgpu_column_histogram(args[0], int(device), *args[1:], *outs)
    return st, L.sgpu_last_error().decode()


def _raw_top(ix, slot, flt, top, order, device, null=None):
    L = _native.lib()
    ids, vals = np.zeros(1024, np.uint32), np.zeros(1024, np.uint32)
    outs = [_p(ids), _p(vals), C.pointer(C.c_uint32(0)), C.pointer(C.c_uint64(0)), C.pointer(C.c_uint64(0))]
    if null is not None:
        outs[null] = None
    fh = None if flt is None else flt.h
    if device is None:
        st = L.sgpu_column_top_host(ix.h, slot, fh, top, order, 1, *outs)
    else:
        st = L.sgpu_column_top(ix.h, int(device), slot, fh, top, order, *outs)
    return st, L.sgpu_last_error().decode()


@pytest.mark.parametrize("device", [None, 0])       # the device call runs the same checks before it looks for a replica
def test_argument_checks_in_the_headers_order(device):
    t, cols = ca.make(33, "u16_f16")
    foreign = cc.make(32, "u16_f16").ix.make_filter([0])
    end = OK if device is None else EDEVICE          # the index is not uploaded
    # stats: 1. null idx / out, the slot - before the filter's index; 2. the filter; 3. the device
    assert _raw_stats(t.ix, cc.U, foreign, device, idx=False)[0] == EINVAL
    assert _raw_stats(t.ix, cc.U, foreign, device, out=False)[0] == EINVAL
    st, msg = _raw_stats(t.ix, 16, foreign, device)
    assert st == EINVAL and "slot 16" in msg
    st, msg = _raw_stats(t.ix, 9, foreign, device)
    assert st == EINVAL and "holds no column" in msg
    st, msg = _raw_stats(t.ix, cc.U, foreign, device)
    assert st == EINVAL and "another index" in msg
    for slot in ca.SLOTS:
        assert _raw_stats(t.ix, slot, None, device)[0] == end
    # histogram: 1. nulls and the slot; 2. n_edges (SGPU_ELIMIT); 3. the edges, the first offending one named; 4. the filter
    good = np.array([1, 2, 3], np.uint32)
    bad = np.array([3, 3], np.uint32)
    for null in ("idx", "edges", 0, 1, 2, 3, 4):
        assert _raw_hist(t.ix, 16, foreign, bad, 1, device, null=null)[0] == EINVAL
    st, msg = _raw_hist(t.ix, 16, foreign, bad, 1, device)
    assert st == EINVAL and "slot 16" in msg
    assert _raw_hist(t.ix, 9, foreign, bad, 1, device)[0] == EINVAL
    many = np.arange(5000, dtype=np.uint32)
    many[7] = 7000                                                      # a descending pair too: the count is judged first
    for n in (0, 1, 4098):
        st, msg = _raw_hist(t.ix, cc.U, foreign, many, n, device)
        assert st == ELIMIT and "4097" in msg, n
    st, msg = _raw_hist(t.ix, cc.U, foreign, many, 4097, device)
    assert st == EINVAL and "edge 8" in msg                             # 8 is not above 7000
    st, msg = _raw_hist(t.ix, cc.U, foreign, bad, 2, device)
    assert st == EINVAL and "edge 1" in msg                             # equal
    st, msg = _raw_hist(t.ix, cc.I, foreign, cc.bits_of([-1, 5, 4], cc.I32), 3, device)
    assert st == EINVAL and "edge 2" in msg                             # descending
    assert _raw_hist(t.ix, cc.I, foreign, cc.bits_of([5, -1], cc.I32), 2, device)[0] == EINVAL    # ascending only as unsigned
    st, msg = _raw_hist(t.ix, cc.F, foreign, cc.bits_of([0.0, 1.0, np.nan, 3.0], cc.F32), 4, device)
    assert st == EINVAL and "edge 2" in msg and "NaN" in msg
    st, msg = _raw_hist(t.ix, cc.F, foreign, cc.bits_of([-1.0, -0.0, 0.0, 3.0], cc.F32), 4, device)
    assert st == EINVAL and "edge 2" in msg                             # the -0.0, +0.0 pair is one value
    st, msg = _raw_hist(t.ix, cc.F, foreign, cc.bits_of([-2.0, -1.0], cc.F32), 2, device)    # ascending as floats, not as bits
    assert st == EINVAL and "another index" in msg
    assert _raw_hist(t.ix, cc.U, None, np.array([0x7fc00000, 0xffc00000], np.uint32), 2, device)[0] == end   # NaN patterns are numbers on u32
    st, msg = _raw_hist(t.ix, cc.U, foreign, good, 3, device)
    assert st == EINVAL and "another index" in msg
    assert _raw_hist(t.ix, cc.U, None, good, 3, device)[0] == end
    assert _raw_hist(t.ix, cc.U, None, np.arange(4097, dtype=np.uint32), 4097, device)[0] == end
    # top: 1. nulls, t, order, the slot; 2. the filter
    for null in range(5):
        assert _raw_top(t.ix, 16, foreign, 0, 2, device, null=null)[0] == EINVAL
    for top in (0, 1025):
        st, msg = _raw_top(t.ix, 16, foreign, top, 2, device)
        assert st == EINVAL and "1024" in msg
    st, msg = _raw_top(t.ix, 16, foreign, 5, 2, device)
    assert st == EINVAL and "order" in msg
    st, msg = _raw_top(t.ix, 16, foreign, 5, 1, device)
    assert st == EINVAL and "slot 16" in msg
    st, msg = _raw_top(t.ix, 9, foreign, 5, 1, device)
    assert st == EINVAL and "holds no column" in msg
    st, msg = _raw_top(t.ix, cc.F, foreign, 5, 1, device)
    assert st == EINVAL and "another index" in msg
    for top in (1, 1024):
        assert _raw_top(t.ix, cc.F, None, top, 0, device)[0] == end


# ---------------------------------------------------------------------------------------------------------------------
# the Python classes
# ---------------------------------------------------------------------------------------------------------------------
def test_python_methods_against_the_native_ones():
    ids, vecs, _ = read_jsonl(os.path.join(GOLD_TOY, "documents.jsonl"))
    ix = seismic_amd.SeismicIndex.build(os.path.join(GOLD_TOY, "documents.jsonl"), n_postings=50, centroid_fraction=0.2, upload=False)
    n = len(ids)
    price = (np.arange(n, dtype=np.float32) * 0.5) % 7
    price[3] = np.nan
    ts = (np.arange(n, dtype=np.int32) * 37) % 101 - 50
    ix.set_column("tenant", np.arange(n, dtype=np.uint32) % 3)
    ix.set_column("price", price)
    ix.set_column("ts", ts)
    f = ix.make_column_filter(must=[("tenant", [1, 2])], device=False)
    mask = np.arange(n) % 3 != 0
    for flt, m in ((None, np.ones(n, bool)), (f, mask)):
        # stats
        s = ix.stats("price", filter=flt, device=False)
        ok = m & ~np.isnan(price)
        slot = ix._column("price")[0]
        raw = ix._ix.column_stats(slot, None if flt is None else flt._f, host=True)
        assert s["docs"] == int(m.sum()) and s["valid"] == int(ok.sum()) == raw["valid"]
        assert s["min"] == float(price[ok].min()) and s["max"] == float(price[ok].max()) and s["sum"] == raw["sum"]
        assert s["mean"] == s["sum"] / s["valid"] and abs(s["sum"] - float(price[ok].astype(np.float64).sum())) < 1e-6
        s = ix.stats("ts", filter=flt, device=False)
        assert (s["min"], s["max"], s["sum"]) == (int(ts[m].min()), int(ts[m].max()), int(ts[m].astype(np.int64).sum()))
        assert isinstance(s["sum"], int) and s["mean"] == s["sum"] / s["valid"]
        # histogram
        edges = [0.0, 1.0, 2.5, 6.5]
        h = ix.histogram("price", edges, filter=flt, device=False)
        want = ca.expected_histogram(price, m, np.array(edges, np.float32))
        assert h["counts"].tolist() == want[0].tolist() and (h["below"], h["above"], h["nan"], h["docs"]) == tuple(want[1:])
        assert h["counts"].tolist() == np.histogram(price[ok], edges)[0].tolist()
        h = ix.histogram("ts", np.array([-50, 0, 50], np.int32), filter=flt, device=False)
        assert h["counts"].tolist() == np.histogram(ts[m], [-50, 0, 50])[0].tolist() and h["below"] == 0 and h["above"] == 0
        # top_by
        for desc in (False, True):
            got_ids, got_vals = ix.top_by("ts", k=7, descending=desc, filter=flt, device=False)
            want = ca.expected_top(ts, m, 7, int(desc))
            assert got_ids == [ids[i] for i in want[0].tolist()] and got_vals.dtype == np.int32
            assert got_vals.tolist() == ts[want[0]].tolist()
    got_ids, got_vals = ix.top_by("price", k=1024, device=False)
    assert len(got_ids) == min(n - 1, 1024) and ids[3] not in got_ids and not np.isnan(got_vals).any()
    empty = ix.make_column_filter(must=[("tenant", [9])], device=False)
    s = ix.stats("price", filter=empty, device=False)
    assert (s["docs"], s["valid"], s["min"], s["max"], s["mean"]) == (0, 0, None, None, None)
    for bad in ([0, 1.5], [0, 2 ** 40], [-1, 5]):
        with pytest.raises(ValueError):
            ix.histogram("tenant", bad, device=False)
    with pytest.raises(ValueError):
        ix.histogram("price", [0.0, float("nan")], device=False)
    with pytest.raises(ValueError):
        ix.stats("no-such-column", device=False)
    with pytest.raises(_native.SeismicHipError) as e:
        ix.histogram("price", [1.0, 1.0], device=False)
    assert e.value.status == EINVAL
