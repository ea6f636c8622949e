"""Document columns without a device: both host twins (sgpu_filter_create_columns_host, sgpu_facet_counts_host) against the
numpy restatement of tests/column_cases.py, word for word and row for row on every case; each wrong reading of the
contract differing from the host twin on the case named for it; the argument checks in the header's order;
sgpu_index_set_column / get_column (replace, retype, drop, wrong n, the bits round trip, nothing saved); and the Python
classes with device=False."""
import ctypes as C
import os

import numpy as np
import pytest

import column_cases as cc
import seismic_amd
from seismic_amd import _native
from seismic_amd.index import read_jsonl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD_TOY = os.path.join(ROOT, "tests", "golden", "toy")
OK, EINVAL, EDEVICE, ELIMIT = 0, 1, 2, 5


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def test_header_declares_the_calls_and_the_abi_version_stays():
    text = open(os.path.join(ROOT, "include", "seismic_hip.h")).read()
    for decl in ("sgpu_status sgpu_index_set_column(sgpu_index* idx, uint32_t slot, uint32_t type, const void* values, uint64_t n);",
                 "sgpu_status sgpu_index_get_column(const sgpu_index* idx, uint32_t slot,",
                 "sgpu_status sgpu_filter_create_columns(sgpu_index* idx, uint32_t replica,",
                 "sgpu_status sgpu_filter_create_columns_host(sgpu_index* idx,",
                 "sgpu_status sgpu_facet_counts(sgpu_index* idx, uint32_t replica, uint32_t slot,",
                 "sgpu_status sgpu_facet_counts_host(const sgpu_index* idx, uint32_t slot,",
                 "#define SGPU_MAX_COLUMNS 16", "enum { SGPU_COL_U32 = 0, SGPU_COL_I32 = 1, SGPU_COL_F32 = 2 };",
                 "enum { SGPU_COLOP_RANGE = 0, SGPU_COLOP_IN = 1 };"):
        assert decl in text, decl
    assert text.index("---- term filters:") < text.index("---- document columns:")
    assert "NOT part of the index file" in text
    assert "sgpu_debug_column_stats" in open(os.path.join(ROOT, "include", "seismic_hip_testing.h")).read()
    L = _native.lib()
    for name in ("sgpu_index_set_column", "sgpu_index_get_column", "sgpu_filter_create_columns", "sgpu_filter_create_columns_host",
                 "sgpu_facet_counts", "sgpu_facet_counts_host", "sgpu_debug_column_stats"):
        assert hasattr(L, name), name
    assert L.sgpu_abi_version() == 4
    assert C.sizeof(seismic_amd._abi.ColumnClause) == 32 == _native.COLUMN_CLAUSE_DTYPE.itemsize


def test_every_wrong_reading_changes_its_case():
    cc.check()


# ---------------------------------------------------------------------------------------------------------------------
# the column filter
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_docs,variant", cc.SHAPES)
def test_host_filter_equals_the_restatement(n_docs, variant):
    t = cc.make(n_docs, variant)
    sets = cc.clause_sets(t)
    for name, (clauses, ms, sv) in sets.items():
        want = cc.expected_bits(t.cols, clauses, ms, sv)
        for threads in (1, 4):
            f = t.ix.make_column_filter(clauses, ms, sv, host=True, num_threads=threads)
            assert cc.bits_diff(f.bits(), want) is None, (name, threads, cc.bits_diff(f.bits(), want))
            assert f.count == cc.popcount(want), name
    for wname, allowed in cc.within_sets(n_docs).items():
        wf = t.ix.make_filter(allowed)
        for name, (clauses, ms, sv) in sets.items():              # every clause set with every `within` set
            want = cc.expected_bits(t.cols, clauses, ms, sv, allowed)
            f = t.ix.make_column_filter(clauses, ms, sv, within=wf, host=True)
            assert cc.bits_diff(f.bits(), want) is None, (name, wname)
            assert f.count == cc.popcount(want)


def test_the_named_sets_are_what_their_names_say():
    t = cc.make(65, "u16_f16")
    sets, f = cc.clause_sets(t), t.cols[cc.F]

    def ids(name):
        clauses, ms, sv = sets[name]
        return set(t.ix.make_column_filter(clauses, ms, sv, host=True).ids().tolist())
    assert ids("none") == ids("u_full") == ids("i_full") == set(range(65))
    assert ids("u_reversed") == ids("in_empty") == ids("should3_min4") == set()
    assert ids("f_full") == set(np.flatnonzero(~np.isnan(f)).tolist()) and len(ids("f_full")) < 65
    assert ids("must_not_f_full") == set(np.flatnonzero(np.isnan(f)).tolist())
    assert ids("f_zero") == set(np.flatnonzero(f == 0).tolist()) and {2, 3} <= ids("f_zero")      # -0.0 and +0.0
    assert 2 in ids("in_f") and 4 in ids("in_f") and 6 in ids("in_f")                             # -0.0, the subnormal, +inf
    assert ids("u_top") == set(np.flatnonzero(t.cols[cc.U] == 0xffffffff).tolist()) != set()
    assert ids("i_low") == set(np.flatnonzero(t.cols[cc.I] < 0).tolist())


@pytest.mark.parametrize("wrong", cc.WRONG)
def test_a_wrong_reading_differs_from_the_host_twin(wrong):
    n_docs, name, wname = cc.WRONG_CASES[wrong]
    t = cc.make(n_docs, "u16_f16")
    clauses, ms, sv = cc.clause_sets(t)[name]
    within = None if wname is None else cc.within_sets(n_docs)[wname]
    wf = None if within is None else t.ix.make_filter(within)
    got = t.ix.make_column_filter(clauses, ms, sv, within=wf, host=True).bits()
    assert cc.bits_diff(got, cc.expected_bits(t.cols, clauses, ms, sv, within)) is None
    assert cc.bits_diff(got, cc.expected_bits(t.cols, clauses, ms, sv, within, wrong=wrong)) is not None


def _raw_filter(ix, clauses, n_clauses, ms, sv, n_sv, within=None, out=True, idx=True, device=None):
    L = _native.lib()
    h = C.c_void_p()
    args = [ix.h if idx else None] + ([] if device is None else [int(device)])
    args += [_p(clauses), n_clauses, ms, _p(sv), n_sv, None if within is None else within.h]
    if device is None:
        st = L.sgpu_filter_create_columns_host(*args, 1, C.byref(h) if out else None)
    else:
        st = L.sgpu_filter_create_columns(*args, C.byref(h) if out else None)
    if st == OK:
        L.sgpu_filter_destroy(h)
    return st, L.sgpu_last_error().decode()


@pytest.mark.parametrize("device", [None, 0])       # the device call runs the same checks before it looks for a replica
def test_filter_argument_checks_in_the_headers_order(device):
    t = cc.make(33, "u16_f16")
    other = cc.make(32, "u16_f16")
    foreign = other.ix.make_filter([0])
    nan = int(cc.bits_of(np.nan, cc.F32))
    good = [cc.rng_clause(cc.U, cc.MUST, cc.U32, 0, 5)]
    sv = np.arange(4, dtype=np.uint32)

    def run(rows, n=None, ms=0, values=sv, n_sv=None, **kw):
        cl = _native.column_clauses(rows) if rows is not None else None
        return _raw_filter(t.ix, cl, len(rows) if n is None else n, ms, values, (0 if values is None else len(values)) if n_sv is None else n_sv,
                           device=device, **kw)
    # 1. null arguments - before anything else, also with clauses that are wrong in every later way
    assert run([(99, 9, 9, 0, 0, 0, 0)], idx=False)[0] == EINVAL
    assert run([(99, 9, 9, 0, 0, 0, 0)], out=False)[0] == EINVAL
    assert run(None, n=3)[0] == EINVAL and "null" in run(None, n=3)[1]
    assert run([], values=None, n_sv=2)[0] == EINVAL
    # 2. the clauses, the first offending one named - before the limits and before `within`
    many = [cc.rng_clause(cc.U, cc.MUST, cc.U32, 0, 5)] * 70
    for bad, word in (((cc.U, 3, cc.RANGE, 0, 0, 0, 0), "occur"), ((cc.U, cc.MUST, 2, 0, 0, 0, 0), "op"),
                      ((16, cc.MUST, cc.RANGE, 0, 0, 0, 0), "slot 16"), ((9, cc.MUST, cc.RANGE, 0, 0, 0, 0), "holds no column"),
                      ((cc.F, cc.MUST, cc.RANGE, nan, 0, 0, 0), "NaN"), ((cc.F, cc.MUST, cc.RANGE, 0, nan, 0, 0), "NaN"),
                      ((cc.U, cc.MUST, cc.IN, 0, 0, 3, 2), "set_begin")):
        st, msg = run(many[:66] + [bad] + many[:3], within=foreign)
        assert st == EINVAL and "clause 66" in msg and word in msg, (bad, msg)
    st, msg = run([(cc.F, cc.SHOULD, cc.IN, 0, 0, 1, 2)], values=np.array([nan, 5, nan, 7], np.uint32))
    assert st == EINVAL and "clause 0" in msg and "NaN" in msg
    assert run([(cc.U, cc.MUST, cc.RANGE, nan, nan, 0, 0), (cc.U, cc.SHOULD, cc.IN, 0, 0, 0, 1)], values=np.array([nan], np.uint32))[0] == (
        OK if device is None else EDEVICE)      # a NaN pattern is a number on a u32 column
    assert run([(cc.U, cc.MUST, cc.IN, 0, 0, 4, 0)])[0] == (OK if device is None else EDEVICE)    # an empty set at the end
    # 3. the limits - before `within`
    st, msg = run(many[:65], within=foreign)
    assert st == ELIMIT and "65" in msg and "64" in msg
    st, msg = run(good, values=np.zeros(8193, np.uint32), within=foreign)
    assert st == ELIMIT and "8193" in msg and "8192" in msg
    # 4. a filter of another index
    st, msg = run(many[:64], within=foreign)
    assert st == EINVAL and "another index" in msg
    # 5. the device call on an index that is not uploaded
    assert run(many[:64], values=np.zeros(8192, np.uint32))[0] == (OK if device is None else EDEVICE)


# ---------------------------------------------------------------------------------------------------------------------
# facet counts
# ---------------------------------------------------------------------------------------------------------------------
def _same_rows(got, want):
    return (np.array_equal(got[0], want[0]) and got[0].dtype == np.uint32 and np.array_equal(got[1], want[1]) and got[2] == want[2]
            and got[3] == want[3])


def facet_filters(t):
    """name -> (NativeFilter or None, bool mask or None): all documents, the `within` sets and a column filter."""
    out = {"all": (None, None)}
    for wname, allowed in cc.within_sets(t.n_docs).items():
        out[wname] = (t.ix.make_filter(allowed), allowed)
    clauses, ms, sv = cc.clause_sets(t)["three_slots"]
    f = t.ix.make_column_filter(clauses, ms, sv, host=True)
    out["column_filter"] = (f, np.unpackbits(f.bits().view(np.uint8), bitorder="little")[:t.n_docs].astype(bool))
    return out


@pytest.mark.parametrize("n_docs", cc.FACET_N_DOCS)
def test_host_facets_equal_the_restatement(n_docs):
    t = cc.fresh(n_docs, "u16_f16")
    filters = facet_filters(t)
    for cname, col in cc.facet_columns(n_docs).items():
        t.ix.set_column(cc.FACET_SLOT, col)
        for fname, (f, mask) in filters.items():
            for top in cc.FACET_T:
                want = cc.expected_facets(col, mask, top)
                for threads in (1, 4):
                    got = t.ix.facet_counts(cc.FACET_SLOT, f, top, host=True, num_threads=threads)
                    assert _same_rows(got, want), (cname, fname, top, threads)
    assert t.ix.facet_counts(cc.FACET_SLOT, filters["empty"][0], 5, host=True)[2:] == (0, 0)


@pytest.mark.parametrize("wrong", cc.FACET_WRONG)
def test_a_wrong_facet_reading_differs_from_the_host_twin(wrong):
    n_docs, cname, wname, top = cc.FACET_WRONG_CASES[wrong]
    t = cc.fresh(n_docs, "u16_f16")
    col = cc.facet_columns(n_docs)[cname]
    t.ix.set_column(cc.FACET_SLOT, col)
    mask = None if wname is None else cc.within_sets(n_docs)[wname]
    f = None if mask is None else t.ix.make_filter(mask)
    got = t.ix.facet_counts(cc.FACET_SLOT, f, top, host=True)
    assert _same_rows(got, cc.expected_facets(col, mask, top))
    assert not _same_rows(got, cc.expected_facets(col, mask, top, wrong=wrong))


def _raw_facets(ix, slot, flt, top, null=None, device=None):
    L = _native.lib()
    vals, cnts = np.zeros(1024, np.uint32), np.zeros(1024, np.uint64)
    n, distinct, docs = C.c_uint32(0), C.c_uint64(0), C.c_uint64(0)
    outs = [_p(vals), _p(cnts), C.byref(n), C.byref(distinct), C.byref(docs)]
    if null is not None:
        outs[null] = None
    fh = None if flt is None else flt.h
    if device is None:
        st = L.sgpu_facet_counts_host(ix.h, slot, fh, top, 1, *outs)
    else:
        st = L.sgpu_facet_counts(ix.h, int(device), slot, fh, top, *outs)
    return st, L.sgpu_last_error().decode()


@pytest.mark.parametrize("device", [None, 0])
def test_facet_argument_checks_in_the_headers_order(device):
    t = cc.fresh(33, "u16_f16")
    foreign = cc.make(32, "u16_f16").ix.make_filter([0])
    over = np.zeros(33, np.uint32)
    over[5] = cc.MAX_BINS                                          # the smallest maximum that is over the limit
    t.ix.set_column(6, over)
    t.ix.set_column(7, over - over + np.uint32(cc.MAX_BINS - 1))    # the largest one that is not
    end = OK if device is None else EDEVICE
    # 1. null outputs, t, the slot, the type - each before the filter's index and the limit
    for null in range(5):
        assert _raw_facets(t.ix, 6, foreign, 5, null=null, device=device)[0] == EINVAL
    for top in (0, 1025):
        st, msg = _raw_facets(t.ix, 6, foreign, top, device=device)
        assert st == EINVAL and "1024" in msg
    assert _raw_facets(t.ix, 16, foreign, 5, device=device)[0] == EINVAL
    st, msg = _raw_facets(t.ix, 9, foreign, 5, device=device)
    assert st == EINVAL and "holds no column" in msg
    for slot in (cc.I, cc.F):
        st, msg = _raw_facets(t.ix, slot, foreign, 5, device=device)
        assert st == EINVAL and "U32" in msg
    # 2. a filter of another index - before the limit
    st, msg = _raw_facets(t.ix, 6, foreign, 5, device=device)
    assert st == EINVAL and "another index" in msg
    # 3. the limit, named
    st, msg = _raw_facets(t.ix, 6, None, 5, device=device)
    assert st == ELIMIT and "4194304" in msg
    assert _raw_facets(t.ix, 7, None, 1024, device=device)[0] == end
    assert _raw_facets(t.ix, cc.U, None, 1, device=device)[0] == ELIMIT     # 0xffffffff is stored there


# ---------------------------------------------------------------------------------------------------------------------
# the columns themselves
# ---------------------------------------------------------------------------------------------------------------------
def test_set_column_replaces_retypes_drops_and_checks_n():
    t = cc.fresh(65, "u16_f16")
    ix, L = t.ix, _native.lib()
    assert ix.get_column(9) is None
    a = np.arange(65, dtype=np.uint32)
    ix.set_column(9, a)
    rng = [cc.rng_clause(9, cc.MUST, cc.U32, 10, 19)]
    assert ix.make_column_filter(rng, host=True).ids().tolist() == list(range(10, 20))
    old = ix.make_column_filter(rng, host=True)
    ix.set_column(9, a[::-1].copy())                                # replaced: the next call sees the new values ...
    assert ix.make_column_filter(rng, host=True).ids().tolist() == list(range(45, 55))
    assert old.ids().tolist() == list(range(10, 20))                # ... and a filter made earlier is a bitmap
    ix.set_column(9, (a.astype(np.int32) - 30))                     # retyped: the bounds are now i32 patterns
    assert ix.get_column(9).dtype == np.int32
    assert ix.make_column_filter([cc.rng_clause(9, cc.MUST, cc.I32, -5, 2)], host=True).ids().tolist() == list(range(25, 33))
    st = L.sgpu_facet_counts_host(ix.h, 9, None, 1, 1, _p(np.zeros(1, np.uint32)), _p(np.zeros(1, np.uint64)), C.byref(C.c_uint32()),
                                  C.byref(C.c_uint64()), C.byref(C.c_uint64()))
    assert st == EINVAL                                             # no facets of an i32 column
    ix.set_column(9, np.linspace(-1, 1, 65).astype(np.float32))
    assert ix.get_column(9).dtype == np.float32
    for n in (0, 64, 66):                                           # a wrong n; NULL values with n != 0
        assert L.sgpu_index_set_column(ix.h, 9, 0, _p(np.zeros(66, np.uint32)), n) == EINVAL
    assert L.sgpu_index_set_column(ix.h, 9, 0, None, 65) == EINVAL
    assert L.sgpu_index_set_column(ix.h, 16, 0, _p(np.zeros(65, np.uint32)), 65) == EINVAL
    assert L.sgpu_index_set_column(ix.h, 9, 3, _p(np.zeros(65, np.uint32)), 65) == EINVAL
    assert L.sgpu_index_set_column(None, 9, 0, _p(np.zeros(65, np.uint32)), 65) == EINVAL
    assert ix.get_column(9).dtype == np.float32                     # the failed calls changed nothing
    ix.set_column(9, None)                                          # dropped
    assert ix.get_column(9) is None
    st, msg = _raw_filter(ix, _native.column_clauses(rng), 1, 0, None, 0)
    assert st == EINVAL and "holds no column" in msg
    ix.set_column(9, None)                                          # dropping an empty slot is not an error
    assert ix.device_bytes() == 0                                   # never uploaded: nothing on a device


def test_get_column_round_trips_the_bits():
    t = cc.make(65, "u16_f16")
    for slot, col in t.cols.items():
        got = t.ix.get_column(slot)
        assert got.dtype == col.dtype and np.array_equal(got.view(np.uint32), col.view(np.uint32))
    f = t.ix.get_column(cc.F).view(np.uint32)
    assert f[8] == 0xffc00123 and f[2] == 0x80000000                # a NaN's payload and the sign of -0.0


def test_columns_are_not_saved(tmp_path):
    t = cc.make(65, "u16_f16")
    path = str(tmp_path / "index.bin")
    t.ix.save(path)
    back = _native.NativeIndex.load(path)
    assert all(back.get_column(s) is None for s in range(16))
    assert all(t.ix.convert(1).get_column(s) is None for s in range(16))
    assert t.ix.get_column(cc.U) is not None
    back.close()


# ---------------------------------------------------------------------------------------------------------------------
# the Python classes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", ["SeismicIndex", "SeismicIndexDotVByte"])
def test_python_columns_on_the_host(cls):
    ids, vecs, _ = read_jsonl(os.path.join(GOLD_TOY, "documents.jsonl"))
    _, qvecs, _ = read_jsonl(os.path.join(GOLD_TOY, "queries.jsonl"))
    qc = [np.array(list(v.keys())) for v in qvecs]
    qv = [np.array(list(v.values()), np.float32) for v in qvecs]
    ix = getattr(seismic_amd, cls).build(os.path.join(GOLD_TOY, "documents.jsonl"), n_postings=50, centroid_fraction=0.2, upload=False)
    n = len(ids)
    tenant = {d: i % 3 for i, d in enumerate(ids)}
    ix.set_column("tenant", tenant)                                 # the dict form
    ix.set_column("price", np.arange(n, dtype=np.float32) * 0.5)    # the array form, in the index's order
    ix.set_column("ts", {ids[0]: -5, ids[1]: 7})                    # a negative value: i32; the others get 0
    with pytest.raises(ValueError):
        ix.set_column("x", {"no-such-document": 1})
    with pytest.raises(ValueError):
        ix.set_column("x", [1, 2, 3])
    f = ix.make_column_filter(must=[("tenant", [1, 2]), ("price", None, 4.0)], must_not=[("ts", 1, None)], device=False)
    want = [i for i in range(n) if i % 3 in (1, 2) and i * 0.5 <= 4.0 and not i == 1]
    assert isinstance(f, seismic_amd.index.SeismicFilter) and f.count == len(want)
    assert np.flatnonzero(np.unpackbits(f.bits().view(np.uint8), bitorder="little")).tolist() == want
    assert ix.make_column_filter(should=[("ts", -5, -5), ("ts", [7])], min_should=1, device=False).count == 2
    assert ix.make_column_filter(must=[("ts", None, None)], within=f, device=False).count == f.count
    assert ix.make_column_filter(must=[("tenant", -3, 0.5)], device=False).count == len([i for i in range(n) if i % 3 == 0])
    assert ix.make_column_filter(must=[("tenant", 5e9, None)], device=False).count == 0
    assert ix.make_column_filter(must=[("tenant", [np.inf, -np.inf, np.nan, 0.5, 1.0, -4, 2 ** 40])], device=False).count == len(
        [i for i in range(n) if i % 3 == 1])                       # set values the column's type cannot hold are dropped
    with pytest.raises(ValueError):
        ix.make_column_filter(must=[("no-such-column", 0, 1)], device=False)
    rows, distinct, docs = ix.facets("tenant", top=2, device=False)
    counts = np.bincount([i % 3 for i in range(n)])
    order = sorted(range(3), key=lambda v: (-counts[v], v))[:2]
    assert rows == [(v, int(counts[v])) for v in order] and distinct == 3 and docs == n
    rows, distinct, docs = ix.facets("tenant", filter=f, top=10, device=False)
    assert sum(c for _, c in rows) == docs == f.count and distinct == 2
    # groups="name": the keys of a u32 column are the explicit keys
    lists = [list(ids[q % n:q % n + 12]) for q in range(len(qc))]
    explicit = [[tenant[d] for d in row] for row in lists]
    assert ix.batch_collapse(qc, qv, lists, None, 3, device=False, groups="tenant") == ix.batch_collapse(qc, qv, lists, explicit, 3, device=False)
    with pytest.raises(ValueError):
        ix.batch_collapse(qc, qv, lists, None, 3, device=False, groups="price")     # not a u32 column
    with pytest.raises(ValueError):
        ix.batch_collapse(qc, qv, lists, None, 3, device=False)                     # set_groups(None) is unchanged: no keys
    # a 17th name; a dropped one frees its slot
    for j in range(13):
        ix.set_column("extra%d" % j, np.zeros(n, np.uint32))
    with pytest.raises(ValueError):
        ix.set_column("seventeenth", np.zeros(n, np.uint32))
    ix.set_column("tenant", np.ones(n, np.uint32))                  # an existing name is replaced, not counted again
    ix.set_column("extra0", None)
    ix.set_column("seventeenth", np.zeros(n, np.uint32))
    assert ix.facets("tenant", device=False) == ([(1, n)], 1, n)


def test_python_columns_on_the_raw_classes(tmp_path):
    t = cc.make(65, "u16_f16")
    path = str(tmp_path / "raw.bin")
    t.ix.save(path)
    ix = seismic_amd.SeismicIndexRaw.load(path, upload=False)
    ix.set_column("u", {3: 9, 64: 9})
    assert ix.make_column_filter(must=[("u", [9])], device=False).count == 2
    assert ix.facets("u", device=False) == ([(0, 63), (9, 2)], 2, 65)
    with pytest.raises(ValueError):
        ix.set_column("u", {65: 1})
