"""Seeded inputs and the reference for the tests of document columns (test_column_cpu.py, test_gpu_columns.py): column
filters and facet counts. TEST INFRASTRUCTURE, pure numpy apart from the index build.

expected_bits() and expected_facets() restate, from the text of include/seismic_hip.h alone, what
sgpu_filter_create_columns[_host] and sgpu_facet_counts[_host] return. A RANGE clause matches d iff lo <= v[d] <= hi in the
order of the column's type (numpy's own uint32 / int32 / float32 comparisons: NaN compares false, -0.0 == +0.0), an IN clause
iff v[d] equals one of its values; A = every MUST matches, no MUST_NOT matches, at least min_should SHOULD clauses match,
intersected with `within`. Facets: the t values with the most documents, count descending then value ascending, only
values that occur. Each has one switch per wrong reading (WRONG, FACET_WRONG); check() shows on the CPU that every switch
changes the answer on its named case.

Index shapes (make(n_docs, variant)): n_docs in N_DOCS - the word edges (31 .. 33), the edges of a wavefront's 64 documents
(63 .. 65), the edges of the W = 8192 documents a workgroup of column_filter_kernel takes (W - 1, W, W + 1) and two
workgroups and a tail (2 W + 5). Columns do not depend on the postings: document d stores component d % 7 (and, every
fifth, the last component of the vocabulary: 70000 components in the u32 variant).
Columns of every index, by slot: U (u32, with 0 and 0xffffffff), I (i32, with INT_MIN, -1, 0, INT_MAX), F (f32, with
-inf, -1.5, -0.0, +0.0, the subnormal 2^-149, 65504, +inf and NaNs of both signs); the first documents hold the special
values in that order, so an index of one document has one.
"""
import functools

import numpy as np

from seismic_amd import _native
from seismic_amd._abi import BuildConfig
from term_filter_cases import bits_diff, popcount, within_sets  # noqa: F401  (the tests use them through this module)

MUST, MUST_NOT, SHOULD = 0, 1, 2
RANGE, IN = 0, 1
U32, I32, F32 = 0, 1, 2
W = 8192                        # documents per workgroup of column_filter_kernel (kColDocsPerWg; the GPU tests check the hook)
LDS_BINS = 32768                # kFacetLdsBins
MAX_BINS = 1 << 22
MAX_CLAUSES, MAX_SET = 64, 8192
N_DOCS = (1, 31, 32, 33, 63, 64, 65, W - 1, W, W + 1, 2 * W + 5)
SHAPES = [(n, "u16_f16") for n in N_DOCS] + [(65, "u32_u8"), (2 * W + 5, "u32_u8")]
U, I, F = 0, 1, 2               # slots
DTYPES = {U32: np.uint32, I32: np.int32, F32: np.float32}
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1
SUBNORMAL = np.float32(2.0 ** -149)
NAN_NEG = np.array([0xffc00123], np.uint32).view(np.float32)[0]      # a negative NaN with a payload
U_SPECIAL = np.array([0, 0xffffffff, 7, 20], np.uint32)
I_SPECIAL = np.array([INT_MIN, -1, 0, INT_MAX, 5], np.int32)
F_SPECIAL = np.array([-np.inf, -1.5, -0.0, 0.0, SUBNORMAL, 65504.0, np.inf, np.nan, NAN_NEG, 1.0], np.float32)


def bits_of(x, type_):
    """The u32 bit pattern(s) of value(s) of a column type."""
    return np.asarray(x, DTYPES[type_]).view(np.uint32)


def _documents(n_docs, dim):
    d = np.arange(n_docs)
    last = d % 5 == 0
    off = np.zeros(n_docs + 1, np.uint64)
    off[1:] = np.cumsum(1 + last)
    comps = np.zeros(int(off[-1]), np.uint32)
    first = off[:-1].astype(np.int64)
    comps[first] = d % 7
    comps[first[last] + 1] = dim - 1
    return off, comps, np.full(len(comps), 1.0, np.float32)


def _columns(n_docs):
    rng = np.random.default_rng(9100 + n_docs)
    u = rng.integers(0, 40, n_docs).astype(np.uint32)
    i = rng.integers(-30, 30, n_docs).astype(np.int32)
    f = rng.choice(np.concatenate([F_SPECIAL, np.array([0.5, 2.5, -3.0, 100.0], np.float32)]), n_docs).astype(np.float32)
    for col, special in ((u, U_SPECIAL), (i, I_SPECIAL), (f, F_SPECIAL)):
        m = min(n_docs, len(special))
        col[:m] = special[:m]
        if n_docs > 2 * len(special):        # and again at the end: the last workgroup's tail holds specials too
            col[n_docs - m:] = special[:m]
    return {U: u, I: i, F: f}


class ColumnIndex:
    def __init__(self, n_docs, variant):
        self.n_docs, self.variant = n_docs, variant
        self.dim = 70000 if variant.startswith("u32") else 40
        off, comps, vals = _documents(n_docs, self.dim)
        base = _native.NativeIndex.build(4 if variant.startswith("u32") else 2, self.dim, off, comps, vals,
                                         BuildConfig.defaults(n_postings=16, centroid_fraction=0.1, summary_energy=0.4))
        self.ix = base if variant.endswith("f16") else base.convert(1)
        self.cols = _columns(n_docs)
        for slot, col in self.cols.items():
            self.ix.set_column(slot, col)


@functools.lru_cache(maxsize=None)
def make(n_docs, variant):
    """The index of (n_docs, variant) with its three columns set, built once per process and not uploaded."""
    return ColumnIndex(n_docs, variant)


def fresh(n_docs, variant):
    """A new index of the same documents and columns (for the tests that upload or change columns)."""
    return ColumnIndex(n_docs, variant)


# ---------------------------------------------------------------------------------------------------------------------
# the reference: column filters
# ---------------------------------------------------------------------------------------------------------------------
WRONG = ("half_open", "i32_unsigned", "f32_bits", "nan_matches", "in_as_min_max", "should_distinct_slot", "min_should_0_as_1",
         "must_not_ignored_without_must", "bits_past_end", "last_partial_workgroup_dropped", "within_or")


def _clause_match(col, clause, set_values, wrong):
    slot, occur, op, lo_bits, hi_bits, begin, count = clause
    type_ = {np.dtype(np.uint32): U32, np.dtype(np.int32): I32, np.dtype(np.float32): F32}[col.dtype]
    as_bits = (wrong == "i32_unsigned" and type_ == I32) or (wrong == "f32_bits" and type_ == F32)
    v = col.view(np.uint32) if as_bits else col
    typed = (lambda b: np.asarray(b, np.uint32)) if as_bits else (lambda b: np.asarray(b, np.uint32).view(col.dtype))
    if op == IN:
        s = typed(set_values[begin:begin + count])
        if wrong == "in_as_min_max":
            return (v >= s.min()) & (v <= s.max()) if len(s) else np.zeros(len(v), bool)
        if type_ == F32 and not as_bits:
            # IEEE equality on numbers: equal bit patterns once -0.0 is written as +0.0 (x + 0.0 does that); a NaN equals nothing
            m = np.isin((v + np.float32(0.0)).view(np.uint32), (s + np.float32(0.0)).view(np.uint32)) & ~np.isnan(v)
            return m | np.isnan(v) if wrong == "nan_matches" else m
        return np.isin(v, s)
    lo, hi = typed([lo_bits])[0], typed([hi_bits])[0]
    if wrong == "nan_matches":
        return ~(v < lo) & ~(v > hi)
    return (v >= lo) & ((v < hi) if wrong == "half_open" else (v <= hi))


def expected_bits(cols, clauses, min_should, set_values=(), within=None, wrong=None):
    """The words of the set (u32, ceil(n_docs / 32), at least one). cols: slot -> array of the column's dtype; clauses:
    (slot, occur, op, lo_bits, hi_bits, set_begin, set_count) rows; set_values: u32 bit patterns; within: bool [n_docs] or
    None. wrong: None, or one of WRONG -
      half_open                        a range is lo <= v < hi
      i32_unsigned                     an i32 column is compared as unsigned
      f32_bits                         an f32 column is compared as bit patterns
      nan_matches                      a stored NaN is inside every range and every set (!(v < lo) && !(v > hi))
      in_as_min_max                    an IN clause is read as the range min(values) .. max(values)
      should_distinct_slot             SHOULD matches are counted per distinct slot, not per clause
      min_should_0_as_1                min_should == 0 is read as 1
      must_not_ignored_without_must    MUST_NOT clauses are dropped when there is no MUST clause
      bits_past_end                    the bits of the last word at and past n_docs are treated as documents that match
      last_partial_workgroup_dropped   the documents past the last multiple of W are left out
      within_or                        `within` is OR-ed in instead of AND-ed"""
    assert wrong is None or wrong in WRONG
    n_docs = len(next(iter(cols.values())))
    n_words = max(-(-n_docs // 32), 1)
    set_values = np.asarray(set_values, np.uint32)
    must, should, banned = np.zeros(n_docs, np.int64), np.zeros(n_docs, np.int64), np.zeros(n_docs, bool)
    n_must = sum(1 for c in clauses if c[1] == MUST)
    by_slot = {}
    for c in clauses:
        hit = _clause_match(cols[c[0]], c, set_values, wrong)
        if c[1] == MUST:
            must += hit
        elif c[1] == MUST_NOT:
            banned |= hit
        elif wrong == "should_distinct_slot":
            by_slot[c[0]] = by_slot.get(c[0], np.zeros(n_docs, bool)) | hit
        else:
            should += hit
    for m in by_slot.values():
        should += m
    if wrong == "must_not_ignored_without_must" and n_must == 0:
        banned[:] = False
    need = 1 if (wrong == "min_should_0_as_1" and min_should == 0) else min_should
    ok = (must == n_must) & ~banned & (should >= need)
    if wrong == "last_partial_workgroup_dropped":
        ok[n_docs // W * W:] = False
    if within is not None:
        ok = (ok | within) if wrong == "within_or" else (ok & within)
    padded = np.zeros(n_words * 32, bool)
    padded[:n_docs] = ok
    if wrong == "bits_past_end" and n_must == 0 and need == 0 and within is None:
        padded[n_docs:] = True
    return np.packbits(padded, bitorder="little").view("<u4").astype(np.uint32)


def rng_clause(slot, occur, type_, lo, hi):
    b = bits_of([lo, hi], type_)
    return (slot, occur, RANGE, int(b[0]), int(b[1]), 0, 0)


def clause_sets(t):
    """name -> (clauses, min_should, set_values) for the index t (a ColumnIndex)."""
    rng = np.random.default_rng(31)
    big = rng.integers(0, 60, MAX_SET).astype(np.uint32)          # 8192 values, unsorted, with repeats
    big[17] = 0xffffffff
    f_set = bits_of([2.5, 0.0, np.inf, 2.5, SUBNORMAL], F32)        # +0.0 in the set: a stored -0.0 is in it
    i_set = bits_of([INT_MIN, 5, -1, 5], I32)
    out = {
        "none": ([], 0, []),
        "u_range": ([rng_clause(U, MUST, U32, 5, 20)], 0, []),       # 20 is a stored value: the closed upper bound
        "u_point": ([rng_clause(U, MUST, U32, 7, 7)], 0, []),
        "u_reversed": ([rng_clause(U, MUST, U32, 8, 7)], 0, []),
        "u_full": ([rng_clause(U, MUST, U32, 0, 0xffffffff)], 0, []),
        "u_top": ([rng_clause(U, MUST, U32, 0x80000000, 0xffffffff)], 0, []),
        "i_range": ([rng_clause(I, MUST, I32, -1, 10)], 0, []),
        "i_full": ([rng_clause(I, MUST, I32, INT_MIN, INT_MAX)], 0, []),
        "i_low": ([rng_clause(I, MUST, I32, INT_MIN, -1)], 0, []),
        "f_range": ([rng_clause(F, MUST, F32, -1.5, 2.5)], 0, []),
        "f_zero": ([rng_clause(F, MUST, F32, 0.0, 0.0)], 0, []),     # -0.0 and +0.0, nothing else
        "f_minus_zero_up": ([rng_clause(F, MUST, F32, -0.0, np.inf)], 0, []),
        "f_full": ([rng_clause(F, MUST, F32, -np.inf, np.inf)], 0, []),   # everything but the NaNs
        "f_subnormal": ([rng_clause(F, MUST, F32, SUBNORMAL, 65504.0)], 0, []),
        "f_negative": ([rng_clause(F, MUST, F32, -np.inf, -1.5)], 0, []),
        "in_empty": ([(U, MUST, IN, 0, 0, 0, 0)], 0, []),
        "in_one": ([(U, MUST, IN, 0, 0, 2, 1)], 0, [99, 98, 7]),
        "in_big": ([(U, MUST, IN, 0, 0, 0, MAX_SET)], 0, big),
        "in_f": ([(F, MUST, IN, 0, 0, 0, len(f_set))], 0, f_set),
        "in_i": ([(I, MUST, IN, 0, 0, 0, len(i_set))], 0, i_set),
        "in_u_spread": ([(U, MUST, IN, 0, 0, 0, 3)], 0, [3, 30, 3]),   # min .. max holds many values that are not in it
        "not_in": ([(U, MUST_NOT, IN, 0, 0, 1, 3)], 0, [1000, 3, 30, 7]),
        "two_on_one_slot": ([rng_clause(U, MUST, U32, 5, 30), rng_clause(U, MUST_NOT, U32, 10, 12)], 0, []),
        "three_slots": ([rng_clause(U, MUST, U32, 0, 25), rng_clause(I, MUST, I32, -10, INT_MAX), rng_clause(F, MUST_NOT, F32, 2.5, np.inf)], 0, []),
        "must_not": ([rng_clause(U, MUST_NOT, U32, 0, 19)], 0, []),
        "must_not_f_full": ([rng_clause(F, MUST_NOT, F32, -np.inf, np.inf)], 0, []),   # the NaNs alone remain
        "should_twice": ([rng_clause(U, SHOULD, U32, 0, 30), rng_clause(U, SHOULD, U32, 10, 0xffffffff)], 2, []),
        "shared_values": ([(U, SHOULD, IN, 0, 0, 0, 4), (U, SHOULD, IN, 0, 0, 2, 4), (I, SHOULD, IN, 0, 0, 0, 6)], 2, [1, 2, 3, 4, 5, 6]),
    }
    three = [rng_clause(U, SHOULD, U32, 0, 19), rng_clause(I, SHOULD, I32, 0, INT_MAX), rng_clause(F, SHOULD, F32, 0.0, np.inf)]
    for ms in (0, 2, 4):
        out["should3_min%d" % ms] = (three, ms, [])
    # 64 clauses: 40 SHOULD ranges and sets over the three slots, 20 repeats of one MUST, four MUST_NOT; the sets share values
    sv = np.concatenate([rng.integers(0, 40, 200).astype(np.uint32), bits_of(rng.integers(-30, 30, 100), I32), bits_of(F_SPECIAL[:7], F32)])
    many = []
    for j in range(40):
        slot = j % 3
        if j % 4 == 3:
            begin, count = ((0, 200), (200, 100), (300, 7))[slot]
            a = int(rng.integers(0, count))
            many.append((slot, SHOULD, IN, 0, 0, begin + a, int(rng.integers(0, count - a + 1))))
        else:
            lo, hi = sorted(rng.integers(-30, 40, 2).tolist())
            many.append(rng_clause(slot, SHOULD, slot, max(lo, 0) if slot == U else lo, max(hi, 0) if slot == U else hi))
    many += [rng_clause(U, MUST, U32, 0, 0xfffffffe)] * 20
    many += [rng_clause(I, MUST_NOT, I32, 29, 29), rng_clause(F, MUST_NOT, F32, 100.0, 100.0), (U, MUST_NOT, IN, 0, 0, 0, 2), rng_clause(U, MUST_NOT, U32, 39, 39)]
    order = rng.permutation(len(many))
    assert len(many) == MAX_CLAUSES
    out["c64"] = ([many[k] for k in order], 12, sv)
    # 64 IN clauses over the same 8192 values: the plan repeats them (more keys than the LDS array holds)
    out["c64_in_big"] = ([(U, SHOULD, IN, 0, 0, 0, MAX_SET)] * 63 + [(U, MUST_NOT, IN, 0, 0, 17, 1)], 63, big)
    return out


# the case on which each wrong reading differs from the contract: (n_docs, clause set, within or None)
WRONG_CASES = {
    "half_open": (65, "u_range", None),
    "i32_unsigned": (65, "i_range", None),
    "f32_bits": (65, "f_range", None),
    "nan_matches": (65, "f_full", None),
    "in_as_min_max": (65, "in_u_spread", None),
    "should_distinct_slot": (65, "should_twice", None),
    "min_should_0_as_1": (65, "should3_min0", None),
    "must_not_ignored_without_must": (65, "must_not", None),
    "bits_past_end": (65, "must_not", None),
    "last_partial_workgroup_dropped": (W + 1, "u_full", None),
    "within_or": (65, "u_range", "sparse"),
}


# ---------------------------------------------------------------------------------------------------------------------
# the reference: facet counts
# ---------------------------------------------------------------------------------------------------------------------
FACET_WRONG = ("ties_value_descending", "zero_counts_listed", "filter_ignored", "cut_before_sort", "distinct_after_cut")
FACET_SLOT = 5
FACET_T = (1, 2, 1024)


def expected_facets(values, mask, t, wrong=None):
    """(values u32 [n], counts u64 [n], distinct, docs). values: the u32 column; mask: bool [n_docs] or None. wrong: None,
    or one of FACET_WRONG -
      ties_value_descending   equal counts are ordered by value descending
      zero_counts_listed      the values 0 .. max that no document holds are rows too (count 0)
      filter_ignored          all documents are counted
      cut_before_sort         the first t values that occur (in value order) are taken, then sorted
      distinct_after_cut      distinct is the number of rows returned"""
    assert wrong is None or wrong in FACET_WRONG
    counted = values if mask is None or wrong == "filter_ignored" else values[mask]
    docs = len(values) if mask is None else int(mask.sum())
    if wrong == "zero_counts_listed":
        cnt = np.bincount(counted.astype(np.int64), minlength=int(values.max()) + 1)
        val = np.arange(len(cnt))
    else:
        val, cnt = np.unique(counted, return_counts=True)
    distinct = len(val)
    if wrong == "cut_before_sort":
        val, cnt = val[:t], cnt[:t]
    order = np.lexsort((-val.astype(np.int64) if wrong == "ties_value_descending" else val.astype(np.int64), -cnt.astype(np.int64)))[:t]
    if wrong == "distinct_after_cut":
        distinct = len(order)
    return val[order].astype(np.uint32), cnt[order].astype(np.uint64), distinct, docs


def facet_columns(n_docs):
    """name -> u32 [n_docs]: a maximum of bins - 1 for the bins at the edges of the LDS histogram and of the limit, one value
    for all, a value per document, and counts that tie in groups."""
    rng = np.random.default_rng(555 + n_docs)
    d = np.arange(n_docs)
    out = {}
    for bins in (1, 2, LDS_BINS - 1, LDS_BINS, LDS_BINS + 1, MAX_BINS):
        v = rng.integers(0, bins, n_docs)
        if bins > 64:                         # a skewed head, so that the rows are not all of count 1
            head =rng.random(n_docs) < 0.6
            v[head] = rng.integers(0, 9, int(head.sum())) ** 2
        v[0] = bins - 1
        out["bins%d" % bins] = v.astype(np.uint32)
    out["own_value"] = d.astype(np.uint32)
    out["ties"] = (d % 6 + 10).astype(np.uint32)        # counts tie in one or two groups: t = 1, 2 cut through a group
    return out


FACET_PATH = {"bins1": 0, "bins2": 0, "bins%d" % (LDS_BINS - 1): 0, "bins%d" % LDS_BINS: 0, "bins%d" % (LDS_BINS + 1): 1,
              "bins%d" % MAX_BINS: 1}
FACET_N_DOCS = (1, 65, 2 * W + 5)

# (n_docs, facet column, filter: None / a within_sets name, t)
FACET_WRONG_CASES = {
    "ties_value_descending": (65, "ties", None, 2),
    "zero_counts_listed": (65, "bins%d" % LDS_BINS, None, 1024),
    "filter_ignored": (65, "ties", "sparse", 2),
    "cut_before_sort": (65, "bins%d" % (LDS_BINS + 1), None, 2),
    "distinct_after_cut": (65, "ties", None, 2),
}


def check():
    """Every wrong reading changes the expected answer on its named case (CPU, no library call beyond the index build)."""
    for wrong, (n_docs, name, wname) in WRONG_CASES.items():
        t = make(n_docs, "u16_f16")
        clauses, ms, sv = clause_sets(t)[name]
        within = None if wname is None else within_sets(n_docs)[wname]
        good, bad = expected_bits(t.cols, clauses, ms, sv, within), expected_bits(t.cols, clauses, ms, sv, within, wrong=wrong)
        assert bits_diff(bad, good) is not None, wrong
    for wrong, (n_docs, name, wname, top) in FACET_WRONG_CASES.items():
        col = facet_columns(n_docs)[name]
        mask = None if wname is None else within_sets(n_docs)[wname]
        good, bad = expected_facets(col, mask, top), expected_facets(col, mask, top, wrong=wrong)
        assert any(not np.array_equal(np.asarray(a), np.asarray(b)) for a, b in zip(good, bad)), wrong
