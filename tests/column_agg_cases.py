"""Seeded inputs and the reference for the tests of the column aggregations (test_column_agg_cpu.py,
test_gpu_column_agg.py): sgpu_column_stats, sgpu_column_histogram, sgpu_column_top. TEST INFRASTRUCTURE, pure numpy apart
from the index build (column_cases.make / fresh, unchanged).

expected_stats(), expected_histogram() and expected_top() restate, from the text of include/seismic_hip.h alone, what the
three calls return - with numpy's own typed comparisons (uint32 / int32 / float32: NaN compares false, -0.0 == +0.0),
np.searchsorted on typed arrays and np.lexsort, never with keys. The canonical F32 sum is written as reshapes and adds in
float64: tiles of 16384 ids, 64 turns of 256 lanes added in turn order, the lanes folded by halves, the tiles added in order.
Each call has one switch per wrong reading (STATS_WRONG, HIST_WRONG, TOP_WRONG); check() shows on the CPU that every switch
changes the answer on its named case.

Sizes (N_DOCS): column_cases.N_DOCS (1, the word and wavefront edges, 8191 .. 16389) and the sum tile's edges 16383, 16384,
16385 and 2 * 16384 + 5 - the smallest sizes at which a tile, a slice boundary or a cross-workgroup tie can go wrong.
Columns: column_cases' U / I / F in slots 0 .. 2 (0 / 0xffffffff, INT_MIN / INT_MAX, +-inf, NaNs of both signs, the
subnormal) and, in slots 3 .., MIXED (finite f32 of mixed magnitudes: 1e30, -1e30, 1, 1e-30 - the order of the adds
decides the sum), CONST (one value: ties only) and BIG (u32 values >= 1 << 22, beyond the facet call's limit).
Filters (filters()): None, all, empty, every third document, one document, the NaN documents only, and one that keeps +inf
but not -inf.
"""
import numpy as np

import column_cases as cc

TILE, LANES = 16384, 256
MAX_BUCKETS, MAX_T = 4096, 1024
N_DOCS = tuple(cc.N_DOCS) + (TILE - 1, TILE, TILE + 1, 2 * TILE + 5)
SHAPES = [(n, "u16_f16") for n in N_DOCS] + [(65, "u32_u8"), (2 * TILE + 5, "u32_u8")]
MIXED, CONST, BIG = 3, 4, 5                     # slots
SLOTS = (cc.U, cc.I, cc.F, MIXED, CONST, BIG)
QUIET_NAN_BITS = 0x7ff8000000000000
TOP_T = (1, 2, 1023, 1024)


def extra_columns(n_docs):
    rng = np.random.default_rng(7700 + n_docs)
    mixed = rng.choice(np.array([1e30, -1e30, 1.0, 1e-30, -1.0, 3.5e10, 0.0, -0.0], np.float32), n_docs).astype(np.float32)
    m = min(n_docs, 4)
    mixed[:m] = np.array([1e30, 1.0, -1e30, 1e-30], np.float32)[:m]     # left to right: (1e30 + 1) - 1e30 = 0, + 1e-30
    const = np.full(n_docs, -7, np.int32)
    big = (rng.integers(0, 1000, n_docs).astype(np.uint32) * np.uint32(4000003) + np.uint32(1 << 22))
    big[0] = 0xfffffffe
    return {MIXED: mixed, CONST: const, BIG: big}


def add_columns(t):
    """Sets the slots 3 .. on a column_cases index (an index of column_cases.make is shared: setting the same values again
    changes nothing) and returns slot -> array of all six columns."""
    cols = dict(t.cols)
    for slot, col in extra_columns(t.n_docs).items():
        t.ix.set_column(slot, col)
        cols[slot] = col
    return cols


def make(n_docs, variant):
    t = cc.make(n_docs, variant)
    return t, add_columns(t)


def fresh(n_docs, variant):
    t = cc.fresh(n_docs, variant)
    return t, add_columns(t)


def filters(n_docs, f_col):
    """name -> bool [n_docs] or None. f_col: the F column (for the NaN-only and the one-infinity filters)."""
    d = np.arange(n_docs)
    one = np.zeros(n_docs, bool)
    one[n_docs - 1] = True
    return {"null": None, "all": np.ones(n_docs, bool), "empty": np.zeros(n_docs, bool), "third": d % 3 == 0, "one": one,
            "nans": np.isnan(f_col), "plus_inf_only": ~(np.isneginf(f_col))}


def native_filters(t, cols):
    """name -> (NativeFilter or None, mask or None) of filters() on the index t"""
    return {name: (None if mask is None else t.ix.make_filter(mask), mask) for name, mask in filters(t.n_docs, cols[cc.F]).items()}


STATS_KEYS = ("docs", "valid", "min_bits", "max_bits", "sum_int", "sum_bits")


def stats_of(ix, slot, f, **kw):
    """NativeIndex.column_stats as the fields expected_stats returns: `sum` as the bits of the double."""
    s = ix.column_stats(slot, f, **kw)
    return {k: s[k] for k in STATS_KEYS}


def same_hist(got, want):
    return np.array_equal(got[0], want[0]) and got[0].dtype == np.uint64 and tuple(got[1:]) == tuple(want[1:])


def same_top(got, want):
    return (np.array_equal(got[0], want[0]) and got[0].dtype == np.uint32 and np.array_equal(got[1], want[1])
            and tuple(got[2:]) == tuple(want[2:]))


def mask_of(mask, n_docs, wrong=None):
    if mask is None or wrong == "filter_ignored":
        return np.ones(n_docs, bool)
    return mask


# ---------------------------------------------------------------------------------------------------------------------
# stats
# ---------------------------------------------------------------------------------------------------------------------
STATS_WRONG = ("sum_left_to_right", "sum_float32", "nan_valid", "i32_unsigned", "f32_bits", "minus_zero_below", "filter_ignored",
               "last_partial_tile_dropped")


def canonical_sum(x):
    """x: float64 [n_docs], the contributions (+0.0 where a document does not count) -> the canonical sum."""
    n_tiles = -(-len(x) // TILE)
    padded = np.zeros(n_tiles * TILE, np.float64)
    padded[:len(x)] = x
    tiles = padded.reshape(n_tiles, TILE // LANES, LANES)
    total = np.float64(0.0)
    for t in range(n_tiles):
        c = np.zeros(LANES, np.float64)
        for r in range(TILE // LANES):
            c = c + tiles[t, r]
        h = LANES // 2
        while h >= 1:
            c = c[:h] + c[h:2 * h]
            h //= 2
        total = total + c[0]
    return total


def f64_bits(x):
    x = np.float64(x)
    return QUIET_NAN_BITS if np.isnan(x) else int(np.array([x], np.float64).view(np.uint64)[0])


def expected_stats(col, mask, wrong=None):
    """dict(docs, valid, min_bits, max_bits, sum_int, sum_bits). col: the column in its dtype; mask: bool or None."""
    assert wrong is None or wrong in STATS_WRONG
    n_docs = len(col)
    on = mask_of(mask, n_docs, wrong).copy()
    docs = int(on.sum()) if mask is not None else n_docs
    if wrong == "last_partial_tile_dropped":
        on[n_docs // TILE * TILE:] = False
    is_f = col.dtype == np.float32
    nan = np.isnan(col) if is_f else np.zeros(n_docs, bool)
    counted = on & ~nan
    valid = int((on if wrong == "nan_valid" else counted).sum())
    if wrong == "last_partial_tile_dropped":
        docs = int(on.sum())
    v = col[counted]
    with np.errstate(all="ignore"):
        if len(v) == 0:
            lo = hi = 0
        elif (wrong == "i32_unsigned" and col.dtype == np.int32) or (wrong == "f32_bits" and is_f):
            u = v.view(np.uint32)
            lo, hi = int(u.min()), int(u.max())
        else:
            lo, hi = v.min(), v.max()
            if is_f:
                if wrong == "minus_zero_below":
                    z = v[v == 0]
                    if lo == 0 and np.signbit(z).any():
                        lo = np.float32(-0.0)
                    elif lo == 0:
                        lo = np.float32(0.0)
                    if hi == 0:
                        hi = np.float32(0.0) if (~np.signbit(z)).any() else np.float32(-0.0)
                else:
                    lo, hi = lo + np.float32(0.0), hi + np.float32(0.0)     # a zero is reported as +0.0
            lo, hi = int(np.array([lo], col.dtype).view(np.uint32)[0]), int(np.array([hi], col.dtype).view(np.uint32)[0])
        if is_f:
            sum_int = 0
            x = np.where(counted, col, np.float32(0.0))
            if wrong == "sum_left_to_right":
                total = np.float64(0.0)
                for y in x.astype(np.float64):
                    total = total + y
            elif wrong == "sum_float32":
                total = _canonical_sum_f32(x)
            else:
                total = canonical_sum(x.astype(np.float64))
            sum_bits = f64_bits(total)
        else:
            s = int(v.astype(np.int64).sum()) if len(v) else 0          # (|sum| < 2^63 at these sizes: int64 is exact)
            sum_int = s & 0xffffffffffffffff
            sum_bits = f64_bits(float(s))
    return dict(docs=docs, valid=valid, min_bits=lo, max_bits=hi, sum_int=sum_int, sum_bits=sum_bits)


def _canonical_sum_f32(x):
    """The canonical order with float32 adds (the wrong reading `sum_float32`)."""
    n_tiles = -(-len(x) // TILE)
    padded = np.zeros(n_tiles * TILE, np.float32)
    padded[:len(x)] = x
    tiles = padded.reshape(n_tiles, TILE // LANES, LANES)
    total = np.float32(0.0)
    for t in range(n_tiles):
        c = np.zeros(LANES, np.float32)
        for r in range(TILE // LANES):
            c = c + tiles[t, r]
        h = LANES // 2
        while h >= 1:
            c = c[:h] + c[h:2 * h]
            h //= 2
        total = total + c[0]
    return np.float64(total)


# ---------------------------------------------------------------------------------------------------------------------
# histogram
# ---------------------------------------------------------------------------------------------------------------------
HIST_WRONG = ("last_half_open", "all_closed", "below_above_swapped", "nan_valid", "i32_unsigned", "f32_bits", "minus_zero_below",
              "filter_ignored", "last_partial_tile_dropped")


def expected_histogram(col, mask, edges, wrong=None):
    """(counts u64 [len(edges) - 1], below, above, nan, docs). edges: an array of the column's dtype, strictly ascending."""
    assert wrong is None or wrong in HIST_WRONG
    n_docs = len(col)
    on = mask_of(mask, n_docs, wrong).copy()
    if wrong == "last_partial_tile_dropped":
        on[n_docs // TILE * TILE:] = False
    docs = int(on.sum()) if (mask is not None or wrong == "last_partial_tile_dropped") else n_docs
    is_f = col.dtype == np.float32
    isnan = np.isnan(col) if is_f else np.zeros(n_docs, bool)
    v, e = col[on & ~isnan], np.asarray(edges, col.dtype)
    nan = int((on & isnan).sum())
    if wrong == "nan_valid":                     # NaNs take part: no comparison holds, they fall past the last edge
        v, nan = col[on], 0
    if (wrong == "i32_unsigned" and col.dtype == np.int32) or (wrong == "f32_bits" and is_f):
        v, e = v.view(np.uint32), np.sort(e.view(np.uint32))
    elif wrong == "minus_zero_below" and is_f:   # total order: -0.0 sorts just below +0.0
        def total(a):
            b = a.view(np.uint32).astype(np.int64)
            return np.where(b & 0x80000000, -(b & 0x7fffffff) - 1, b)
        v, e = total(v), total(e)
    nb = len(e) - 1
    with np.errstate(all="ignore"):
        if wrong == "all_closed":                # every bucket e[b] <= v <= e[b + 1]: a value on an inner edge counts twice
            counts = np.array([int(((v >= e[b]) & (v <= e[b + 1])).sum()) for b in range(nb)], np.uint64)
        else:
            b = np.searchsorted(e, v, side="right") - 1          # the number of edges <= v, minus one
            inside = (v >= e[0]) & (v <= e[-1]) if wrong != "last_half_open" else (v >= e[0]) & (v < e[-1])
            b = np.minimum(b[inside], nb - 1)
            counts = np.bincount(b, minlength=nb).astype(np.uint64)
        below, above = int((v < e[0]).sum()), int((v > e[-1]).sum())
        if wrong == "nan_valid":
            above += int(np.isnan(v).sum()) if is_f else 0
        if wrong == "last_half_open":
            above += int((v == e[-1]).sum())
    if wrong == "below_above_swapped":
        below, above = above, below
    return counts, below, above, nan, docs


def edge_sets(slot, col):
    """name -> edges (the column's dtype) for the column of `slot`: one bucket, values exactly on every edge, the type's
    extremes, and 4096 buckets."""
    dt = col.dtype
    if dt == np.uint32:
        if slot == BIG:
            return {"big": np.array([1 << 22, 1 << 30, 0xfffffffe], dt), "big_4096": (np.arange(4097, dtype=np.uint64) * 1048000 + 5).astype(dt)}
        return {"one": np.array([7, 20], dt), "on_edges": np.array([0, 7, 20, 39, 0xffffffff], dt), "extremes": np.array([0, 0xffffffff], dt),
                "inner": np.array([1, 5, 6, 30], dt), "b4096": np.arange(4097, dtype=dt)}
    if dt == np.int32:
        return {"one": np.array([-1, 5], dt), "on_edges": np.array([cc.INT_MIN, -30, -1, 0, 5, 29, cc.INT_MAX], dt),
                "extremes": np.array([cc.INT_MIN, cc.INT_MAX], dt), "inner": np.array([-10, -7, 0, 10], dt),
                "b4096": (np.arange(4097, dtype=np.int64) - 2048).astype(dt)}
    return {"one": np.array([-1.5, 2.5], dt), "on_edges": np.array([-np.inf, -3.0, -1.5, 0.0, cc.SUBNORMAL, 0.5, 1.0, 2.5, 100.0, 65504.0, np.inf], dt),
            "extremes": np.array([-np.inf, np.inf], dt), "minus_zero_edge": np.array([-1.5, -0.0, 2.5], dt),
            "zero_edge": np.array([-1.5, 0.0, 2.5], dt),
            "zero_top": np.array([-3.0, 0.0], dt), "finite": np.array([-1e30, -1.0, 1e-30, 1.0, 1e30], dt),
            "b4096": np.linspace(-4.0, 4.0, 4097).astype(dt)}


# ---------------------------------------------------------------------------------------------------------------------
# top
# ---------------------------------------------------------------------------------------------------------------------
TOP_WRONG = ("nan_last", "i32_unsigned", "f32_bits", "minus_zero_below", "ties_id_descending", "descending_reversed", "filter_ignored",
             "last_partial_tile_dropped")


def expected_top(col, mask, t, order, wrong=None):
    """(doc_ids u32 [n], value_bits u32 [n], valid, docs)."""
    assert wrong is None or wrong in TOP_WRONG
    n_docs = len(col)
    on = mask_of(mask, n_docs, wrong).copy()
    if wrong == "last_partial_tile_dropped":
        on[n_docs // TILE * TILE:] = False
    docs = int(on.sum()) if (mask is not None or wrong == "last_partial_tile_dropped") else n_docs
    is_f = col.dtype == np.float32
    isnan = np.isnan(col) if is_f else np.zeros(n_docs, bool)
    ids = np.flatnonzero(on & ~isnan)
    valid = len(ids)
    v = col[ids]
    if (wrong == "i32_unsigned" and col.dtype == np.int32) or (wrong == "f32_bits" and is_f):
        v = v.view(np.uint32)
    if is_f and v.dtype == np.float32:
        if wrong == "minus_zero_below":
            v = np.where((v == 0) & np.signbit(v), -1e-60, v.astype(np.float64))      # -0.0 just below +0.0
        else:
            v = v + np.float32(0.0)              # -0.0 == +0.0: one value
    v = v.astype(np.float64) if v.dtype.kind == "f" else v.astype(np.int64)
    tie = -ids if wrong == "ties_id_descending" else ids
    if wrong == "descending_reversed" and order == 1:
        rows = np.lexsort((tie, v))[::-1][:t]                       # the ascending rows read backwards: ties by id descending
    else:
        rows = np.lexsort((tie, -v if order == 1 else v))[:t]
    out_ids = ids[rows]
    if wrong == "nan_last" and len(out_ids) < t:                     # NaN documents follow the numbers, in id order
        out_ids = np.concatenate([out_ids, np.flatnonzero(on & isnan)])[:t]
    return out_ids.astype(np.uint32), col.view(np.uint32)[out_ids], valid, docs


# ---------------------------------------------------------------------------------------------------------------------
# the case on which each wrong reading differs from the contract
# ---------------------------------------------------------------------------------------------------------------------
# stats: (n_docs, slot, filter name)
STATS_WRONG_CASES = {
    "sum_left_to_right": (4, MIXED, "null"),              # 1e30, 1, -1e30, 1e-30: 1e-30 left to right, 1 in the canonical order
    "sum_float32": (cc.W + 1, MIXED, "null"),
    "nan_valid": (65, cc.F, "null"),
    "i32_unsigned": (65, cc.I, "null"),
    "f32_bits": (65, cc.F, "null"),
    "minus_zero_below": (3, cc.F, "one"),                 # document 2 alone: the stored -0.0
    "filter_ignored": (65, cc.U, "third"),
    "last_partial_tile_dropped": (TILE + 1, cc.U, "null"),
}
# histogram: (n_docs, slot, filter name, edge set)
HIST_WRONG_CASES = {
    "last_half_open": (65, cc.U, "null", "one"),
    "all_closed": (65, cc.U, "null", "on_edges"),
    "below_above_swapped": (65, cc.I, "null", "one"),
    "nan_valid": (65, cc.F, "null", "one"),
    "i32_unsigned": (65, cc.I, "null", "one"),
    "f32_bits": (65, cc.F, "null", "one"),
    "minus_zero_below": (65, cc.F, "null", "zero_edge"),
    "filter_ignored": (65, cc.U, "third", "one"),
    "last_partial_tile_dropped": (TILE + 1, cc.U, "null", "extremes"),
}
# top: (n_docs, slot, filter name, t, order)
TOP_WRONG_CASES = {
    "nan_last": (65, cc.F, "null", 1024, 0),
    "i32_unsigned": (65, cc.I, "null", 2, 0),
    "f32_bits": (65, cc.F, "null", 2, 0),
    "minus_zero_below": (65, cc.F, "plus_inf_only", 1024, 0),
    "ties_id_descending": (65, CONST, "null", 2, 0),
    "descending_reversed": (65, CONST, "null", 2, 1),
    "filter_ignored": (65, cc.U, "third", 2, 0),
    "last_partial_tile_dropped": (TILE + 1, cc.U, "null", 2, 1),
}


def _differs(a, b):
    if isinstance(a, dict):
        return a != b
    return any(not np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(a, b))


def check():
    """Every wrong reading changes the expected answer on its named case (CPU, no library call beyond the index build)."""
    for wrong, (n_docs, slot, fname) in STATS_WRONG_CASES.items():
        t, cols = make(n_docs, "u16_f16")
        mask = filters(n_docs, cols[cc.F])[fname]
        assert _differs(expected_stats(cols[slot], mask), expected_stats(cols[slot], mask, wrong=wrong)), wrong
    for wrong, (n_docs, slot, fname, ename) in HIST_WRONG_CASES.items():
        t, cols = make(n_docs, "u16_f16")
        mask = filters(n_docs, cols[cc.F])[fname]
        edges = edge_sets(slot, cols[slot])[ename]
        assert _differs(expected_histogram(cols[slot], mask, edges), expected_histogram(cols[slot], mask, edges, wrong=wrong)), wrong
    for wrong, (n_docs, slot, fname, top, order) in TOP_WRONG_CASES.items():
        t, cols = make(n_docs, "u16_f16")
        mask = filters(n_docs, cols[cc.F])[fname]
        assert _differs(expected_top(cols[slot], mask, top, order), expected_top(cols[slot], mask, top, order, wrong=wrong)), wrong
