"""Shared helpers of the rerank tests (tests/test_rerank_cpu.py, tests/test_gpu_rerank.py). TEST INFRASTRUCTURE.

The cases are tests/score_cases.py as they are. The expected rows come from the oracle's bits alone, in numpy: the
query's distinct ids, their oracle bits, ordered by (score descending, id ascending), the first k.
"""
import numpy as np

import score_cases

KS_CPU = (1, 3, 10, 1000, 1024)


def expected_row(case, q, ids, k):
    """(score bits u32 [k], ids u64 [k], n) of query q over the candidate list `ids`; slots past n are zero."""
    bits = case.oracle_bits()
    d = np.unique(np.asarray(ids, np.int64))                      # (distinct, ascending)
    s = bits[q, d].view(np.float32)
    assert not np.isnan(s).any() and not (bits[q, d] == 0x80000000).any()   # (the cases hold no NaN and no -0.0)
    order = np.lexsort((d, -s.astype(np.float64)))[:k]            # (last key first: score descending, then id ascending)
    out_b, out_i = np.zeros(k, np.uint32), np.zeros(k, np.uint64)
    out_b[:len(order)] = bits[q, d[order]]
    out_i[:len(order)] = d[order]
    return out_b, out_i, len(order)


def expected_rows(case, cand_off, cand_ids, k, queries=None):
    """The same for candidate lists in CSR form: (bits [nq, k], ids [nq, k], n [nq]). queries: the case's query of each row
    (default: row q is query q)."""
    off = np.asarray(cand_off).astype(np.int64)
    nq = len(off) - 1
    b, i, n = np.zeros((nq, k), np.uint32), np.zeros((nq, k), np.uint64), np.zeros(nq, np.uint32)
    for q in range(nq):
        b[q], i[q], n[q] = expected_row(case, q if queries is None else queries[q], cand_ids[off[q]:off[q + 1]], k)
    return b, i, n


def assert_rows(got, want, what=""):
    """got = (scores f32, ids, n) of a rerank call; want = expected_rows(...): out_n, ids, score bits and zero padding."""
    sc, ids, n = got
    wb, wi, wn = want
    assert np.array_equal(np.asarray(n, np.uint32), wn), (what, n, wn)
    assert sc.shape == wb.shape and ids.shape == wi.shape, (what, sc.shape, wb.shape)
    bad = np.argwhere(ids != wi)
    assert len(bad) == 0, "%s: %d ids differ, first at %r: %r != %r" % (what, len(bad), bad[0], ids[tuple(bad[0])], wi[tuple(bad[0])])
    gb = np.ascontiguousarray(sc, np.float32).view(np.uint32)
    bad = np.argwhere(gb != wb)
    assert len(bad) == 0, "%s: %d scores differ, first at %r: %#x != %#x" % (what, len(bad), bad[0], gb[tuple(bad[0])], wb[tuple(bad[0])])


_CHECKED = {}


def discrimination(name, ks=KS_CPU):
    """What the case's own lists can tell apart, from the oracle alone: the (query, k) whose k-th and (k+1)-th distinct
    candidates have equal score bits (the tie rule decides the row), the (query, k) whose row holds both signs, and those
    whose row's ids are not monotone."""
    key = (name, tuple(ks))
    if key not in _CHECKED:
        case = score_cases.make(name)
        ties, signs, mixed = [], [], []
        for q, ids in enumerate(case.lists):
            for k in ks:
                b, i, n = expected_row(case, q, ids, k + 1)
                if n == k + 1 and b[k - 1] == b[k]:
                    ties.append((q, k))
                s, i = b[:min(n, k)].view(np.float32), i[:min(n, k)].astype(np.int64)
                if (s < 0).any() and (s > 0).any():
                    signs.append((q, k))
                if len(i) > 2 and (np.diff(i) < 0).any() and (np.diff(i) > 0).any():
                    mixed.append((q, k))
        _CHECKED[key] = dict(ties=ties, signs=signs, mixed=mixed)
    return _CHECKED[key]


def assert_discriminates(ks=KS_CPU):
    """Before any library call: every value type has a (query, k) the tie rule decides; some row holds both negative and
    positive scores; some row's ids are not monotone in id."""
    by_type = {}
    for name, (_, _, vt) in score_cases.CASES.items():
        by_type.setdefault(vt, []).append(name)
    any_signs = any_mixed = False
    for vt, names in sorted(by_type.items()):
        found = [discrimination(n, ks) for n in names]
        assert any(f["ties"] for f in found), "value type %d: no (query, k) with a tie at the cut" % vt
        any_signs |= any(f["signs"] for f in found)
        any_mixed |= any(f["mixed"] for f in found)
    assert any_signs, "no row holds both negative and positive scores"
    assert any_mixed, "no row's ids are out of id order"
