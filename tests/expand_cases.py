"""Shared data of the expand_queries tests (tests/test_expand_cpu.py, tests/test_gpu_expand.py). TEST INFRASTRUCTURE.

A case = one small document collection built into an index of one form (component width, vocabulary size, value type)
and a list of named CALLS of sgpu_expand_queries on it; expand_numpy() is a RESTATEMENT of the contract written from the
text of include/seismic_hip.h alone: it decodes the descriptor's forward arrays, keeps the table W in np.float32, adds
the documents one after the other and selects by (W descending, component ascending). With reading=... it implements
one WRONG reading of the contract instead; every named call says which reading it catches.

Index forms (CASES): u16 components at dim 32767 - the last vocabulary whose table (dim + 1 floats) fits the device's
128 KiB of LDS - with binary16, fixed-u8 and DotVByte values; dim 32768, the first that does not fit, with u16 and u32
components; and a 300-component vocabulary. Components 0 and dim - 1 are in use (`edge`, `far`, the call `many`). Stored
values are multiples of 1/16 up to 15, so every form holds the same numbers (fixed-u8: val_scale = 1/16).
Documents by name: len_N (N = 0, 1, 7, 8, 9, 127, 128, 129, 300: slice padding, the 128-element pass, several passes),
edge, far (dim >= 20000: gaps no DotVByte field holds - the raw record form), o1 o2 o3, rep, neg, qadd, then random ones.
Calls and the wrong reading each catches:
  lengths    the len_N documents as one query's feedback                  (padding elements added to a component)
  empty      no candidates / empty query with candidates / both empty     (rows not zeroed, a query dropped)
  alpha0     alpha = 0
  order      o1 o2 o3 share a component with value 1, weights 2^24, 1, -2^24: W is exactly 0 in the given order (no term)
             and 1 in the reversed order or summed in float64             ("reversed", "float64")
  repeat     rep listed twice, p = 3 onto 2^24: fl(fl(a + p) + p) != fl(a + 2 p) != fl(a + p)   ("dedupe", "presum")
  negative   a term cancels to exactly 0, another goes negative: both dropped               ("abs")
  unrounded  alpha = 0.1f: fl(alpha * w) is rounded BEFORE the document's product is added  ("unrounded")
  ties       40 components share one weight across the cut, 10 above, 10 below, 10 negative of larger magnitude; t = 1, 30,
             count - 1, count, count + 1, 1024                            ("ties_high", "abs", "weight_order")
  many       (dim >= 32767) 1500 components of four different weights: more than 1024 terms at t = 1024
  random     eight random queries, ten signed-weight documents each
"""
import numpy as np

import orc
from seismic_amd import _native
from seismic_amd._abi import BuildConfig

N_DOCS = 200
SPECIAL_LENS = (0, 1, 7, 8, 9, 127, 128, 129, 300)
BUILD = dict(n_postings=50, centroid_fraction=0.2, summary_energy=0.5, max_fraction=6.0)
CO, CR, CN1, CN2, CQ, CFREE = 50, 60, 70, 71, 80, 90
TIE_COMPS = np.arange(100, 170)

# name -> (component width, dim, value type)
CASES = {
    "u16_f16_32767": (2, 32767, 0),
    "u16_u8_32767": (2, 32767, 1),
    "u16_dvb_32767": (2, 32767, 2),
    "u16_f16_32768": (2, 32768, 0),
    "u32_f16_32768": (4, 32768, 0),
    "u32_u8_32768": (4, 32768, 1),
    "u16_f16_300": (2, 300, 0),
}
READINGS = ("reversed", "float64", "dedupe", "presum", "abs", "unrounded", "ties_high", "weight_order")


def _values(rng, n):
    return (rng.integers(1, 129, n) / 16.0).astype(np.float32)   # multiples of 1/16 in (0, 8]


class Call:
    def __init__(self, name, queries, lists, weights, alpha, ts):
        self.name, self.queries, self.lists, self.alpha, self.ts = name, queries, lists, np.float32(alpha), tuple(ts)
        self.weights = [np.asarray(w, np.float32) for w in weights]
        assert len(queries) == len(lists) == len(weights) and all(len(a) == len(b) for a, b in zip(lists, self.weights))
        self.nq = len(queries)
        self.q_off, self.qc, self.qv = orc.csr(queries)
        self.cand_off = np.zeros(self.nq + 1, np.uint64)
        self.cand_off[1:] = np.cumsum([len(x) for x in lists])
        self.cand_ids = (np.concatenate(lists) if lists else np.zeros(0)).astype(np.uint64)
        self.cand_w = (np.concatenate(self.weights) if lists else np.zeros(0)).astype(np.float32)

    def args(self):
        return self.q_off, self.qc, self.qv, self.cand_off, self.cand_ids, self.cand_w, float(self.alpha)


class ExpandCase:
    def __init__(self, name):
        self.name = name
        self.cw, self.dim, self.value_type = CASES[name]
        dim = self.dim
        rng = np.random.default_rng(47)
        window = min(2000, dim)
        p = 1.0 / (np.arange(window) + 20.0)
        p /= p.sum()
        docs, named = [], {}

        def add(label, c, v):
            named[label] = len(docs)
            docs.append((np.asarray(c, np.uint32), np.asarray(v, np.float32)))

        def window_doc(n):
            return np.sort(rng.choice(window, n, replace=False, p=p)), _values(rng, n)

        for n in SPECIAL_LENS:
            add("len_%d" % n, *window_doc(n))
        add("edge", [0, 1, dim - 1], [1.0, 15.0, 2.5])
        if dim >= 20000:
            add("far", [0, 5000, 15000, dim - 1], [3.0, 0.5, 1.25, 4.0])
        for i in range(3):
            add("o%d" % (i + 1), [CO, 200 + i], [1.0, 0.5])
        add("rep", [CR, CR + 1], [1.0, 2.0])
        add("neg", [CN1, CN2], [2.0, 1.0])
        add("qadd", [CQ], [1.0])
        while len(docs) < N_DOCS:
            c, v = window_doc(int(rng.integers(2, 81)))
            if dim >= 20000 and len(docs) % 4 == 0:   # a far tail: the raw record form in a DotVByte index
                c = np.concatenate([c, [9000 + int(rng.integers(0, 50)), 20000 + int(rng.integers(0, 50))]])
                v = np.concatenate([v, _values(rng, 2)])
            docs.append((c.astype(np.uint32), v))
        self.docs, self.named, self.n_docs = docs, named, len(docs)
        self.off, self.comps, self.vals = orc.csr(docs)
        self._index = None
        self._stored = None
        self._expected = {}

        def rq(n):
            return np.sort(rng.choice(window, n, replace=False, p=p)).astype(np.uint32), _values(rng, n)

        none = np.zeros(0, np.int64)
        empty_q = (np.zeros(0, np.uint32), np.zeros(0, np.float32))
        d = named
        calls = []
        lens = np.array([d["len_%d" % n] for n in SPECIAL_LENS])
        calls.append(Call("lengths", [rq(20)], [lens], [rng.integers(1, 17, len(lens)) / 16.0], 1.0, (64, 1024)))
        signed = rq(12)
        signed[1][::3] *= -1.0
        three = rng.integers(0, N_DOCS, 3)
        calls.append(Call("empty", [signed, empty_q, empty_q], [none, three, none], [[], [0.25, 0.25, 0.25], []], 1.0, (8, 64)))
        calls.append(Call("alpha0", [rq(15), signed], [rng.integers(0, N_DOCS, 5), three], [[0.15] * 5, [0.25, -0.5, 0.25]], 0.0, (16,)))
        calls.append(Call("order", [empty_q], [[d["o1"], d["o2"], d["o3"]]], [[2.0 ** 24, 1.0, -2.0 ** 24]], 1.0, (16,)))
        calls.append(Call("repeat", [(np.array([CR], np.uint32), np.array([2.0 ** 24], np.float32))], [[d["rep"], d["rep"]]],
                          [[3.0, 3.0]], 1.0, (16,)))
        calls.append(Call("negative", [(np.array([CN1, CFREE], np.uint32), np.array([2.0, 1.0], np.float32))], [[d["neg"]]],
                          [[-1.0]], 1.0, (16,)))
        # unrounded: a weight w for which fl(fl(0.1f * w) + 1) differs from the float64 sum 0.1f * w + 1 rounded once
        alpha = np.float32(0.1)
        w = None
        for cand in np.random.default_rng(5).random(4000).astype(np.float32):
            if np.float32(alpha * cand) + np.float32(1.0) != np.float32(np.float64(alpha) * np.float64(cand) + 1.0):
                w = cand
                break
        assert w is not None
        calls.append(Call("unrounded", [(np.array([CQ], np.uint32), np.array([w], np.float32))], [[d["qadd"]]], [[1.0]], alpha, (4,)))
        tw = np.array([5.0] * 10 + [2.0] * 40 + [1.0] * 10 + [-9.0] * 10, np.float32)
        rng.shuffle(tw)
        calls.append(Call("ties", [(TIE_COMPS.astype(np.uint32), tw)], [none], [[]], 1.0, (1, 30, 59, 60, 61, 1024)))
        if dim >= 32767:
            mc = np.unique(np.concatenate([[0, dim - 1], rng.choice(dim, 1500, replace=False)]))[:1500]
            mc[-1] = dim - 1
            mw = rng.integers(1, 5, len(mc)).astype(np.float32)
            calls.append(Call("many", [(mc.astype(np.uint32), mw)], [[d["edge"], d["far"]]], [[0.5, 0.25]], 1.0, (1000, 1024)))
        calls.append(Call("random", [rq(int(rng.integers(5, 40))) for _ in range(8)], [rng.integers(0, N_DOCS, 10) for _ in range(8)],
                          [rng.integers(-4, 13, 10) / 64.0 for _ in range(8)], 1.0, (10, 64)))
        self.calls = {c.name: c for c in calls}

    def build(self):
        """A fresh index object of the case (not uploaded)."""
        ix = _native.NativeIndex.build(self.cw, self.dim, self.off, self.comps, self.vals, BuildConfig.defaults(**BUILD))
        if self.value_type:
            ix = ix.convert(self.value_type)
        return ix

    @property
    def index(self):
        """The case's shared host index: never uploaded, never changed."""
        if self._index is None:
            self._index = self.build()
        return self._index

    def stored(self):
        """The forward index as the descriptor gives it: offsets, components, the values as the f32 they stand for in the
        product (binary16 widened; fixed-u8: the code), and the scale a code is multiplied with (None for binary16)."""
        if self._stored is None:
            desc = self.index.desc
            a = orc.desc_arrays(desc)
            off = a["fwd_offsets"].astype(np.int64)
            if desc.value_type == 0:
                x, scale = a["fwd_vals"].view(np.float16).astype(np.float32), None
            else:
                x, scale = a["fwd_vals"].astype(np.float32), np.float32(desc.val_scale)
            self._stored = (off, a["fwd_comps"].astype(np.int64), x, scale)
        return self._stored

    def expected(self, call, t):
        """expand_numpy of the named call at t, computed once and shared (read-only)."""
        key = (call, t)
        if key not in self._expected:
            got = expand_numpy(self, self.calls[call], t)
            for a in got:
                a.setflags(write=False)
            self._expected[key] = got
        return self._expected[key]

    def check(self):
        """The case holds the edges it is named for (asserted with the restatement and the stored arrays alone)."""
        off, comps, x, scale = self.stored()
        lens = np.diff(off)
        assert np.array_equal(lens, np.diff(self.off.astype(np.int64))), "the index stores other document lengths"
        for n in SPECIAL_LENS:
            assert lens[self.named["len_%d" % n]] == n
        assert comps.min() == 0 and comps.max() == self.dim - 1
        if scale is not None:
            assert scale == np.float32(1.0 / 16.0)
        assert np.array_equal((x if scale is None else x * scale), self.vals), "the forms do not hold the same values"
        if self.value_type == 2:
            raw, _ = self.index.stream_stats()
            assert 1 <= raw < self.n_docs
        oc, ov, on = self.expected("order", 16)
        assert CO not in oc[0, :on[0]].tolist() and on[0] == 2
        oc, ov, on = self.expected("repeat", 16)
        assert ov[0, 0] == np.float32(2.0 ** 24 + 8) and oc[0, 0] == CR
        oc, ov, on = self.expected("negative", 16)
        assert oc[0, :on[0]].tolist() == [CFREE]
        assert self.expected("ties", 1024)[2][0] == 60
        if "many" in self.calls:
            mo = expand_numpy(self, self.calls["many"], 1024, count_only=True)
            assert mo > 1024 and self.expected("many", 1024)[2][0] == 1024


def expand_numpy(case, call, t, reading=None, count_only=False):
    """(out_comps u32 [nq, t], out_vals f32 [nq, t], out_n u32 [nq]) of sgpu_expand_queries as include/seismic_hip.h
    defines it; reading: one of READINGS, a wrong reading of the contract implemented instead."""
    off, comps, x, scale = case.stored()
    f32 = np.float32
    oc, ov, on = np.zeros((call.nq, t), np.uint32), np.zeros((call.nq, t), np.float32), np.zeros(call.nq, np.uint32)
    for q, (qc, qw) in enumerate(call.queries):
        wide = reading in ("float64", "unrounded")
        W = np.zeros(case.dim, np.float64 if wide else np.float32)
        for c, w in zip(qc.tolist(), qw):
            W[c] = np.float64(call.alpha) * np.float64(w) if reading == "unrounded" else f32(call.alpha * f32(w))
        ids, ws = np.asarray(call.lists[q], np.int64), call.weights[q]
        if reading == "reversed":
            ids, ws = ids[::-1], ws[::-1]
        if reading == "dedupe":
            ids, first = np.unique(ids, return_index=True)
            ws = ws[first]
        if reading == "presum":   # a document's weights summed first, the document added once
            uniq = list(dict.fromkeys(ids.tolist()))
            ws = np.array([np.sum(ws[ids == u], dtype=np.float32) for u in uniq], np.float32)
            ids = np.array(uniq, np.int64)
        for doc, cw in zip(ids.tolist(), ws):
            c, v = comps[off[doc]:off[doc + 1]], x[off[doc]:off[doc + 1]]
            p = f32(cw) * v if scale is None else f32(f32(cw) * scale) * v   # (f32 arrays: one rounding per product)
            assert p.dtype == np.float32
            W[c] = W[c] + p   # (a document's components are distinct: its additions are independent)
        W = W.astype(np.float32)
        terms = np.flatnonzero(W != 0) if reading == "abs" else np.flatnonzero(W > 0)
        if count_only:
            return len(terms)
        rank = np.abs(W[terms]) if reading == "abs" else W[terms]
        tie = -terms if reading == "ties_high" else terms
        best = terms[np.lexsort((tie, -rank.astype(np.float64)))][:t]
        if reading != "weight_order":
            best = np.sort(best)
        on[q] = len(best)
        oc[q, :len(best)] = best
        ov[q, :len(best)] = W[best]
    return oc, ov, on


def u8_products_both_ways(case, cand_w):
    """The fixed-u8 product of every stored element with the weight cand_w as the contract states it,
    fl(fl(w * val_scale) * code), and as fl(w * fl(code * val_scale)): two f32 arrays."""
    _, _, x, scale = case.stored()
    w = np.float32(cand_w)
    return np.float32(w * scale) * x, w * (x * scale).astype(np.float32)


def same(got, want):
    """None if the three arrays agree bit for bit, else the name of the first that does not and where."""
    for name, a, b in zip(("out_comps", "out_vals", "out_n"), got, want):
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        if a.shape != b.shape:
            return "%s: shape %r != %r" % (name, a.shape, b.shape)
        bad = np.argwhere(a.view(np.uint32) != b.view(np.uint32))
        if len(bad):
            i = tuple(bad[0])
            return "%s differs at %d places, first %r: %r != %r" % (name, len(bad), i, a[i], b[i])
    return None


_MADE = {}


def make(name):
    """The case `name`, built and checked once per process."""
    if name not in _MADE:
        case = ExpandCase(name)
        case.check()
        _MADE[name] = case
    return _MADE[name]
