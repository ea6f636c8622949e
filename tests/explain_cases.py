"""Shared data of the explain_documents tests (tests/test_explain_cpu.py, tests/test_gpu_explain.py). TEST INFRASTRUCTURE.

A case = a small document collection built into an index of one (component width, value type), eight queries, one
candidate list per query, and a numpy RESTATEMENT of sgpu_explain_documents written from the text of
include/seismic_hip.h alone: it decodes the descriptor's forward arrays, multiplies with np.float32 operations, places
every element in the 16-accumulator canonical sum by its position (with the xor combine) and orders the terms by the
integer image of the product bits. It is computed once per case and shared.

Every document and list is named for the edge it sits on (ExplainCase.named):
  len_N          document lengths 0, 1, 7, 8, 9, 127, 128, 129, 257: the 8-element slice and the 128-element pass
  terms_T        exactly T terms with the probe query, T in 0, 1, 2, 9, 10, 11, 31, 32, 33: n_terms of 0, 1, m - 1, m and
                 m + 1 for m = 1, 10 and 32
  big            257 elements, all terms of the long query: more than 128 terms, the best m from different passes, the
                 best one the last element of the last pass
  ties           six equal products on different components (then the component decides)
  zeros          stored values 0 on carried components of a negative and a positive weight: terms whose products are
                 -0.0 and +0.0, the -0.0 one on the smaller component (so that comparing products as numbers, with the
                 component as the tie rule, gives another order than the contract's); and the two components the probe
                 query carries with the weights 0.0 and -0.0: no terms
The restatement follows the header also where it narrows the definition of a term: for fixed-u8 codes a weight whose
product with val_scale is +-0 counts as +-0 (`table != 0` below, not `given != 0`); tests/test_explain_cpu.py has the
case (a weight of 2^-149).
  far            (dim >= 20000) components whose gaps do not fit a DotVByte field: that index keeps the document in the raw
                 record form, the others as packed slices
Queries: 0 the probe (signed weights, six equal ones, a 0.0 and a -0.0), 1 the long one (300 components), 2 empty,
3 one component, 4 .. 7 random signed. Candidate lists: 0 every document ascending plus one id three times, 1 127 ids
with `big` first, 2 128 ids, 3 129 ids, 4 none, 5 one id, 6 every document descending, 7 100 random ids with repeats.
u16 components keep the device's weight table dense (dim < 32768), u32 cases have dim >= 32768: the hashed table.
"""
import numpy as np

import orc
from seismic_amd import _native
from seismic_amd._abi import BuildConfig

WINDOW = 2000
SPECIAL_LENS = (0, 1, 7, 8, 9, 127, 128, 129, 257)
TERM_COUNTS = (0, 1, 2, 9, 10, 11, 31, 32, 33)
N_DOCS = 300
N_QUERIES = 8
MS = (1, 10, 32)
BUILD = dict(n_postings=50, centroid_fraction=0.2, summary_energy=0.5, max_fraction=6.0)

# name -> (component width, dim, value type)
CASES = {
    "u16_f16": (2, 3000, 0),
    "u16_u8": (2, 20000, 1),
    "u16_dvb": (2, 20000, 2),
    "u32_f16": (4, 70000, 0),
    "u32_u8": (4, 40000, 1),
}

_WINDOW_P = 1.0 / (np.arange(WINDOW) + 20.0)
_WINDOW_P /= _WINDOW_P.sum()


def _values(rng, n):
    """Signed binary16 values, magnitudes 2^-6 .. 2^3, mostly positive and above 1 (a fixed-u8 index turns negative values
    and those below half its step into code 0)."""
    small = rng.random(n) < 1.0 / 3.0
    mag = np.exp2(np.where(small, rng.uniform(-6.0, 3.0, n), rng.uniform(0.0, 3.0, n)))
    sign = np.where(small, rng.choice([-1.0, 1.0], n), 1.0)
    return (mag * sign).astype(np.float16).astype(np.float32)


def ordered(x):
    """The monotone integer image of f32 bits: all bits of a negative flipped, the sign bit of the others set."""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return np.where(b >> 31 == 1, ~b, b | np.uint32(0x80000000)).astype(np.uint32)


class ExplainCase:
    def __init__(self, name):
        self.name = name
        self.cw, self.dim, self.value_type = CASES[name]
        rng = np.random.default_rng(31)
        wide = self.dim >= 20000
        # the probe query's components: 40 of the window (38 with a weight, then a 0.0 and a -0.0) and, in a wide
        # vocabulary, two far ones
        probe = np.sort(rng.choice(WINDOW, 40, replace=False, p=_WINDOW_P)).astype(np.int64)
        other = np.setdiff1d(np.arange(WINDOW), probe)           # window components the probe query does not carry
        far = np.array([9000, 15000], np.int64) if wide else np.zeros(0, np.int64)
        pw = _values(rng, 40)
        pw[pw == 0] = 1.0
        pw[:6] = 1.5                                             # ties
        pw[6], pw[7] = -2.5, 2.5                                 # zeros: the -0.0 product on the SMALLER component
        pw[8], pw[9] = 3.0, -1.25
        pw[38], pw[39] = 0.0, -0.0
        docs, named = [], {}

        def add(label, c, v):
            order = np.argsort(c, kind="stable")
            named[label] = len(docs)
            docs.append((np.asarray(c, np.int64)[order].astype(np.uint32), np.asarray(v, np.float32)[order]))

        def window_doc(n):
            return np.sort(rng.choice(WINDOW, n, replace=False, p=_WINDOW_P)), _values(rng, n)

        for n in SPECIAL_LENS:
            add("len_%d" % n, *window_doc(n))
        for t in TERM_COUNTS:
            c = np.concatenate([probe[:t], rng.choice(other, 20, replace=False)])
            add("terms_%d" % t, c, _values(rng, len(c)))
        # big: 257 window components, values of magnitude <= 8; the last element holds 15 and the long query weighs it 16
        bc, bv = window_doc(257)
        bv[-1] = 15.0
        add("big", bc, bv)
        add("ties", np.concatenate([probe[:6], probe[8:10], other[:3]]),
            np.array([2.0] * 6 + [1.0, 4.0] + [1.0, 2.0, 3.0], np.float32))
        add("zeros", np.concatenate([probe[6:10], probe[38:40], other[3:5]]),
            np.array([0.0, 0.0, 1.0, -1.0, 3.0, 3.0, 1.0, 0.0], np.float32))
        if wide:
            add("far", np.concatenate([probe[:12], far, [5000, 19000]]), _values(rng, 16))
        while len(docs) < N_DOCS:
            n = int(rng.integers(2, 81))
            c, v = window_doc(n)
            if wide and len(docs) % 4 == 0:   # every fourth random document: a far tail (raw form in a DotVByte index)
                c = np.concatenate([c, [9000 + 4200 * i + int(rng.integers(0, 50)) * (i > 0) for i in range(2)]])
                v = np.concatenate([v, _values(rng, 2)])
            docs.append((c.astype(np.uint32), v))
        self.docs, self.named = docs, named
        self.n_docs = len(docs)
        self.off, self.comps, self.vals = orc.csr(docs)

        qs = [(np.concatenate([probe, far]).astype(np.uint32), np.concatenate([pw, np.array([2.0, -3.0], np.float32)[:len(far)]]))]
        extra = rng.choice(np.setdiff1d(np.arange(WINDOW), bc), 43, replace=False)
        lc = np.sort(np.concatenate([bc, extra]))
        lw = _values(rng, 300)
        lw[lw == 0] = 1.0
        lw[np.searchsorted(lc, bc[-1])] = 16.0
        qs.append((lc.astype(np.uint32), lw))
        qs.append((np.zeros(0, np.uint32), np.zeros(0, np.float32)))
        qs.append((np.array([probe[0]], np.uint32), np.array([1.375], np.float32)))
        df = np.bincount(self.comps.astype(np.int64), minlength=self.dim)
        common = np.argsort(-df, kind="stable")[:300]
        while len(qs) < N_QUERIES:
            n = int(rng.integers(5, 61))
            qs.append((np.sort(rng.choice(common, n, replace=False)).astype(np.uint32), _values(rng, n)))
        self.queries = qs
        self.q_off, self.qc, self.qv = orc.csr(qs)

        every = np.arange(self.n_docs, dtype=np.uint64)
        rest = np.setdiff1d(every, [named["big"]]).astype(np.uint64)
        self.lists = [np.concatenate([every, np.array([5, 5, 5], np.uint64)]),
                      np.concatenate([np.array([named["big"]], np.uint64), rest[:126]]),
                      every[:128], every[100:229], np.zeros(0, np.uint64), np.array([named["terms_10"]], np.uint64),
                      every[::-1].copy(), rng.integers(0, self.n_docs, 100).astype(np.uint64)]
        self.cand_off = np.zeros(N_QUERIES + 1, np.uint64)
        self.cand_off[1:] = np.cumsum([len(x) for x in self.lists])
        self.cand_ids = np.concatenate(self.lists).astype(np.uint64)
        self._index = None
        self._pairs = None
        self._expected = {}

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

    def row_of(self, query, label):
        """The row (candidate number) of document `label` in the list of `query` (its first occurrence)."""
        at = np.flatnonzero(self.lists[query] == self.named[label])[0]
        return int(self.cand_off[query]) + int(at)

    def tiny_weight_call(self):
        """(q_off, comps, vals, cand_off, cand_ids, want n_terms): two one-component queries on the first probe component
        against the document `terms_1`, which stores it - the weights 2^-149, whose product with a val_scale below 1 is
        +0.0, and 2^-100, whose product is not. The header counts the first as a weight of +-0 for fixed-u8 codes: no term."""
        c = self.queries[0][0][:1]
        tiny = np.array([2.0 ** -149, 2.0 ** -100], np.float32)
        want = [int(tiny[0] * self.stored()[3] != 0), 1]
        doc = np.array([self.named["terms_1"]] * 2, np.uint64)
        two = np.array([0, 1, 2], np.uint64)
        return two, np.concatenate([c, c]).astype(np.uint32), tiny, two.copy(), doc, want

    # ---- the restatement ----
    def stored(self):
        """The forward index as the descriptor gives it: offsets, components, the values as the f32 they stand for in the
        product (binary16 widened; fixed-u8: the code), and the scale a code is multiplied with (1 for binary16)."""
        d = self.index.desc
        a = orc.desc_arrays(d)
        off = a["fwd_offsets"].astype(np.int64)
        if d.value_type == 0:
            x, scale = a["fwd_vals"].view(np.float16).astype(np.float32), np.float32(1.0)
        else:
            x, scale = a["fwd_vals"].astype(np.float32), np.float32(d.val_scale)
        return off, a["fwd_comps"].astype(np.int64), x, scale

    def pairs(self):
        """Per candidate: (score f32, the pair's terms in the contract's order as arrays component, w, document value,
        product, element position)."""
        if self._pairs is not None:
            return self._pairs
        off, comps, x, scale = self.stored()
        lane_of = (np.arange(512) // 8) % 16
        xor = np.arange(16)
        out = []
        for q, (qc, qw) in enumerate(self.queries):
            given = np.zeros(self.dim, np.float32)
            given[qc.astype(np.int64)] = qw
            table = given if self.value_type == 0 else given * scale   # (f32 * f32, a power of two: exact)
            cache = {}
            for d in self.lists[q].astype(np.int64).tolist():
                if d not in cache:
                    c, v = comps[off[d]:off[d + 1]], x[off[d]:off[d + 1]]
                    p = table[c] * v                                 # one f32 rounding per element
                    lane = lane_of[:len(c)]
                    t = np.zeros(16, np.float32)
                    for j in range(16):
                        pj = p[lane == j]
                        if len(pj):
                            t[j] = np.cumsum(np.concatenate([np.zeros(1, np.float32), pj]), dtype=np.float32)[-1]
                    for s in (8, 4, 2, 1):
                        t = t + t[xor ^ s]
                    # terms: stored elements of a weight that is not +-0 (fixed-u8: nor is its product with val_scale)
                    e = np.flatnonzero((given[c] != 0) & (table[c] != 0))
                    key = (ordered(p[e]).astype(np.uint64) << np.uint64(32)) | (~c[e].astype(np.uint32)).astype(np.uint64)
                    e = e[np.argsort(key, kind="stable")[::-1]]
                    cache[d] = (t[0], c[e].astype(np.uint32), given[c[e]], (v[e] * scale).astype(np.float32), p[e], e)
                out.append(cache[d])
        self._pairs = out
        return out

    def expected(self, m, pairs=None):
        """The six output arrays of the call on (cand_off, cand_ids) with `m`, from pairs() (or a variant of it)."""
        if pairs is None and m in self._expected:
            return self._expected[m]
        src = self.pairs() if pairs is None else pairs
        n = len(src)
        sc, nt = np.zeros(n, np.float32), np.zeros(n, np.uint32)
        tc, tq, td, tp = (np.zeros((n, m), np.uint32), np.zeros((n, m), np.float32), np.zeros((n, m), np.float32),
                          np.zeros((n, m), np.float32))
        for i, (s, c, w, v, p, _) in enumerate(src):
            k = min(m, len(c))
            sc[i], nt[i] = s, len(c)
            tc[i, :k], tq[i, :k], td[i, :k], tp[i, :k] = c[:k], w[:k], v[:k], p[:k]
        got = (sc, nt, tc, tq, td, tp)
        if pairs is None:
            for a in got:
                a.setflags(write=False)
            self._expected[m] = got
        return got

    def check(self):
        """The case holds the edges it is named for (asserted with the restatement and the stored arrays alone)."""
        off, comps, x, scale = self.stored()
        lens = np.diff(off)
        assert np.array_equal(lens, np.diff(self.off.astype(np.int64))), "the index stores other document lengths"
        for n in SPECIAL_LENS:
            assert lens[self.named["len_%d" % n]] == n
        pr = self.pairs()
        for t in TERM_COUNTS:
            assert len(pr[self.row_of(0, "terms_%d" % t)][1]) == t
        big = pr[self.row_of(1, "big")]
        assert len(big[1]) == 257 and big[5][0] == 256 and len(set((big[5][:10] // 128).tolist())) > 1
        ties = pr[self.row_of(0, "ties")]
        assert len(np.unique(ties[4].view(np.uint32))) < len(ties[4])
        z = pr[self.row_of(0, "zeros")]
        bits = z[4].view(np.uint32).tolist()
        assert 0 in bits and 0x80000000 in bits and len(z[1]) == 4 and np.count_nonzero(z[3] == 0) >= 2
        # the -0.0 term on the smaller component: the contract puts it AFTER the +0.0 term, a numeric comparison before
        assert z[1][bits.index(0x80000000)] < z[1][bits.index(0)] and bits.index(0) < bits.index(0x80000000)
        assert any((p[4] < 0).any() for p in pr)
        if self.value_type == 2:
            raw, _ = self.index.stream_stats()
            assert 1 <= raw < self.n_docs and self.dim < 32768
        assert (self.dim >= 32768) == (self.cw == 4)


def same(got, want):
    """None if the six arrays agree bit for bit, else the name of the first that does not and where."""
    for name, a, b in zip(("scores", "n_terms", "comps", "q_vals", "d_vals", "products"), got, want):
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
        case = ExplainCase(name)
        case.check()
        _MADE[name] = case
    return _MADE[name]
