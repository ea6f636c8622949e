"""Shared data of the collapse_documents tests (tests/test_collapse_cpu.py, tests/test_gpu_collapse.py). TEST
INFRASTRUCTURE.

A case = one small document collection built into an index of one form (the forms of tests/diversify_cases.py: u16 / u32
components, binary16 / fixed-u8 / DotVByte values, dim 32767 and 32768 for the dense and the hash table, dim 300) and a
list of named CALLS of sgpu_collapse_documents on it; collapse_numpy() is a RESTATEMENT of the contract written from the
text of include/seismic_hip.h alone: it decodes the descriptor's forward arrays, scores in np.float32 in the canonical
order, forms the groups' members, sums and rows with Python's own sort. With reading=... it implements one WRONG reading
of the contract instead; every named call says which reading it catches.

Documents by name: one_0 .. one_5 (one stored value 1.0 each, on components of their own), tie_0 .. tie_5 (exact duplicates
of one another), len_N (N = 0, 1, 7, 8, 9, 127, 128, 129, 300), far (dim >= 20000: the raw record form of a DotVByte
index), then random ones; stored values are multiples of 1/16 up to 8, so every form holds the same numbers.
Calls and the wrong reading each catches:
  sum_order  one group of the scores 2^24, 1, 1 (query weights 16777216, 1, 1 on the one_ documents): best first gives
             2^24, ascending or a float64 sum 2^24 + 2                                  ("ascending", "float64")
  top_m      groups of 1, 2, 3, 4, 63, 64, 65 members at m = 1, 2, 3, 64: m - 1, m and m + 1 each   ("sum_all")
  dups       a pair listed three times                                                  ("dup_twice": sum and members)
  two_keys   one id under two keys                                                      ("group_of_id": one group only)
  ties       groups of equal score ("ties_high": key descending); equal-score members ("best_high": the larger id)
  keys       the group keys 0, 1, 0x7fffffff, 0x80000000, 0xfffffffe, 0xffffffff at once, k beyond the group count
             (a padding value that collides with a key)
  negative   groups whose scores are all negative, beside an empty query whose groups all score +0.0 (key order)
  counts     queries of 1, 2, 63, 64, 65, 127, 128, 129, 511, 512, 513, 1023, 1024, 1025, 4095, 4096 entries (the edges of
             the device's four sort sizes); at 4096 also one single
             group, all keys distinct, and runs of 3 (which straddle every thread's and wave's span of the sorted array)
  ks         k = 1, groups - 1, groups, groups + 1, 1024
  empty      no candidates / empty query with candidates / both                         (rows not zeroed)
  random     eight queries of signed weights, 40 entries, about 12 groups
"""
import numpy as np

import orc
from diversify_cases import BUILD, CASES, _q, _values
from diversify_cases import same as _same
from seismic_amd import _native
from seismic_amd._abi import BuildConfig

N_DOCS = 200
SPECIAL_LENS = (0, 1, 7, 8, 9, 127, 128, 129, 300)
COUNTS = (1, 2, 63, 64, 65, 127, 128, 129, 511, 512, 513, 1023, 1024, 1025, 4095, 4096)
EDGE_KEYS = (0, 1, 0x7fffffff, 0x80000000, 0xfffffffe, 0xffffffff)
READINGS = ("ascending", "float64", "sum_all", "dup_twice", "group_of_id", "ties_high", "best_high")
NAMES = ("out_groups", "out_scores", "out_best_ids", "out_best_scores", "out_members", "out_n")


def same(got, want, names=NAMES):
    """None if the arrays agree bit for bit, else the name of the first that does not and where."""
    return _same(got, want, names)


class Call:
    def __init__(self, name, queries, lists, groups, ms, ks):
        self.name, self.queries, self.ms, self.ks = name, queries, tuple(ms), tuple(ks)
        self.lists = [np.asarray(x, np.uint64) for x in lists]
        self.groups = [np.asarray(x, np.uint32) for x in groups]
        assert len(queries) == len(lists) == len(groups)
        assert [len(x) for x in self.lists] == [len(x) for x in self.groups]
        self.nq = len(queries)
        self.q_off, self.qc, self.qv = orc.csr(queries)
        self.cand_off = np.zeros(self.nq + 1, np.uint64)
        self.cand_off[1:] = np.cumsum([len(x) for x in self.lists])
        self.cand_ids = np.concatenate(self.lists).astype(np.uint64)
        self.cand_groups = np.concatenate(self.groups).astype(np.uint32)

    def args(self, order=None):
        """The call's arguments up to cand_groups; order: per query a permutation of its entries."""
        if order is None:
            return self.q_off, self.qc, self.qv, self.cand_off, self.cand_ids, self.cand_groups
        ids = np.concatenate([x[o] for x, o in zip(self.lists, order)]).astype(np.uint64)
        grp = np.concatenate([x[o] for x, o in zip(self.groups, order)]).astype(np.uint32)
        return self.q_off, self.qc, self.qv, self.cand_off, ids, grp


class CollapseCase:
    def __init__(self, name):
        self.name = name
        self.cw, self.dim, self.value_type = CASES[name]
        dim = self.dim
        rng = np.random.default_rng(71)
        window = min(2000, dim)
        p = 1.0 / (np.arange(window - 1) + 20.0)
        p /= p.sum()
        docs, named = [], {}

        def add(label, c, v):
            assert len(c) == len(v) and (np.diff(np.asarray(c, np.int64)) > 0).all()
            named[label] = len(docs)
            docs.append((np.asarray(c, np.uint32), np.asarray(v, np.float32)))

        def window_doc(n, last=False):
            if n == 0:
                return np.zeros(0, np.int64), np.zeros(0, np.float32)
            if n >= window:
                return np.arange(window), _values(rng, window)
            if last:   # ends on the window's last component
                return np.append(np.sort(rng.choice(window - 1, n - 1, replace=False, p=p)), window - 1), _values(rng, n)
            return np.sort(rng.choice(window - 1, n, replace=False, p=p)), _values(rng, n)

        for i in range(6):
            add("one_%d" % i, [100 + i], [1.0])
        for i in range(6):
            add("tie_%d" % i, [160, 161], [4.0, 2.0])
        for n in SPECIAL_LENS:
            add("len_%d" % n, *window_doc(n, last=True))
        if dim >= 20000:
            add("far", [0, 5000, 15000, dim - 1], [3.0, 0.5, 1.25, 4.0])
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
        self._scores = {}

        def rq(n, signed=False):
            c = np.sort(rng.choice(window, n, replace=False)).astype(np.uint32)
            w = _values(rng, n)
            if signed:
                w[rng.random(n) < 0.3] *= -1.0
            return c, w

        def draw(n):
            return rng.integers(0, N_DOCS, n)

        none = np.zeros(0, np.int64)
        empty_q = (np.zeros(0, np.uint32), np.zeros(0, np.float32))
        d = named
        calls = []
        calls.append(Call("sum_order", [_q([(100, 16777216.0), (101, 1.0), (102, 1.0)])], [[d["one_1"], d["one_0"], d["one_2"]]],
                          [[7, 7, 7]], (3, 2), (1,)))
        sizes = (1, 2, 3, 4, 63, 64, 65)
        scoring = np.array([i for i in range(N_DOCS) if i != d["len_0"]])   # (a score above 0 for the query of every component)
        ids = np.concatenate([rng.choice(scoring, n, replace=False) for n in sizes])
        grp = np.concatenate([np.full(n, 1000 + n) for n in sizes])
        mix = rng.permutation(len(ids))
        all_q = (np.arange(window, dtype=np.uint32), _values(rng, window))
        calls.append(Call("top_m", [all_q], [ids[mix]], [grp[mix]], (1, 2, 3, 64), (7, 3)))
        some = [d["len_127"], d["len_128"], d["len_129"], d["len_9"]]
        calls.append(Call("dups", [rq(min(300, window))], [[some[0], some[1], some[0], some[2], some[0]]], [[5, 5, 5, 6, 5]],
                          (2, 1), (2, 1)))
        calls.append(Call("two_keys", [rq(min(300, window))], [[some[0], some[1], some[0], some[3]]], [[9, 9, 3, 3]], (1, 2), (3, 1)))
        tq = _q([(160, 2.0), (161, 1.0)])
        t = [d["tie_%d" % i] for i in range(6)]
        calls.append(Call("ties", [tq], [[t[0], t[5], t[1], t[3], t[2], t[4]]], [[10, 20, 4, 20, 8, 20]], (1, 2), (1, 2, 4, 5)))
        ids = draw(3 * len(EDGE_KEYS))
        grp = np.repeat(np.array(EDGE_KEYS, np.uint32), 3)
        mix = rng.permutation(len(ids))
        calls.append(Call("keys", [rq(30)], [ids[mix]], [grp[mix]], (1, 2), (6, 7, 1024)))
        neg_q = (np.arange(window, dtype=np.uint32), np.full(window, -1.0, np.float32))
        ids = np.concatenate([draw(20), [d["len_1"]]])
        ids = ids[ids != d["len_0"]]   # (the empty document scores +0.0)
        grp = rng.integers(0, 6, len(ids))
        calls.append(Call("negative", [neg_q, empty_q], [ids, ids[::-1]], [grp, (grp[::-1] * 977) % 13], (1, 3), (6, 2)))
        lists = [draw(n) for n in COUNTS] + [draw(4096) for _ in range(3)]
        groups = [rng.integers(0, max(1, n // 4), n) for n in COUNTS]
        groups += [np.full(4096, 0xffffffff, np.uint32), rng.permutation(4096) * 1048573 % (2 ** 32), np.arange(4096) // 3]
        calls.append(Call("counts", [rq(int(rng.integers(5, 30))) for _ in lists], lists, groups, (1, 3), (1, 10)))
        grp = np.concatenate([np.arange(12), rng.integers(0, 12, 28)])
        calls.append(Call("ks", [rq(30)], [draw(40)], [grp], (1, 2), (1, 11, 12, 13, 1024)))
        signed = rq(12, signed=True)
        calls.append(Call("empty", [signed, empty_q, empty_q], [none, draw(3), none], [none, [5, 2, 5], none], (1, 2), (1, 8)))
        calls.append(Call("random", [rq(int(rng.integers(5, 40)), signed=True) for _ in range(8)], [draw(40) for _ in range(8)],
                          [rng.integers(0, 12, 40) * 1000003 for _ in range(8)], (1, 3), (10, 40)))
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

    def expected(self, call, m, k):
        """collapse_numpy of the named call at m and k, computed once and shared (read-only)."""
        key = (call, m, k)
        if key not in self._expected:
            got = collapse_numpy(self, self.calls[call], m, k)
            for a in got:
                a.setflags(write=False)
            self._expected[key] = got
        return self._expected[key]

    def check(self):
        """The case holds the edges it is named for (asserted with the restatement and the stored arrays alone)."""
        off, comps, x, scale = self.stored()
        lens = np.diff(off)
        assert np.array_equal(lens, np.diff(self.off.astype(np.int64))), "the index stores other document lengths"
        assert np.array_equal((x if scale is None else x * scale), self.vals), "the index does not hold the values given"
        if self.value_type == 2:
            raw, _ = self.index.stream_stats()
            assert 1 <= raw < self.n_docs
        g, s, ids, bs, mem, n = self.expected("sum_order", 3, 1)
        assert s[0, 0] == np.float32(2.0 ** 24) and bs[0, 0] == s[0, 0] and mem[0, 0] == 3 and ids[0, 0] == self.named["one_0"]
        g, s, ids, bs, mem, n = self.expected("top_m", 64, 7)
        assert sorted(mem[0].tolist()) == [1, 2, 3, 4, 63, 64, 65]
        g, s, ids, bs, mem, n = self.expected("dups", 2, 2)
        assert n[0] == 2 and dict(zip(g[0].tolist(), mem[0].tolist())) == {5: 2, 6: 1}
        g, s, ids, bs, mem, n = self.expected("two_keys", 1, 3)
        assert n[0] == 2 and sorted(mem[0, :2].tolist()) == [2, 2]
        g, s, ids, bs, mem, n = self.expected("ties", 1, 5)
        assert n[0] == 4 and g[0, :4].tolist() == [4, 8, 10, 20] and len(set(s[0, :4].tolist())) == 1
        assert ids[0, 3] == self.named["tie_3"] and mem[0, 3] == 3
        g, s, ids, bs, mem, n = self.expected("keys", 1, 1024)
        assert n[0] == 6 and sorted(g[0, :6].tolist()) == list(EDGE_KEYS) and not g[0, 6:].any()
        g, s, ids, bs, mem, n = self.expected("negative", 1, 6)
        assert (s[0, :n[0]] < 0).all() and n[0] >= 2
        assert not s[1].view(np.uint32).any() and (np.diff(g[1, :n[1]].astype(np.int64)) > 0).all() and n[1] >= 2
        g, s, ids, bs, mem, n = self.expected("counts", 1, 10)
        assert n[-3:].tolist() == [1, 10, 10] and mem[-3, 0] == len(set(self.calls["counts"].lists[-3].tolist()))
        g, s, ids, bs, mem, n = self.expected("ks", 1, 1024)
        assert n[0] == 12
        g, s, ids, bs, mem, n = self.expected("empty", 1, 8)
        assert n.tolist() == [0, 2, 0] and g[1, :2].tolist() == [2, 5]


def _ordered(x):
    b = int(np.float32(x).view(np.uint32))
    return (~b) & 0xffffffff if b & 0x80000000 else b | 0x80000000


def collapse_numpy(case, call, m, k, reading=None, order=None):
    """(out_groups u32, out_scores f32, out_best_ids u64, out_best_scores f32, out_members u32 - all [nq, k] -, out_n u32
    [nq]) of sgpu_collapse_documents as include/seismic_hip.h defines it; reading: one of READINGS, a wrong reading of the
    contract implemented instead; order: per query a permutation of its entries."""
    off, comps, x, scale = case.stored()
    f32, f64 = np.float32, np.float64

    def score(W, d):
        """The canonical sum of document d against the table W."""
        c, v = comps[off[d]:off[d + 1]], x[off[d]:off[d + 1]]
        prod = W[c] * v   # (f32 arrays: one rounding per product)
        assert prod.dtype == f32
        padded = np.zeros((len(prod) + 127) // 128 * 128, f32)   # (+0.0 added to an accumulator changes no bit of it)
        padded[:len(prod)] = prod
        rows = padded.reshape(-1, 16, 8).transpose(1, 0, 2).reshape(16, -1)   # accumulator j: its elements in increasing e
        t = np.add.accumulate(np.concatenate([np.zeros((16, 1), f32), rows], axis=1), axis=1)[:, -1]
        j = np.arange(16)
        for s in (8, 4, 2, 1):
            t = t + t[j ^ s]
        return f32(t[0])

    out_g, out_s = np.zeros((call.nq, k), np.uint32), np.zeros((call.nq, k), f32)
    out_ids, out_bs = np.zeros((call.nq, k), np.uint64), np.zeros((call.nq, k), f32)
    out_mem, out_n = np.zeros((call.nq, k), np.uint32), np.zeros(call.nq, np.uint32)
    for q, (qc, qw) in enumerate(call.queries):
        ids, grp = call.lists[q], call.groups[q]
        if order is not None:
            ids, grp = ids[order[q]], grp[order[q]]
        ids, grp = [int(i) for i in ids], [int(g) for g in grp]
        score_of = case._scores.setdefault((call.name, q), {})   # (a document's score for this query, computed once)
        W = None
        for i in set(ids) - set(score_of):
            if W is None:
                W = np.zeros(case.dim, f32)
                W[qc.astype(np.int64)] = qw if scale is None else qw * scale   # (f32 arrays; a power of two: exact)
            score_of[i] = score(W, i)
        if reading == "group_of_id":   # every id in the group of its first listing only
            first = {}
            grp = [first.setdefault(i, g) for i, g in zip(ids, grp)]
        members = {}
        for i, g in zip(ids, grp):
            mem = members.setdefault(g, [])
            if reading == "dup_twice" or i not in mem:
                mem.append(i)
        rows = []
        for g, mem in members.items():
            mem.sort(key=lambda i: (-_ordered(score_of[i]), -i if reading == "best_high" else i))
            head = [score_of[i] for i in (mem if reading == "sum_all" else mem[:m])]
            if reading == "ascending":
                head = head[::-1]
            if reading == "float64":
                s = f32(sum(f64(v) for v in head))
            else:
                s = head[0]
                for v in head[1:]:
                    s = f32(s + v)
            rows.append((g, s, mem[0], score_of[mem[0]], len(mem)))
        rows.sort(key=lambda r: (-_ordered(r[1]), -r[0] if reading == "ties_high" else r[0]))
        rows = rows[:k]
        for j, (g, s, best, bs, cnt) in enumerate(rows):
            out_g[q, j], out_s[q, j], out_ids[q, j], out_bs[q, j], out_mem[q, j] = g, s, best, bs, cnt
        out_n[q] = len(rows)
    return out_g, out_s, out_ids, out_bs, out_mem, out_n


def permuted(call, seed=3):
    """Per query a permutation of its entries."""
    rng = np.random.default_rng(seed)
    return [rng.permutation(len(x)) for x in call.lists]


_MADE = {}


def make(name):
    """The case `name`, built and checked once per process."""
    if name not in _MADE:
        case = CollapseCase(name)
        case.check()
        _MADE[name] = case
    return _MADE[name]
