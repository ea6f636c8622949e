"""Shared data of the fuse_documents tests (tests/test_fuse_cpu.py, tests/test_gpu_fuse.py). TEST INFRASTRUCTURE.

A case = one document collection built into an index of one form (the forms of tests/diversify_cases.py: u16 / u32
components, binary16 / fixed-u8 / DotVByte values, dim 32767 and 32768 for the dense and the hash table, dim 300) and a
list of named CALLS of sgpu_fuse_documents on it; fuse_numpy() is a RESTATEMENT of the contract written from the text of
include/seismic_hip.h alone: it decodes the descriptor's forward arrays, scores in np.float32 in the canonical order,
picks every document's external score, ranks with Python's own sort and fuses in np.float32, one rounding per operation.
With reading=... it implements one WRONG reading of the contract instead; every named call says which reading it catches.

Documents: the 200 of tests/collapse_cases.py (one_0 .. one_5, tie_0 .. tie_5, len_N, far, random ones), then 4000 short
ones (1 - 6 components): the documents of a query are its distinct IDS, so a query of 4096 documents needs that many ids.
External scores are normal f32 numbers, NaN (of several payloads) where the document is not in the other list.
Calls and the wrong reading each catches:
  ties       the six tie_ documents (one sparse score) with equal, different and absent external scores
                                                                        ("shared_ranks", "ties_high", "zero_based")
  dups       ids listed three times and twice: largest external score not listed first, NaN between, all NaN
                                                                        ("dup_first", "dup_twice")
  absent     half the documents absent, the present ones' scores on both sides of 0      ("absent_is_zero")
  flat       one sparse score for all (the tie_ documents), one present document, one external score for all
                                                                        ("flat_is_zero")
  negzero    an empty query (every sparse score +0.0) under w_sparse = -1: the present document with ext = -0.0 fuses to
             -0.0, the absent one to +0.0, and the smaller id is the present one's       ("neg_zero_equal")
  methods    all three methods with positive, negative and zero weights, rrf_c 0, 1, 60  ("float64", "contracted")
  counts     queries of 1, 2, 63, 64, 65, 127, 128, 129, 511, 512, 513, 1023, 1024, 1025, 4095, 4096 entries (the edges of
             the device's four sort sizes); at 4096 also all entries one id, every id listed twice with two external
             scores (2048 documents), 4096 documents none present, and all present
  ks         k = 1, |D| - 1, |D|, |D| + 1, 1024
  empty      no candidates / empty query with candidates / both                          (rows not zeroed)
  random     eight queries of signed weights, 60 entries, about half present
"""
import numpy as np

import orc
from collapse_cases import CASES, COUNTS, CollapseCase
from diversify_cases import _q, _values
from diversify_cases import same as _same

RRF, MINMAX, SUM = 0, 1, 2
N_FILL = 4000
READINGS = ("shared_ranks", "zero_based", "absent_is_zero", "dup_first", "dup_twice", "float64", "contracted", "flat_is_zero",
            "ties_high", "neg_zero_equal")
NAMES = ("out_scores", "out_doc_ids", "out_sparse", "out_ext", "out_rank_sparse", "out_rank_ext", "out_n")
NAN_BITS = (0x7fc00000, 0xffc00000, 0x7fc00001, 0x7f800001, 0xffffffff, 0x7fffffff)   # quiet, negative, payloads, signalling


def same(got, want, names=NAMES):
    """None if the arrays agree bit for bit, else the name of the first that does not and where."""
    return _same(got, want, names)


def _ext(values, nan_at=()):
    """f32 array of `values`; None, and every place of nan_at, becomes a NaN whose payload changes from place to place."""
    x = np.array([np.nan if v is None else v for v in values], np.float32)
    bits = x.view(np.uint32)
    for n, i in enumerate(sorted(set(np.flatnonzero(np.isnan(x)).tolist()) | set(nan_at))):
        bits[i] = NAN_BITS[n % len(NAN_BITS)]
    return x


class Call:
    def __init__(self, name, queries, lists, exts, configs, ks):
        """configs: (method, w_sparse, w_ext, rrf_c) each."""
        self.name, self.queries, self.ks = name, queries, tuple(ks)
        self.configs = tuple((int(m), float(np.float32(a)), float(np.float32(b)), float(np.float32(c))) for m, a, b, c in configs)
        self.lists = [np.asarray(x, np.uint64) for x in lists]
        self.exts = [x if isinstance(x, np.ndarray) and x.dtype == np.float32 else _ext(list(x)) for x in exts]
        assert len(queries) == len(lists) == len(exts)
        assert [len(x) for x in self.lists] == [len(x) for x in self.exts]
        self.nq = len(queries)
        self.q_off, self.qc, self.qv = orc.csr(queries)
        self.cand_off = np.zeros(self.nq + 1, np.uint64)
        self.cand_off[1:] = np.cumsum([len(x) for x in self.lists])
        self.cand_ids = np.concatenate(self.lists).astype(np.uint64)
        self.cand_ext = np.concatenate(self.exts).astype(np.float32)
        assert not np.isinf(self.cand_ext).any()

    def args(self, order=None):
        """The call's arguments up to cand_ext; order: per query a permutation of its entries."""
        if order is None:
            return self.q_off, self.qc, self.qv, self.cand_off, self.cand_ids, self.cand_ext
        ids = np.concatenate([x[o] for x, o in zip(self.lists, order)]).astype(np.uint64)
        ext = np.concatenate([x[o] for x, o in zip(self.exts, order)]).astype(np.float32)
        return self.q_off, self.qc, self.qv, self.cand_off, ids, ext


DEFAULT = ((RRF, 1.0, 1.0, 60.0), (MINMAX, 0.5, 0.25, 0.0), (SUM, 1.0, 0.5, 0.0))


class FuseCase(CollapseCase):
    def __init__(self, name):
        super().__init__(name)   # (the 200 documents of the collapse cases, by name)
        rng = np.random.default_rng(91)
        dim = self.dim
        window = min(2000, dim)
        for _ in range(N_FILL):
            n = int(rng.integers(1, 7))
            self.docs.append((np.sort(rng.choice(window, n, replace=False)).astype(np.uint32), _values(rng, n)))
        self.n_docs = len(self.docs)
        self.off, self.comps, self.vals = orc.csr(self.docs)
        n_docs, d = self.n_docs, self.named

        def rq(n, signed=False):
            c = np.sort(rng.choice(window, n, replace=False)).astype(np.uint32)
            w = _values(rng, n)
            if signed:
                w[rng.random(n) < 0.3] *= -1.0
            return c, w

        def draw(n):
            return rng.integers(0, n_docs, n)

        def ext(n, present=0.5):
            """n external scores, normal f32 numbers of either sign, absent with probability 1 - present."""
            x = rng.normal(0.0, 4.0, n).astype(np.float32)
            x[np.abs(x) < 1e-3] = 1.0
            return _ext(x, np.flatnonzero(rng.random(n) >= present).tolist())

        none = np.zeros(0, np.int64)
        empty_q = (np.zeros(0, np.uint32), np.zeros(0, np.float32))
        calls = []
        t = [d["tie_%d" % i] for i in range(6)]
        tq = _q([(160, 2.0), (161, 1.0)])
        calls.append(Call("ties", [tq], [[t[0], t[5], t[1], t[3], t[2], t[4], d["one_0"], d["len_9"]]],
                          [[1.0, 1.0, None, 1.0, 2.0, None, 1.0, 2.0]],
                          ((RRF, 1.0, 1.0, 60.0), (RRF, 1.0, 0.5, 0.0), (MINMAX, 1.0, 1.0, 0.0), (SUM, 1.0, 1.0, 0.0)), (1, 4, 8)))
        a, b, c, e, f = d["len_127"], d["len_128"], d["len_129"], d["len_9"], d["len_8"]
        calls.append(Call("dups", [rq(min(300, window))], [[a, b, a, c, a, b, e, e, f]],
                          [[1.0, None, 3.0, 0.5, None, None, -2.0, -1.0, 0.75]], DEFAULT, (2, 5, 6)))
        ids = rng.choice(n_docs, 12, replace=False)
        calls.append(Call("absent", [rq(40)], [ids], [[-3.0, None, 2.5, None, -0.5, None, 1.25, None, -7.0, None, 4.0, None]],
                          DEFAULT, (12, 5)))
        others = rng.choice(np.arange(200, n_docs), 6, replace=False)
        calls.append(Call("flat", [tq, rq(30), rq(30)], [t, others, others],
                          [[0.5, 1.5, None, -2.0, 3.0, 0.25], [None, None, 1.5, None, None, None], [2.5] * 6],
                          ((MINMAX, 1.0, 1.0, 0.0), (MINMAX, 0.5, -2.0, 0.0), (RRF, 1.0, 1.0, 1.0)), (6, 3)))
        lo, hi = sorted(rng.choice(n_docs, 2, replace=False).tolist())
        calls.append(Call("negzero", [empty_q], [[hi, lo]], [[None, -0.0]], ((SUM, -1.0, 1.0, 0.0), (SUM, 1.0, 1.0, 0.0)), (2, 1)))
        weights = ((1.0, 1.0), (-1.0, 0.5), (0.0, 1.0), (1.0, 0.0), (0.3, -0.7), (0.0, 0.0), (0.1, 0.3))
        configs = [(RRF, a, b, c) for a, b in weights for c in (0.0, 1.0, 60.0)]
        configs += [(m, a, b, 0.0) for m in (MINMAX, SUM) for a, b in weights]
        calls.append(Call("methods", [rq(25, signed=True)], [draw(60)], [ext(60)], configs, (20,)))
        lists = [draw(n) for n in COUNTS]
        exts = [ext(n) for n in COUNTS]
        one = int(draw(1)[0])
        lists.append(np.full(4096, one))                               # all entries one id
        exts.append(ext(4096, 0.9))
        twice = rng.permutation(np.repeat(rng.choice(n_docs, 2048, replace=False), 2))
        lists.append(twice)                                            # every id twice, two external scores
        exts.append(ext(4096, 1.0))
        lists.append(rng.choice(n_docs, 4096, replace=False))          # 4096 documents, none present
        exts.append(ext(4096, 0.0))
        lists.append(rng.choice(n_docs, 4096, replace=False))          # 4096 documents, all present
        exts.append(ext(4096, 1.0))
        calls.append(Call("counts", [rq(int(rng.integers(5, 30))) for _ in lists], lists, exts, DEFAULT, (1, 10)))
        ids = rng.choice(n_docs, 12, replace=False)
        calls.append(Call("ks", [rq(30)], [np.concatenate([ids, rng.choice(ids, 28)])], [ext(40)], DEFAULT[:1], (1, 11, 12, 13, 1024)))
        signed = rq(12, signed=True)
        two = rng.choice(n_docs, 2, replace=False)
        calls.append(Call("empty", [signed, empty_q, empty_q], [none, two[[0, 1, 0]], none], [_ext([]), _ext([None, 2.0, -1.0]), _ext([])],
                          DEFAULT, (1, 8)))
        calls.append(Call("random", [rq(int(rng.integers(5, 40)), signed=True) for _ in range(8)], [draw(60) for _ in range(8)],
                          [ext(60) for _ in range(8)], DEFAULT + ((SUM, 0.3, -0.7, 0.0), (MINMAX, -0.3, 0.7, 0.0)), (10, 60)))
        self.calls = {c.name: c for c in calls}

    def expected(self, call, config, k):
        """fuse_numpy of the named call under config and k, computed once and shared (read-only)."""
        key = (call, config, k)
        if key not in self._expected:
            got = fuse_numpy(self, self.calls[call], config, k)
            for a in got:
                a.setflags(write=False)
            self._expected[key] = got
        return self._expected[key]

    def check(self):
        """The case holds the edges it is named for (asserted with the restatement and the stored arrays alone)."""
        off, comps, x, scale = self.stored()
        assert np.array_equal(np.diff(off), np.diff(self.off.astype(np.int64))), "the index stores other document lengths"
        assert np.array_equal((x if scale is None else x * scale), self.vals), "the index does not hold the values given"
        call = self.calls["ties"]
        f, ids, sp, ex, rs, re, n = self.expected("ties", call.configs[0], 8)
        tie = [self.named["tie_%d" % i] for i in range(6)]
        at = [ids[0].tolist().index(i) for i in tie]
        assert len(set(sp[0, at].tolist())) == 1 and sorted(rs[0, at].tolist()) == list(range(1, 7)) and n[0] == 8
        assert sorted(re[0].tolist()) == [0, 0, 1, 2, 3, 4, 5, 6]
        f, ids, sp, ex, rs, re, n = self.expected("dups", self.calls["dups"].configs[0], 6)
        got = dict(zip(ids[0, :5].tolist(), ex[0, :5].tolist()))
        assert n[0] == 5 and got == {self.named["len_127"]: 3.0, self.named["len_128"]: 0.0, self.named["len_129"]: 0.5,
                                     self.named["len_9"]: -1.0, self.named["len_8"]: 0.75}
        f, ids, sp, ex, rs, re, n = self.expected("negzero", self.calls["negzero"].configs[0], 2)
        assert f[0].view(np.uint32).tolist() == [0, 0x80000000] and ids[0, 0] > ids[0, 1] and re[0].tolist() == [0, 1]
        call = self.calls["counts"]
        f, ids, sp, ex, rs, re, n = self.expected("counts", call.configs[0], 10)
        docs = [len(set(x.tolist())) for x in call.lists]
        assert docs[-4:] == [1, 2048, 4096, 4096] and n.tolist() == [min(10, x) for x in docs]
        assert not re[-2].any() and re[-1].all() and rs[-1].max() <= 4096
        assert not np.isnan(call.exts[-1]).any() and np.isnan(call.exts[-2]).all()
        f, ids, sp, ex, rs, re, n = self.expected("ks", self.calls["ks"].configs[0], 1024)
        assert n[0] == 12
        f, ids, sp, ex, rs, re, n = self.expected("empty", self.calls["empty"].configs[0], 8)
        assert n.tolist() == [0, 2, 0]


def _ordered(x):
    b = int(np.float32(x).view(np.uint32))
    return (~b) & 0xffffffff if b & 0x80000000 else b | 0x80000000


def _scores(case, W, docs):
    """{document: its canonical f32 sum against the table W}: 16 accumulators, element e to accumulator (e / 8) % 16 in
    increasing e, then t[j] += t[j ^ s] for s = 8, 4, 2, 1."""
    off, comps, x, scale = case.stored()
    f32 = np.float32
    by_len, out = {}, {}
    for d in docs:
        by_len.setdefault(max(1, (int(off[d + 1] - off[d]) + 127) // 128) * 128, []).append(d)
    j = np.arange(16)
    for width, ds in by_len.items():
        prod = np.zeros((len(ds), width), f32)   # (+0.0 added to an accumulator changes no bit of it)
        for r, d in enumerate(ds):
            a, b = off[d], off[d + 1]
            p = W[comps[a:b]] * x[a:b]   # (f32 arrays: one rounding per product)
            assert p.dtype == f32
            prod[r, :b - a] = p
        rows = prod.reshape(len(ds), -1, 16, 8).transpose(0, 2, 1, 3).reshape(len(ds), 16, -1)   # accumulator j: its elements in order
        t = np.add.accumulate(np.concatenate([np.zeros((len(ds), 16, 1), f32), rows], axis=2), axis=2)[:, :, -1]
        for s in (8, 4, 2, 1):
            t = t + t[:, j ^ s]
        assert t.dtype == f32
        for r, d in enumerate(ds):
            out[d] = f32(t[r, 0])
    return out


def fuse_numpy(case, call, config, k, reading=None, order=None):
    """(out_scores f32, out_doc_ids u64, out_sparse f32, out_ext f32, out_rank_sparse u32, out_rank_ext u32 - all [nq, k] -,
    out_n u32 [nq]) of sgpu_fuse_documents as include/seismic_hip.h defines it; config: (method, w_sparse, w_ext, rrf_c);
    reading: one of READINGS, a wrong reading of the contract implemented instead; order: per query a permutation of its
    entries."""
    off, comps, x, scale = case.stored()
    f32, f64 = np.float32, np.float64
    method = config[0]
    ws, we, c = f32(config[1]), f32(config[2]), f32(config[3])
    outs = (np.zeros((call.nq, k), f32), np.zeros((call.nq, k), np.uint64), np.zeros((call.nq, k), f32), np.zeros((call.nq, k), f32),
            np.zeros((call.nq, k), np.uint32), np.zeros((call.nq, k), np.uint32), np.zeros(call.nq, np.uint32))

    def ranks(members, value):
        """{document: its ordinal rank from 1} by (ordered(value) descending, id ascending)."""
        pool = [i for i in listed if i in value] if reading == "dup_twice" else members
        pool = sorted(pool, key=lambda i: (-_ordered(value[i]), i))
        first, first_key = {}, {}
        for at, i in enumerate(pool):
            first.setdefault(i, at)
            first_key.setdefault(_ordered(value[i]), at)
        base = 0 if reading == "zero_based" else 1
        if reading == "shared_ranks":
            return {i: base + first_key[_ordered(value[i])] for i in members}
        return {i: base + first[i] for i in members}

    def normalised(members, value):
        lo, hi = min((value[i] for i in members), key=_ordered), max((value[i] for i in members), key=_ordered)
        v = np.array([value[i] for i in members], f32)
        if hi == lo:
            return dict(zip(members, np.full(len(members), 0.0 if reading == "flat_is_zero" else 1.0, f32)))
        if reading == "float64":
            return dict(zip(members, (v.astype(f64) - f64(lo)) / (f64(hi) - f64(lo))))
        return dict(zip(members, (v - lo) / f32(hi - lo)))   # (f32 arrays and scalars: each operation rounded once)

    def combine(a, wa, b, wb, there):
        """fl(fl(wa * a) + (there ? fl(wb * b) : +0.0)) over arrays."""
        if reading == "float64":
            return (f64(wa) * a.astype(f64) + np.where(there, f64(wb) * b.astype(f64), 0.0)).astype(f32)
        t = np.where(there, wb * b, f32(0.0)).astype(f32)
        if reading == "contracted":   # (the product of two f32 is exact in f64)
            return (f64(wa) * a.astype(f64) + t.astype(f64)).astype(f32)
        return (wa * a).astype(f32) + t

    with np.errstate(all="ignore"):
        for q, (qc, qw) in enumerate(call.queries):
            ids, ext = call.lists[q], call.exts[q]
            if order is not None:
                ids, ext = ids[order[q]], ext[order[q]]
            listed = [int(i) for i in ids]
            if not listed:
                continue
            score_of = case._scores.setdefault(("fuse", call.name, q), {})   # (a document's score for this query, computed once)
            todo = sorted(set(listed) - set(score_of))
            if todo:
                W = np.zeros(case.dim, f32)
                W[qc.astype(np.int64)] = qw if scale is None else qw * scale   # (f32 arrays; a power of two: exact)
                score_of.update(_scores(case, W, todo))
            given = {}
            for i, v in zip(listed, ext):
                given.setdefault(i, []).append(v)
            D = sorted(given)
            ext_of = {}
            for i, vs in given.items():
                if reading == "dup_first":
                    vs = vs[:1]
                live = [v for v in vs if not np.isnan(v)]
                if live:
                    ext_of[i] = max(live, key=_ordered)
                elif reading == "absent_is_zero":
                    ext_of[i] = f32(0.0)
            P = [i for i in D if i in ext_of]
            sparse = {i: score_of[i] for i in D}
            rs, re = ranks(D, sparse), ranks(P, ext_of)
            there = np.array([i in ext_of for i in D])
            sp = np.array([sparse[i] for i in D], f32)
            ex = np.array([ext_of.get(i, f32(0.0)) for i in D], f32)
            if method == RRF:
                fs = np.array([rs[i] for i in D]).astype(f32)
                fe = np.array([re.get(i, 1) for i in D]).astype(f32)
                if reading == "float64":
                    fused = (f64(ws) / (f64(c) + fs.astype(f64)) + np.where(there, f64(we) / (f64(c) + fe.astype(f64)), 0.0)).astype(f32)
                else:
                    fused = (ws / (c + fs)) + np.where(there, we / (c + fe), f32(0.0)).astype(f32)
            elif method == MINMAX:
                ns = normalised(D, sparse)
                ne = normalised(P, ext_of) if P else {}
                kind = f64 if reading == "float64" else f32   # (the right reading never leaves f32)
                fused = combine(np.array([ns[i] for i in D], kind), ws, np.array([ne.get(i, 0.0) for i in D], kind), we, there)
            else:
                fused = combine(sp, ws, ex, we, there)
            assert fused.dtype == f32
            key = (lambda v: _ordered(f32(v) + f32(0.0))) if reading == "neg_zero_equal" else _ordered
            rows = sorted(range(len(D)), key=lambda r: (-key(fused[r]), -D[r] if reading == "ties_high" else D[r]))[:k]
            for j, r in enumerate(rows):
                i = D[r]
                outs[0][q, j], outs[1][q, j], outs[2][q, j], outs[3][q, j] = fused[r], i, sp[r], ex[r]
                outs[4][q, j], outs[5][q, j] = rs[i], re.get(i, 0)
            outs[6][q] = len(rows)
    return outs


def permuted(call, seed=3):
    """Per query a permutation of its entries."""
    rng = np.random.default_rng(seed)
    return [rng.permutation(len(x)) for x in call.lists]


_MADE = {}


def make(name):
    """The case `name`, built and checked once per process."""
    if name not in _MADE:
        case = FuseCase(name)
        case.check()
        _MADE[name] = case
    return _MADE[name]
