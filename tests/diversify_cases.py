"""Shared data of the diversify_documents tests (tests/test_diversify_cpu.py, tests/test_gpu_diversify.py). TEST
INFRASTRUCTURE.

A case = one small document collection built into an index of one form (component width, vocabulary size, value type)
and a list of named CALLS of sgpu_diversify_documents on it; diversify_numpy() is a RESTATEMENT of the contract written
from the text of include/seismic_hip.h alone: it decodes the descriptor's forward arrays, scores in np.float32 in the
canonical order (16 accumulators, element e to accumulator (e / 8) % 16, the butterfly 8, 4, 2, 1) and runs the greedy
selection entry by entry. With reading=... it implements one WRONG reading of the contract instead; every named call
says which reading it catches.

Index forms (CASES): u16 components at dim 32767 - the last vocabulary whose dense table fits the device's 128 KiB - with
binary16, fixed-u8 and DotVByte values; dim 32768, the first that takes the hash table, with u16 and u32 components; and a
300-component vocabulary. Stored values of the common documents are multiples of 1/16 up to 8, so every form holds the
same numbers (fixed-u8: val_scale = 1/16); the binary16 forms add documents with signed and with very large values.
Documents by name: len_N (N = 0, 1, 7, 8, 9, 127, 128, 129, 300; all but len_0 end on the same component, so that a
padding element of one would hit an element of the others), far (dim >= 20000: gaps no DotVByte field holds - the raw
record form), mA mB mC mD1 mD2, tie_0 .. tie_5 and dup_0 .. dup_2 (exact duplicates of one another), near_0 near_1, rS rX rY,
big_8192 big_8193 (dim 32768), then random ones; binary16 only: nP nN nM, oS oD oE.
Calls and the wrong reading each catches:
  lengths      the len_N documents as candidates, k = all of them: each is the selected one in turn, the empty one too
               (its table is empty, every sim is 0)                              ("padding": padding elements counted)
  order        (binary16) oD has 136 elements; the products +65504^2, 1, -65504^2 share accumulator 0 in oD's element
               order (sum 0) and lie in accumulators 0, 1, 2 in oS's (sum 1)      ("symmetric", "float64")
  max_not_sum  mA mB mC mutually similar, mD1 apart                               ("pen_sum")
  negative     (binary16) sim(nN, nP) = -4                                        ("signed_pen")
  stale        as max_not_sum with mD2: mC falls behind it only once mB's pick raises its pen      ("no_refresh")
  dups         dup_0 listed three times among its duplicates and near-duplicates  ("dup_twice": also out_n)
  ties         six duplicates lead; k = 1, 3, distinct - 1, distinct, distinct + 1, 256              ("ties_high")
  rounding     lambda = 0.1f, mu = 0.3f: rX and rY tie in f32 (the smaller id wins), not when rounded once  ("fused")
  empty        no candidates / empty query with candidates / both                 (rows not zeroed)
  empty_first  every document but len_0 scores below 0: the first pick leaves an empty table
  counts       queries of 1, 2, 63, 64, 65, 127, 128, 129 and 2048 candidates
  big          (dim 32768) the 8192-component document among others
  random       eight queries of signed weights, 40 candidates each
"""
import numpy as np

import orc
from seismic_amd import _native
from seismic_amd._abi import BuildConfig

N_DOCS = 200
SPECIAL_LENS = (0, 1, 7, 8, 9, 127, 128, 129, 300)
COUNTS = (1, 2, 63, 64, 65, 127, 128, 129, 2048)
BUILD = dict(n_postings=50, centroid_fraction=0.2, summary_energy=0.5, max_fraction=6.0)

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
READINGS = ("padding", "symmetric", "float64", "pen_sum", "signed_pen", "no_refresh", "dup_twice", "ties_high", "fused")
F16_ONLY = ("order", "negative")


def _values(rng, n):
    return (rng.integers(1, 129, n) / 16.0).astype(np.float32)   # multiples of 1/16 in (0, 8]


def _rounding_pair():
    """(rel X, rel Y, pen X, pen Y) with fl(fl(0.1f rX) - fl(0.3f pX)) == fl(fl(0.1f rY) - fl(0.3f pY)) as bits while the
    same expressions rounded once put X strictly above Y. pens are multiples of 1/4 (products of stored values)."""
    f32, f64 = np.float32, np.float64
    lam, mu = f32(0.1), f32(0.3)
    rng = np.random.default_rng(11)
    for _ in range(20000):
        rx = f32(rng.uniform(4.0, 8.0))
        px, py = f32(rng.integers(1, 9) / 4.0), f32(rng.integers(9, 17) / 4.0)
        ry = f32((f64(lam) * f64(rx) - f64(mu) * f64(px) + f64(mu) * f64(py)) / f64(lam))
        for step in range(-3, 4):
            y = ry
            for _ in range(abs(step)):
                y = np.nextafter(y, f32(np.inf if step > 0 else -np.inf))
            a, b = f32(f32(lam * rx) - f32(mu * px)), f32(f32(lam * y) - f32(mu * py))
            ea, eb = f64(lam) * f64(rx) - f64(mu) * f64(px), f64(lam) * f64(y) - f64(mu) * f64(py)
            if a == b and f32(ea) > f32(eb):
                return rx, y, px, py
    raise AssertionError("no rounding pair found")


class Call:
    def __init__(self, name, queries, lists, lam, mu, ks):
        self.name, self.queries, self.ks = name, queries, tuple(ks)
        self.lists = [np.asarray(x, np.uint64) for x in lists]
        self.lam, self.mu = np.float32(lam), np.float32(mu)
        assert len(queries) == len(lists)
        self.nq = len(queries)
        self.q_off, self.qc, self.qv = orc.csr(queries)
        self.cand_off = np.zeros(self.nq + 1, np.uint64)
        self.cand_off[1:] = np.cumsum([len(x) for x in self.lists])
        self.cand_ids = (np.concatenate(self.lists) if lists else np.zeros(0)).astype(np.uint64)

    def args(self, lists=None):
        """The call's arguments up to mu; lists: other candidate lists for the same queries (a permutation)."""
        if lists is None:
            return self.q_off, self.qc, self.qv, self.cand_off, self.cand_ids, float(self.lam), float(self.mu)
        ids = np.concatenate([np.asarray(x, np.uint64) for x in lists]).astype(np.uint64)
        return self.q_off, self.qc, self.qv, self.cand_off, ids, float(self.lam), float(self.mu)


def _q(pairs):
    c = np.array([p[0] for p in pairs], np.uint32)
    w = np.array([p[1] for p in pairs], np.float32)
    o = np.argsort(c)
    return c[o], w[o]


class DiversifyCase:
    def __init__(self, name):
        self.name = name
        self.cw, self.dim, self.value_type = CASES[name]
        dim = self.dim
        rng = np.random.default_rng(53)
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

        for n in SPECIAL_LENS:
            add("len_%d" % n, *window_doc(n, last=True))
        if dim >= 20000:
            add("far", [0, 5000, 15000, dim - 1], [3.0, 0.5, 1.25, 4.0])
        # max_not_sum / stale: one shared component (150), one private each
        add("mA", [150, 151], [2.0, 8.0])
        add("mB", [150, 152], [2.5, 8.0])
        add("mC", [150, 153], [2.0, 8.0])
        add("mD1", [154], [8.0])
        add("mD2", [155], [8.0])
        for i in range(6):
            add("tie_%d" % i, [160, 161], [4.0, 2.0])
        for i in range(3):
            add("dup_%d" % i, [165, 166, 167], [4.0, 2.0, 1.0])
        add("near_0", [165, 166, 168], [4.0, 2.0, 1.0])
        add("near_1", [165, 167, 169], [3.5, 1.0, 2.0])
        # rounding: rS is picked first; pen X = 0.5 * vx, pen Y = 0.5 * vy on the shared component 170
        self.round_pair = _rounding_pair()
        rx, ry, px, py = self.round_pair
        add("rS", [170, 171], [0.5, 8.0])
        add("rY", [170, 173], [float(py) * 2.0, 1.0])   # (the smaller id: it wins the f32 tie)
        add("rX", [170, 172], [float(px) * 2.0, 1.0])
        if dim >= 32768:
            for n in (8192, 8193):
                c = np.sort(rng.choice(dim, n, replace=False))
                add("big_%d" % n, c, _values(rng, n))
        while len(docs) < N_DOCS:
            c, v = window_doc(int(rng.integers(2, 81)))
            if dim >= 20000 and len(docs) % 4 == 0:   # a far tail: the raw record form in a DotVByte index
                c = np.concatenate([c, [9000 + int(rng.integers(0, 50)), 20000 + int(rng.integers(0, 50))]])
                v = np.concatenate([v, _values(rng, 2)])
            docs.append((c.astype(np.uint32), v))
        self.n_common = len(docs)
        if self.value_type == 0:
            add("nP", [180, 181], [2.0, 8.0])
            add("nN", [180, 182], [-2.0, 8.0])
            add("nM", [183], [8.0])
            big = 65504.0
            # oS: elements 0, 8, 16 are the components 100, 108, 242; oD: elements 0, 1, 128 are
            s_c = list(range(100, 116)) + [242]
            s_v = [big] + [0.25] * 7 + [1.0] + [0.25] * 7 + [big]
            add("oS", s_c, s_v)
            d_c = [100, 108] + list(range(116, 242)) + [242] + list(range(243, 250))
            d_v = [big, 1.0] + [0.125] * 126 + [-big] + [1.0] * 7
            add("oD", d_c, d_v)
            add("oE", [250], [1.0])
        self.docs, self.named, self.n_docs = docs, named, len(docs)
        self.off, self.comps, self.vals = orc.csr(docs)
        self._index = None
        self._stored = None
        self._expected = {}

        def rq(n, signed=False):
            c = np.sort(rng.choice(window, n, replace=False)).astype(np.uint32)
            w = _values(rng, n)
            if signed:
                w[rng.random(n) < 0.3] *= -1.0
            return c, w

        allowed = np.array([i for i in range(self.n_docs) if i != named.get("big_8193")])   # (big_8193: over the limit)

        def draw(n, top=None):
            pool = allowed if top is None else allowed[allowed < top]
            return pool[rng.integers(0, len(pool), n)]

        none = np.zeros(0, np.int64)
        empty_q = (np.zeros(0, np.uint32), np.zeros(0, np.float32))
        d = named
        calls = []
        lens = np.array([d["len_%d" % n] for n in SPECIAL_LENS])
        calls.append(Call("lengths", [rq(20), rq(min(300, window))], [lens, lens[::-1]], 0.5, 0.5, (len(lens), 3)))
        m_query = _q([(151, 1.25), (152, 1.125), (153, 0.875), (154, 0.125), (155, 0.3125)])
        calls.append(Call("max_not_sum", [m_query], [[d["mC"], d["mD1"], d["mA"], d["mB"]]], 1.0, 1.0, (4, 3)))
        calls.append(Call("stale", [m_query], [[d["mD2"], d["mC"], d["mB"], d["mA"]]], 1.0, 1.0, (4, 3)))
        dq = _q([(165, 1.0), (166, 0.5), (168, 0.25), (169, 0.25), (190, 1.0)])
        filler = self.n_common - 1
        calls.append(Call("dups", [dq], [[d["dup_0"], d["near_1"], d["dup_0"], d["dup_1"], d["near_0"], d["dup_0"], d["dup_2"], filler]],
                          0.5, 0.5, (6, 8, 9)))
        tq = _q([(160, 2.0), (161, 1.0), (151, 0.5), (154, 0.25)])
        tie_list = [d["tie_3"], d["mA"], d["tie_0"], d["tie_5"], d["tie_1"], d["mD1"], d["tie_4"], d["tie_2"], d["tie_3"]]
        calls.append(Call("ties", [tq], [tie_list], 0.5, 1.0 / 64.0, (1, 3, 7, 8, 9, 256)))
        r_query = _q([(171, 100.0), (172, float(rx)), (173, float(ry))])
        calls.append(Call("rounding", [r_query], [[d["rX"], d["rS"], d["rY"]]], np.float32(0.1), np.float32(0.3), (3, 2)))
        signed = rq(12, signed=True)
        three = draw(3, N_DOCS)
        calls.append(Call("empty", [signed, empty_q, empty_q], [none, three, none], 0.5, 0.5, (1, 8)))
        neg_q = (np.arange(window, dtype=np.uint32), np.full(window, -1.0, np.float32))
        calls.append(Call("empty_first", [neg_q], [[d["len_9"], d["len_0"], d["len_7"], d["len_129"], d["len_0"]]], 0.5, 0.5, (4, 2)))
        calls.append(Call("counts", [rq(int(rng.integers(5, 30))) for _ in COUNTS], [draw(n, N_DOCS) for n in COUNTS],
                          0.5, 0.5, (1, 4)))
        if dim >= 32768:
            calls.append(Call("big", [rq(40)], [[d["len_300"], d["big_8192"], d["len_129"], 0, 5]], 0.5, 0.5, (5,)))
        calls.append(Call("random", [rq(int(rng.integers(5, 40)), signed=True) for _ in range(8)],
                          [draw(40) for _ in range(8)], 0.7, 0.3, (10, 40)))
        if self.value_type == 0:
            calls.append(Call("negative", [_q([(181, 1.25), (182, 0.5), (183, 0.625)])], [[d["nN"], d["nM"], d["nP"]]], 1.0, 1.0, (3, 2)))
            o_query = _q([(101, 4000.0), (243, 10.0), (250, 9.5)])
            calls.append(Call("order", [o_query], [[d["oE"], d["oD"], d["oS"]]], 1.0, 1.0, (3, 2)))
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

    def expected(self, call, k):
        """diversify_numpy of the named call at k, computed once and shared (read-only)."""
        key = (call, k)
        if key not in self._expected:
            got = diversify_numpy(self, self.calls[call], k)
            for a in got:
                a.setflags(write=False)
            self._expected[key] = got
        return self._expected[key]

    def ids_of(self, call, k):
        sc, pen, ids, n = self.expected(call, k)
        return [ids[q, :n[q]].tolist() for q in range(len(n))]

    def check(self):
        """The case holds the edges it is named for (asserted with the restatement and the stored arrays alone)."""
        off, comps, x, scale = self.stored()
        lens = np.diff(off)
        assert np.array_equal(lens, np.diff(self.off.astype(np.int64))), "the index stores other document lengths"
        for n in SPECIAL_LENS:
            assert lens[self.named["len_%d" % n]] == min(n, self.dim)
        if scale is not None:
            assert scale == np.float32(1.0 / 16.0)
        assert np.array_equal((x if scale is None else x * scale), self.vals), "the index does not hold the values given"
        if self.value_type == 2:
            raw, _ = self.index.stream_stats()
            assert 1 <= raw < self.n_docs
        if self.dim >= 32768:
            assert lens[self.named["big_8192"]] == 8192 and lens[self.named["big_8193"]] == 8193
        d = self.named
        assert self.ids_of("max_not_sum", 4) == [[d["mA"], d["mB"], d["mC"], d["mD1"]]]
        assert self.ids_of("stale", 4) == [[d["mA"], d["mB"], d["mD2"], d["mC"]]]
        sc, pen, ids, n = self.expected("dups", 9)
        assert n[0] == 6 and len(set(ids[0, :6].tolist())) == 6
        sc, pen, ids, n = self.expected("ties", 256)
        assert n[0] == 8 and ids[0, :6].tolist() == [d["tie_%d" % i] for i in range(6)]
        assert self.ids_of("rounding", 3) == [[d["rS"], d["rY"], d["rX"]]]
        sc, pen, ids, n = self.expected("rounding", 3)
        rx, ry, px, py = self.round_pair
        assert pen[0, 1] == py and sc[0, 1] == ry and sc[0, 2] == rx
        assert self.ids_of("empty_first", 4)[0][0] == d["len_0"]
        sc, pen, ids, n = self.expected("empty_first", 4)
        assert n[0] == 4 and not pen[0, :2].view(np.uint32).any() and (sc[0, 1:] < 0).all()
        assert self.expected("counts", 4)[3].tolist() == [min(4, len(set(x.tolist()))) for x in self.calls["counts"].lists]
        if self.value_type == 0:
            assert self.ids_of("negative", 3) == [[d["nP"], d["nM"], d["nN"]]]
            sc, pen, ids, n = self.expected("negative", 3)
            assert pen[0, 2] == 0 and not np.signbit(pen[0, 2])
            assert self.ids_of("order", 3) == [[d["oS"], d["oD"], d["oE"]]]
            assert self.expected("order", 3)[1][0, 1] == 0


def _ordered(x):
    b = int(np.float32(x).view(np.uint32))
    return (~b) & 0xffffffff if b & 0x80000000 else b | 0x80000000


def diversify_numpy(case, call, k, reading=None, lists=None):
    """(out_scores f32 [nq, k], out_penalties f32 [nq, k], out_doc_ids u64 [nq, k], out_n u32 [nq]) of
    sgpu_diversify_documents as include/seismic_hip.h defines it; reading: one of READINGS, a wrong reading of the
    contract implemented instead; lists: other candidate lists than the call's."""
    off, comps, x, scale = case.stored()
    f32, f64 = np.float32, np.float64
    ft = f64 if reading == "float64" else f32
    lists = call.lists if lists is None else lists

    def score(W, d):
        """The canonical sum of document d against the table W."""
        c, v = comps[off[d]:off[d + 1]], x[off[d]:off[d + 1]]
        prod = W[c] * v.astype(ft)   # (arrays of one type: one rounding per product)
        assert prod.dtype == ft
        padded = np.zeros((len(prod) + 127) // 128 * 128, ft)   # (+0.0 added to an accumulator changes no bit of it)
        padded[:len(prod)] = prod
        rows = padded.reshape(-1, 16, 8).transpose(1, 0, 2).reshape(16, -1)   # accumulator j: its elements in increasing e
        t = np.add.accumulate(np.concatenate([np.zeros((16, 1), ft), rows], axis=1), axis=1)[:, -1]
        j = np.arange(16)
        for s in (8, 4, 2, 1):
            t = t + t[j ^ s]
        return f32(t[0])

    def query_table(qc, qw):
        W = np.zeros(case.dim, ft)
        W[qc.astype(np.int64)] = qw if scale is None else qw * scale   # (f32 arrays; a power of two: exact)
        return W

    def doc_table(s):
        c, v = comps[off[s]:off[s + 1]], x[off[s]:off[s + 1]]
        W = np.zeros(case.dim, ft)
        W[c] = v if scale is None else (v * scale) * scale
        if reading == "padding" and len(c) % 8:   # the padding elements repeat the last component with value 0
            W[c[-1]] = 0.0
        return W

    out_sc, out_pen = np.zeros((call.nq, k), f32), np.zeros((call.nq, k), f32)
    out_ids, out_n = np.zeros((call.nq, k), np.uint64), np.zeros(call.nq, np.uint32)
    for q, (qc, qw) in enumerate(call.queries):
        ids = [int(i) for i in lists[q]]
        n = len(ids)
        Wq = query_table(qc, qw)
        rel_of = {i: score(Wq, i) for i in set(ids)}
        rel = [rel_of[i] for i in ids]
        pen = [f32(0.0)] * n
        touched = [False] * n
        taken = [False] * n
        r = 0
        while r < k and not all(taken):
            best, pick = None, None
            for i in range(n):
                if taken[i]:
                    continue
                if reading == "fused":
                    mmr = f32(f64(call.lam) * f64(rel[i]) - f64(call.mu) * f64(pen[i]))
                else:
                    mmr = f32(f32(call.lam * rel[i]) - f32(call.mu * pen[i]))
                key = (_ordered(mmr), ids[i] if reading == "ties_high" else -ids[i])
                if best is None or key > best:
                    best, pick = key, i
            sel = ids[pick]
            out_ids[q, r], out_sc[q, r], out_pen[q, r] = sel, rel[pick], pen[pick]
            r += 1
            for i in range(n):
                if (i == pick) if reading == "dup_twice" else (ids[i] == sel):
                    taken[i] = True
            if r == k or all(taken):
                break
            if reading == "no_refresh" and r > 1:
                continue
            Ws = doc_table(sel)
            sim_of = {}
            for i in range(n):
                if taken[i]:
                    continue
                if ids[i] not in sim_of:
                    sim_of[ids[i]] = score(doc_table(ids[i]), sel) if reading == "symmetric" else score(Ws, ids[i])
                s = sim_of[ids[i]]
                if reading == "pen_sum":
                    pen[i] = f32(pen[i] + s)
                elif reading == "signed_pen" and not touched[i]:
                    pen[i] = s
                else:
                    pen[i] = pen[i] if pen[i] >= s else s
                touched[i] = True
        out_n[q] = r
    return out_sc, out_pen, out_ids, out_n


def same(got, want, names=("out_scores", "out_penalties", "out_doc_ids", "out_n")):
    """None if the arrays agree bit for bit, else the name of the first that does not and where."""
    for name, a, b in zip(names, got, want):
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        if a.shape != b.shape:
            return "%s: shape %r != %r" % (name, a.shape, b.shape)
        bits = np.uint64 if a.dtype.itemsize == 8 else np.uint32
        bad = np.argwhere(a.view(bits) != b.view(bits))
        if len(bad):
            i = tuple(bad[0])
            return "%s differs at %d places, first %r: %r != %r" % (name, len(bad), i, a[i], b[i])
    return None


def permuted(call, seed=3):
    """The call's candidate lists, each in another order."""
    rng = np.random.default_rng(seed)
    return [np.asarray(x, np.uint64)[rng.permutation(len(x))] for x in call.lists]


_MADE = {}


def make(name):
    """The case `name`, built and checked once per process."""
    if name not in _MADE:
        case = DiversifyCase(name)
        case.check()
        _MADE[name] = case
    return _MADE[name]
