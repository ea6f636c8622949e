"""Shared data of the score_documents tests (tests/test_score_cpu.py, tests/test_gpu_score.py). TEST INFRASTRUCTURE.

A case = a document collection built into an index of one (component width, value type), twelve queries, one candidate
list per query, and the oracle's score bits of EVERY (query, document) pair - computed once per case and shared.

  document lengths   0, 1, 7, 8, 9, 127, 128, 129, 255, 256, 257, 300 (the 8-element slice and the 128-element round of
                     the canonical accumulation order), each in the window form and - where a document can have one - in
                     the form with far components, plus random lengths 2 .. 80
  values             signed, magnitudes 2^-10 .. 2^4 (the accumulation order matters); query weights of both signs
  queries            empty; 1 component; 300 components; both signs; a 0.0 and a -0.0 weight on components documents carry
  candidate lists    empty; one id; one id three times; 0 and n_docs - 1; an empty document; every document descending
  wide vocabularies  (dim 60 000 / 70 000) half of the documents draw their components from a 2 000-id window, the others
                     add components whose gaps are at least 4096: a DotVByte index keeps the first as 20-byte slices and
                     the second in the raw record form

make() asserts with the oracle alone that the case can discriminate: at least 5 % of its pairs have other bits in the
canonical order (ORDER_LANES16) than left to right (ORDER_SEQ), and a DotVByte case holds at least 50 documents of each
record form (sgpu_index_stream_stats).
"""
import ctypes as C

import numpy as np

import orc
from seismic_amd import _native
from seismic_amd._abi import BuildConfig

WINDOW = 2000
SPECIAL_LENS = (0, 1, 7, 8, 9, 127, 128, 129, 255, 256, 257, 300)
N_DOCS = 2000
N_QUERIES = 12
BUILD = dict(n_postings=100, centroid_fraction=0.2, summary_energy=0.5, max_fraction=6.0)

# name -> (component width, dim, value type)
CASES = {
    "u16_f16": (2, 60000, 0),
    "u16_u8": (2, 60000, 1),
    "u16_dvb": (2, 60000, 2),
    "u32_f16": (4, 70000, 0),
    "u32_u8": (4, 70000, 1),
    # small vocabularies: the device keeps the query in a dense table
    "u16_f16_small": (2, 2500, 0),
    "u16_dvb_small": (2, 2500, 2),
    "u32_u8_small": (4, 2500, 1),
}


_WINDOW_P = 1.0 / (np.arange(WINDOW) + 20.0)   # skewed use of the window's ids: queries and documents share components
_WINDOW_P /= _WINDOW_P.sum()


def _values(rng, n):
    """Signed, magnitudes 2^-10 .. 2^4; two thirds of them at 1 and above and positive, so that a fixed-u8 index (negative
    values and those below half its step become code 0) keeps enough non-zero codes for the order to matter there too."""
    small = rng.random(n) < 1.0 / 3.0
    mag = np.exp2(np.where(small, rng.uniform(-10.0, 4.0, n), rng.uniform(0.0, 4.0, n)))
    sign = np.where(small, rng.choice([-1.0, 1.0], n), 1.0)
    return (mag * sign).astype(np.float32)


def _document(rng, n, dim, far):
    """n ascending components: from the window, or (far) all but a few from the window and the last ones at least 4096
    apart beyond it - two of them, so that one of the two gaps does not fall on a slice's first element."""
    n_far = 0
    if far and n >= 2:
        n_far = min(n - 1, 2 + int(rng.integers(0, 3)), (dim - 10000) // 4200)
    c = np.sort(rng.choice(WINDOW, n - n_far, replace=False, p=_WINDOW_P)).astype(np.int64)
    if n_far:
        base = 10000 + int(rng.integers(0, 500))
        tail = base + 4200 * np.arange(n_far) + rng.integers(0, 100, n_far)
        c = np.concatenate([c, tail])
    return c.astype(np.uint32), _values(rng, n)


def documents(dim, seed=11):
    rng = np.random.default_rng(seed)
    wide = dim > 10000 + 3 * 4200
    lens = []
    for n in SPECIAL_LENS:
        lens += [(n, False), (n, wide)]
    while len(lens) < N_DOCS:
        lens.append((int(rng.integers(2, 81)), wide and len(lens) % 2 == 1))
    lens[N_DOCS - 1] = (33, False)           # (the last document is an ordinary one)
    lens[40] = (0, False)                    # (an empty document away from the start)
    return [_document(rng, n, dim, far) for n, far in lens]


def queries(docs, dim, seed=12):
    rng = np.random.default_rng(seed)
    df = np.bincount(np.concatenate([c for c, _ in docs]).astype(np.int64), minlength=dim)
    common = np.argsort(-df, kind="stable")[:400]   # components many documents carry
    vecs = [(np.zeros(0, np.uint32), np.zeros(0, np.float32))]
    vecs.append((np.array([common[0]], np.uint32), np.array([1.375], np.float32)))
    n_far = min(40, dim - WINDOW)
    far = 10000 + rng.choice(max(dim - 10000, 1), n_far, replace=False) if dim > 10000 + n_far else np.zeros(0, np.int64)
    c300 = np.concatenate([rng.choice(WINDOW, 300 - len(far), replace=False), far])
    vecs.append((np.sort(c300).astype(np.uint32), _values(rng, 300)))
    while len(vecs) < N_QUERIES:
        n = int(rng.integers(5, 61))
        c = np.sort(rng.choice(common, n, replace=False)).astype(np.uint32)
        vecs.append((c, _values(rng, n)))
    # query 3: a 0.0 and a -0.0 weight on components the documents carry
    c, v = vecs[3]
    v = v.copy()
    v[0], v[1] = 0.0, -0.0
    vecs[3] = (c, v)
    return vecs


def candidate_lists(docs):
    n = len(docs)
    empty_doc = 40
    assert len(docs[empty_doc][0]) == 0
    every = np.arange(n - 1, -1, -1, dtype=np.uint64)
    lists = [every, every, every, np.zeros(0, np.uint64), np.array([5], np.uint64), np.array([7, 7, 7], np.uint64),
             np.array([0, n - 1], np.uint64), np.array([empty_doc], np.uint64)]
    rng = np.random.default_rng(13)
    while len(lists) < N_QUERIES:
        lists.append(every if len(lists) % 2 == 0 else rng.integers(0, n, 100).astype(np.uint64))   # (with repeats)
    return lists


class ScoreCase:
    def __init__(self, name):
        self.name = name
        self.cw, self.dim, self.value_type = CASES[name]
        self.docs = documents(self.dim)
        self.n_docs = len(self.docs)
        self.off, self.comps, self.vals = orc.csr(self.docs)
        self.queries = queries(self.docs, self.dim)
        self.q_off, self.qc, self.qv = orc.csr(self.queries)
        self.lists = candidate_lists(self.docs)
        self.cand_off = np.zeros(N_QUERIES + 1, np.uint64)
        self.cand_off[1:] = np.cumsum([len(x) for x in self.lists])
        self.cand_ids = np.concatenate(self.lists).astype(np.uint64)
        # every (query, document) pair, documents ascending
        self.all_off = (np.arange(N_QUERIES + 1, dtype=np.uint64) * np.uint64(self.n_docs))
        self.all_ids = np.tile(np.arange(self.n_docs, dtype=np.uint64), N_QUERIES)
        self._index = None
        self._bits = {}

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

    def oracle_bits(self, order=orc.ORDER_LANES16):
        """uint32 [N_QUERIES, n_docs]: the oracle's score bits of every pair."""
        if order not in self._bits:
            desc = self.index.desc
            L = orc.lib()
            out = np.zeros((N_QUERIES, self.n_docs), np.float32)
            for q, (c, v) in enumerate(self.queries):
                c = np.ascontiguousarray(c, np.uint32)
                v = np.ascontiguousarray(v, np.float32)
                pc, pv = c.ctypes.data_as(C.c_void_p), v.ctypes.data_as(C.c_void_p)
                for d in range(self.n_docs):
                    out[q, d] = L.orc_score_doc(C.byref(desc), d, pc, pv, len(c), order)
            bits = out.view(np.uint32)
            bits.setflags(write=False)
            self._bits[order] = bits
        return self._bits[order]

    def expected(self, cand_off, cand_ids):
        """The oracle's bits for candidate lists in CSR form."""
        bits = self.oracle_bits()
        q = np.repeat(np.arange(N_QUERIES), np.diff(cand_off.astype(np.int64)))
        return bits[q, cand_ids.astype(np.int64)]

    def check(self):
        lanes, seq = self.oracle_bits(orc.ORDER_LANES16), self.oracle_bits(orc.ORDER_SEQ)
        share = float(np.mean(lanes != seq))
        assert share >= 0.05, "%s: only %.3f of the pairs depend on the accumulation order" % (self.name, share)
        lens = np.diff(self.off.astype(np.int64))
        assert set(SPECIAL_LENS) <= set(lens.tolist()) and ((lens >= 2) & (lens <= 80)).sum() > 100
        if self.value_type == 2 and self.dim >= 60000:
            raw, _ = self.index.stream_stats()
            assert raw >= 50 and self.n_docs - raw >= 50, "%s: %d raw of %d documents" % (self.name, raw, self.n_docs)
        return share


_MADE = {}


def make(name):
    """The case `name`, built and checked once per process."""
    if name not in _MADE:
        case = ScoreCase(name)
        case.check()
        _MADE[name] = case
    return _MADE[name]
