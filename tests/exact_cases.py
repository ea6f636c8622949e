"""Seeded inputs for the tests of device exact search at the structural edges of its kernels (test_exact_cases_cpu.py,
test_gpu_exact_edges.py). TEST INFRASTRUCTURE, pure numpy apart from the index build.

A case = a document collection, its queries and a check() that asserts, from the arrays of a descriptor built from the
case alone, that the case has the property it exists for - a later edit (another seed, another sampling rule) then
fails there instead of leaving a test that passes for nothing. The constants are those of
seismic_amd/csrc/exact_device.hip: ranges of 32 768 documents, steps of 8 x 1024 entries, query components resolved 256
at a time, a scan tile of 4 x 1024 counts.

  segments       (range, component) segments of 8191 ... 32 768 entries: the same component over several steps
  long_u16/_u32  queries of 255 ... 1000 components: the refill of the segment table between groups of 256
  scan_<dim>     dim + 1 = 4095, 4096, 4097, 8192, 8193 with mass on both sides of every tile boundary
  documents      documents of 0, 1, 63, 64, 65, 128, 129 and 5000 components, the longest two across a range boundary
  ties           65 537 documents, every second one holding component 0 with one value: every score ties

Every case has signed document values (the order of a document's additions shows in its bits) and a non-negative copy
(|value|) that the fixed-u8 and DotVByte variants are converted from; query values are signed.

The second half restates exact search in numpy (Restated) with switches for one wrong reading each - segments cut at one
step, only the first group of query components, descending component order, ties by descending id - and the offset scan
with and without the carry between tiles: test_exact_cases_cpu.py shows that each disagrees with the host on its case.
"""
import functools

import numpy as np

import model64 as M64
import orc
from seismic_amd import _native
from seismic_amd._abi import BuildConfig

RANGE = 32768          # kRange
STEP = 8 * 1024        # kE * kBS
GROUP = 256            # kGroup
TILE = 4 * 1024        # counts per turn of the scan
MAX_K = 1024           # kMaxK
# test_gpu_exact.py: _forward_only (the config SeismicDataset._freeze uses: exact search only needs the forward index)
FORWARD_ONLY = dict(n_postings=1, centroid_fraction=1.0, min_cluster_size=0, summary_energy=1.0, max_fraction=1.0, doc_cut=1)

_signed = M64.VALUE_LAWS["signed"]


def _csr_of_pairs(n_docs, dim, doc, comp):
    """(offsets, comps) of the distinct (document, component) pairs, components ascending within a document."""
    key = np.unique(np.asarray(doc, np.int64) * dim + np.asarray(comp, np.int64))
    off = np.zeros(n_docs + 1, np.uint64)
    off[1:] = np.cumsum(np.bincount(key // dim, minlength=n_docs))
    return off, (key % dim).astype(np.uint32)


def _strided(rng, lens, universe, strides):
    """lens[d] distinct indices below `universe` per document: start + j * stride (mod universe), the stride coprime with
    universe. (document of every pair, index of every pair)"""
    lens = np.asarray(lens, np.int64)
    assert lens.max() <= universe
    start = rng.integers(0, universe, len(lens))
    stride = rng.choice(strides, len(lens))
    doc = np.repeat(np.arange(len(lens), dtype=np.int64), lens)
    j = np.arange(int(lens.sum()), dtype=np.int64) - np.repeat(np.cumsum(lens) - lens, lens)
    return doc, (start[doc] + j * stride[doc]) % universe


def _coprime(universe, n=200):
    return np.array([s for s in range(7, universe) if np.gcd(s, universe) == 1][:n], np.int64)


def _query(rng, comps):
    c = np.sort(np.asarray(comps, np.int64)).astype(np.uint32)
    assert len(np.unique(c)) == len(c)
    return c, _signed(rng, len(c))


def segment_counts(arrays, dim):
    """int64 [n_ranges, dim]: the documents of every range that carry every component (the exact file's segment lengths)."""
    off = np.asarray(arrays["fwd_offsets"]).astype(np.int64)
    comp = np.asarray(arrays["fwd_comps"]).astype(np.int64)
    n_docs = len(off) - 1
    n_ranges = (n_docs + RANGE - 1) // RANGE
    doc_of = np.repeat(np.arange(n_docs, dtype=np.int64), np.diff(off))
    return np.bincount((doc_of // RANGE) * dim + comp, minlength=n_ranges * dim).reshape(n_ranges, dim)


class ExactCase:
    def __init__(self, name, cw, dim, off, comps, vals, queries, check, paths):
        self.name, self.cw, self.dim = name, cw, dim
        self.off, self.comps, self.vals = off, comps, np.asarray(vals, np.float32)
        self.n_docs = len(off) - 1
        self.queries = queries
        self.q_off, self.qc, self.qv = orc.csr(queries)
        self._check, self.paths = check, paths
        for a in (self.off, self.comps, self.vals, self.q_off, self.qc, self.qv):
            a.setflags(write=False)

    @property
    def value_types(self):
        """0 on the signed values; 1 (and 2: there is no DotVByte for u32) on the non-negative copy."""
        return (0, 1, 2) if self.cw == 2 else (0, 1)

    def build(self, value_type=0):
        """A fresh forward-only index of the case (not uploaded): binary16 from the signed values, or fixed-u8 / DotVByte
        converted from the non-negative copy."""
        vals = self.vals if value_type == 0 else np.abs(self.vals)
        ix = _native.NativeIndex.build(self.cw, self.dim, self.off, self.comps, vals, BuildConfig.defaults(**FORWARD_ONLY))
        return ix if value_type == 0 else ix.convert(value_type)

    def check(self, arrays):
        """Asserts the case's property from orc.desc_arrays of an index built from it; returns what it found."""
        return self._check(self, arrays)

    def query(self, i):
        return self.queries[i]


# ---------------------------------------------------------------------------------------------------------------------
# segments
# ---------------------------------------------------------------------------------------------------------------------
SEG_DIM = 64
SEG_N_DOCS = RANGE + 20000
# components 0 .. 8 in range 0; 7 lives in range 1 only (9000 documents there), 8 in range 0 only, 9 nowhere
SEG_HEAVY_R0 = (8191, 8192, 8193, 16384, 16385, 24577, 32768, 0, 8193)
SEG_ABSENT = 9


def _segments():
    rng = np.random.default_rng(101)
    dim, n_docs = SEG_DIM, SEG_N_DOCS
    sizes = (RANGE, n_docs - RANGE)
    doc, comp = [], []
    for c in range(dim):
        if c == SEG_ABSENT:
            continue
        for r in (0, 1):
            if c < 9:
                n = SEG_HEAVY_R0[c] if r == 0 else (9000 if c == 7 else 0 if c == 8 else int(rng.integers(200, 600)))
            else:
                n = int(rng.integers(200, 500))
            doc.append(r * RANGE + rng.choice(sizes[r], n, replace=False))
            comp.append(np.full(n, c, np.int64))
    off, comps = _csr_of_pairs(n_docs, dim, np.concatenate(doc), np.concatenate(comp))
    vals = _signed(rng, len(comps))
    heavy = list(range(9))
    light = list(range(10, dim))
    # 0 .. 8: each heavy component alone, with a positive weight (on the non-negative copy a negative one sends every holder
    # below the documents at +0.0, and the top-k could not tell how long the segment was); the other queries are signed
    qs = [(c, np.abs(v)) for c, v in (_query(rng, [c]) for c in heavy)]
    qs.append(_query(rng, heavy))                                            # 9: all of them
    qs.append(_query(rng, heavy + light[::2]))                               # 10: heavy and light ones
    qs.append(_query(rng, [1, 3, 5, 7] + light[1::3]))                       # 11
    qs.append(_query(rng, [SEG_ABSENT, 12, 40]))                             # 12: the absent component first,
    qs.append(_query(rng, [3, 6, SEG_ABSENT, 15, 63]))                       # 13: in the middle (after a 32 768-entry segment),
    qs.append(_query(rng, [0, 5, 8, SEG_ABSENT]))                            # 14: last
    qs.append((np.zeros(0, np.uint32), np.zeros(0, np.float32)))             # 15: empty
    return ExactCase("segments", 2, dim, off, comps, vals, qs, _check_segments,
                     "segments longer than one step (pos / npos, prefetch at s_b[nj] + npos), empty segments")


def _check_segments(case, arrays):
    cnt = segment_counts(arrays, case.dim)
    assert cnt.shape == (2, SEG_DIM) and case.n_docs == SEG_N_DOCS
    assert tuple(cnt[0, :9]) == SEG_HEAVY_R0, cnt[0, :9]
    assert cnt[1, 7] == 9000 and cnt[1, 8] == 0 and ((cnt[1, :7] >= 200) & (cnt[1, :7] < 600)).all(), cnt[1, :9]
    assert not cnt[:, SEG_ABSENT].any()
    assert ((cnt[:, 10:] >= 200) & (cnt[:, 10:] < 500)).all()
    steps = -(-cnt // STEP)
    assert sorted(set(steps[0, :9].tolist())) == [0, 1, 2, 3, 4] and steps[1, 7] == 2
    # exactly one step, one step and one entry, a whole number of steps, a whole range
    assert STEP - 1 in cnt[0] and STEP in cnt[0] and STEP + 1 in cnt[0] and 2 * STEP in cnt[0] and RANGE in cnt[0]
    return dict(steps_range0=steps[0, :9].tolist(), steps_range1=steps[1, :9].tolist())


# ---------------------------------------------------------------------------------------------------------------------
# long queries
# ---------------------------------------------------------------------------------------------------------------------
LONG_N_DOCS = 33000
LONG_LENS = (255, 256, 257, 511, 512, 513, 1000)
LONG_USED = 1200                    # component ids the documents draw from
LONG_Q_EMPTY, LONG_Q_1000, LONG_Q_GROUP, LONG_Q_255_256, LONG_Q_LAST = 0, 7, 8, 9, 10
LONG_CHUNK_QUERIES = (0, 7, 1, 2, 3, 5, 8, 9, 10)   # the empty one, the 1000-component one and seven others


def _long_band(dim):
    return (600, 899) if dim == 1500 else (30000, 31000)   # (dim 1500: 1200 ids remain beside the band and dim - 1)


def _long(cw, dim, seed):
    rng = np.random.default_rng(seed)
    n_docs = LONG_N_DOCS
    b0, b1 = _long_band(dim)
    outside = np.concatenate([np.arange(0, b0), np.arange(b1, dim - 1)])      # (dim - 1 stays unused too)
    used = np.sort(rng.choice(outside, LONG_USED, replace=False)) if len(outside) > LONG_USED else outside
    assert len(used) == LONG_USED
    lens = rng.integers(1, 41, n_docs)
    lens[::50] = rng.integers(200, 401, len(lens[::50]))
    doc, idx = _strided(rng, lens, LONG_USED, _coprime(LONG_USED))
    comp = used[idx]
    if dim > 65536:     # one more id from anywhere outside the band for a third of the documents (ids above 2^16)
        extra = np.flatnonzero(rng.random(n_docs) < 0.33)
        doc = np.concatenate([doc, extra])
        comp = np.concatenate([comp, rng.choice(outside, len(extra))])
    off, comps = _csr_of_pairs(n_docs, dim, doc, comp)
    vals = _signed(rng, len(comps))
    lo, hi, band = used[used < b0], used[used >= b1], np.arange(b0, b1)
    qs = [(np.zeros(0, np.uint32), np.zeros(0, np.float32))]                                          # 0: empty
    qs += [_query(rng, rng.choice(used, n, replace=False)) for n in LONG_LENS]                       # 1 .. 7
    # 8: positions 256 .. 511 - one whole group - are ids no document has
    qs.append(_query(rng, np.concatenate([rng.choice(lo, GROUP, replace=False), band[:GROUP], rng.choice(hi, 100, replace=False)])))
    # 9: positions 255 and 256 - a group's last and the next one's first - are absent
    qs.append(_query(rng, np.concatenate([rng.choice(lo, GROUP - 1, replace=False), band[5:7], rng.choice(hi, 60, replace=False)])))
    # 10: the last component is absent
    qs.append(_query(rng, np.concatenate([rng.choice(used, 40, replace=False), [dim - 1]])))
    return ExactCase("long_u%d" % (8 * cw), cw, dim, off, comps, vals, qs, _check_long,
                     "queries of more than 256 components (the g0 += kGroup refill, order across it, empty segments at a "
                     "group's first and last position); dim + 1 = %d: %d scan tiles" % (dim + 1, -(-(dim + 1) // TILE)))


def _check_long(case, arrays):
    dim = case.dim
    b0, b1 = _long_band(dim)
    off = np.asarray(arrays["fwd_offsets"]).astype(np.int64)
    comp = np.asarray(arrays["fwd_comps"]).astype(np.int64)
    assert len(off) - 1 == LONG_N_DOCS
    lens = np.diff(off)
    assert ((lens[::50] >= 200) & (lens[::50] <= 401)).all() and np.median(lens) <= 41 and lens.min() >= 1
    used = np.zeros(dim, bool)
    used[comp] = True
    assert b1 - b0 >= GROUP and not used[b0:b1].any() and not used[dim - 1]
    if dim > 65536:
        assert used[65536:].sum() > 100
    qlens = [len(c) for c, _ in case.queries]
    assert qlens[1:8] == list(LONG_LENS) and qlens[LONG_Q_EMPTY] == 0
    c = case.queries[LONG_Q_GROUP][0].astype(np.int64)
    assert len(c) > 2 * GROUP and not used[c[GROUP:2 * GROUP]].any() and used[c[:GROUP]].all() and used[c[2 * GROUP:]].all()
    c = case.queries[LONG_Q_255_256][0].astype(np.int64)
    assert not used[c[GROUP - 1]] and not used[c[GROUP]] and used[c[GROUP - 2]] and used[c[GROUP + 1]]
    c = case.queries[LONG_Q_LAST][0].astype(np.int64)
    assert not used[c[-1]] and used[c[:-1]].all()
    # sums that cross a group boundary: documents sharing more than 256 components with the 1000-component query
    present = np.zeros(dim, bool)
    present[case.queries[LONG_Q_1000][0]] = True
    doc_of = np.repeat(np.arange(LONG_N_DOCS, dtype=np.int64), lens)
    shared = np.bincount(doc_of, present[comp], LONG_N_DOCS)
    assert (shared > GROUP).sum() >= 50, int((shared > GROUP).sum())
    return dict(docs_sharing_more_than_256=int((shared > GROUP).sum()), most_shared=int(shared.max()))


# ---------------------------------------------------------------------------------------------------------------------
# the scan's tile edges
# ---------------------------------------------------------------------------------------------------------------------
SCAN_DIMS = (4094, 4095, 4096, 8191, 8192)
# (a second range of 1024 documents, not 64: 64 documents of at most 5 components cannot carry every forced component 300 times)
SCAN_N_DOCS = RANGE + 1024
SCAN_FORCED_MIN = 300


def scan_forced(dim):
    return sorted({c for c in (4093, 4094, 4095, 4096, 4097, 8190, 8191, 8192) if c < dim} | {dim - 1})


def _scan(dim):
    rng = np.random.default_rng(300 + dim)
    n_docs = SCAN_N_DOCS
    forced = scan_forced(dim)
    have = np.zeros(n_docs, np.int64)
    doc, comp = [], []
    for r, (d0, d1) in enumerate(((0, RANGE), (RANGE, n_docs))):
        for c in forced:
            room = d0 + np.flatnonzero(have[d0:d1] < 4)
            pick = rng.choice(room, SCAN_FORCED_MIN, replace=False)
            have[pick] += 1
            doc.append(pick)
            comp.append(np.full(len(pick), c, np.int64))
    more = np.maximum(rng.integers(1, 6, n_docs) - have, 0)     # up to 1 .. 5 in all (a repeat of an id the document has is dropped)
    more = np.minimum(more, 5 - have)
    doc.append(np.repeat(np.arange(n_docs, dtype=np.int64), more))
    comp.append(rng.integers(0, dim, int(more.sum())))
    off, comps = _csr_of_pairs(n_docs, dim, np.concatenate(doc), np.concatenate(comp))
    vals = _signed(rng, len(comps))
    qs = [_query(rng, [c]) for c in forced] + [_query(rng, forced)]
    return ExactCase("scan_%d" % dim, 2, dim, off, comps, vals, qs, _check_scan,
                     "the offset scan at dim + 1 = %d (%d tile%s), mass on both sides of each tile boundary, the range's total "
                     "in the table's last slot" % (dim + 1, -(-(dim + 1) // TILE), "s" if dim + 1 > TILE else ""))


def _check_scan(case, arrays):
    dim = case.dim
    assert dim + 1 in (4095, 4096, 4097, 8192, 8193) and case.n_docs == SCAN_N_DOCS
    lens = np.diff(np.asarray(arrays["fwd_offsets"]).astype(np.int64))
    assert lens.min() >= 1 and lens.max() <= 5
    cnt = segment_counts(arrays, dim)
    forced = scan_forced(dim)
    assert (cnt[:, forced] >= SCAN_FORCED_MIN).all(), cnt[:, forced]
    assert dim - 1 in forced
    for edge in (TILE, 2 * TILE):       # mass in the last count of a tile and in the first of the next, where the table has both
        if edge < dim:
            assert edge - 1 in forced and edge in forced
    assert sorted(set(case.qc.tolist())) == forced
    return dict(forced=forced, tiles=-(-(dim + 1) // TILE))


# ---------------------------------------------------------------------------------------------------------------------
# document lengths (the count and scatter kernels' lane strides)
# ---------------------------------------------------------------------------------------------------------------------
DOCS_DIM = 6000
DOCS_N = RANGE + 5
DOCS_LENS = (0, 1, 63, 64, 65, 128, 129)
DOCS_LONG = 5000


def _documents():
    rng = np.random.default_rng(401)
    dim, n_docs = DOCS_DIM, DOCS_N
    lens = np.ones(n_docs, np.int64)
    third = np.arange(0, n_docs, 3)
    lens[third] = np.array(DOCS_LENS)[(third // 3) % len(DOCS_LENS)]
    # around the range boundary: 128, 129, 5000 | 5000, 65, 64, 63, and the last document empty
    lens[RANGE - 3: RANGE + 5] = (128, 129, DOCS_LONG, DOCS_LONG, 65, 64, 63, 0)
    doc, comp = _strided(rng, lens, dim, _coprime(dim))
    off, comps = _csr_of_pairs(n_docs, dim, doc, comp)
    vals = _signed(rng, len(comps))
    qs = [(np.zeros(0, np.uint32), np.zeros(0, np.float32))]
    qs += [_query(rng, rng.choice(dim, int(n), replace=False)) for n in (1, 5, 17, 33, 60, 60, 300)]
    return ExactCase("documents", 2, dim, off, comps, vals, qs, _check_documents,
                     "count and scatter lane strides: documents of 0, 1, 63, 64, 65, 128, 129 and 5000 components, the "
                     "5000-component ones on both sides of a range boundary; dim + 1 = 6001: 2 scan tiles")


def _check_documents(case, arrays):
    lens = np.diff(np.asarray(arrays["fwd_offsets"]).astype(np.int64))
    assert len(lens) == DOCS_N
    assert set(lens.tolist()) == set(DOCS_LENS) | {DOCS_LONG}
    assert lens[RANGE - 1] == DOCS_LONG and lens[RANGE] == DOCS_LONG and lens[-1] == 0 and lens[0] == 0
    assert tuple(lens[RANGE - 3: RANGE - 1]) == (128, 129) and tuple(lens[RANGE + 1: RANGE + 4]) == (65, 64, 63)
    for n in DOCS_LENS:
        assert (lens == n).sum() >= 100, n
    # the queries meet the long documents on both sides of the boundary
    present = np.zeros(case.dim, bool)
    present[case.qc] = True
    comp = np.asarray(arrays["fwd_comps"]).astype(np.int64)
    off = np.asarray(arrays["fwd_offsets"]).astype(np.int64)
    for d in (RANGE - 1, RANGE):
        assert present[comp[off[d]: off[d + 1]]].sum() > 100
    return dict(lengths=sorted(set(lens.tolist())))


# ---------------------------------------------------------------------------------------------------------------------
# ties
# ---------------------------------------------------------------------------------------------------------------------
TIES_N = 2 * RANGE + 1
TIES_DIM = 4
TIES_VALUE = 0.75
TIES_KS = (64, 1024)
TIES_COUNTS = lambda k: (0, 1, k - 1, k, k + 1)   # noqa: E731


def _ties():
    holders = np.arange(0, TIES_N, 2)
    off, comps = _csr_of_pairs(TIES_N, TIES_DIM, holders, np.zeros(len(holders), np.int64))
    vals = np.full(len(comps), TIES_VALUE, np.float32)
    one = np.zeros(1, np.uint32)
    qs = [(one, np.array([1.0], np.float32)), (one, np.array([-1.0], np.float32)), (np.zeros(0, np.uint32), np.zeros(0, np.float32))]
    return ExactCase("ties", 2, TIES_DIM, off, comps, vals, qs, _check_ties,
                     "selection inside one tie group that spans ranges (all six byte passes, a bin of 32 768), the merge's "
                     "tie break by global id; with tie_filters: ranges of 0, 1, k - 1, k, k + 1 allowed documents")


def _check_ties(case, arrays):
    off = np.asarray(arrays["fwd_offsets"]).astype(np.int64)
    lens = np.diff(off)
    assert len(lens) == TIES_N == 2 * RANGE + 1
    assert (lens[0::2] == 1).all() and (lens[1::2] == 0).all()
    assert not np.asarray(arrays["fwd_comps"]).any()
    assert len(np.unique(np.asarray(arrays["fwd_vals"]))) == 1 and np.asarray(arrays["fwd_vals"])[0] != 0
    return dict(holders=int(lens.sum()))


def ties_expected(query, k, allowed=None, value=TIES_VALUE):
    """What exact search returns on the ties case, by reasoning alone: (scores, ids). `value`: the stored value as the
    index decodes it. Query 0 (+1): the holders by ascending id, then the empty documents; query 1 (-1): the empty
    documents at +0.0 first; query 2 (empty): every document at +0.0 by ascending id."""
    ids = np.arange(TIES_N, dtype=np.int64) if allowed is None else np.unique(np.asarray(allowed, np.int64))
    holder = ids % 2 == 0
    w = (1.0, -1.0, 0.0)[query]
    s = np.where(holder, np.float32(w) * np.float32(value), np.float32(0.0)).astype(np.float32) + np.float32(0.0)
    order = np.lexsort((ids, -s.astype(np.float64)))[:k]
    return s[order], ids[order].astype(np.uint64)


def tie_filters(k):
    """name -> allowed ids (ascending) of the filters the ties case runs under for k = 64 / 1024: ids 0 .. k/2 removed; all of
    range 0 removed; range 0 with exactly 0, 1, k - 1, k, k + 1 allowed documents beside the whole of the other ranges; range 1
    with exactly that many and nothing else."""
    rng = np.random.default_rng(500 + k)
    every = np.arange(TIES_N, dtype=np.int64)
    out = {"head_removed": every[k // 2 + 1:], "range0_removed": every[RANGE:]}
    for c in TIES_COUNTS(k):
        out["range0_has_%d" % c] = np.concatenate([np.sort(rng.choice(RANGE, c, replace=False)), every[RANGE:]])
        out["only_%d_of_range1" % c] = RANGE + np.sort(rng.choice(RANGE, c, replace=False))
    return out


def check_tie_filters(k, filters):
    per_range = {n: np.bincount(a // RANGE, minlength=3).tolist() for n, a in filters.items()}
    assert per_range["head_removed"] == [RANGE - k // 2 - 1, RANGE, 1] and filters["head_removed"][0] == k // 2 + 1
    assert per_range["range0_removed"] == [0, RANGE, 1]
    for c in TIES_COUNTS(k):
        assert per_range["range0_has_%d" % c] == [c, RANGE, 1]
        assert per_range["only_%d_of_range1" % c] == [0, c, 0]
    return per_range


# ---------------------------------------------------------------------------------------------------------------------
CASE_NAMES = ("segments", "long_u16", "long_u32") + tuple("scan_%d" % d for d in SCAN_DIMS) + ("documents", "ties")
# (case, value type) of every index the tests build
VARIANTS = [(n, vt) for n in CASE_NAMES for vt in ((0, 1) if n == "long_u32" else (0, 1, 2))]
VARIANT_IDS = ["%s-vt%d" % v for v in VARIANTS]


@functools.lru_cache(maxsize=None)
def make(name):
    """The case `name` (built once per process; its arrays are read-only)."""
    if name == "segments":
        return _segments()
    if name == "long_u16":
        return _long(2, 1500, 201)
    if name == "long_u32":
        return _long(4, 70000, 202)
    if name.startswith("scan_"):
        return _scan(int(name[5:]))
    if name == "documents":
        return _documents()
    if name == "ties":
        return _ties()
    raise KeyError(name)


def default_chunk_case():
    """The shipped candidate buffer, once: 163 841 documents (6 ranges), dim 400, 1 - 4 components per document, and
    (256 MiB) // (6 * 1024 * 8) + 3 = 5464 queries at k = 1024 - two chunks. (cw, dim, documents CSR, queries CSR)"""
    rng = np.random.default_rng(601)
    dim, n_docs = 400, 5 * RANGE + 1
    nq = (256 << 20) // (6 * MAX_K * 8) + 3
    doc, comp = _strided(rng, rng.integers(1, 5, n_docs), dim, _coprime(dim))
    off, comps = _csr_of_pairs(n_docs, dim, doc, comp)
    vals = _signed(rng, len(comps))
    qd, qcomp = _strided(rng, rng.integers(0, 4, nq), dim, _coprime(dim))
    q_off, qc = _csr_of_pairs(nq, dim, qd, qcomp)
    return 2, dim, (off, comps, vals), (q_off, qc, _signed(rng, len(qc)))


# ---------------------------------------------------------------------------------------------------------------------
# Exact search restated in numpy, with one switch per wrong reading.
# ---------------------------------------------------------------------------------------------------------------------
class Restated:
    """score(d) = +0.0f, then for each query component in ascending order that d carries: score = score + q * w, the
    product and the sum rounded to binary32 once each; the k best by (score descending, id ascending)."""

    def __init__(self, arrays, val_scale, value_type, dim):
        off = np.asarray(arrays["fwd_offsets"]).astype(np.int64)
        comp = np.asarray(arrays["fwd_comps"]).astype(np.int64)
        self.n_docs, self.dim = len(off) - 1, dim
        if value_type == 0:
            w = np.ascontiguousarray(arrays["fwd_vals"], np.uint16).view(np.float16).astype(np.float32)
        else:
            w = np.asarray(arrays["fwd_vals"]).astype(np.float32) * np.float32(val_scale)
        doc_of = np.repeat(np.arange(self.n_docs, dtype=np.int64), np.diff(off))
        order = np.argsort(comp, kind="stable")          # documents ascending within a component
        self.ptr = np.zeros(dim + 1, np.int64)
        self.ptr[1:] = np.cumsum(np.bincount(comp, minlength=dim))
        self.idoc, self.ival = doc_of[order], w[order]

    def scores(self, comps, vals, descending=False, max_comps=None, segment_cap=None):
        """float32 [n_docs]. Wrong readings: descending = the components added in descending order; max_comps = only the
        first that many query components; segment_cap = only the first that many entries of a (range, component) segment."""
        acc = np.zeros(self.n_docs, np.float32)
        pairs = list(zip(np.asarray(comps).tolist(), np.asarray(vals, np.float32)))
        if max_comps is not None:
            pairs = pairs[:max_comps]
        if descending:
            pairs = pairs[::-1]
        for c, q in pairs:
            d, w = self.idoc[self.ptr[c]: self.ptr[c + 1]], self.ival[self.ptr[c]: self.ptr[c + 1]]
            if segment_cap is not None and len(d):
                r = d // RANGE
                first = np.searchsorted(r, r, side="left")           # where the entry's range starts in the list
                keep = np.arange(len(d)) - first < segment_cap
                d, w = d[keep], w[keep]
            acc[d] = acc[d] + np.float32(q) * w
        return acc

    def topk(self, acc, k, allowed=None, ties_descending=False):
        ids = np.arange(self.n_docs, dtype=np.int64) if allowed is None else np.unique(np.asarray(allowed, np.int64))
        s = acc[ids].astype(np.float64)
        order = np.lexsort((-ids if ties_descending else ids, -s))[:k]
        return acc[ids][order], ids[order].astype(np.uint64)


def scan_offsets(counts, carry=True):
    """Exclusive scan of one range's dim + 1 counts (the last is 0) as exact_scan_kernel does it, tile by tile; carry=False:
    the wrong reading that forgets what the tiles before held."""
    counts = np.asarray(counts, np.int64)
    out = np.zeros(len(counts), np.int64)
    run = 0
    for base in range(0, len(counts), TILE):
        t = counts[base: base + TILE]
        out[base: base + TILE] = np.cumsum(t) - t + (run if carry else 0)
        run += int(t.sum())
    return out
