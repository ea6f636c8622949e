"""Seeded inputs for the build-parity tests (test_build_parity_cpu.py, test_gpu_build_parity.py): every case is a
small collection plus a build configuration plus a PREDICATE that proves the case reaches the edge it is named after.
TEST INFRASTRUCTURE, pure numpy apart from the oracle build one predicate asks for.

A predicate takes (case, arrays) - arrays = orc.desc_arrays of an index built from the case - and asserts, from the
inputs and the descriptor alone, that the edge is there: a list of exactly 64 centroids, a block of exactly 4096
entries, a block that holds -0.0 before +0.0 for one component. The CPU tier asserts every predicate, so a case that
silently stops reaching its edge (another seed, another sampling rule) fails there instead of passing for nothing.

The edges are those of seismic_amd/csrc/build_assign.hip (64-lane argmax by (total_cmp key, centroid index), dissolved
clusters, "centroid 0 when every one is avoided"), build_summaries.hip (bitonic sorts over power-of-two paddings, 16
keys per thread, a sequential energy cut, quant = 0/0, 4096 entries of capacity) and builder.cpp's assign_docs (touched
and untouched centroids: its tie logic matters only where a touched centroid scores +0.0, -0.0 or below).
"""
import functools

import numpy as np

import model64 as M64
import orc
from seismic_amd._abi import BuildConfig

ZEROS = np.array([0.0, 1e-9, -1e-9, -2.0 ** -25, 2.0 ** -25], np.float32)   # binary16: +0, +0, -0, -0, +0 (tie to even)
SIGNED_TIES = np.array([-2, -1, -0.5, 0.5, 1, 2], np.float32)


def _signed_ties(rng, n):
    return rng.choice(SIGNED_TIES, n).astype(np.float32)


def _with_zeros(base):
    def law(rng, n):
        v = base(rng, n)
        hit = rng.random(n) < 0.10
        v[hit] = rng.choice(ZEROS, int(hit.sum()))
        return v
    return law


LAWS = {
    "exp": M64.VALUE_LAWS["exp"],
    "ties": M64.VALUE_LAWS["ties"],
    "signed": M64.VALUE_LAWS["signed"],
    "signed_ties": _signed_ties,
    "zeros": _with_zeros(_signed_ties),
    # no positive value at all: a block's maxima are then mostly zeros, the energy cut keeps the FIRST entry of the
    # (value descending by total_cmp, component ascending) order, and which zero a component's maximum is decides it
    "zeros_nonpos": _with_zeros(lambda rng, n: rng.choice(SIGNED_TIES[:3], n).astype(np.float32)),
    "edges": lambda rng, n: rng.choice(M64.EDGE_SPECIAL, n).astype(np.float32),
}
DEFAULT_CFG = dict(n_postings=100, centroid_fraction=0.1, summary_energy=0.4, max_fraction=1.5, min_cluster_size=2,
                   doc_cut=15)


class Case:
    def __init__(self, name, cw, dim, docs, cfg, check):
        self.name, self.cw, self.dim, self.docs, self.cfg, self._check = name, cw, dim, docs, dict(cfg), check
        self.n_docs = len(docs[0]) - 1

    def build_config(self, **kw):
        return BuildConfig.defaults(**dict(self.cfg, **kw))

    def check(self, arrays):
        """Assert that the case reaches its edge (arrays: desc_arrays of an index built from it)."""
        self._check(self, arrays)


# ---------------------------------------------------------------------------------------------------------------------
# what the predicates read from a descriptor
# ---------------------------------------------------------------------------------------------------------------------
def f16_bits(vals):
    return M64.f16_of(vals).view(np.uint16)


def list_lengths(A):
    return np.diff(A["block_post_start"][A["list_block_start"]].astype(np.int64))


def centroids_of(lens, fraction):
    """n_centroids of lists of `lens` postings: max(1, (usize)(f32 fraction * f32 len)), at most len; 0 for no list."""
    nc = (np.float32(fraction) * lens.astype(np.float32)).astype(np.int64)
    return np.where(lens > 0, np.minimum(np.maximum(nc, 1), lens), 0)


def list_blocks(A):
    return np.diff(A["list_block_start"].astype(np.int64))


def block_sizes(A):
    return np.diff(A["block_post_start"].astype(np.int64))


def block_list(A):
    return np.repeat(np.arange(len(A["list_block_start"]) - 1, dtype=np.int64), list_blocks(A))


def block_entries(A, off):
    """Document entries per block: what decides whether the device or the host summarises it."""
    off = off.astype(np.int64)
    post = A["post_doc"].astype(np.int64)
    per_post = off[post + 1] - off[post]
    return np.add.reduceat(per_post, A["block_post_start"][:-1].astype(np.int64))


def block_kept(A):
    """Summary entries kept per block."""
    dim = len(A["list_block_start"]) - 1
    row_list = np.repeat(np.arange(dim, dtype=np.int64), np.diff(A["list_row_start"].astype(np.int64)))
    ent_list = np.repeat(row_list, np.diff(A["row_ptr"].astype(np.int64)))
    ent_blk = A["list_block_start"].astype(np.int64)[ent_list] + A["sum_bid"].astype(np.int64)
    return np.bincount(ent_blk, None, len(A["blk_min"]))


def block_entry_table(A, docs):
    """Every document entry of every block in posting order: (block, component, binary16 bits)."""
    off, comps, vals = docs
    off = off.astype(np.int64)
    post = A["post_doc"].astype(np.int64)
    e, owner = M64._ranges(off[post], off[post + 1] - off[post])
    post_blk = np.repeat(np.arange(len(A["blk_min"]), dtype=np.int64), block_sizes(A))
    return post_blk[owner], comps.astype(np.int64)[e], f16_bits(vals)[e]


def block_maxima(A, docs, dim):
    """(block, component, maximum as float64) of every (block, component) pair, blocks ascending."""
    blk, comp, bits = block_entry_table(A, docs)
    key = blk * dim + comp
    order = np.argsort(key, kind="stable")
    key, v = key[order], bits[order].view(np.float16).astype(np.float64)
    first = np.flatnonzero(np.r_[True, key[1:] != key[:-1]])
    return key[first] // dim, key[first] % dim, np.maximum.reduceat(v, first)


def _per_block(blk, n_blocks, values, op):
    first = np.flatnonzero(np.r_[True, blk[1:] != blk[:-1]])
    assert len(first) == n_blocks
    return op.reduceat(values, first)


# ---------------------------------------------------------------------------------------------------------------------
# collections
# ---------------------------------------------------------------------------------------------------------------------
def _law_docs(seed, law, n_docs, dim, lo=1, hi=60, components=None):
    """Documents of lo..hi components (popular low ids, as model64.make_case draws them), 2 % empty."""
    rng = np.random.default_rng(seed)
    draw = components or (lambda n: M64._components(rng, n, dim))
    docs = []
    for _ in range(n_docs):
        if rng.random() < 0.02:
            docs.append((np.zeros(0, np.uint32), np.zeros(0, np.float32)))
            continue
        c = draw(int(rng.integers(lo, hi + 1)))
        docs.append((c, LAWS[law](rng, len(c))))
    return M64._csr(docs)


def _df_docs(seed, law, n_docs, dim, df, lo, hi):
    """Component j < len(df) occurs in exactly df[j] documents; the others (len(df) .. dim-1) are drawn uniformly,
    lo..hi per document. With pruning and the cap out of reach a list's length is its component's document count."""
    rng = np.random.default_rng(seed)
    r = len(df)
    member = [[] for _ in range(n_docs)]
    for j, n in enumerate(df):
        for d in rng.choice(n_docs, n, replace=False):
            member[d].append(j)
    docs = []
    for d in range(n_docs):
        bg = r + rng.choice(dim - r, int(rng.integers(lo, hi + 1)), replace=False)
        c = np.sort(np.concatenate([np.array(member[d], np.int64), bg])).astype(np.uint32)
        docs.append((c, LAWS[law](rng, len(c))))
    return M64._csr(docs)


NO_PRUNING = dict(n_postings=6000, max_fraction=1.0)   # dim * n_postings >= nnz and cap >= n_docs in every case below


def _assert_unpruned(case, A):
    assert int(case.docs[0][-1]) <= case.dim * case.cfg["n_postings"] and len(A["post_doc"]) == int(case.docs[0][-1])


# ---- value laws x the default configuration ----
def _check_law(law):
    def check(case, A):
        bits = f16_bits(case.docs[2])
        lens = np.diff(case.docs[0].astype(np.int64))
        assert (lens == 0).any() and lens.max() <= 60
        assert int(case.docs[0][-1]) > case.dim * case.cfg["n_postings"]          # the pruning is active
        assert (list_blocks(A) > 1).any()
        if law in ("signed", "signed_ties", "zeros", "zeros_nonpos", "edges"):
            assert (bits > 0x8000).any()                                           # negative values
        if law == "edges":
            for want in (0x0000, 0x8000, 0x7bff, 0xfbff, 0x0001, 0x0200, 0x0400):   # +-0, +-65504, subnormals, 2^-14
                assert (bits == want).any(), hex(want)
        if law in ("zeros", "zeros_nonpos"):
            _check_zeros(case, A)
    return check


def _check_zeros(case, A):
    blk, comp, bits = block_entry_table(A, case.docs)
    z = (bits & 0x7fff) == 0
    key, neg = (blk * case.dim + comp)[z], (bits[z] == 0x8000)
    order = np.argsort(key, kind="stable")              # posting order kept within a (block, component) pair
    key, neg = key[order], neg[order]
    first = np.flatnonzero(np.r_[True, key[1:] != key[:-1]])
    both = np.add.reduceat(neg.astype(np.int64), first)
    n = np.diff(np.r_[first, len(key)])
    both = (both > 0) & (both < n)
    assert (both & neg[first]).any(), "no block holds -0.0 before +0.0 for one component"
    assert (both & ~neg[first]).any(), "no block holds +0.0 before -0.0 for one component"
    # a zero among a document's doc_cut heaviest components: fewer than doc_cut values are above it
    off = case.docs[0].astype(np.int64)
    doc_of = np.repeat(np.arange(case.n_docs), np.diff(off))
    allbits = f16_bits(case.docs[2])
    positive = np.bincount(doc_of, (allbits < 0x8000) & (allbits > 0), case.n_docs)
    has_zero = np.bincount(doc_of, (allbits & 0x7fff) == 0, case.n_docs) > 0
    assert (has_zero & (positive < case.cfg["doc_cut"])).any()


def _law_case(law, seed):
    return lambda name: Case(name, 2, 300, _law_docs(seed, law, 1500, 300), DEFAULT_CFG, _check_law(law))


# ---- the assignment kernel ----
NC_WANTED = (1, 63, 64, 65, 128, 129)


def _nc_edges(name):
    # centroid_fraction 0.25 is exact in binary32: 252 -> 63, 256 -> 64, 260 -> 65, 512 -> 128, 516 -> 129; 1 and 3 -> 1
    cfg = dict(DEFAULT_CFG, centroid_fraction=0.25, **NO_PRUNING)
    docs = _df_docs(21, "signed_ties", 3000, 400, [1, 3, 252, 256, 260, 512, 516], 4, 14)

    def check(case, A):
        _assert_unpruned(case, A)
        lens = list_lengths(A)
        assert list(lens[:7]) == [1, 3, 252, 256, 260, 512, 516]
        nc = centroids_of(lens, 0.25)
        assert set(NC_WANTED) <= set(nc.tolist()), sorted(set(nc.tolist()))
        assert (lens == 1).any()                               # a list of one posting
    return Case(name, 2, 400, docs, cfg, check)


def _nc_eq_len(name):
    cfg = dict(DEFAULT_CFG, centroid_fraction=1.0, **NO_PRUNING)

    def check(case, A):
        _assert_unpruned(case, A)
        lens = list_lengths(A)
        assert np.array_equal(centroids_of(lens, 1.0), lens) and lens.max() > 128
    return Case(name, 2, 100, _law_docs(22, "ties", 1200, 100, 1, 20), cfg, check)


def _doc_cut(doc_cut, seed):
    def make(name):
        def check(case, A):
            lens = np.diff(case.docs[0].astype(np.int64))
            assert (lens > 1).any() and (doc_cut == 1 or lens.max() < doc_cut)
        return Case(name, 2, 300, _law_docs(seed, "signed", 1500, 300), dict(DEFAULT_CFG, doc_cut=doc_cut), check)
    return make


def _min_cluster(mcs, seed):
    def make(name):
        def check(case, A):
            # the first pass (= the oracle's index at min_cluster_size 0) leaves clusters of one document next to
            # larger ones: they survive at 0 and are dissolved from 1 on
            first = None if mcs == 0 else _first_pass(case)    # (kept alive: the arrays are views of it)
            F = A if mcs == 0 else orc.desc_arrays(first.desc)
            nb, sizes, bl = list_blocks(F), block_sizes(F), block_list(F)
            assert ((sizes == 1) & (nb[bl] > 1)).any() and ((sizes > 1) & (nb[bl] > 1)).any()
            assert case.cfg["min_cluster_size"] == mcs and (list_blocks(A) > 1).any()
        return Case(name, 2, 200, _law_docs(seed, "signed_ties", 1500, 200, 1, 30),
                    dict(DEFAULT_CFG, centroid_fraction=0.3, min_cluster_size=mcs), check)
    return make


def _first_pass(case):
    return orc.OracleIndex(case.cw, case.dim, *case.docs, case.build_config(min_cluster_size=0))


def _all_dissolved(name):
    """min_cluster_size above the longest list: every cluster of the first pass is dissolved. Where the first pass used
    every centroid, every centroid is then avoided and the "centroid 0" rule puts the whole list into one block."""
    cfg = dict(DEFAULT_CFG, centroid_fraction=0.25, min_cluster_size=100000)
    docs = _law_docs(25, "exp", 600, 60, 1, 12)

    def check(case, A):
        first = _first_pass(case)
        F = orc.desc_arrays(first.desc)                        # min_cluster_size 0: the clusters of the first pass
        lens = list_lengths(F)
        assert np.array_equal(lens, list_lengths(A)) and lens.max() <= case.cfg["min_cluster_size"]
        every = (list_blocks(F) == centroids_of(lens, 0.25)) & (centroids_of(lens, 0.25) > 1)
        assert every.any(), "no list whose first pass used every one of its (more than one) centroids"
        assert (list_blocks(A)[every] == 1).all()
    return Case(name, 2, 60, docs, cfg, check)


def _common_component(name):
    cfg = dict(DEFAULT_CFG, centroid_fraction=0.25, **NO_PRUNING)
    docs = _df_docs(26, "signed_ties", 1000, 300, [1000], 2, 10)

    def check(case, A):
        _assert_unpruned(case, A)
        lens = list_lengths(A)
        assert lens[0] == case.n_docs and centroids_of(lens, 0.25)[0] >= 200      # > 64 entries under component 0
        assert np.diff(case.docs[0].astype(np.int64)).max() < case.cfg["doc_cut"]  # ... which every document scores with
    return Case(name, 2, 300, docs, cfg, check)


def _wide_centroids(name):
    def check(case, A):
        lens = np.diff(case.docs[0].astype(np.int64))
        assert lens[lens > 0].min() > 64 and (list_blocks(A) > 1).any()
    return Case(name, 2, 400, _law_docs(27, "signed", 600, 400, 65, 120), dict(DEFAULT_CFG, centroid_fraction=0.2), check)


def _identical_docs(name):
    """Lists 0..4 hold the same 40 identical documents: every centroid scores the same, the last one wins."""
    rng = np.random.default_rng(28)
    same = (np.arange(5, dtype=np.uint32), np.array([1, 0.5, 2, 1, 0.5], np.float32))
    docs = []
    for d in range(800):
        if d % 20 == 7:
            docs.append(same)
        else:
            c = np.sort(5 + rng.choice(195, int(rng.integers(2, 20)), replace=False)).astype(np.uint32)
            docs.append((c, LAWS["signed_ties"](rng, len(c))))
    cfg = dict(DEFAULT_CFG, centroid_fraction=0.25, **NO_PRUNING)

    def check(case, A):
        _assert_unpruned(case, A)
        lens = list_lengths(A)
        assert (lens[:5] == 40).all() and (centroids_of(lens, 0.25)[:5] == 10).all()
        members = A["post_doc"][: 40].astype(np.int64)
        assert (members % 20 == 7).all()
        assert (list_blocks(A)[:5] == 1).all()                 # one winner takes the list
    return Case(name, 2, 200, M64._csr(docs), cfg, check)


def _no_overlap(name):
    """doc_cut 1 and a heaviest component no other document has: against every centroid but itself a document scores
    +0.0 (untouched), so the largest centroid index wins unless the document is a centroid."""
    rng = np.random.default_rng(29)
    n_docs, shared = 1200, 100
    docs = []
    for d in range(n_docs):
        c = np.sort(rng.choice(shared, int(rng.integers(2, 9)), replace=False)).astype(np.uint32)
        v = rng.uniform(0.1, 1.0, len(c)).astype(np.float32)
        docs.append((np.r_[c, np.uint32(shared + d)], np.r_[v, np.float32(5.0)]))
    cfg = dict(DEFAULT_CFG, centroid_fraction=0.25, doc_cut=1, **NO_PRUNING)

    def check(case, A):
        _assert_unpruned(case, A)
        off, comps, vals = case.docs
        top = comps[off[1:].astype(np.int64) - 1]              # the last component holds the largest value
        assert (np.maximum.reduceat(vals, off[:-1].astype(np.int64)) == 5.0).all() and (vals[off[1:].astype(np.int64) - 1] == 5.0).all()
        assert (np.bincount(comps, None, case.dim)[top] == 1).all()
        assert (centroids_of(list_lengths(A), 0.25)[:shared] > 1).all()
    return Case(name, 2, shared + n_docs, M64._csr(docs), cfg, check)


def _u32_wide(name):
    rng0 = np.random.default_rng(30)
    pool = np.sort(rng0.choice(70000, 3000, replace=False))
    rng = np.random.default_rng(31)
    docs = _law_docs(31, "signed_ties", 1500, 70000, 1, 60,
                     components=lambda n: np.sort(rng.choice(pool, n, replace=False)).astype(np.uint32))
    cfg = dict(DEFAULT_CFG, n_postings=2, centroid_fraction=0.5, max_fraction=6.0)

    def check(case, A):
        lens = list_lengths(A)
        assert A["fwd_comps"].dtype == np.uint32 and np.flatnonzero(lens).max() > 65535
        assert lens.max() == 12 and (list_blocks(A) > 1).any()            # the cap 2 x 6.0 is reached
    return Case(name, 4, 70000, docs, cfg, check)


# ---- the summary kernel ----
ENTRY_COUNTS = (1, 2, 3, 255, 256, 257, 2047, 2048, 2049, 4095, 4096, 4097)


def _summary_docs(seed, dim):
    """One block per list (centroid_fraction so small that every list has one centroid). List j < 12 holds documents
    made for it alone, whose lengths add up to ENTRY_COUNTS[j]; lists 12..17 are the value cases; the other components
    fill those documents."""
    rng = np.random.default_rng(seed)
    r = 18
    docs = []

    def fill(j, n, values):
        c = np.sort(np.r_[j, r + rng.choice(dim - r, n - 1, replace=False)]).astype(np.uint32)
        docs.append((c, values(len(c)).astype(np.float32)))

    signed = lambda n: LAWS["signed"](rng, n)
    for j, total in enumerate(ENTRY_COUNTS):
        while total > 0:
            n = min(total, int(rng.integers(40, 61)))
            fill(j, n, signed)
            total -= n
    for _ in range(5):                                          # 12: five documents of that one component, m == 1
        fill(12, 1, signed)
    for _ in range(6):                                          # 13: every maximum is 1.0, quant == 0 / 0
        fill(13, 30, lambda n: np.ones(n))
    for _ in range(6):                                          # 14: every value negative, the total and `until` too
        fill(14, 30, lambda n: -np.abs(LAWS["signed"](rng, n)) - 0.25)
    c = np.sort(np.r_[15, r + rng.choice(dim - r, 3, replace=False)]).astype(np.uint32)
    docs.append((c, np.array([2, 1, -1, -2], np.float32)[rng.permutation(4)]))    # 15: the total is exactly 0.0
    fill(16, 1, lambda n: np.full(n, -0.5))                     # 16: one negative entry
    fill(17, 1, lambda n: np.full(n, 2.0 ** -25))               # 17: one entry, +0.0 in binary16
    return M64._csr(docs)


def _summary_case(seed, dim, energy):
    def make(name):
        cfg = dict(DEFAULT_CFG, centroid_fraction=0.0005, summary_energy=energy, **NO_PRUNING)

        def check(case, A):
            _assert_unpruned(case, A)
            assert (list_blocks(A) <= 1).all()
            ent = block_entries(A, case.docs[0])
            b_of = A["list_block_start"].astype(np.int64)          # one block per list: block of list j
            assert (np.diff(b_of[:19]) == 1).all()
            assert tuple(ent[b_of[:12]]) == ENTRY_COUNTS, ent[b_of[:12]]
            mblk, mcomp, M = block_maxima(A, case.docs, case.dim)
            n_blocks = len(ent)
            m = np.bincount(mblk, None, n_blocks)
            kept = block_kept(A)
            assert m[b_of[12]] == 1 and ent[b_of[12]] == 5
            assert A["blk_quant"][b_of[13]] == 0 and (kept[b_of[13]] > 1 or energy == 0.0)
            total = _per_block(mblk, n_blocks, M, np.add)
            mass = _per_block(mblk, n_blocks, np.abs(M), np.add)
            assert total[b_of[14]] < -float(M64.gamma(m[b_of[14]])) * mass[b_of[14]]
            # until < 0: the first entry reaches it. (summary_energy 0: until is -0.0, no negative sum reaches it)
            assert kept[b_of[14]] == (1 if energy > 0 else m[b_of[14]])
            assert total[b_of[15]] == 0.0 and m[b_of[15]] == 4 and kept[b_of[15]] == 1   # small dyadic values: exact
            assert kept[b_of[16]] == 1 and kept[b_of[17]] == 1 and ent[b_of[16]] == 1
            if energy == 1.0:
                assert (kept[total > 0] > 1).any()
            if energy == 0.0:
                top = _per_block(mblk, n_blocks, M, np.maximum)
                assert (kept[top >= 0] == 1).all()                 # until == +-0.0: a first entry >= 0 reaches it
        return Case(name, 2, dim, _summary_docs(seed, dim), cfg, check)
    return make


_MAKERS = {
    "law_exp": _law_case("exp", 41), "law_ties": _law_case("ties", 42), "law_signed": _law_case("signed", 43),
    "law_signed_ties": _law_case("signed_ties", 44), "law_zeros": _law_case("zeros", 45),
    "law_zeros_nonpos": _law_case("zeros_nonpos", 46), "law_edges": _law_case("edges", 47),
    "nc_edges": _nc_edges, "nc_eq_len": _nc_eq_len, "doc_cut_1": _doc_cut(1, 23), "doc_cut_64": _doc_cut(64, 24),
    "min_cluster_0": _min_cluster(0, 32), "min_cluster_1": _min_cluster(1, 33), "all_dissolved": _all_dissolved,
    "common_component": _common_component, "wide_centroids": _wide_centroids, "identical_docs": _identical_docs,
    "no_overlap": _no_overlap, "u32_wide": _u32_wide,
    "sum_d300_e04": _summary_case(51, 300, 0.4), "sum_d2000_e0": _summary_case(52, 2000, 0.0),
    "sum_d2000_e04": _summary_case(52, 2000, 0.4), "sum_d2000_e1": _summary_case(52, 2000, 1.0),
}
NAMES = tuple(_MAKERS)
ZEROS_CASES = ("law_zeros", "law_zeros_nonpos")


@functools.lru_cache(maxsize=None)
def get(name):
    return _MAKERS[name](name)
