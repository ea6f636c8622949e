"""Seeded inputs for the tests of the streamed stage 2 (seismic_amd/csrc/search_stream.inc) at the edges of its ring, its
queues and its feeder (test_stream_cases_cpu.py, test_gpu_stream_edges.py). TEST INFRASTRUCTURE, pure numpy apart from
the index build.

A case = a document collection in one index form, its named queries, a list of RUNS (queries + search parameters + knobs,
each there for one edge) and a check() that asserts, from the descriptor's arrays, orc.batch_search_counts and model64
alone, that every edge is reached - a later edit (another seed, a halved n_postings) then fails there instead of leaving
a test that passes for nothing. The constants are those of search_stream.inc and launch_config.cpp: rings of 256, 512 and
1024 item slots replayed in windows of 64, feed batches of 64 x SGPU_STREAM_NCH = 384 items, feeder steps of
kStreamFeedPos = 192 positions, a lead of at most ring - 64 items, the short / long queue boundary at 128 components.

How block sizes are made exact: a list of `len` postings is clustered around max(1, floor(centroid_fraction * len))
sampled documents. centroid_fraction 1e-6 makes every list ONE block of all its postings, in ascending document order;
centroid_fraction 1.0 makes every document a centroid, and documents that carry two heavy signature components of their
own are each their own best centroid: blocks of one posting. n_postings is large enough that nothing is pruned, so a
list's length is the number of documents the case gave its component (halve it and the sizes below no longer hold).

  blocks   one block per list: blocks of 383, 384, 385 (the feed batch), 192, 256, 257 (ring 256: ring - 64, ring,
           ring + 1), 448 ... 1025 (the same for rings 512 and 1024), 1100 and 3100 postings; queries of >= 3 x 1024
           postings seen (every ring rewritten three times, the queue counters past the ring size), every heap variant, a
           heap that never fills, negative scores under five heap factors, the budget knobs, one list per group, groups
           of 4 + 4 + 1, an empty list in the middle of the walk, a filtered ring-wrapping query
  units    blocks of one posting: list groups of 191, 192, 193, 384 and 385 positions (one list, and two), a group of 50
           (a step of fewer than 64 items), a list whose last 600 blocks are skippable once the heap is full (whole steps
           with total == 0), scores that fall and that rise along the traversal, kNN refinement, and the batch of more
           queries than workgroups that cycles through seven queries
  lengths  documents of 1, 8, 127, 128, 129, 255, 256, 257, 384, 385 and 600 components: a query whose items are all
           short, one whose items are all long, one where every window holds both, and two lists that share documents
           placed so that one window holds the same document twice

Values are multiples of 1/64 below 4, so binary16, fixed-u8 (val_scale 1/64) and DotVByte hold the same numbers. The
DotVByte form has a vocabulary of 6000 and documents with a component above 5200: gaps that no field of a slice holds,
i.e. the raw record form (raw_documents() restates pack_index.cpp's rule on the descriptor's arrays).
"""
import ctypes as C
import functools

import numpy as np

import model64 as M64
import orc
from seismic_amd import _native
from seismic_amd._abi import BuildConfig, IndexDesc

WINDOW = 64                 # slots per replay window
FEED_POS = 192              # kStreamFeedPos
FEED_BATCH = 64 * 6         # 64 x SGPU_STREAM_NCH
RINGS = (256, 512, 1024)
BLOCKS = (512, 1024)        # SGPU_BLOCK
SHORT_MAX = 128             # items of <= 128 components go to the short queue
WRAP = 3 * 1024             # postings a ring-wrapping query must see
KS = (1, 64, 65, 128, 129, 256, 257, 1000)
FACTORS = (-0.5, 0.0, 0.8, 1.0, 1.3)

# name -> (component width, value type)
FORMS = {"u16_f16": (2, 0), "u16_u8": (2, 1), "u16_dvb": (2, 2), "u32_f16": (4, 0), "u32_u8": (4, 1)}
BODY = (100, 1000)          # logical components of a document's body
FAR = (5200, 6000)          # ... of the far component of the DotVByte form's raw documents


def _values(rng, n):
    return (rng.integers(1, 256, n) / 64.0).astype(np.float32)


class Run:
    """One launch: queries (names), search parameters, knobs (environment), filtered or not, and the batch size (`cycle`:
    the queries repeated in turn up to that many)."""

    def __init__(self, name, queries, k, cut, hf, first_sorted=False, n_knn=0, env=None, filtered=False, cycle=0):
        self.name, self.queries, self.k, self.cut, self.hf = name, tuple(queries), k, cut, float(hf)
        self.first_sorted, self.n_knn, self.env, self.filtered, self.cycle = first_sorted, n_knn, dict(env or {}), filtered, cycle


class StreamCase:
    def __init__(self, kind, form, n_docs, docs, queries, runs, cfg, check):
        self.kind, self.form, self.name = kind, form, "%s-%s" % (kind, form)
        self.cw, self.value_type = FORMS[form]
        self.logical_dim = FAR[1] if self.value_type == 2 else BODY[1]
        self.dim = 70 * self.logical_dim if self.cw == 4 else self.logical_dim
        self.n_docs, self.cfg, self._check = n_docs, cfg, check
        self.off, self.comps, self.vals = orc.csr([(self.phys(c), v) for c, v in docs])
        self.queries = {n: (self.phys(c), np.asarray(v, np.float32)) for n, (c, v) in queries.items()}
        self.runs = {r.name: r for r in runs}
        for a in (self.off, self.comps, self.vals):
            a.setflags(write=False)

    def phys(self, c):
        """Logical component ids -> the index's: u32 forms spread them over a vocabulary of 70 x as many (ids above 2^16)."""
        c = np.asarray(c, np.int64)
        return (c * 70 if self.cw == 4 else c).astype(np.uint32)

    def build(self):
        """A fresh host index of the case (not uploaded)."""
        ix = _native.NativeIndex.build(self.cw, self.dim, self.off, self.comps, self.vals, BuildConfig.defaults(**self.cfg))
        return ix if self.value_type == 0 else ix.convert(self.value_type)

    def batch(self, run):
        """(q_off, comps, vals) of a run's queries."""
        names = run.queries if not run.cycle else [run.queries[i % len(run.queries)] for i in range(run.cycle)]
        return orc.csr([self.queries[n] for n in names])

    def allowed(self):
        """The filtered runs' allowed documents (a boolean mask): four of five."""
        return np.random.default_rng(77).random(self.n_docs) < 0.8

    def check(self, ix):
        """Asserts the case's edges from an index built from it (descriptor arrays, oracle counts, model64); returns what
        it found."""
        return self._check(self, ix)


# ---------------------------------------------------------------------------------------------------------------------
# what the checks read
# ---------------------------------------------------------------------------------------------------------------------
class FilteredDesc:
    """The descriptor of `desc` with the postings of documents outside `allowed` deleted (blocks kept, some now empty):
    what filtered search of the index equals the unchanged oracle on (tests/test_gpu_filter.py)."""

    def __init__(self, desc, allowed):
        a = orc.desc_arrays(desc)
        keep = allowed[a["post_doc"]]
        cum = np.concatenate([[0], np.cumsum(keep, dtype=np.uint64)]).astype(np.uint64)
        self.bps = np.ascontiguousarray(cum[a["block_post_start"].astype(np.int64)], np.uint64)
        self.post_doc = np.ascontiguousarray(a["post_doc"][keep], np.uint32)
        self.desc = IndexDesc()
        C.memmove(C.byref(self.desc), C.byref(desc), C.sizeof(IndexDesc))
        self.desc.n_postings = len(self.post_doc)
        self.desc.block_post_start = self.bps.ctypes.data_as(type(desc.block_post_start))
        self.desc.post_doc = (self.post_doc if len(self.post_doc) else np.zeros(1, np.uint32)).ctypes.data_as(type(desc.post_doc))


def list_blocks(arrays, c):
    """Sizes of the blocks of list c (postings), in traversal order without first_sorted."""
    lbs = arrays["list_block_start"].astype(np.int64)
    bps = arrays["block_post_start"].astype(np.int64)
    return np.diff(bps[lbs[c]: lbs[c + 1] + 1])


def list_docs(arrays, c):
    lbs = arrays["list_block_start"].astype(np.int64)
    bps = arrays["block_post_start"].astype(np.int64)
    return arrays["post_doc"][bps[lbs[c]]: bps[lbs[c + 1]]].astype(np.int64)


def walked(case, query, cut):
    """The lists a query walks, in order: its `cut` heaviest components, ties by ascending component (distinct here)."""
    c, v = case.queries[query]
    assert len(np.unique(v)) == len(v)
    return [int(x) for x in c[np.argsort(-v.astype(np.float64), kind="stable")[:cut]]]


def counts(case, desc, run):
    """name -> the oracle's work counts of every query of a run (orc.COUNT_NAMES)."""
    r = run
    Q = orc.csr([case.queries[n] for n in r.queries])
    out = orc.batch_search_counts(desc, *Q, r.k, r.cut, r.hf, r.first_sorted)[3]
    return {n: dict(zip(orc.COUNT_NAMES, (int(x) for x in out[i]))) for i, n in enumerate(r.queries)}


def raw_documents(arrays):
    """Boolean per document: a DotVByte index keeps it in the raw record form - some element that is not the first of its
    slice of eight lies 4096 (elements 1 - 3) or 2048 (elements 4 - 7) or more above its predecessor."""
    off = arrays["fwd_offsets"].astype(np.int64)
    comp = arrays["fwd_comps"].astype(np.int64)
    pos = np.arange(len(comp), dtype=np.int64) - np.repeat(off[:-1], np.diff(off))
    gap = np.diff(comp, prepend=0)
    limit = np.where((pos & 7) <= 3, 4096, 2048)
    bad = ((pos & 7) != 0) & (gap >= limit)
    return np.bincount(np.repeat(np.arange(len(off) - 1), np.diff(off)), bad, len(off) - 1) > 0


def _doc(rng, case_far, heads, head_vals, n, far):
    """One document of n components: its list components `heads`, then body components; `far`: the last one above 5200."""
    nb = n - len(heads)
    assert nb >= 0
    body = rng.choice(np.arange(*BODY), nb, replace=False)
    if far and case_far and nb >= 1:
        body[-1] = int(rng.integers(*FAR))
    c = np.concatenate([np.asarray(heads, np.int64), np.sort(body)])
    order = np.argsort(c, kind="stable")
    v = np.concatenate([np.asarray(head_vals, np.float32), _values(rng, nb)])
    return c[order], v[order]


def _q(rng, heads, weights, n_body=0):
    """A query: list components with the given (distinct, descending) weights, body components with small distinct ones."""
    body = rng.choice(np.arange(*BODY), n_body, replace=False)
    c = np.concatenate([np.asarray(heads, np.int64), body])
    v = np.concatenate([np.asarray(weights, np.float32), (np.arange(n_body) + 1).astype(np.float32) / 256.0])
    order = np.argsort(c, kind="stable")
    return c[order], v[order]


EMPTY_Q = (np.zeros(0, np.int64), np.zeros(0, np.float32))
ONE_BLOCK = dict(n_postings=4000, centroid_fraction=1e-6, min_cluster_size=0, summary_energy=0.5, max_fraction=1.0, doc_cut=15)
UNIT_BLOCKS = dict(ONE_BLOCK, centroid_fraction=1.0, summary_energy=1.0)


# ---------------------------------------------------------------------------------------------------------------------
# blocks: one block per list
# ---------------------------------------------------------------------------------------------------------------------
BLOCK_SIZES = (3100, 1025, 1100, 1024, 383, 384, 385, 192, 256, 257, 448, 512, 513, 960, 1)   # list i holds BLOCK_SIZES[i] documents
B_ONE, B_EMPTY = 14, 99                      # the list of one posting; a component no document has
B_QUERIES = {                                # name -> lists, heaviest first
    "wrap1": (0,), "wrap3": (1, 2, 3), "ring256": (4, 5, 6, 7, 8, 9), "nine": (4, 5, 6, 7, 8, 9, 10, 11, 12),
    "rings": (10, 11, 12, 13, 3, 1), "big": (2, 11, 13), "small767": (4, 5), "one": (B_ONE,), "hole": (4, B_EMPTY, 5),
}
B_WRAPPING = ("wrap1", "wrap3", "nine", "rings")
B_ALL = tuple(B_QUERIES) + ("neg", "empty")


def _blocks(form):
    rng = np.random.default_rng(1001)
    far = FORMS[form][1] == 2
    docs = []
    for lst, size in enumerate(BLOCK_SIZES):
        for _ in range(size):
            docs.append(_doc(rng, far, [lst], _values(rng, 1), int(rng.integers(3, 33)), len(docs) % 3 == 0))
    queries = {n: _q(rng, lists, 2.0 - 0.125 * np.arange(len(lists)), 3) for n, lists in B_QUERIES.items()}
    c, v = _q(rng, (1, 2, 4), (2.0, 1.5, 1.0), 3)
    queries["neg"] = (c, -v)                                       # every score is negative, and so is the threshold
    queries["empty"] = EMPTY_Q
    runs = [Run("wrap", B_ALL, 10, 9, 0.0)]
    runs += [Run("k%d" % k, B_ALL, k, 9, 0.9, first_sorted=bool(k % 2)) for k in KS]
    runs += [Run("never_fills", ("small767",), 1000, 2, 1.0)]
    runs += [Run("factor%g" % hf, ("neg", "wrap3", "nine", "hole"), 10, 9, hf, first_sorted=i % 2 == 1) for i, hf in enumerate(FACTORS)]
    runs += [Run("flush", B_ALL, 10, 9, 0.9, env=dict(SGPU_ITEMS_INIT="16", SGPU_ITEMS_MIN="16")),
             Run("clamp", B_ALL, 10, 9, 0.0, env=dict(SGPU_ITEMS_INIT="1024")),
             Run("halves", ("wrap3", "rings", "big"), 10, 3, 1.3),
             Run("one_list_groups", B_ALL, 10, 9, 0.9, env=dict(SGPU_DOTS_CAP="1")),
             Run("one_list_groups_sorted", B_ALL, 10, 9, 0.9, first_sorted=True, env=dict(SGPU_DOTS_CAP="1")),
             Run("groups_4_4_1", ("nine", "rings", "hole"), 10, 9, 0.9, env=dict(SGPU_LIST_GROUP="4")),
             Run("groups_4_4_1_sorted", ("nine", "rings", "hole"), 10, 9, 0.9, first_sorted=True, env=dict(SGPU_LIST_GROUP="4")),
             Run("filtered", ("rings", "nine", "wrap1", "hole", "empty"), 10, 9, 0.0, filtered=True)]
    return StreamCase("blocks", form, len(docs), docs, queries, runs, ONE_BLOCK, _check_blocks)


def _check_blocks(case, ix):
    a = orc.desc_arrays(ix.desc)
    P = lambda lst: int(case.phys([lst])[0])   # noqa: E731
    found = {}
    # one block per list, of exactly the size the case asked for
    for lst, size in enumerate(BLOCK_SIZES):
        assert list_blocks(a, P(lst)).tolist() == [size], (lst, list_blocks(a, P(lst)))
    assert len(list_blocks(a, P(B_EMPTY))) == 0
    sizes = set(BLOCK_SIZES)
    assert {FEED_BATCH - 1, FEED_BATCH, FEED_BATCH + 1} <= sizes                      # against the feed batch
    for ring in RINGS:
        assert {ring - WINDOW, ring, ring + 1} <= sizes, ring                         # against bud_max and the ring
    assert max(sizes) > 3 * 1024 and 1100 in sizes                                    # blocks over several rewrites of every ring
    # ring wrap: every ring is rewritten at least three times, and both u32 queue counters together pass it
    seen = counts(case, ix.desc, case.runs["wrap"])
    for q in B_WRAPPING:
        assert seen[q]["postings_seen"] >= WRAP, (q, seen[q])
        assert seen[q]["postings_seen"] >= sum(BLOCK_SIZES[i] for i in B_QUERIES[q])    # heap_factor 0: nothing is skipped
    found["wrap_postings_seen"] = {q: seen[q]["postings_seen"] for q in B_WRAPPING}
    assert seen["empty"]["postings_seen"] == 0 and seen["one"]["blocks_scored"] >= 1
    # the walk: the named lists first (heaviest), in the order given
    for q, lists in B_QUERIES.items():
        assert walked(case, q, len(lists)) == [P(i) for i in lists], q
    assert len(B_QUERIES["nine"]) == 9 and all(len(case.queries[q][0]) >= 9 for q in ("nine", "rings"))   # 4 + 4 + 1 at query_cut 9
    # a heap that never fills: fewer documents than k
    r = case.runs["never_fills"]
    got = orc.batch_search_counts(ix.desc, *case.batch(r), r.k, r.cut, r.hf)
    assert got[2][0] == 767 < r.k and got[3][0][4] == 767
    # negative scores, a negative threshold
    r = case.runs["factor0.8"]
    sc, _, n, _ = orc.batch_search_counts(ix.desc, *case.batch(r), r.k, r.cut, r.hf, r.first_sorted)
    assert n[0] == r.k and (sc[0] < 0).all()
    # a query that prunes hard: the oracle skips whole lists of more than a ring, which the stream's lead reaches into
    seen = counts(case, ix.desc, case.runs["halves"])
    found["halves_blocks_scored"] = {q: (seen[q]["blocks_scored"], seen[q]["blocks_total"]) for q in seen}
    assert any(v["blocks_scored"] < v["blocks_total"] for v in seen.values()), seen
    # the filtered ring-wrapping query still wraps
    r = case.runs["filtered"]
    fd = FilteredDesc(ix.desc, case.allowed())
    seen = counts(case, fd.desc, r)
    assert seen["rings"]["postings_seen"] >= WRAP, seen["rings"]
    found["filtered_postings_seen"] = seen["rings"]["postings_seen"]
    found["raw_documents"] = _check_raw(case, a)
    return found


def _check_raw(case, a):
    """(DotVByte) raw-form documents among the short and among the long items; none elsewhere."""
    if case.value_type != 2:
        return 0
    raw = raw_documents(a)
    lens = np.diff(a["fwd_offsets"].astype(np.int64))
    assert (raw & (lens <= SHORT_MAX)).sum() >= 20, int((raw & (lens <= SHORT_MAX)).sum())
    if case.kind == "lengths":
        assert (raw & (lens > SHORT_MAX)).sum() >= 20, int((raw & (lens > SHORT_MAX)).sum())
    assert (~raw).sum() >= 20
    return int(raw.sum())


# ---------------------------------------------------------------------------------------------------------------------
# units: blocks of one posting
# ---------------------------------------------------------------------------------------------------------------------
# list -> (documents, value law along the document ids)
U_LISTS = {"f191": (191, "rand"), "f192": (192, "rand"), "f193": (193, "rand"), "f384": (384, "rand"), "f385": (385, "rand"),
           "a100": (100, "rand"), "b91": (91, "rand"), "b92": (92, "rand"), "b93": (93, "rand"), "t50": (50, "rand"),
           "cliff": (984, "cliff"), "fall": (600, "fall"), "rise": (600, "rise"), "one": (1, "rand")}
U_ID = {n: i for i, n in enumerate(U_LISTS)}
U_CLIFF_HIGH = 384                  # documents of `cliff` with values in [1.75, 2); the other 600 have values <= 0.125
U_SIG = (20, 100)                   # signature components (two per document, value 3.0)
U_QUERIES = {"f191": ("f191",), "f192": ("f192",), "f193": ("f193",), "f384": ("f384",), "f385": ("f385",),
             "p191": ("a100", "b91"), "p192": ("a100", "b92"), "p193": ("a100", "b93"), "t50": ("t50",),
             "cliff": ("cliff",), "fall": ("fall",), "rise": ("rise",), "one": ("one",),
             "wrap": ("cliff", "fall", "rise", "f385", "f384", "f193", "f192", "f191", "a100")}
U_POSITIONS = {"f191": 191, "f192": 192, "f193": 193, "f384": 384, "f385": 385, "p191": 191, "p192": 192, "p193": 193, "t50": 50}
U_POOL = ("wrap", "empty", "one", "cliff", "fall", "f191", "t50")   # 7 queries: coprime to any grid that is a multiple of the CU count
U_CYCLE = 2100


def _units(form):
    rng = np.random.default_rng(2002)
    pairs = [(i, j) for i in range(*U_SIG) for j in range(i + 1, U_SIG[1])]
    docs = []
    for name, (size, law) in U_LISTS.items():
        i = np.arange(size)
        if law == "rand":
            v = rng.integers(8, 97, size) / 64.0
        elif law == "fall":
            v = (96 - i // 8) / 64.0                                  # 1.5 down to 0.34, eight documents per step
        elif law == "rise":
            v = (22 + i // 8) / 64.0
        else:
            v = np.where(i < U_CLIFF_HIGH, rng.integers(112, 128, size), rng.integers(1, 9, size)) / 64.0
        for x in v:
            s = pairs[len(docs) % len(pairs)]
            docs.append((np.array([U_ID[name], s[0], s[1]], np.int64), np.array([x, 3.0, 3.0], np.float32)))
    queries = {n: _q(rng, [U_ID[x] for x in lists], 2.0 - 0.125 * np.arange(len(lists))) for n, lists in U_QUERIES.items()}
    queries["empty"] = EMPTY_Q
    steps = tuple(U_POSITIONS) + ("cliff", "fall", "rise", "one", "empty")
    runs = [Run("steps", steps, 10, 2, 0.0), Run("steps_sorted", steps, 10, 2, 0.0, first_sorted=True),
            Run("pruned", steps, 10, 2, 0.8), Run("pruned_k64", steps, 64, 2, 1.0),
            Run("wrap", ("wrap",), 10, 9, 0.0), Run("wrap_k1000", ("wrap",), 1000, 9, 0.8),
            Run("wrap_flush", ("wrap", "cliff"), 10, 9, 0.8, env=dict(SGPU_ITEMS_INIT="16", SGPU_ITEMS_MIN="16")),
            Run("knn1", ("wrap", "cliff", "f193", "p192", "one", "empty"), 10, 9, 0.8, n_knn=1),
            Run("knn5", ("wrap", "cliff", "f193", "p192", "one", "empty"), 10, 9, 0.8, n_knn=5),
            Run("next_query", U_POOL, 10, 9, 0.8, cycle=U_CYCLE)]
    return StreamCase("units", form, len(docs), docs, queries, runs, UNIT_BLOCKS, _check_units)


U_KNN = 5   # neighbours per document of the graph the knn runs use


def _check_units(case, ix):
    a = orc.desc_arrays(ix.desc)
    P = lambda name: int(case.phys([U_ID[name]])[0])   # noqa: E731
    found = {}
    assert (np.diff(a["block_post_start"].astype(np.int64)) == 1).all()               # every block is one posting
    for name, (size, _) in U_LISTS.items():
        assert len(list_blocks(a, P(name))) == size, name
        assert np.array_equal(list_docs(a, P(name)), np.sort(list_docs(a, P(name))))  # traversal = ascending document id
    # feeder steps: groups of 191, 192, 193 (one list, and two), 384, 385 positions; a step of fewer than 64 items
    for q, want in U_POSITIONS.items():
        lists = walked(case, q, 2)
        assert lists == [P(x) for x in U_QUERIES[q]] and sum(len(list_blocks(a, c)) for c in lists) == want, q
    assert {FEED_POS - 1, FEED_POS, FEED_POS + 1, 2 * FEED_POS, 2 * FEED_POS + 1} <= set(U_POSITIONS.values())
    assert U_POSITIONS["t50"] < WINDOW
    seen = counts(case, ix.desc, case.runs["steps"])
    for q, want in U_POSITIONS.items():
        assert seen[q]["postings_seen"] == want == seen[q]["blocks_total"], (q, seen[q])   # heap_factor 0: every position is live
    # block boundaries at the end of a lane register: positions 63 | 64 and 127 | 128 of a step are blocks of their own, both live
    assert seen["f193"]["blocks_scored"] == 193
    # whole steps pruned: once the heap is full - after ANY k items, the threshold is at least the smallest score of the
    # first U_CLIFF_HIGH documents - the summary dot of every later position is below heap_factor x threshold
    r = case.runs["pruned"]
    model = M64.Model(a, ix.desc.val_scale, ix.desc.value_type)
    mq = model.query(*case.queries["cliff"])
    dot, tol = model.summary_dots(P("cliff"), mq)
    ids = list_docs(a, P("cliff"))
    floor = float((mq.s[ids[:U_CLIFF_HIGH]] - mq.tol[ids[:U_CLIFF_HIGH]]).min())
    skippable = dot + tol < r.hf * floor
    assert r.k <= U_CLIFF_HIGH and not skippable[:U_CLIFF_HIGH].any() and skippable[U_CLIFF_HIGH:].all()
    whole = [s for s in range(-(-len(dot) // FEED_POS)) if skippable[s * FEED_POS: (s + 1) * FEED_POS].all()]
    assert len(whole) >= 3 and U_CLIFF_HIGH % FEED_POS == 0, whole
    found["steps_all_skippable"] = whole
    seen = counts(case, ix.desc, r)
    assert seen["cliff"]["blocks_scored"] == U_CLIFF_HIGH and seen["cliff"]["blocks_total"] == 984, seen["cliff"]
    # scores that fall along the traversal: after the first k no item enters the heap (k-th of the first k = the final k-th);
    # scores that rise: the last k are the result
    for rn in ("steps", "pruned"):
        r = case.runs[rn]
        sc, ids, n, _ = orc.batch_search_counts(ix.desc, *case.batch(r), r.k, r.cut, r.hf)
        i = r.queries.index("fall")
        assert set(ids[i].tolist()) <= set(list_docs(a, P("fall"))[:16].tolist()), rn
        i = r.queries.index("rise")
        assert set(ids[i].tolist()) <= set(list_docs(a, P("rise"))[-16:].tolist()), rn
    # the ring-wrapping query of this case, and the batch that cycles through seven queries
    seen = counts(case, ix.desc, case.runs["wrap"])
    assert seen["wrap"]["postings_seen"] >= WRAP, seen["wrap"]
    found["wrap_postings_seen"] = seen["wrap"]["postings_seen"]
    assert walked(case, "wrap", 9) == [P(x) for x in U_QUERIES["wrap"]]
    r = case.runs["next_query"]
    assert len(r.queries) == 7 and r.cycle % 7 == 0 and r.cycle > 4 * 512            # more queries than a chip's workgroups
    assert {"wrap", "empty", "one"} <= set(r.queries)
    return found


# ---------------------------------------------------------------------------------------------------------------------
# lengths: the length classes, and a window with the same document twice
# ---------------------------------------------------------------------------------------------------------------------
L_SHORT, L_LONG = (1, 8, 127, 128), (129, 255, 256, 257, 384, 385, 600)
L_S, L_G, L_M, L_A, L_B = 0, 1, 2, 3, 4          # lists: short documents, long ones, alternating, and the two that share documents
L_N, L_MIXED_N = 200, 256
L_A_DOCS, L_B_FROM, L_B_DOCS = 100, 70, 100       # A: documents [x, x + 100), B: [x + 70, x + 170)


def _lengths(form):
    rng = np.random.default_rng(3003)
    far = FORMS[form][1] == 2
    docs = []

    def length(short, i):
        cyc = L_SHORT if short else L_LONG
        if i % 2 == 0:
            return cyc[(i // 2) % len(cyc)]
        return int(rng.integers(2, SHORT_MAX + 1)) if short else int(rng.integers(SHORT_MAX + 1, 420))

    for i in range(L_N):
        docs.append(_doc(rng, far, [L_S], _values(rng, 1), length(True, i), i % 2 == 1))
    for i in range(L_N):
        docs.append(_doc(rng, far, [L_G], _values(rng, 1), length(False, i), i % 2 == 1))
    for i in range(L_MIXED_N):
        docs.append(_doc(rng, far, [L_M], _values(rng, 1), length(i % 2 == 0, i // 2), i % 4 >= 2))
    for i in range(L_B_FROM + L_B_DOCS):
        heads = ([L_A] if i < L_A_DOCS else []) + ([L_B] if i >= L_B_FROM else [])
        n = int(rng.integers(5, 41)) if i % 3 else int(rng.integers(130, 300))
        docs.append(_doc(rng, far, heads, _values(rng, len(heads)), n, i % 5 == 0))
    queries = {"short": _q(rng, [L_S], [2.0], 5), "long": _q(rng, [L_G], [2.0], 5), "mixed": _q(rng, [L_M], [2.0], 5),
               "straddle": _q(rng, [L_A, L_B], [2.0, 1.0], 5), "empty": EMPTY_Q}
    classes = ("short", "long", "mixed", "empty")
    runs = [Run("classes", classes, 10, 1, 0.0), Run("classes_k129", classes, 129, 1, 0.9),
            Run("classes_flush", classes, 10, 1, 0.0, env=dict(SGPU_ITEMS_INIT="16", SGPU_ITEMS_MIN="16")),
            Run("straddle_open", ("straddle",), 200, 2, 0.0), Run("straddle_open_k100", ("straddle",), 100, 2, 0.9),
            Run("straddle_full", ("straddle",), 10, 2, 0.0), Run("straddle_full_k64", ("straddle",), 64, 2, 0.8),
            Run("all_lists", ("short", "long", "mixed", "straddle"), 65, 7, 0.9, first_sorted=True)]
    return StreamCase("lengths", form, len(docs), docs, queries, runs, ONE_BLOCK, _check_lengths)


def _check_lengths(case, ix):
    a = orc.desc_arrays(ix.desc)
    P = lambda lst: int(case.phys([lst])[0])   # noqa: E731
    lens = np.diff(a["fwd_offsets"].astype(np.int64))
    assert set(L_SHORT) | set(L_LONG) <= set(lens.tolist()) and lens.max() > 512
    for lst in (L_S, L_G, L_M, L_A, L_B):
        assert len(list_blocks(a, P(lst))) == 1, lst                                   # one block: items in ascending document order
    s, g, m = (lens[list_docs(a, P(x))] for x in (L_S, L_G, L_M))
    assert len(s) == L_N and (s <= SHORT_MAX).all() and set(L_SHORT) <= set(s.tolist())              # every item short
    assert len(g) == L_N and (g > SHORT_MAX).all() and set(L_LONG) <= set(g.tolist())                # every item long
    assert (g > 256).sum() >= 20 and ((g > 128) & (g <= 256)).sum() >= 20 and (g > 512).any()        # both register slots, the tail loop
    assert len(m) == L_MIXED_N
    for w in range(0, L_MIXED_N, WINDOW):                                                            # every window holds both classes
        assert (m[w: w + WINDOW] <= SHORT_MAX).any() and (m[w: w + WINDOW] > SHORT_MAX).any(), w
    for q, lst in (("short", L_S), ("long", L_G), ("mixed", L_M)):
        assert walked(case, q, 1) == [P(lst)]
    seen = counts(case, ix.desc, case.runs["classes"])
    assert [seen[q]["postings_seen"] for q in ("short", "long", "mixed")] == [L_N, L_N, L_MIXED_N]
    # the straddle: list A is walked first; the window that holds A's last items and B's first holds a document twice
    assert walked(case, "straddle", 2) == [P(L_A), P(L_B)]
    da, db = list_docs(a, P(L_A)), list_docs(a, P(L_B))
    assert len(da) == L_A_DOCS and len(db) == L_B_DOCS and len(da) % WINDOW != 0
    w0 = len(da) // WINDOW * WINDOW
    window = np.concatenate([da[w0:], db[: WINDOW - (len(da) - w0)]])
    twice = np.intersect1d(da[w0:], db[: WINDOW - (len(da) - w0)])
    assert len(window) == WINDOW and len(twice) >= 10, twice
    distinct = len(np.union1d(da, db))
    for rn, full in (("straddle_open", False), ("straddle_open_k100", False), ("straddle_full", True), ("straddle_full_k64", True)):
        r = case.runs[rn]
        # not full: k exceeds the distinct documents before the window's second copies; full: the heap fills inside A's first window
        assert (r.k > len(np.unique(np.concatenate([da, db[: WINDOW - (len(da) - w0)]]))) - 1) if not full else (r.k <= WINDOW), rn
        n = orc.batch_search_counts(ix.desc, *case.batch(r), r.k, r.cut, r.hf)[2]
        assert n[0] == min(r.k, distinct), (rn, n[0], distinct)
    return dict(lengths=sorted(set(lens.tolist()))[-4:], same_document_twice_in_window=len(twice), raw_documents=_check_raw(case, a))


# ---------------------------------------------------------------------------------------------------------------------
KINDS = {"blocks": (_blocks, ("u16_f16", "u16_u8", "u32_f16")),
         "units": (_units, ("u16_f16", "u32_u8")),
         "lengths": (_lengths, ("u16_f16", "u16_u8", "u16_dvb", "u32_f16", "u32_u8"))}
CASE_NAMES = tuple("%s-%s" % (k, f) for k, (_, forms) in KINDS.items() for f in forms)


@functools.lru_cache(maxsize=None)
def make(name):
    """The case `name` = "<kind>-<form>" (built once per process; its arrays are read-only)."""
    kind, form = name.split("-")
    return KINDS[kind][0](form)


def knob_sets(case, run):
    """The (ring, workgroup size asked for, workgroup size expected, environment) sets a run is launched under: SGPU_COOP=0,
    SGPU_RING_MAX x SGPU_BLOCK; 1024-thread variants exist for k <= 128, a larger k falls back to 512."""
    out = []
    for ring in RINGS:
        for block in BLOCKS:
            env = dict(SGPU_COOP="0", SGPU_RING_MAX=str(ring), SGPU_BLOCK=str(block))
            if FORMS[case.form] == (4, 0):
                env["SGPU_NO_HASH"] = "1"      # (unforced runs keep the other layouts; the hashed lookup has test_gpu_hash_lookup.py)
            env.update(run.env)
            out.append((ring, block, 512 if run.k > 128 else block, env))
    return out


def plan_facts(case, ix, run, Q):
    """The facts of a run's launch that sgpu_debug_launch_config wants, the plan's from sgpu_debug_plan (no device)."""
    q_off, qc, qv = (np.ascontiguousarray(x, t) for x, t in zip(Q, (np.uint64, np.uint32, np.float32)))
    nq = len(q_off) - 1
    max_nnz = int(np.diff(q_off.astype(np.int64)).max())
    qn = max(4, (max_nnz + 3) & ~3)
    order, out3 = np.zeros(max(nq, 1), np.uint32), np.zeros(3, np.uint32)
    vp = C.c_void_p
    fn = _native.lib().sgpu_debug_plan
    fn.argtypes = [vp, vp, vp, vp, C.c_uint32, C.c_uint32, vp, vp]
    _native.check(fn(ix.h, *(x.ctypes.data_as(vp) for x in (q_off, qc, qv)), nq, min(run.cut, qn), order.ctypes.data_as(vp),
                     out3.ctypes.data_as(vp)))
    return dict(comp_width=case.cw, value_type=case.value_type, dim=case.dim, nq=nq, max_nnz=max_nnz, k_max=run.k, k=run.k,
                query_cut=run.cut, has_plan=1, hash_ok=0, n_knn=run.n_knn, first_sorted=int(run.first_sorted),
                dots_cap=int(out3[0]), max_nb=int(out3[1]), max_list_nb=int(out3[2]))
