"""The counted pass (sgpu_batch_run_counted: the search kernel's COUNTED instantiation, a visited bitmap per resident
workgroup) and the work counters it writes, query by query: counters [0..6] of sgpu_batch_fetch_stats equal the oracle's
per-query counts (orc.batch_search_counts) and, where the float64 model defines them (model64.Model.work_counts), the
model's - exact integers, no tolerance. Every roofline fraction the project publishes is computed from these counters.
Run with `-m gpu`."""
import functools

import numpy as np
import pytest

import model64 as M64
import orc
from seismic_amd import _native
from seismic_amd._abi import BuildConfig
from test_gpu_filter import FilteredDesc

pytestmark = pytest.mark.gpu

N_DOCS = 3009            # 94 bitmap words, the last one holds 1 bit: ids 3008 and 3007 are the highest in play
NQ = 64
CFG = dict(n_postings=100, centroid_fraction=0.2, summary_energy=0.5, max_fraction=6.0)
# (k, query_cut, heap_factor, first_sorted): every k, query_cut and heap_factor of the issue, both traversals
GRID = [(10, 4, 1.0, False), (10, 4, 1.0, True), (1, 1, 0.7, False), (1, 20, 0.0, True), (129, 4, 0.7, True),
        (129, 20, -0.5, False), (300, 1, 1.0, True), (300, 4, 0.0, False), (300, 20, 0.7, False), (10, 20, -0.5, True),
        (129, 1, 0.0, False)]
SMALL_RING = dict(SGPU_ITEMS_MAX="64", SGPU_ITEMS_INIT="16", SGPU_ITEMS_MIN="16", SGPU_RBLOCKS="1")


def _documents(seed, dim, spread):
    """N_DOCS documents of 6 to 120 components below dim - 1 (the last list stays empty). spread: "uniform"; "popular"
    (low ids far more popular: model64's law, lists of very different lengths at a wide vocabulary); "gappy" (as
    test_gpu_fixedu8._gappy_dataset: every fifth document in the low ids - small gaps, the packed DotVByte record - the
    others anywhere - gaps too wide for their fields, the raw record). The last two documents carry four times the
    weight: they survive the pruning of most of their lists."""
    rng = np.random.default_rng(seed)
    vecs = []
    for d in range(N_DOCS):
        n = int(rng.integers(6, 121))
        if spread == "popular":
            c = M64._components(rng, n, dim)
        elif spread == "gappy" and d % 5 == 0:
            c = np.sort(rng.choice(min(dim - 1, 3000), n, replace=False)).astype(np.uint32)
        else:
            c = np.sort(rng.choice(dim - 1, n, replace=False)).astype(np.uint32)
        v = (rng.exponential(0.45, len(c)) + 0.02).astype(np.float32)
        vecs.append((c, v * 4 if d >= N_DOCS - 2 else v))
    return orc.csr(vecs)


def _weights(rng, n):
    """n pairwise distinct, positive query values (the model's counts are defined for those only)."""
    v = (rng.exponential(0.45, n) + 0.02).astype(np.float32) + np.arange(n, dtype=np.float32) * np.float32(1e-4)
    assert len(np.unique(v)) == n
    return v


def _queries(seed, desc, nq, nnz_lo, nnz_hi, docs):
    """Query 0 is empty; query 1's heaviest component is dim - 1, whose list is empty; queries 2 and 3 put their two
    heaviest weights on lists that hold document 3008 resp. 3007; the others draw nnz_lo..nnz_hi components of a random
    document's neighbourhood (half from that document, so the walked lists share documents)."""
    rng = np.random.default_rng(seed)
    a = orc.desc_arrays(desc)
    dim = int(desc.dim)
    lbs, bps, pd = (a[n].astype(np.int64) for n in ("list_block_start", "block_post_start", "post_doc"))
    assert lbs[dim] == lbs[dim - 1], "the last list is not empty"
    post_list = np.repeat(np.arange(dim), np.diff(bps[lbs]))
    d_off, d_c = docs[0].astype(np.int64), docs[1]
    vecs = [(np.zeros(0, np.uint32), np.zeros(0, np.float32))]
    c = np.unique(np.concatenate([rng.choice(dim - 1, min(5, nnz_hi - 1), replace=False), [dim - 1]])).astype(np.uint32)
    v = _weights(rng, len(c))
    v[-1] = v.max() + 1
    vecs.append((c, v))
    for doc in (N_DOCS - 1, N_DOCS - 2):
        lists = np.unique(post_list[pd == doc])
        assert len(lists) >= 2, "document %d is in fewer than two lists" % doc
        heavy = rng.choice(lists, 2, replace=False)
        others = np.setdiff1d(rng.choice(dim - 1, max(nnz_lo, min(6, nnz_hi)), replace=False), heavy)[: max(nnz_hi - 2, 0)]
        c = np.concatenate([heavy, others]).astype(np.uint32)
        v = _weights(rng, len(c))
        v[:2] += v.max() + 1
        o = np.argsort(c)
        vecs.append((c[o], v[o]))
    while len(vecs) < nq:
        n = int(rng.integers(nnz_lo, nnz_hi + 1))
        src = int(rng.integers(0, N_DOCS))
        own = d_c[d_off[src]: d_off[src + 1]]
        own = rng.choice(own, min(len(own), (n + 1) // 2), replace=False)
        c = np.unique(np.concatenate([own, rng.choice(dim - 1, n - len(own), replace=False)])).astype(np.uint32)
        vecs.append((c, _weights(rng, len(c))))
    return orc.csr(vecs)


class Case:
    """A collection, its index (host handle; upload() gives a device copy of its own), its queries."""

    def __init__(self, name):
        base, _, vt = name.partition("-")
        self.cw, self.dim, spread, seed = {"u16": (2, 300, "uniform", 201), "u32": (4, 70_000, "popular", 202),
                                           "gappy": (2, 20_000, "gappy", 203)}[base]
        self.docs = _documents(seed, self.dim, spread)
        self.f16 = _native.NativeIndex.build(self.cw, self.dim, *self.docs, BuildConfig.defaults(**CFG))
        self.host = self.f16.convert({"": 0, "u8": 1, "dvb": 2}[vt]) if vt else self.f16
        self.desc = self.host.desc
        self.vt = int(self.desc.value_type)
        self.val_bytes = 1 if self.vt else 2
        assert int(self.desc.n_docs) == N_DOCS and N_DOCS % 32 == 1
        self.q = _queries(seed + 50, self.desc, NQ, 3, 60, self.docs)
        self._dev = None
        self._oracle = {}

    @property
    def dev(self):
        """The index uploaded under the environment of the first caller (no test changes it before asking)."""
        if self._dev is None:
            self._dev = self.upload()
        return self._dev

    def upload(self):
        return _native.NativeIndex.from_desc(self.desc).upload(0)

    def oracle(self, k, qcut, hf, srt, q=None, n_knn=0):
        """Rows and per-query counts of the oracle, computed once per parameter set and shared (never written to)."""
        key = (k, qcut, hf, srt, n_knn, id(q))
        if key not in self._oracle:
            r = orc.batch_search_counts(self.desc, *(q or self.q), k, qcut, hf, srt, n_knn=n_knn)
            for x in r:
                x.setflags(write=False)
            self._oracle[key] = r
        return self._oracle[key]


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)


def _same(g, c):
    gs, gi, gn = g
    cs, ci, cn = c
    assert np.array_equal(gn, cn), (np.flatnonzero(gn != cn)[:5], gn[gn != cn][:5], cn[gn != cn][:5])
    for q in range(len(gn)):
        n = int(gn[q])
        assert np.array_equal(gi[q, :n], ci[q, :n]), (q, gi[q, :n], ci[q, :n])
        assert np.array_equal(gs[q, :n].view(np.uint32), cs[q, :n].view(np.uint32)), q


def _same_counts(st, want, cols=slice(0, 7), what=""):
    got = st[:, cols].astype(np.int64)
    want = np.asarray(want)[:, cols].astype(np.int64)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, "%s: query %d counter [%d]: kernel %d, expected %d (%d differences; kernel row %s, expected %s)" % (
        what, bad[0][0], bad[0][1] + (cols.start or 0), got[tuple(bad[0])], want[tuple(bad[0])], len(bad),
        got[bad[0][0]].tolist(), want[bad[0][0]].tolist())


def _counted(C, batch, params, q=None, n_knn=0, what=""):
    """One counted pass: rows, counters [0..6] and the per-query bytes equal the oracle's; [7] >= [5]. Returns the stats."""
    k, qcut, hf, srt = params
    ls = batch.run_counted(k, qcut, hf, srt, n_knn=n_knn)
    assert ls.block == 512 and ls.n_queries == batch.nq
    sc, ids, n, counts = C.oracle(k, qcut, hf, srt, q, n_knn)
    what = "%s %s n_knn %d" % (what, params, n_knn)
    _same(batch.fetch(k), (sc, ids, n))
    by, st = batch.algorithmic_bytes_per_query(k, C.cw, C.val_bytes)
    _same_counts(st, counts, what=what)
    assert np.array_equal(by, counts[:, 7].astype(np.int64)), (what, np.flatnonzero(by != counts[:, 7].astype(np.int64))[:5])
    assert batch.algorithmic_bytes(k, C.cw, C.val_bytes)[0] == int(counts[:, 7].sum())    # (the summed form bench.py uses)
    assert (st[:, 7] >= st[:, 5]).all(), what
    return st


def test_base_collection_is_what_the_tests_need():
    """Asserted from the descriptor and the oracle: the highest ids sit in heavily weighted lists, documents recur."""
    C = case("u16")
    a = orc.desc_arrays(C.desc)
    lbs, bps, pd = (a[n].astype(np.int64) for n in ("list_block_start", "block_post_start", "post_doc"))
    model = M64.Model(a)
    for qi, doc in ((2, N_DOCS - 1), (3, N_DOCS - 2)):
        q = model.query(*M64.query_at(C.q, qi), index=qi)
        for c in model.selected_lists(q, 2):
            assert doc in model.list_postings(int(c)), (qi, doc, c)
    q1 = model.query(*M64.query_at(C.q, 1), index=1)
    assert int(model.selected_lists(q1, 1)[0]) == C.dim - 1 and lbs[C.dim] == lbs[C.dim - 1]
    assert C.q[0][1] == 0                                        # query 0 is empty
    assert (np.diff(lbs) > 1).sum() > C.dim // 2                 # lists of several blocks
    for params in ((10, 4, 1.0, False), (300, 20, 0.0, False)):
        counts = C.oracle(*params)[3].astype(np.int64)
        assert (counts[:, 4] > counts[:, 5]).sum() > NQ * 3 // 4, params   # documents are met again in later lists
        assert counts[0].tolist() == [0] * 7 + [12 * params[0]]
    pruned = C.oracle(10, 4, 1.0, False)[3].astype(np.int64)
    assert (pruned[:, 3] < pruned[:, 0]).sum() > NQ // 2         # and blocks are skipped
    # ids 3008 and 3007 are scored: the last bitmap word (1 bit used) and the last bit of the word before it are set
    ids = C.oracle(300, 20, 0.0, False)[1]
    assert (ids[2] == N_DOCS - 1).any() and (ids[3] == N_DOCS - 2).any()


# ---- (a) per-query counter equality, (b) per-query bytes ----
@pytest.mark.parametrize("name", ["u16", "u32", "u16-u8", "u16-dvb", "gappy-u8", "gappy-dvb"])
def test_counters_equal_the_oracles_over_the_parameter_grid(name):
    C = case(name)
    if name == "gappy-dvb":
        # the header's record rule: per slice of eight components the first in 16 bits, three 12-bit and four 11-bit gaps
        off, comps = C.docs[0].astype(np.int64), C.docs[1].astype(np.int64)
        pos = np.arange(len(comps)) - np.repeat(off[:-1], np.diff(off))
        gap = np.diff(comps, prepend=0)
        wide = ((pos % 8 >= 1) & (pos % 8 <= 3) & (gap >= 4096)) | ((pos % 8 >= 4) & (gap >= 2048))
        raw = np.zeros(N_DOCS, bool)
        raw[np.repeat(np.arange(N_DOCS), np.diff(off))[wide]] = True
        assert C.host.stream_stats() == (int(raw.sum()), int(np.diff(off)[raw].sum()))
        assert raw.sum() > 300 and (~raw).sum() > 300                         # both record forms are stored ...
        sc, ids, n, _ = C.oracle(300, 20, 0.0, False)
        got = np.concatenate([ids[i, :int(n[i])] for i in range(NQ)]).astype(np.int64)
        assert raw[got].sum() > 100 and (~raw[got]).sum() > 100               # ... and scored: both are among the results
    elif C.vt == 2:
        assert C.host.stream_stats() == (0, 0)
    b = _native.DeviceBatch(C.dev, *C.q, 300)
    for params in GRID if name in ("u16", "u32") else GRID[::3]:
        _counted(C, b, params, what=name)


ENVS = [("u32", dict(SGPU_FORCE_HASH="1")), ("u32", dict(SGPU_NO_HASH="1")), ("u32", dict(SGPU_FORCE_SPLIT="1")),
        ("u16", dict(SGPU_NO_DENSE="1")), ("u16", dict(SGPU_FWD_LAYOUT="doc")), ("gappy-dvb", dict(SGPU_FWD_LAYOUT="doc")),
        ("u16", dict(SGPU_DOTS_CAP="1")), ("u16", SMALL_RING), ("u32", SMALL_RING), ("u16", dict(SGPU_BLOCK="1024"))]


@pytest.mark.parametrize("name,env", ENVS, ids=["%s-%s" % (n, "+".join("%s=%s" % kv for kv in e.items())[:40]) for n, e in ENVS])
def test_counters_under_every_lookup_layout_and_launch_shape(name, env, monkeypatch):
    """The hooks that choose the lookup layout, the forward layout, the dots area and the round size change nothing the
    counters see; SGPU_BLOCK=1024 is not honoured by the counted pass (it has 512-thread variants only)."""
    C = case(name)
    for k_, v_ in env.items():
        monkeypatch.setenv(k_, v_)
    ix = C.upload()                                     # (the forward layout is chosen at upload)
    b = _native.DeviceBatch(ix, *C.q, 129)
    for params in ((10, 4, 1.0, False), (129, 20, 0.7, True), (1, 4, 0.0, False)):
        _counted(C, b, params, what="%s %s" % (name, env))
    if "SGPU_BLOCK" in env:
        assert b.run(10, 4, 1.0, False).block == 1024   # the hook does reach the default pass of this batch
        _same(b.fetch(10), C.oracle(10, 4, 1.0, False)[:3])
    b.close()
    ix.close()


# ---- (c) model tier ----
@pytest.mark.parametrize("name", ["u16", "u32"])
def test_counters_equal_the_float64_models(name):
    """Against the model alone (descriptor + header text, nothing of the oracle): [0..2] under pruning, [0..6] where
    nothing may be skipped. No query is left out: every query's values are pairwise distinct (asserted by the model)."""
    C = case(name)
    model = M64.Model(orc.desc_arrays(C.desc))
    queries = [model.query(*M64.query_at(C.q, i), index=i) for i in range(NQ)]
    b = _native.DeviceBatch(C.dev, *C.q, 300)
    for k, qcut, hf, srt in ((10, 4, 1.0, False), (129, 20, 0.7, True), (1, 1, -0.5, False)):
        b.run_counted(k, qcut, hf, srt)
        want = np.array([model.work_counts(q, qcut) for q in queries])
        _same_counts(b.fetch_stats(), want, slice(0, 3), "%s model %s" % (name, (k, qcut, hf, srt)))
    for k, qcut, srt in ((1, 1, False), (10, 4, True), (300, 20, False)):
        b.run_counted(k, qcut, 0.0, srt)
        want = np.array([model.work_counts(q, qcut, exhaustive=True) for q in queries])
        _same_counts(b.fetch_stats(), want, slice(0, 7), "%s model exhaustive %s" % (name, (k, qcut, srt)))


# ---- (d) repeated passes ----
@pytest.mark.parametrize("name", ["u16", "u32"])
def test_repeated_passes_leave_nothing_behind(name):
    C = case(name)
    b = _native.DeviceBatch(C.dev, *C.q, 129)
    for params in ((10, 4, 1.0, False), (129, 20, 0.7, True)):
        k = params[0]
        want = C.oracle(*params)
        b.run(*params)
        r1, s1 = b.fetch(k), b.fetch_stats().copy()
        st2 = _counted(C, b, params, what=name).copy()
        b.run_counted(*params)
        st3 = b.fetch_stats().copy()
        assert np.array_equal(st2[:, :8], st3[:, :8])         # [7] is added to, not stored: it must start from zero
        _same(b.fetch(k), want[:3])
        b.run(*params)
        r3, s3 = b.fetch(k), b.fetch_stats().copy()
        _same(r1, want[:3])
        _same(r3, want[:3])
        assert np.array_equal(s1[:, :3], s3[:, :3])           # (how much a default pass scores in vain depends on timing)
        # the default pass: [0..2] are the counted pass's; [3..6] are documented as inexact and are not asserted;
        # [7] counts what was scored, in every pass no less than [5]
        assert np.array_equal(s1[:, :3], st2[:, :3])
        assert (s1[:, 7] >= s1[:, 5]).all() and (st2[:, 7] >= st2[:, 5]).all()


# ---- (e) many queries per workgroup ----
@pytest.mark.parametrize("env", [dict(), dict(SGPU_WG_PER_CU="1")], ids=["default", "one-workgroup-per-cu"])
def test_many_queries_through_every_workgroup(env, monkeypatch):
    """4000 short queries: every workgroup clears its visited bitmap some four (default) to fifteen (one workgroup per
    CU) times and starts the next query on it. A bit left behind makes a later query of that workgroup skip a document:
    [5], [6] and possibly its rows differ."""
    for k_, v_ in env.items():
        monkeypatch.setenv(k_, v_)
    C = case("u16")
    q = _many(C)
    b = _native.DeviceBatch(C.dev, *q, 10)
    for params in ((10, 4, 0.0, False), (10, 4, 1.0, True)):
        ls = b.run_counted(*params)
        assert ls.n_queries == 4000 and 4000 >= 3 * ls.grid, ls.grid
        assert np.bincount(b.fetch_stats()[:, 20]).max() >= 4         # [20]: the workgroup that served the query
        _counted(C, b, params, q=q, what="4000 queries %s" % env)


@functools.lru_cache(maxsize=None)
def _many(C):
    return _queries(260, C.desc, 4000, 1, 6, C.docs)


# ---- (f) graph ----
@pytest.mark.parametrize("name", ["u16", "u32", "gappy-dvb"])
def test_counters_and_bytes_with_a_graph(name):
    """Knn::refine scores documents too: they are counted in [5] and [6] ("as the reference would") and charged in the
    algorithmic bytes like every other scored document - by the kernel's counters and by the oracle alike."""
    C = case(name)
    graph = orc.knn_build(C.desc, 5)
    ix = C.upload()
    ix.set_knn(graph, 5)
    b = _native.DeviceBatch(ix, *C.q, 129)
    orc.knn_attach(graph, 5)
    try:
        for n_knn in (3, 7):
            for params in ((10, 4, 1.0, False), (129, 1, 0.7, True)):
                st = _counted(C, b, params, n_knn=n_knn, what=name)
                plain = C.oracle(*params)[3].astype(np.int64)
                # the refine step does score documents here: the comparison above is not the graph-less one
                assert (st[:, 5].astype(np.int64) > plain[:, 5]).sum() > NQ // 2, (n_knn, params)
                assert np.array_equal(st[:, :5].astype(np.int64), plain[:, :5])
    finally:
        orc.knn_attach(None, 0)
    b.close()
    ix.close()


# ---- (g) the entry point with the bitmap ----
@pytest.mark.parametrize("name", ["u16", "u32"])
def test_batch_search_with_the_visited_bitmap(name, monkeypatch):
    """SGPU_VISITED_BITMAP=1 sends sgpu_batch_search (staged batches, several lanes, each with bitmaps of its own) and
    its filtered form through the counted kernel: rows only, no counters are reachable here."""
    C = case(name)
    ix = C.dev
    many = _many(C) if name == "u16" else _queries(261, C.desc, 3000, 1, 6, C.docs)
    allowed = np.random.default_rng(262).random(N_DOCS) < 0.5
    allowed[N_DOCS - 1] = True
    f = ix.make_filter(allowed)
    fd = FilteredDesc(C.desc, allowed)
    monkeypatch.setenv("SGPU_VISITED_BITMAP", "1")
    for nq in (1, 16, 64, 3000):
        src = C.q if nq <= NQ else many
        first = 2 if nq == 1 else 0                        # (the single query: the one that scores document 3008)
        off = (src[0][first: first + nq + 1] - src[0][first]).astype(np.uint64)
        lo = int(src[0][first])
        q = (off, src[1][lo: lo + int(off[-1])], src[2][lo: lo + int(off[-1])])
        for k, qcut, hf, srt in ((10, 4, 1.0, False), (129, 20, 0.0, True)):
            _same(ix.batch_search(*q, k, qcut, hf, srt), orc.batch_search(C.desc, *q, k, qcut, hf, srt)[:3])
            _same(ix.batch_search(*q, k, qcut, hf, srt, filter=f), orc.batch_search(fd.desc, *q, k, qcut, hf, srt)[:3])
    f.close()


# ---- (h) a second replica ----
def test_counted_pass_on_a_second_replica():
    C = case("u16")
    ix = _native.NativeIndex.from_desc(C.desc)
    ix.upload_many([0, 0])
    assert ix.replicas == 2
    b = _native.DeviceBatch(ix, *C.q, 10, replica=1)
    for params in ((10, 4, 1.0, False), (10, 20, 0.0, True)):
        _counted(C, b, params, what="replica 1")
    b.close()
    ix.close()
