"""The HIP path against the float64 model of tests/model64.py: every result comes from the device, every expectation
from the model - no oracle search, no host exact search, no bit patterns of a CPU result. The model states what a score,
a candidate set, a summary dot and a built index ARE, with derived rounding bounds (model64's docstring);
test_model_cpu.py shows that the oracle and the host library satisfy the same checkers and that each checker can fail.
Lines starting "model64:" report the largest |device - model| / tolerance per family (run with -s). Run with `-m gpu`."""
import functools

import numpy as np
import pytest

import model64 as M64
import orc
from seismic_amd import _native
from seismic_amd._abi import BuildConfig

pytestmark = pytest.mark.gpu

VARIANTS = [(name, 0) for name in M64.CASES] + [("exp_w2_300", 1), ("exp_w2_300", 2), ("flat_w4_70000", 1)]
VARIANT_IDS = ["%s-vt%d" % v for v in VARIANTS]
NONNEG = [v for v in VARIANTS if M64.law_of(v[0]) != "signed"]
NONNEG_IDS = ["%s-vt%d" % v for v in NONNEG]
# (SGPU_BLOCK, SGPU_COOP): workgroup size and the cooperative variant off / by the library's rule / forced
LAUNCHES = [("512", "0"), ("1024", None), ("512", "force"), ("1024", "0"), ("512", None), ("1024", "force")]


def _say(what, **kv):
    print("model64: %-34s %s" % (what, " ".join("%s=%s" % (k, ("%.4g" % v) if isinstance(v, float) else v)
                                                 for k, v in kv.items())))


def _launch(monkeypatch, block, coop):
    monkeypatch.setenv("SGPU_BLOCK", block)
    if coop is None:
        monkeypatch.delenv("SGPU_COOP", raising=False)
    else:
        monkeypatch.setenv("SGPU_COOP", coop)


@functools.lru_cache(maxsize=None)
def _built(name, vt):
    """A case's index, built with the clustering and the summaries on the device, converted, uploaded (the ties case on
    two replicas sharing the device), with its model and modelled queries."""
    cw, dim, D, Q, law, cfg = M64.make_case(name)
    base = _native.NativeIndex.build(cw, dim, *D, BuildConfig.defaults(use_device=1, **cfg))
    ix = base if vt == 0 else base.convert(vt)
    if law == "ties":
        ix.upload_many([0, 0])
    else:
        ix.upload(0)
    d = ix.desc
    model = M64.Model(orc.desc_arrays(d), d.val_scale, d.value_type)
    queries = [model.query(*M64.query_at(Q, i), index=i) for i in range(len(Q[0]) - 1)]
    return dict(ix=ix, base=base, model=model, queries=queries, Q=Q, law=law, cfg=cfg, D=D)


def _check_rows(S, rows, k, pool_of, tally=None):
    """check_rows + check_scores + check_topk over pool_of(q) for every query (verdicts to `tally`); worst score ratio."""
    model, worst = S["model"], 0.0
    tally = M64.Tally() if tally is None else tally
    sc, ids, n = rows
    for q in S["queries"]:
        i, m = q.index, int(n[q.index])
        model.check_rows(sc[i], ids[i], m, k, i)
        worst = max(worst, model.check_scores(q, ids[i, :m], sc[i, :m]))
        tally.add(model.check_topk(q, ids[i, :m], sc[i, :m], pool_of(q), k))
    return worst


# ---- exact search on the device ----
@pytest.mark.parametrize("variant", VARIANTS, ids=VARIANT_IDS)
def test_exact_search_device_is_the_models_topk(variant):
    S = _built(*variant)
    ix, n_docs = S["ix"], S["model"].n_docs
    rng = np.random.default_rng(5)
    filters = [None, np.flatnonzero(rng.random(n_docs) < 0.3), rng.choice(n_docs, 70, replace=False),
               np.zeros(0, np.int64)]
    tally, worst = M64.Tally(), 0.0
    for allowed in filters:
        f = None if allowed is None else ix.make_filter(allowed)
        for k in M64.KS:
            got = ix.exact_search_device(*S["Q"], k, replica=ix.replicas - 1, filter=f)
            worst = max(worst, _check_rows(S, got, k, lambda q: allowed, tally))
    _say("device exact %s-vt%d" % variant, unambiguous=tally, score_ratio=worst)


@pytest.mark.parametrize("n_docs", [50, 32_767, 32_768, 32_769])
def test_exact_search_device_at_the_range_edges_and_k_above_n_docs(n_docs):
    """The exact file cuts the documents into ranges of 32 768; 50 documents: k above n_docs."""
    rng = np.random.default_rng(n_docs)
    dim = 300
    docs = []
    for d in range(n_docs):
        c = np.sort(rng.choice(dim - 1, int(rng.integers(0, 7)), replace=False)).astype(np.uint32)
        docs.append((c, M64.VALUE_LAWS["exp"](rng, len(c))))
    D = M64._csr(docs)
    qs = [(np.zeros(0, np.uint32), np.zeros(0, np.float32))]
    for _ in range(7):
        c = np.sort(rng.choice(dim, int(rng.integers(1, 25)), replace=False)).astype(np.uint32)
        qs.append((c, M64.VALUE_LAWS["signed"](rng, len(c))))
    Q = M64._csr(qs)
    ix = _native.NativeIndex.build(2, dim, *D, BuildConfig.defaults(n_postings=1, centroid_fraction=1.0, min_cluster_size=0,
                                                                   summary_energy=1.0, max_fraction=1.0, doc_cut=1)).upload(0)
    model = M64.Model(orc.desc_arrays(ix.desc))
    S = dict(model=model, queries=[model.query(*M64.query_at(Q, i), index=i) for i in range(len(qs))])
    allowed = np.flatnonzero(rng.random(n_docs) < 0.5)
    allowed = np.union1d(allowed, [n_docs - 1, max(n_docs - 32_768, 0)])      # the last document, the first of the last range
    worst = 0.0
    for pool, f in ((None, None), (allowed, ix.make_filter(allowed))):
        for k in (10, 64, 1000):
            got = ix.exact_search_device(*Q, k, filter=f)
            assert (got[2] == min(k, n_docs if pool is None else len(pool))).all()
            worst = max(worst, _check_rows(S, got, k, lambda q: pool))
    _say("device exact n_docs=%d" % n_docs, score_ratio=worst)


# ---- approximate search, nothing skipped: heap_factor 0 on non-negative data ----
@pytest.mark.parametrize("variant", NONNEG, ids=NONNEG_IDS)
def test_exhaustive_search_is_the_topk_of_the_candidates(variant, monkeypatch):
    S = _built(*variant)
    ix, model, Q = S["ix"], S["model"], S["Q"]
    rng = np.random.default_rng(8)
    allowed = np.flatnonzero(rng.random(model.n_docs) < 0.4)
    f = ix.make_filter(allowed)
    tally, worst, i = M64.Tally(), 0.0, 0
    for qcut in (1, 4, 1000):
        C = {q.index: model.candidates(q, qcut) for q in S["queries"]}
        for launch in LAUNCHES:
            _launch(monkeypatch, *launch)
            k = M64.KS[i % len(M64.KS)]
            i += 1
            both = []
            for srt in (False, True):
                got = ix.batch_search(*Q, k, qcut, 0.0, srt)
                worst = max(worst, _check_rows(S, got, k, lambda q: C[q.index], tally))
                both.append(got)
            # the walk order of the first list does not matter to an exhaustive search: same sets on unambiguous rows
            # (asserted against the model above), same counts everywhere
            assert np.array_equal(both[0][2], both[1][2]), (qcut, launch, k)
            got = ix.batch_search(*Q, k, qcut, 0.0, bool(i % 2), filter=f)
            worst = max(worst, _check_rows(S, got, k, lambda q: np.intersect1d(C[q.index], allowed)))
        # the single-query entry points: sgpu_search, and the sequential loop over the whole set
        _launch(monkeypatch, "1024", None)
        for k in (10, 129):
            sc, ids, n, _, _ = ix.search_sequential(*Q, k, qcut, 0.0, False)
            worst = max(worst, _check_rows(S, (sc, ids, n), k, lambda q: C[q.index]))
        for q in S["queries"][:8]:
            s, d = ix.search(q.comps, q.vals.astype(np.float32), 65, qcut, 0.0, True)
            model.check_scores(q, d, s)
            model.check_topk(q, d, s, C[q.index], 65)
    _say("device exhaustive %s-vt%d" % variant, unambiguous=tally, score_ratio=worst)


@pytest.mark.parametrize("variant", NONNEG, ids=NONNEG_IDS)
def test_exhaustive_search_with_a_graph_adds_the_neighbours_of_the_first_phase(variant, monkeypatch):
    """A random neighbour table (4 per document; set_knn takes ids below n_docs only). On rows whose first phase is
    unambiguous the answer is the top-k of C plus the first n_knn neighbours of the top-k of C."""
    S = _built(*variant)
    ix, model, Q = S["ix"], S["model"], S["Q"]
    rng = np.random.default_rng(9)
    knn_dim = 4
    graph = rng.integers(0, model.n_docs, (model.n_docs, knn_dim)).astype(np.uint32)
    ix.set_knn(graph.ravel(), knn_dim)
    used, needed, worst = 0, 0, 0.0
    for j, (qcut, k, n_knn) in enumerate(((1, 10, 2), (4, 10, 4), (4, 64, 1), (1000, 10, 3), (2, 129, 9), (4, 1, 4))):
        _launch(monkeypatch, *LAUNCHES[j % len(LAUNCHES)])
        sc, ids, n = ix.batch_search(*Q, k, qcut, 0.0, bool(j % 2), n_knn=n_knn)
        for q in S["queries"]:
            i, m = q.index, int(n[q.index])
            model.check_rows(sc[i], ids[i], m, k, i)
            worst = max(worst, model.check_scores(q, ids[i, :m], sc[i, :m]))
            C = model.candidates(q, qcut)
            order = C[np.argsort(-q.s[C], kind="stable")]
            T = q.tol[C].max() if len(C) else 0.0
            if len(C) > k and not q.s[order[k - 1]] - q.s[order[k]] > 2 * T:
                continue                     # the first phase's own top-k is not determined: nothing to say
            nb = graph[order[:k], : min(n_knn, knn_dim)].ravel().astype(np.int64)
            pool = np.union1d(C, nb)
            model.check_topk(q, ids[i, :m], sc[i, :m], pool, k)
            used += 1
            # rows that show the refinement at work: a neighbour outside C that clears the band, so check_topk (above)
            # demanded it - a search that ignored n_knn could not have returned it
            if len(pool) > k:
                extra = np.setdiff1d(nb, C)
                t = np.sort(q.s[pool])[-k]
                needed += bool((q.s[extra] > t + 2 * q.tol[pool].max()).any())
    assert used >= 100 and needed > 0, (used, needed)
    _say("device exhaustive + graph %s-vt%d" % variant, rows=used, rows_needing_a_neighbour=needed, score_ratio=worst)


# ---- approximate search with pruning ----
@pytest.mark.parametrize("variant", VARIANTS, ids=VARIANT_IDS)
def test_pruned_search_skips_only_what_the_rule_allows(variant, monkeypatch):
    S = _built(*variant)
    ix, model, Q = S["ix"], S["model"], S["Q"]
    nonneg = S["law"] != "signed"
    worst, witnessed, j = 0.0, 0, 0
    for hf in (0.5, 0.8, 1.0, 1.3):
        for qcut in range(1, 13):
            _launch(monkeypatch, *LAUNCHES[j % len(LAUNCHES)])
            k = M64.KS[j % len(M64.KS)]
            j += 1
            sc, ids, n = ix.batch_search(*Q, k, qcut, hf, bool(j % 3 == 0))
            for q in S["queries"]:
                i, m = q.index, int(n[q.index])
                model.check_rows(sc[i], ids[i], m, k, i)
                worst = max(worst, model.check_scores(q, ids[i, :m], sc[i, :m]))
                if nonneg:
                    witnessed += model.check_pruned(q, ids[i, :m], sc[i, :m], k, qcut, hf)
                else:     # (the skip rule's condition is stated for non-negative data; the candidates hold anyway)
                    assert np.isin(ids[i, :m].astype(np.int64), model.candidates(q, qcut)).all(), (i, qcut, hf)
    _say("device pruned %s-vt%d" % variant, score_ratio=worst, skipped_better_documents=witnessed)


# ---- summary dots ----
def _check_dots(ix, model, q, lists):
    worst = 0.0
    for c in lists:
        got = ix.summary_distances(int(c), q.comps, q.vals.astype(np.float32)).astype(np.float64)
        dot, tol = model.summary_dots(int(c), q)
        assert len(got) == len(dot), (c, len(got), len(dot))
        r = np.where(got == dot, 0.0, np.abs(got - dot) / np.where(tol > 0, tol, 1e-300))
        assert (r <= 1.0).all(), "query %d, list %d, block %d: %r, model %r +- %r" % (
            q.index, c, int(np.argmax(r)), got[np.argmax(r)], dot[np.argmax(r)], tol[np.argmax(r)])
        worst = max(worst, float(r.max()) if len(r) else 0.0)
    return worst


@pytest.mark.parametrize("variant", [(name, 0) for name in M64.CASES], ids=list(M64.CASES))
def test_summary_dots_are_the_models(variant):
    S = _built(*variant)
    model, worst = S["model"], 0.0
    lists = np.flatnonzero(np.diff(model.lbs) > 0)
    empty = np.flatnonzero(np.diff(model.lbs) == 0)[:1]
    for q in S["queries"]:
        some = list(lists[:: max(1, len(lists) // 6)]) + [int(x) for x in model.selected_lists(q, 2)] + list(empty)
        worst = max(worst, _check_dots(S["ix"], model, q, some))
    _say("device summary dots %s" % variant[0], dot_ratio=worst)


def test_long_summary_rows_and_more_than_4096_centroids_per_list():
    """Summary rows of more than 64 * 64 * 2 entries and lists of thousands of one-document blocks, built with the
    clustering on the device (more than 4096 centroids per list): the structure of the index and its summary dots."""
    rng = np.random.default_rng(77)
    dim, n_docs = 3000, 12000
    vecs = []
    for d in range(n_docs):   # three ubiquitous light components + a few heavy rare ones
        extra = rng.choice(np.arange(3, dim), int(rng.integers(2, 7)), replace=False)
        c = np.sort(np.concatenate([[0, 1, 2], extra])).astype(np.uint32)
        v = np.where(c < 3, rng.uniform(0.01, 0.05, len(c)), rng.uniform(1.0, 3.0, len(c))).astype(np.float32)
        vecs.append((c, v))
    D = M64._csr(vecs)
    cfg = dict(n_postings=n_docs, centroid_fraction=0.75, summary_energy=1.0, max_fraction=1.0, min_cluster_size=0, doc_cut=10)
    ix = _native.NativeIndex.build(2, dim, *D, BuildConfig.defaults(use_device=1, **cfg)).upload(0)
    model = M64.check_index(orc.desc_arrays(ix.desc), D, cfg)
    nb0 = int(model.lbs[1] - model.lbs[0])
    rows0 = model.row_ptr[model.lrs[0]: model.lrs[1] + 1]
    assert nb0 > 5000 and int(np.diff(rows0).max()) > 64 * 64 * 2, (nb0, np.diff(rows0).max())
    worst = 0.0
    for i, n in enumerate((3, 10, 70, 150)):
        c = np.union1d(rng.choice(dim, n, replace=False), [0]).astype(np.uint32)
        v = M64.VALUE_LAWS["exp"](rng, len(c))
        v[0] = 9.0
        q = model.query(c, v, index=i)
        worst = max(worst, _check_dots(ix, model, q, (0, 1, 2, 5)))
        for k, hf in ((10, 0.0), (100, 0.0), (5, 1.0)):
            s, d = ix.search(c, v, k, 1, hf, False)
            model.check_scores(q, d, s)
            if hf == 0.0:
                model.check_topk(q, d, s, model.candidates(q, 1), k)
            else:
                model.check_pruned(q, d, s, k, 1, hf)
    _say("device summary dots long rows", dot_ratio=worst)


# ---- the built index ----
@pytest.mark.parametrize("name", list(M64.CASES) + ["edges"])
def test_device_assisted_build_and_conversions_are_what_the_header_describes(name):
    if name == "edges":
        cw, dim, D, cfg = M64.edge_inputs()
        base = _native.NativeIndex.build(cw, dim, *D, BuildConfig.defaults(use_device=1, **cfg))
    else:
        S = _built(name, 0)
        base, D, cfg, cw = S["base"], S["D"], S["cfg"], M64.CASES[name][0]
    M64.check_index(orc.desc_arrays(base.desc), D, cfg)
    if name != "edges":
        for vt in (1, 2) if cw == 2 else (1,):
            conv = base.convert(vt)
            assert conv.desc.value_type == vt
            M64.check_index(orc.desc_arrays(conv.desc), D, cfg, conv.desc.val_scale, vt)
