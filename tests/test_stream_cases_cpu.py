"""The reference side of tests/test_gpu_stream_edges.py, without a device: every case of tests/stream_cases.py reaches the
edges it exists for (check(): wrap counts, block sizes, position counts, document lengths, the straddle, the skippable
run), every knob set the GPU file launches is - by the launch configuration's own test hook - a streamed launch with the
intended ring and workgroup size (and the round loop under SGPU_STREAM=0), the host's search equals the oracle's on every
case, and the oracle's rows of every run satisfy the float64 model's checkers with the model's own bounds. The library has
no approximate search on the host: "the host's search" is exact search, compared with the oracle's sequential brute force.
Lines starting "model64:" report the model's verdicts (run with -s)."""
import functools

import numpy as np
import pytest

import model64 as M64
import orc
import stream_cases as SC
from seismic_amd import _native


@functools.lru_cache(maxsize=None)
def built(name):
    """(case, host index) - nothing is uploaded."""
    case = SC.make(name)
    return case, case.build()


@functools.lru_cache(maxsize=None)
def graph(name):
    """The kNN graph of a case's index (the oracle's Knn::new)."""
    return orc.knn_build(built(name)[1].desc, SC.U_KNN)


@functools.lru_cache(maxsize=None)
def oracle_rows(name, run_name):
    """(scores, ids, n) the oracle returns for a run's DISTINCT queries, in the run's order; a filtered run searches the
    descriptor without the postings of the documents the filter removes."""
    case, ix = built(name)
    run = case.runs[run_name]
    desc, keep = ix.desc, None
    if run.filtered:
        keep = SC.FilteredDesc(ix.desc, case.allowed())
        desc = keep.desc
    Q = orc.csr([case.queries[n] for n in run.queries])
    if run.n_knn:
        orc.knn_attach(graph(name), SC.U_KNN)
    try:
        return orc.batch_search(desc, *Q, run.k, run.cut, run.hf, run.first_sorted, n_knn=run.n_knn)[:3]
    finally:
        if run.n_knn:
            orc.knn_attach(None, 0)


@functools.lru_cache(maxsize=None)
def _model(name):
    case, ix = built(name)
    d = ix.desc
    model = M64.Model(orc.desc_arrays(d), d.val_scale, d.value_type)
    return model, {n: model.query(c, v, index=i) for i, (n, (c, v)) in enumerate(case.queries.items())}


@functools.lru_cache(maxsize=None)
def check_rows_against_the_model(name, run_name):
    """model64's checkers on the oracle's rows of a run (test_gpu_stream_edges.py calls this once the device's rows are
    these bit for bit): every row is well-formed, every score is the full dot product within the model's bound, the ids
    come from the walked lists (the allowed ones), the row is the top-k of that pool where nothing may be skipped
    (heap_factor 0 on non-negative weights) and pruning skipped only what the summary dots allowed (heap_factor >= 0).
    kNN refinement and filters leave the pool rules out. Returns (tally, worst score ratio, documents pruning cost)."""
    case, ix = built(name)
    run = case.runs[run_name]
    model, queries = _model(name)
    sc, ids, n = oracle_rows(name, run_name)
    allowed = np.flatnonzero(case.allowed()) if run.filtered else None
    tally, worst, witnessed = M64.Tally(), 0.0, 0
    for i, qn in enumerate(run.queries):
        q, m = queries[qn], int(n[i])
        model.check_rows(sc[i], ids[i], m, run.k, i)
        worst = max(worst, model.check_scores(q, ids[i, :m], sc[i, :m]))
        if run.n_knn:
            continue
        pool = model.candidates(q, run.cut)
        if allowed is not None:
            pool = np.intersect1d(pool, allowed)
        assert np.isin(ids[i, :m].astype(np.int64), pool).all(), (run_name, qn)
        nonneg = len(q.vals) == 0 or q.vals.min() >= 0
        if nonneg and run.hf == 0.0:
            tally.add(model.check_topk(q, ids[i, :m], sc[i, :m], pool, run.k))
        elif nonneg and run.hf > 0 and allowed is None:
            witnessed += model.check_pruned(q, ids[i, :m], sc[i, :m], run.k, run.cut, run.hf)
    return tally, worst, witnessed


@pytest.mark.parametrize("name", SC.CASE_NAMES)
def test_case_reaches_its_edges(name):
    case, ix = built(name)
    assert ix.desc.n_docs == case.n_docs <= 20000 and ix.desc.value_type == case.value_type and ix.desc.comp_width == case.cw
    found = case.check(ix)
    print("stream case %s: %s" % (name, found))
    if case.value_type == 2:
        assert ix.stream_stats()[0] == found["raw_documents"] > 0      # the library keeps exactly those documents raw


@pytest.mark.parametrize("name", SC.CASE_NAMES)
def test_every_knob_set_is_a_streamed_launch_with_the_intended_ring(name, monkeypatch):
    case, ix = built(name)
    seen = set()
    for run in case.runs.values():
        Q = case.batch(run)
        for ring, asked, block, env in SC.knob_sets(case, run):
            for k_, v_ in env.items():
                monkeypatch.setenv(k_, v_)
            facts = SC.plan_facts(case, ix, run, Q)
            out = _native.debug_launch_config(heap_factor=run.hf, **facts)
            assert (out["streamed"], out["coop"], out["ring"], out["p_ring"], out["block"]) == (1, 0, ring, ring, block), (run.name, env, out)
            assert out["items_init"] <= ring and out["items_min"] <= out["items_init"]
            if run.env.get("SGPU_ITEMS_INIT") == "16":
                assert out["items_init"] == out["items_min"] == 16 < SC.WINDOW       # a budget below one window
            if run.env.get("SGPU_ITEMS_INIT") == "1024":
                assert out["items_init"] == ring                                       # (256: above bud_max = ring - 64, clamped there)
            if run.env.get("SGPU_DOTS_CAP") == "1":
                assert out["dots_cap"] == facts["max_list_nb"]                         # one list per group
            if run.env.get("SGPU_LIST_GROUP") == "4":
                assert out["qg"] == 4 and out["qc"] == 9                               # groups of 4 + 4 + 1
            seen.add((ring, block))
            monkeypatch.setenv("SGPU_STREAM", "0")
            off = _native.debug_launch_config(heap_factor=run.hf, **facts)
            assert (off["streamed"], off["coop"], off["ring"], off["block"]) == (0, 0, 0, block), (run.name, off)
            for k_ in list(env) + ["SGPU_STREAM"]:
                monkeypatch.delenv(k_)
    assert {r for r, _ in seen} == set(SC.RINGS) and {b for _, b in seen} == set(SC.BLOCKS)


@pytest.mark.parametrize("name", SC.CASE_NAMES)
def test_host_search_equals_the_oracles(name):
    case, ix = built(name)
    names = [n for n in case.queries]
    Q = orc.csr([case.queries[n] for n in names])
    for k in (1, 10, 100):
        host = ix.exact_search(*Q, k)
        for i, n in enumerate(names):
            es, ei = orc.exact_search(ix.desc, *case.queries[n], k, orc.ORDER_SEQ)
            m = int(host[2][i])
            assert m == len(ei) and np.array_equal(host[1][i, :m], ei), (k, n)
            assert np.array_equal(host[0][i, :m].view(np.uint32), es.view(np.uint32)), (k, n)


@pytest.mark.parametrize("name", SC.CASE_NAMES)
def test_oracle_rows_pass_the_models_checkers(name):
    case, _ = built(name)
    total, worst, witnessed = M64.Tally(), 0.0, 0
    for run_name in case.runs:
        tally, w, wit = check_rows_against_the_model(name, run_name)
        total.clear, total.chosen, total.trivial = total.clear + tally.clear, total.chosen + tally.chosen, total.trivial + tally.trivial
        worst, witnessed = max(worst, w), witnessed + wit
    print("model64: %-34s unambiguous=%s score_ratio=%.4g skipped_better_documents=%d" % ("oracle stream %s" % name, total, worst, witnessed))
    assert worst <= 1.0


def test_a_weakened_collection_fails_its_check():
    """Halving n_postings prunes the long lists: the block sizes and wrap counts no longer hold, and check() says so."""
    case = SC.make("blocks-u16_f16")
    weak = SC.StreamCase.__new__(SC.StreamCase)
    weak.__dict__.update(case.__dict__)
    weak.cfg = dict(case.cfg, n_postings=case.cfg["n_postings"] // 2)
    with pytest.raises(AssertionError):
        weak.check(weak.build())
