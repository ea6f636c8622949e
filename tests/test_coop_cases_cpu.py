"""The reference side of tests/test_gpu_coop_edges.py, without a device: every case of tests/coop_cases.py reaches the
edges it exists for (check(): block sizes, positions per group, each round's nc against the max_cand the launch
configuration's hook reports for both workgroup sizes), the restatement of the forced schedule reproduces the oracle's rows
bit for bit on every run, six WRONG readings of the protocol each fail on a named case, and the hook says of every run and
both SGPU_BLOCK values what the GPU file relies on: cooperative (forced: 2, auto: 1), not streamed, max_cand, chunk and
chunk_min clamped as launch_config.cpp clamps them."""
import functools

import numpy as np
import pytest

import coop_cases as CC
import model64 as M64
import orc
import stream_cases as SC

LOOKUP = dict(packed=0, dense=1, split=2, hashed=3)      # device_types.hpp: LK_*


@functools.lru_cache(maxsize=None)
def built(name):
    """(case, host index) - nothing is uploaded."""
    case = CC.make(name)
    return case, case.build()


@functools.lru_cache(maxsize=None)
def graph(name):
    return orc.knn_build(built(name)[1].desc, CC.U_KNN)


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
        orc.knn_attach(graph(name), CC.U_KNN)
    try:
        return orc.batch_search(desc, *Q, run.k, run.cut, run.hf, run.first_sorted, n_knn=run.n_knn)[:3]
    finally:
        if run.n_knn:
            orc.knn_attach(None, 0)


@functools.lru_cache(maxsize=None)
def restated(name, run_name, block, n_cu=256, max_lds=160 * 1024):
    """The restatement of every distinct query of a forced run under one workgroup size (and one chip)."""
    case, ix = built(name)
    run = case.runs[run_name]
    return [CC.restate(case, ix, run, block, q, n_cu=n_cu, max_lds=max_lds) for q in run.queries]


@functools.lru_cache(maxsize=None)
def _model(name):
    case, ix = built(name)
    d = ix.desc
    model = M64.Model(orc.desc_arrays(d), d.val_scale, d.value_type)
    return model, {n: model.query(c, v, index=i) for i, (n, (c, v)) in enumerate(case.queries.items())}


@functools.lru_cache(maxsize=None)
def check_rows_against_the_model(name, run_name):
    """model64's checkers on the oracle's rows of a run (test_gpu_coop_edges.py calls this once the device's rows are these
    bit for bit): rows well-formed, every score the full dot product within the model's bound, ids from the walked lists
    (the allowed ones), the row the top-k of that pool where nothing may be skipped (heap_factor 0, non-negative weights).
    Returns the worst score ratio."""
    case, ix = built(name)
    run = case.runs[run_name]
    model, queries = _model(name)
    sc, ids, n = oracle_rows(name, run_name)
    allowed = np.flatnonzero(case.allowed()) if run.filtered else None
    worst = 0.0
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
        if (len(q.vals) == 0 or q.vals.min() >= 0) and run.hf == 0.0:
            model.check_topk(q, ids[i, :m], sc[i, :m], pool, run.k)
    assert worst <= 1.0
    return worst


@pytest.mark.parametrize("name", CC.CASE_NAMES)
def test_case_reaches_its_edges(name):
    case, ix = built(name)
    assert ix.desc.n_docs == case.n_docs <= (140000 if case.kind == "big" else 20000) and ix.desc.value_type == case.value_type and ix.desc.comp_width == case.cw
    assert all(r.edge for r in case.runs.values())
    found = case.check(ix)
    print("coop case %s: %s" % (name, found))


@pytest.mark.parametrize("name", CC.CASE_NAMES)
def test_the_hook_says_cooperative_with_the_clamps(name):
    case, ix = built(name)
    for run in case.runs.values():
        for block in CC.BLOCKS:
            h = CC.hook(case, ix, run, block)
            what = (name, run.name, block)
            if run.k > 256:
                assert (h["coop"], h["streamed"]) == (0, 1), (what, h)      # no cooperative symbol: the plain (streamed) variant
                continue
            want_block = 512 if run.k > 128 else block
            assert (h["coop"], h["streamed"], h["block"]) == (2 if run.mode == "force" else 1, 0, want_block), (what, h)
            uni = h["lds_bytes"] - h["uni"]
            knob = lambda n, d: int(run.env.get(n, d))   # noqa: E731
            assert h["max_cand"] == min(knob("SGPU_COOP_MAX_CAND", 1024), want_block, uni // 20) >= 1, (what, h["max_cand"], uni)
            assert h["chunk"] == min(max(knob("SGPU_COOP_CHUNK", 128), 1), want_block, 1023, uni // 16), (what, h["chunk"])
            assert h["chunk_min"] == min(h["chunk"], max(knob("SGPU_COOP_CHUNK_MIN", 4), 1)), (what, h["chunk_min"])
            assert h["min_items"] == 0 and h["first_reach"] == knob("SGPU_COOP_FIRST_REACH", 256) and h["items_init"] == run.init
            if run.mode == "force":
                assert h["idle_min"] == h["idle_ratio"] == 0
            assert h["max_pos"] == min(65535, max(h["dots_cap"], 1))
            if run.name.startswith("helpers"):                      # the lookup layout the run is named after
                layout = run.name.split("_")[1]
                hh = CC.hook(case, ix, run, block, hash_ok=1) if layout == "hashed" else h
                assert hh["lookup"] == LOOKUP[layout], (what, hh["lookup"])


@pytest.mark.parametrize("name", CC.CASE_NAMES)
def test_the_restatement_reproduces_the_oracles_rows(name):
    case, _ = built(name)
    for run in case.runs.values():
        if run.mode != "force" or run.k > 256:
            continue
        ws, wi, wn = oracle_rows(name, run.name)
        for block in CC.BLOCKS:
            for i, res in enumerate(restated(name, run.name, block)):
                lo, hi = res["spec"]
                assert 0 <= lo <= hi
                if run.hf <= 0 and run.queries[i] != "neg":
                    assert lo == hi, (run.name, run.queries[i])          # nothing is skipped: the counter is one figure
                if run.n_knn:
                    continue                                             # (the restatement stops in front of the refinement)
                what = (name, run.name, block, run.queries[i])
                assert res["n"] == int(wn[i]), what
                assert np.array_equal(res["ids"], wi[i]), (what, res["ids"], wi[i])
                assert np.array_equal(res["scores"].view(np.uint32), ws[i].view(np.uint32)), what


@pytest.mark.parametrize("name", CC.CASE_NAMES)
def test_oracle_rows_pass_the_models_checkers(name):
    case, _ = built(name)
    worst = max(check_rows_against_the_model(name, rn) for rn in case.runs)
    print("model64: %-34s score_ratio=%.4g" % ("oracle coop %s" % name, worst))


@pytest.mark.parametrize("reading", CC.READINGS)
def test_a_wrong_reading_of_the_protocol_fails(reading):
    name, run_name, q, what = CC.WRONG[reading]
    case, ix = built(name)
    run = case.runs[run_name]
    i = run.queries.index(q)
    ws, wi, wn = oracle_rows(name, run_name)
    for block in CC.BLOCKS:
        good = restated(name, run_name, block)[i]
        bad = CC.restate(case, ix, run, block, q, reading=reading)
        same_rows = bad["n"] == int(wn[i]) and np.array_equal(bad["ids"], wi[i]) and np.array_equal(bad["scores"].view(np.uint32), ws[i].view(np.uint32))
        if what == "rows":
            assert not same_rows, (reading, block)
        else:
            assert good["spec"][0] == good["spec"][1]
            assert (bad["rounds"], bad["spec"]) != (good["rounds"], good["spec"]), (reading, block)
            assert not (bad["spec"][0] <= good["spec"][0] <= bad["spec"][1]), (reading, block, bad["spec"], good["spec"])   # counter [7] tells them apart


def test_a_weakened_collection_fails_its_check():
    """Unit blocks rest on the two signature components: without summary_energy 1.0 the blocks merge and check() says so."""
    case = CC.make("units-u16_f16")
    weak = CC.CoopCase.__new__(CC.CoopCase)
    weak.__dict__.update(case.__dict__)
    weak.cfg = dict(case.cfg, centroid_fraction=1e-6)
    with pytest.raises(AssertionError):
        weak.check(weak.build())
