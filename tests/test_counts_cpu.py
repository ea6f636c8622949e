"""Per-query work counts of the oracle (orc.batch_search_counts: the quantities of sgpu_batch_fetch_stats counters
[0..6] and the query's algorithmic bytes), pinned three ways without a GPU: they sum to the batch totals the oracle has
always returned, they equal the float64 model's counts (tests/model64.py: Model.work_counts, derived from the descriptor
and the header's text alone) wherever the model is defined, and they equal a known answer derived by hand.
tests/test_gpu_counters.py then holds the kernel's counters to the same numbers."""
import functools

import numpy as np
import pytest

import model64 as M64
import orc
from seismic_amd._abi import BuildConfig

TOTALS = {"blocks_total": 0, "summary_entries": 2, "blocks_scored": 3, "postings_seen": 4, "docs_scored": 5,
          "algo_bytes": 7}   # field of orc.Stats -> column of the per-query counts
# (k, query_cut, heap_factor, first_sorted)
PARAMS = [(10, 4, 1.0, False), (1, 1, 0.7, True), (129, 20, 0.0, False), (300, 4, -0.5, True), (10, 20, 0.7, False)]
VARIANTS = [(name, 0) for name in M64.CASES] + [("exp_w2_300", 1), ("flat_w4_70000", 1)]
VARIANT_IDS = ["%s-vt%d" % v for v in VARIANTS]


@functools.lru_cache(maxsize=None)
def _setup(name, vt):
    cw, dim, D, Q, law, cfg = M64.make_case(name)
    keep = orc.OracleIndex(cw, dim, *D, BuildConfig.defaults(**cfg))
    if vt == 1:
        keep = keep.convert_fixedu8()
    Q = M64.distinct_weights(Q)
    model = M64.Model(orc.desc_arrays(keep.desc), keep.desc.val_scale, keep.desc.value_type)
    queries = [model.query(*M64.query_at(Q, i), index=i) for i in range(len(Q[0]) - 1)]
    return dict(keep=keep, desc=keep.desc, model=model, queries=queries, Q=Q, law=law, cw=cw)


def _same_rows(a, b):
    assert np.array_equal(a[2], b[2]) and np.array_equal(a[1], b[1])
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))


@pytest.mark.parametrize("variant", VARIANTS, ids=VARIANT_IDS)
def test_per_query_counts_sum_to_the_batch_totals(variant):
    S = _setup(*variant)
    graph = orc.knn_build(S["desc"], 4)
    for n_knn in (0, 3):
        orc.knn_attach(graph if n_knn else None, 4 if n_knn else 0)
        try:
            for k, qcut, hf, srt in PARAMS:
                got = orc.batch_search_counts(S["desc"], *S["Q"], k, qcut, hf, srt, n_knn=n_knn)
                ref = orc.batch_search(S["desc"], *S["Q"], k, qcut, hf, srt, n_knn=n_knn, num_threads=2)
                _same_rows(got[:3], ref[:3])
                for name, col in TOTALS.items():
                    assert int(got[3][:, col].sum()) == ref[3][name], (name, k, qcut, hf, srt, n_knn)
                # the bytes are the header's seven quantities and nothing else, query by query
                c = got[3].astype(np.int64)
                nnz_q = np.diff(S["Q"][0].astype(np.int64))
                per_elem = S["cw"] + (1 if S["desc"].value_type else 2)
                want = (nnz_q * (S["cw"] + 4) + 12 * k + 8 * c[:, 0] + 8 * c[:, 1] + 3 * c[:, 2] + 4 * (c[:, 3] + c[:, 4])
                        + 8 * c[:, 5] + per_elem * c[:, 6])
                assert np.array_equal(c[:, 7], want), (k, qcut, hf, srt, n_knn)
        finally:
            orc.knn_attach(None, 0)


@pytest.mark.parametrize("variant", VARIANTS, ids=VARIANT_IDS)
def test_model_counts_equal_the_oracles(variant):
    """[0..2] under every parameter set; [3..6] where nothing may be skipped (heap_factor 0.0, no negative value)."""
    S = _setup(*variant)
    model = S["model"]
    for k, qcut, hf, srt in PARAMS:
        counts = orc.batch_search_counts(S["desc"], *S["Q"], k, qcut, hf, srt)[3].astype(np.int64)
        for q in S["queries"]:
            assert np.array_equal(counts[q.index, :3], model.work_counts(q, qcut)), (q.index, k, qcut, hf, srt)
    if S["law"] == "signed":
        return
    for k, qcut, srt in ((1, 1, False), (10, 4, True), (129, 20, False), (1000, 1000, True)):
        counts = orc.batch_search_counts(S["desc"], *S["Q"], k, qcut, 0.0, srt)[3].astype(np.int64)
        for q in S["queries"]:
            assert np.array_equal(counts[q.index, :7], model.work_counts(q, qcut, exhaustive=True)), (q.index, k, qcut, srt)
    # the cases do meet documents again in later lists, and lists with more than one block
    assert (counts[:, 4] > counts[:, 5]).sum() > len(counts) // 2 and (counts[:, 0] > counts[:, 0].min()).any()


def test_hand_derived_counts_on_four_documents():
    """The four documents of golden/kat_empty_vectors.json, built with summary_energy 1.0 (every component of a block
    is summarised; no tie between equal maxima decides what is kept):
      d0 = {0: 1, 2: 2, 4: 3}   d1 = d2 = {}   d3 = {0: 1, 1: 2, 2: 3, 3: 4}
    Nothing is pruned (7 values against dim x n_postings slots) and every list has at most two postings, hence ONE block:
      list 0 = {d0, d3}  list 1 = {d3}  list 2 = {d0, d3}  list 3 = {d3}  list 4 = {d0}
    A block's summary has one row per component any of its documents has, one entry per row (one block per list):
      list 0 and list 2: rows 0 1 2 3 4     list 1 and list 3: rows 0 1 2 3     list 4: rows 0 2 4
    Query A = {0: 1, 1: 2, 2: 3, 3: 4}, k 10, query_cut 5: lists 3, 2, 1, 0 (descending weight); the heap never fills.
      [0] 4 blocks  [1] rows matched 4 + 4 + 4 + 4 = 16  [2] 16 entries  [3] 4 blocks pass  [4] postings 1 + 2 + 1 + 2 = 6
      [5] d3 (list 3) and d0 (list 2) are scored; d3 is met again in lists 2, 1, 0 and d0 in list 0: 2 documents
      [6] 4 + 3 = 7 components
      bytes = 4 * (2 + 4) + 12 * 10 + 8 * 4 + 8 * 16 + 3 * 16 + 4 * (6 + 4) + 8 * 2 + 7 * (2 + 2) = 436
    Query B = {1: 1, 4: 2}, k 10, query_cut 1: list 4 only. Its rows 0 2 4 meet the query in row 4:
      [0] 1  [1] 1  [2] 1  [3] 1  [4] 1  [5] 1 (d0)  [6] 3
      bytes = 2 * 6 + 120 + 8 + 8 + 3 + 4 * 2 + 8 + 3 * 4 = 179
    Query C = {1: 3, 4: 1}, k 1, query_cut 2, heap_factor 1.0: list 1 first. d3 scores 3 * 2 = 6 and fills the heap.
      List 4's block: its summary meets the query in row 4 only, dot = about 3 * 1 (the block's maximum of component 4)
      < 1.0 * 6: skipped. Both lists' summaries were read, one block passed:
      [0] 2  [1] 1 + 1 = 2  [2] 2  [3] 1  [4] 1  [5] 1 (d3)  [6] 4
      bytes = 2 * 6 + 12 + 8 * 2 + 8 * 2 + 3 * 2 + 4 * 2 + 8 + 4 * 4 = 94"""
    import json
    import os
    g = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "kat_empty_vectors.json")))
    ix = orc.OracleIndex(2, g["dim"], *orc.csr([(d["components"], d["values"]) for d in g["docs"]]),
                         BuildConfig.defaults(summary_energy=1.0))
    a = orc.desc_arrays(ix.desc)
    assert np.diff(a["list_block_start"].astype(np.int64)).tolist() == [1, 1, 1, 1, 1]
    cases = [(([0, 1, 2, 3], [1.0, 2.0, 3.0, 4.0]), (10, 5, 0.7), [4, 16, 16, 4, 6, 2, 7, 436], [3, 0]),
             (([1, 4], [1.0, 2.0]), (10, 1, 0.7), [1, 1, 1, 1, 1, 1, 3, 179], [0]),
             (([1, 4], [3.0, 1.0]), (1, 2, 1.0), [2, 2, 2, 1, 1, 1, 4, 94], [3])]
    for q, (k, qcut, hf), want, want_ids in cases:
        sc, ids, n, counts = orc.batch_search_counts(ix.desc, *orc.csr([q]), k, qcut, hf)
        assert counts[0].tolist() == want, (q, counts[0].tolist())
        assert ids[0, :int(n[0])].tolist() == want_ids
    # two in one batch: each query keeps its own counts (B with query_cut 5 also walks list 1: rows 0 1 2 3 meet it in
    # row 1, d3 is scored: two of everything, 3 + 4 components)
    counts = orc.batch_search_counts(ix.desc, *orc.csr([c[0] for c in cases[:2]]), 10, 5, 0.7)[3]
    assert counts[0].tolist() == cases[0][2] and counts[1, :7].tolist() == [2, 2, 2, 2, 2, 2, 7]
