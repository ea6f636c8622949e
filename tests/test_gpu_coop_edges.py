"""The cooperative search rounds (search_coop.inc) at the edges of their board and their replay, on the cases of
tests/coop_cases.py: round geometry against first_reach, list ends and list groups, the candidate limit at max_cand - 1,
max_cand and max_cand + 1, fallbacks in the first and in the second round (the `wl != l` resume), replay windows of 63 ...
129 and 711 candidates, a block of 65 536 postings and one of 65 537, `decided` across windows, documents met twice, every heap variant, negative scores, chunk sizes
and chunks without a live block, document lengths up to 600 components, helpers that change query and lookup form, a
workgroup's next query, more than 1024 rounds of one workgroup, kNN refinement behind a wide round, a filtered search. Every run is launched under SGPU_BLOCK in
{512, 1024} through a resident batch (filtered runs through batch_search): the launch configuration's hook, fed the launch's
facts (hash_ok from sgpu_debug_plan_seeds), must say cooperative and agree with the launch's own statistics and with the
lane's report of the variant that ran (sgpu_debug_lane_variant); the rows are the oracle's bit for bit (n, ids in
order, score bits) and pass the float64 model's checkers; for FORCED runs work counter [7] of sgpu_batch_fetch_stats
(documents scored) equals, query by query, the figure of the restatement in coop_cases.py - the proof that the wide round,
the fallback or the resume really ran on the device; the same call under SGPU_COOP=0 returns the same rows, which only
localises a failure. test_coop_cases_cpu.py proves without a device that the cases reach their edges.
Where counter [7] is not one figure, the test asserts the restatement's bounds and says why: after a fallback under
heap_factor > 0 the local rounds skip blocks against the threshold at each ROUND's start (the restatement gives [blocks
live at their own start, every posting left]); a kNN refinement scores at most n x n_knn more documents.
No test here forces a wait to give up (codes 1, 2, 3), stalls a role or provokes an abort. Run with `-m gpu`."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import coop_cases as CC
import hash_cases as H
import stream_cases as SC
import test_coop_cases_cpu as CPU
from seismic_amd import _native
from seismic_amd._abi import LaunchStats

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _uploaded(name):
    """(case, uploaded index, its filter) - once per module; the kNN graph of the `units` cases is the oracle's."""
    case = CC.make(name)
    ix = case.build()
    if case.kind == "units":
        ix.set_knn(CPU.graph(name), CC.U_KNN)
    ix.upload(0)
    return case, ix, ix.make_filter(case.allowed())


def _chip():
    p = torch.cuda.get_device_properties(0)
    return p.multi_processor_count, int(getattr(p, "shared_memory_per_block", 160 * 1024))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _launch(case, ix, flt, run, Q):
    """One call of the run: (rows, launch statistics, work counters or None). A filtered run goes through batch_search (its
    statistics: the last launch's), the others through a resident batch."""
    if run.filtered:
        rows = ix.batch_search(*Q, run.k, run.cut, run.hf, run.first_sorted, n_knn=run.n_knn, filter=flt)
        stats = LaunchStats()
        _native.check(_native.lib().sgpu_batch_sync(ix.h, ctypes.byref(stats)))
        return rows, stats, None
    b = _native.DeviceBatch(ix, *Q, run.k)
    stats = b.run(run.k, run.cut, run.hf, run.first_sorted, n_knn=run.n_knn)      # (raises unless SGPU_OK: a flagged launch fails here)
    rows = b.fetch(run.k)
    counters = b.fetch_stats()
    b.close()
    return rows, stats, counters


def _assert_rows(got, want, pick, what):
    """Device rows = the oracle's rows of the run's distinct queries (`pick`: which of them each device row is)."""
    (gs, gi, gn), (ws, wi, wn) = got, want
    assert np.array_equal(gn, wn[pick]), (what, np.flatnonzero(gn != wn[pick])[:8])
    bad = np.flatnonzero((gi != wi[pick]).any(axis=1) | (_bits(gs) != _bits(ws)[pick]).any(axis=1))
    if len(bad):
        q = int(bad[0])
        at = int(np.flatnonzero((gi[q] != wi[pick[q]]) | (_bits(gs)[q] != _bits(ws)[pick[q]]))[0])
        raise AssertionError("%s: query %d differs first at rank %d: device (%r, %d), oracle (%r, %d); %d of %d rows differ" % (
            what, q, at, gs[q, at], gi[q, at], ws[pick[q], at], wi[pick[q], at], len(bad), len(gn)))


def _cooperative(case, ix, flt, name, run, block, chip, seen):
    """The cooperative launch of one run and every assertion on it; returns its rows."""
    n_cu, max_lds = chip
    Q = case.batch(run)
    nq = len(Q[0]) - 1
    pick = np.arange(nq) % len(run.queries)
    what = "%s %s block %d (%s)" % (name, run.name, block, run.edge)
    rows, stats, counters = _launch(case, ix, flt, run, Q)
    # proof of variant: the hook, fed this launch's facts under this environment, says cooperative, and the launch took
    # that workgroup size and that much LDS
    # (hash_ok of this very batch from the host plan's own seed search, equal to the restatement's: hash_cases.py)
    ok, _ = _native.debug_plan_seeds(ix, *Q, run.cut)
    assert ok == H.seeds(Q[0], Q[1], case.dim, case.cw, case.value_type, os.environ.get("SGPU_NO_HASH") == "1")[0], (what, ok)
    facts = dict(SC.plan_facts(case, ix, run, Q), hash_ok=ok)
    hook = _native.debug_launch_config(n_cu=n_cu, max_lds=max_lds, heap_factor=run.hf, **facts)
    if run.k > 256:
        assert hook["coop"] == 0, (what, hook)                       # no cooperative symbol for this k: the plain variant
    else:
        assert (hook["coop"], hook["streamed"]) == (2 if run.mode == "force" else 1, 0), (what, hook)
    assert stats.block == hook["block"], (what, stats.block, hook)
    # the lane reports the variant that ran: a resident batch launches on the main lane; a filtered run goes through the
    # entry point, whose first (here: only) chunk takes pool lane 0. The lookup and the counted word are the hook's exactly;
    # so are streamed and cooperative where the hook was fed the launch's own size (the resident batch)
    v = _native.debug_lane_variant(ix, 0 if run.filtered else -1)
    assert v is not None and (v["lookup"], v["counted"]) == (hook["lookup"], hook["counted"]), (what, v, hook)
    if not run.filtered:
        assert v == {k_: hook[k_] for k_ in ("lookup", "streamed", "coop", "counted")}, (what, v, hook)
    if "SGPU_FORCE_HASH" in run.env:
        # every query of these batches has a seed, so the forced launch IS the hashed one
        assert ok == 1 and hook["lookup"] == CPU.LOOKUP["hashed"], (what, ok, hook["lookup"])
    seen.setdefault("hashed", []).append(v["lookup"] == CPU.LOOKUP["hashed"])       # (what the LANE said ran)
    # (a filtered run goes through the entry point, which may cut the call into several launches and reports the last
    # one's statistics: its workgroup size is compared, its LDS bytes are not)
    assert run.filtered or stats.lds_bytes == hook["lds_bytes"], (what, stats.lds_bytes, hook)
    assert stats.n_queries == nq or (run.filtered and 0 < stats.n_queries < nq)
    if run.name == "next_query":
        assert stats.grid < nq and np.gcd(stats.grid, len(run.queries)) == 1, (what, stats.grid)   # every workgroup goes on to a next query
    # results: the oracle's rows, bit for bit (every occurrence of a repeated query the same row)
    _assert_rows(rows, CPU.oracle_rows(name, run.name), pick, what)
    CPU.check_rows_against_the_model(name, run.name)      # (the float64 checks, on these very rows)
    # documents scored, query by query: the restatement's figure
    if run.mode == "force" and counters is not None and run.k <= 256:
        res = CPU.restated(name, run.name, block, n_cu, max_lds)
        lo = np.array([r["spec"][0] for r in res], np.int64)[pick]
        hi = np.array([r["spec"][1] for r in res], np.int64)[pick]
        if run.n_knn:   # the refinement behind the rounds scores the neighbours of the n results: at most n_knn each
            hi = hi + rows[2].astype(np.int64) * run.n_knn
        got = counters[:, 7].astype(np.int64)
        for q in range(min(nq, 8)):
            print("%s query %d (%s): documents scored %d, restated [%d, %d]" % (what, q, run.queries[pick[q]], got[q], lo[q], hi[q]))
        bad = np.flatnonzero((got < lo) | (got > hi))
        assert len(bad) == 0, (what, [(int(q), run.queries[pick[q]], int(got[q]), int(lo[q]), int(hi[q])) for q in bad[:8]])
        assert (counters[:, 20] < stats.grid).all()
        if run.name == "wrap":
            # the rounds each workgroup opened: the restated round counts of the queries it served (stats word 20)
            per_wg = np.bincount(counters[:, 20], np.array([CC.wide_rounds(r) for r in res], np.int64)[pick], stats.grid)
            print("%s: grid %d, wide rounds per workgroup min %d mean %.0f max %d, %d workgroups above %d" % (
                what, stats.grid, per_wg.min(), per_wg.mean(), per_wg.max(), (per_wg > CC.SEQ_WRAP).sum(), CC.SEQ_WRAP))
            assert stats.grid <= CC.MAX_GRID and per_wg.max() > CC.SEQ_WRAP, (what, stats.grid, per_wg.max())
    return rows


@pytest.mark.parametrize("block", CC.BLOCKS)
@pytest.mark.parametrize("name", CC.CASE_NAMES)
def test_cooperative_rows_and_documents_scored_are_the_restatements(name, block, monkeypatch):
    case, ix, flt = _uploaded(name)
    chip = _chip()
    failures, rows, seen = [], {}, {}
    # First every cooperative launch of the case, one straight after the other on one lane: launches of 1, 2, 7, some, 1050
    # and 52000 queries meet what the launch before left on the board (slots, open bits, counters). A run that fails an
    # assertion is reported at the end with the others. (Anything but an AssertionError - a flagged or failed launch - ends
    # the test at once: nothing more is started on the device.)
    for run in case.runs.values():
        with monkeypatch.context() as m:
            for k_, v_ in CC.knob_env(case, run, block).items():
                m.setenv(k_, v_)
            try:
                rows[run.name] = _cooperative(case, ix, flt, name, run, block, chip, seen)
            except AssertionError as e:
                failures.append("%s: %s" % (run.name, str(e)[:2000]))
    if case.form == "u32_f16":
        assert any(seen.get("hashed", [])), "no launch took the hashed lookup: %r" % seen
    # then the cross-check, which only localises a failure: the plain launch of the same call returns the same rows
    for run in case.runs.values():
        if run.name not in rows:
            continue
        with monkeypatch.context() as m:
            for k_, v_ in CC.knob_env(case, run, block).items():
                m.setenv(k_, v_)
            m.setenv("SGPU_COOP", "0")
            Q = case.batch(run)
            off_rows, off_stats, _ = _launch(case, ix, flt, run, Q)
            off = _native.debug_launch_config(n_cu=chip[0], max_lds=chip[1], heap_factor=run.hf, **SC.plan_facts(case, ix, run, Q))
            try:
                assert off["coop"] == 0 and off_stats.block == off["block"], run.name
                for a, b in zip(rows[run.name], off_rows):
                    assert np.array_equal(_bits(a) if a.dtype == np.float32 else a, _bits(b) if b.dtype == np.float32 else b), run.name
            except AssertionError as e:
                failures.append("%s under SGPU_COOP=0: %s" % (run.name, str(e)[:500]))
    assert not failures, "%d run(s) failed:\n%s" % (len(failures), "\n".join(failures))
