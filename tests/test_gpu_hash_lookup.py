"""The hashed query lookup (LK_HASH: sk_u32_hash.hip, search_score.inc accumulate_chunk, search_stage01.inc build_lookup)
on the batches of tests/hash_cases.py, over a vocabulary of 70 000 and one of 2^24 - 1 ids. Every batch runs through a
resident batch under 512- and 1024-thread workgroups x the round loop (SGPU_STREAM=0), the streamed variant and the forced
cooperative variant, through the counted pass, once with n_knn > 0, and through batch_search (the staged entry point)
unfiltered and filtered. Per launch: the lane hook (sgpu_debug_lane_variant) reports the lookup, streamed, cooperative and
counted words of the launch configuration's hook fed the launch's facts and the restatement's hash_ok - lookup == 3 exactly
where every query has a seed (and the batch is not the one named case the LDS fitting declines: alone_fit on the small
vocabulary; on the large one nothing else fits and it must be hashed), otherwise the hook's fallback layout, or SGPU_ELIMIT
from both where a query has no seed and no fallback fits the vocabulary; the launch took the hook's LDS bytes; the
rows are the oracle's bit for bit, every occurrence of a repeated query the same row; the counted pass's counters [0..6]
are the oracle's. Staged calls: every chunk was planned by the host and ran the layout the hook names for that chunk.
Slot-mates: the device's score of every mate document is the oracle's f32 score, within the float64 model's bound, and is
NOT the score a kernel without the id compare would give (hash_cases.wrong_score). test_hash_cases_cpu.py proves without a
device that the cases reach their edges. No test here provokes a fault. Run with `-m gpu`."""
import functools

import numpy as np
import pytest
import torch

import coop_cases as CC
import hash_cases as H
import orc
import stream_cases as SC
import test_hash_cases_cpu as CPU
from seismic_amd import _native

pytestmark = pytest.mark.gpu
HASHED = {"sizes", "cycle", "alone", "mates"}          # the batches named hashed: every launch of them must report lookup == 3
BATCHES = ("sizes", "cycle", "mixed", "alone", "alone_fit", "rule", "mates")
VARIANT_WORDS = {"loop": (0, 0, 0), "stream": (1, 0, 0), "coop": (0, 2, 0), "counted": (0, 0, 1)}   # streamed, coop, counted


@functools.lru_cache(maxsize=None)
def _uploaded(vocab):
    """(case, uploaded index with the oracle's kNN graph, its filter) - once per module."""
    case, ix = CPU.built(vocab)
    ix.set_knn(CPU.graph(vocab), H.KNN)
    ix.upload(0)
    return case, ix, ix.make_filter(case.allowed())


def _chip():
    p = torch.cuda.get_device_properties(0)
    return dict(n_cu=p.multi_processor_count, max_lds=int(getattr(p, "shared_memory_per_block", 160 * 1024)))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _assert_rows(got, want, pick, what):
    (gs, gi, gn), (ws, wi, wn) = got, want
    assert np.array_equal(gn, wn[pick]), (what, np.flatnonzero(gn != wn[pick])[:8])
    bad = np.flatnonzero((gi != wi[pick]).any(axis=1) | (_bits(gs) != _bits(ws)[pick]).any(axis=1))
    if len(bad):
        q = int(bad[0])
        at = int(np.flatnonzero((gi[q] != wi[pick[q]]) | (_bits(gs)[q] != _bits(ws)[pick[q]]))[0])
        raise AssertionError("%s: query %d differs first at rank %d: device (%r, %d), oracle (%r, %d); %d of %d rows differ" % (
            what, q, at, gs[q, at], gi[q, at], ws[pick[q], at], wi[pick[q], at], len(bad), len(gn)))
    for j in range(int(pick.max()) + 1):                # every occurrence of a repeated query: the same row
        same = np.flatnonzero(pick == j)
        assert (gi[same] == gi[same[0]]).all() and (_bits(gs)[same] == _bits(gs)[same[0]]).all(), (what, j)


def _oracle(case, ix, run, n_knn=0, desc=None):
    Q = orc.csr([case.queries[n] for n in run.queries])
    if n_knn:
        orc.knn_attach(CPU.graph(case.vocab), H.KNN)
    try:
        return orc.batch_search(desc or ix.desc, *Q, run.k, run.cut, run.hf, run.first_sorted, n_knn=n_knn)[:3]
    finally:
        if n_knn:
            orc.knn_attach(None, 0)


@functools.lru_cache(maxsize=None)
def _mate_references(vocab):
    """Per mate document, once: (the oracle's f32 score, the float64 score, its f32 bound, the score without the id compare)."""
    case, ix, _ = _uploaded(vocab)
    qc, qv = case.queries["mates"]
    out = []
    for j, (dc, dv) in enumerate(case.mate_docs):
        right, tol = H.right_score(qc, qv, dc, dv.astype(np.float64))
        out.append((np.float32(orc.score_doc(ix.desc, H.N_DOCS + j, qc, qv)), right, tol, H.wrong_score(qc, qv, dc, dv, H.DIMS[vocab])))
    return out


def _mate_scores(case, ix, rows, what):
    """The slot-mate and sentinel documents of the row of `mates`: the oracle's f32 score, inside the float64 bound, and not
    the score without the id compare."""
    gs, gi, gn = rows
    row = {int(d): gs[0, i] for i, d in enumerate(gi[0, : gn[0]])}
    for j, (want, right, tol, wrong) in enumerate(_mate_references(case.vocab)):
        doc = H.N_DOCS + j
        assert doc in row, (what, doc)
        got = row[doc]
        assert _bits(got) == _bits(want), (what, doc, got, want)
        assert abs(float(got) - right) <= tol, (what, doc, got, right, tol)
        assert np.float32(wrong) != got and abs(wrong - float(got)) > tol, (what, doc, got, wrong)


def _lane_report(ix, lane=-1):
    v = _native.debug_lane_variant(ix, lane)
    assert v is not None, "the lane has launched nothing"
    return v


@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("vocab", H.VOCABS)
def test_resident_launches_report_the_lookup_and_return_the_oracles_rows(vocab, batch):
    case, ix, _ = _uploaded(vocab)
    run = case.runs[batch]
    Q = case.batch(run)
    nq = len(Q[0]) - 1
    pick = np.arange(nq) % len(run.queries)
    ws, wi, wn, wc = CPU.oracle_counts(vocab, batch)
    for variant, block, env, mode in CPU.launches():
        env = CPU.launch_env(run, env)
        what = "%s %s %s block %d" % (vocab, batch, variant, block)
        ok, h = CPU.expectation(case, ix, run, env, mode, **_chip())
        with CC.knobs(env):
            b = _native.DeviceBatch(ix, *Q, run.k)
            try:
                if h is None:                           # no lookup layout fits: the launch says so, as the hook did
                    assert vocab == "large" and not ok, what
                    with pytest.raises(_native.SeismicHipError) as e:
                        b.run(run.k, run.cut, run.hf)
                    assert e.value.status == CPU.SGPU_ELIMIT, (what, e.value)
                    print("%s: hash_ok %d, SGPU_ELIMIT from the hook and from the launch" % (what, ok))
                    continue
                stats = (b.run_counted if mode == 2 else b.run)(run.k, run.cut, run.hf)
                rows = b.fetch(run.k)
                v = _lane_report(ix)
                print("%s: hash_ok %d, lookup %d streamed %d coop %d counted %d, lds %d" % (
                    what, ok, v["lookup"], v["streamed"], v["coop"], v["counted"], stats.lds_bytes))
                assert v == {k_: h[k_] for k_ in ("lookup", "streamed", "coop", "counted")}, (what, v, h)
                assert (v["lookup"] == H.LK_HASH) == bool(ok and (vocab, batch) not in H.LDS_DECLINES), (what, v, ok)
                assert batch not in HASHED or v["lookup"] == H.LK_HASH, (what, v)
                assert (v["streamed"], v["coop"], v["counted"]) == VARIANT_WORDS[variant], (what, v)
                assert (stats.block, stats.lds_bytes, stats.n_queries) == (h["block"], h["lds_bytes"], nq), (what, stats.block, stats.lds_bytes, h)
                if run.cycle and variant != "coop":     # more queries than workgroups; `cycle`: seven queries against a grid coprime to 7
                    assert stats.grid < nq and (batch != "cycle" or np.gcd(stats.grid, len(run.queries)) == 1), (what, stats.grid)
                _assert_rows(rows, (ws, wi, wn), pick, what)
                if batch == "mates":
                    _mate_scores(case, ix, rows, what)
                if mode == 2:
                    got = b.fetch_stats()[:, :7].astype(np.int64)
                    want = wc[pick][:, :7].astype(np.int64)
                    bad = np.flatnonzero((got != want).any(axis=1))
                    assert len(bad) == 0, "%s: counters of query %d: device %s, oracle %s (%s)" % (
                        what, bad[0], got[bad[0]].tolist(), want[bad[0]].tolist(), ", ".join(orc.COUNT_NAMES[:7]))
            finally:
                b.close()


@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("vocab", H.VOCABS)
def test_knn_refinement_behind_the_hashed_lookup(vocab, batch):
    case, ix, _ = _uploaded(vocab)
    run = case.runs[batch]
    env = CPU.launch_env(run, dict(H.VARIANTS["stream"], SGPU_BLOCK="512"))
    knn_run = SC.Run(run.name, run.queries, run.k, run.cut, run.hf, n_knn=H.KNN, env=run.env, cycle=run.cycle)
    ok, h = CPU.expectation(case, ix, knn_run, env, **_chip())
    Q = case.batch(run)
    pick = np.arange(len(Q[0]) - 1) % len(run.queries)
    with CC.knobs(env):
        b = _native.DeviceBatch(ix, *Q, run.k)
        try:
            if h is None:                               # no lookup layout fits: the launch says so, as the hook did
                assert vocab == "large" and not ok
                with pytest.raises(_native.SeismicHipError) as e:
                    b.run(run.k, run.cut, run.hf, n_knn=H.KNN)
                assert e.value.status == CPU.SGPU_ELIMIT, e.value
                return
            stats = b.run(run.k, run.cut, run.hf, n_knn=H.KNN)
            v = _lane_report(ix)
            what = "%s %s n_knn %d" % (vocab, batch, H.KNN)
            print("%s: hash_ok %d, lookup %d" % (what, ok, v["lookup"]))
            assert v["lookup"] == h["lookup"] and stats.lds_bytes == h["lds_bytes"], (what, v, h)
            assert (v["lookup"] == H.LK_HASH) == bool(ok and (vocab, batch) not in H.LDS_DECLINES) and (batch not in HASHED or v["lookup"] == H.LK_HASH), (what, v)
            _assert_rows(b.fetch(run.k), _oracle(case, ix, run, n_knn=H.KNN), pick, what)
        finally:
            b.close()


def _chunks(ix, nq):
    """The pool lanes that served the last entry-point call of this thread, in order: lanes are handed out lowest first and
    chunk j takes lane j, so the call's chunks tile [0, nq) from lane 0 on."""
    out, pos = [], 0
    for lane in range(8):
        if pos == nq:
            break
        c = _native.debug_lane_chunk(ix, lane)
        assert c is not None and c["q_base"] == pos, (lane, c, pos)
        out.append((lane, c))
        pos += c["nq"]
    assert pos == nq, (pos, nq)
    return out


@pytest.mark.parametrize("filtered", (False, True))
@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("vocab", H.VOCABS)
def test_staged_calls_are_planned_by_the_host_and_report_the_lookup(vocab, batch, filtered):
    case, ix, flt = _uploaded(vocab)
    run = case.runs[batch]
    Q = case.batch(run)
    nq = len(Q[0]) - 1
    pick = np.arange(nq) % len(run.queries)
    what = "%s %s staged%s" % (vocab, batch, " filtered" if filtered else "")
    ok = case.restated(run)[0]
    keep = SC.FilteredDesc(ix.desc, case.allowed()) if filtered else None
    with CC.knobs(run.env):
        if vocab == "large" and not ok:               # the capacity limit: no layout for a query without a seed
            with pytest.raises(_native.SeismicHipError) as e:
                ix.batch_search(*Q, run.k, run.cut, run.hf, False, filter=flt if filtered else None)
            assert e.value.status == CPU.SGPU_ELIMIT, (what, e.value)
            return
        rows = ix.batch_search(*Q, run.k, run.cut, run.hf, False, filter=flt if filtered else None)
        off = Q[0].astype(np.int64)
        for lane, c in _chunks(ix, nq):
            q0, q1 = c["q_base"], c["q_base"] + c["nq"]
            Qc = (np.ascontiguousarray(off[q0: q1 + 1] - off[q0]).astype(np.uint64), Q[1][off[q0]: off[q1]], Q[2][off[q0]: off[q1]])
            ok_c = H.seeds(Qc[0], Qc[1], case.dim)[0]
            h = _native.debug_launch_config(heap_factor=run.hf, **dict(SC.plan_facts(case, ix, run, Qc), hash_ok=ok_c, staged=1, **_chip()))
            v = _lane_report(ix, lane)
            print("%s: lane %d queries [%d, %d) planned by %d, hash_ok %d, lookup %d streamed %d coop %d" % (
                what, lane, q0, q1, c["planned_by"], ok_c, v["lookup"], v["streamed"], v["coop"]))
            assert c["planned_by"] == 0, (what, lane, c)                              # the host: the seeds are its work
            assert v == {k_: h[k_] for k_ in ("lookup", "streamed", "coop", "counted")}, (what, lane, v, h)
            assert (v["lookup"] == H.LK_HASH) == bool(ok_c and (vocab, batch) not in H.LDS_DECLINES), (what, lane, v)
            assert batch not in HASHED or v["lookup"] == H.LK_HASH, (what, lane, v)
    _assert_rows(rows, _oracle(case, ix, run, desc=keep.desc if keep else None), pick, what)
