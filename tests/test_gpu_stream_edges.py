"""The streamed stage 2 (search_stream.inc) at the edges of its ring, its queues and its feeder, on the cases of
tests/stream_cases.py: ring wrap, blocks against the feed batch and the ring, feeder steps of 191 ... 385 positions and
pruned whole steps, the length classes, a window with the same document twice, every heap variant, threshold publication
under falling, rising and negative scores, the speculation budget's knobs, list groups, kNN refinement behind the ring, a
workgroup's next query, a filtered search. Every run is launched with SGPU_COOP=0 under SGPU_RING_MAX in {256, 512, 1024}
x SGPU_BLOCK in {512, 1024}: the launch configuration's hook, fed the launch's facts, must say "streamed, this ring, this
workgroup size" and agree with the launch's own statistics; the rows are the oracle's bit for bit (n, ids in order, score
bits) and pass the float64 model's checkers; the same call under SGPU_STREAM=0 (the round loop) returns the same rows,
which only localises a failure. test_stream_cases_cpu.py proves without a device that the cases reach their edges.
No test here forces a wait to give up (abort codes 16 / 17 / 18). Run with `-m gpu`."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import orc
import stream_cases as SC
import test_stream_cases_cpu as CPU
from seismic_amd import _native
from seismic_amd._abi import LaunchStats

pytestmark = pytest.mark.gpu
PARAMS = [(ring, block) for ring in SC.RINGS for block in SC.BLOCKS]


@functools.lru_cache(maxsize=None)
def _uploaded(name):
    """(case, uploaded index, its filter) - once per module; the kNN graph of the `units` cases is the oracle's."""
    case = SC.make(name)
    ix = case.build()
    if case.kind == "units":
        ix.set_knn(CPU.graph(name), SC.U_KNN)
    ix.upload(0)
    return case, ix, ix.make_filter(case.allowed())


def _chip():
    p = torch.cuda.get_device_properties(0)
    return p.multi_processor_count, int(getattr(p, "shared_memory_per_block", 160 * 1024))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _launch(case, ix, flt, run, Q):
    """One call of the run: (rows, launch statistics). A filtered run goes through batch_search (its statistics: the last
    launch's), the others through a resident batch."""
    if run.filtered:
        rows = ix.batch_search(*Q, run.k, run.cut, run.hf, run.first_sorted, n_knn=run.n_knn, filter=flt)
        stats = LaunchStats()
        _native.check(_native.lib().sgpu_batch_sync(ix.h, ctypes.byref(stats)))
        return rows, stats
    b = _native.DeviceBatch(ix, *Q, run.k)
    stats = b.run(run.k, run.cut, run.hf, run.first_sorted, n_knn=run.n_knn)      # (raises unless SGPU_OK)
    rows = b.fetch(run.k)
    b.close()
    return rows, stats


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


@pytest.mark.parametrize("ring,block", PARAMS)
@pytest.mark.parametrize("name", SC.CASE_NAMES)
def test_streamed_rows_are_the_oracles(name, ring, block, monkeypatch):
    case, ix, flt = _uploaded(name)
    n_cu, max_lds = _chip()
    for run in case.runs.values():
        asked, want_block, env = next((a, b, e) for r, a, b, e in SC.knob_sets(case, run) if (r, a) == (ring, block))
        for k_, v_ in env.items():
            monkeypatch.setenv(k_, v_)
        Q = case.batch(run)
        nq = len(Q[0]) - 1
        pick = np.arange(nq) % len(run.queries)
        what = "%s %s ring %d block %d" % (name, run.name, ring, block)
        # proof of variant: the hook, fed this launch's facts under this environment, says streamed / ring / block, and the
        # launch took that workgroup size and that much LDS
        rows, stats = _launch(case, ix, flt, run, Q)
        hook = _native.debug_launch_config(n_cu=n_cu, max_lds=max_lds, heap_factor=run.hf, **SC.plan_facts(case, ix, run, Q))
        assert (hook["streamed"], hook["coop"], hook["ring"], hook["block"]) == (1, 0, ring, want_block), (what, hook)
        # (a filtered run goes through the entry point, which may cut the call into several launches and reports the last
        # one's statistics: its workgroup size is compared, its LDS bytes are not)
        assert stats.block == hook["block"] and (run.filtered or stats.lds_bytes == hook["lds_bytes"]), (what, stats.block, stats.lds_bytes, hook)
        assert stats.n_queries == nq or (run.filtered and 0 < stats.n_queries < nq)      # (the entry point may cut its call into launches)
        if run.cycle:
            assert stats.grid < nq and np.gcd(stats.grid, len(run.queries)) == 1, (what, stats.grid)   # every workgroup goes on to a next query
        # results: the oracle's rows, bit for bit (every occurrence of a repeated query the same row)
        _assert_rows(rows, CPU.oracle_rows(name, run.name), pick, what)
        CPU.check_rows_against_the_model(name, run.name)      # (the float64 checks, on these very rows)
        # cross-check: the round loop on the same call
        monkeypatch.setenv("SGPU_STREAM", "0")
        loop_rows, loop_stats = _launch(case, ix, flt, run, Q)
        off = _native.debug_launch_config(n_cu=n_cu, max_lds=max_lds, heap_factor=run.hf, **SC.plan_facts(case, ix, run, Q))
        assert off["streamed"] == 0 and loop_stats.block == off["block"] and (run.filtered or loop_stats.lds_bytes == off["lds_bytes"]), what
        for a, b in zip(rows, loop_rows):
            assert np.array_equal(_bits(a) if a.dtype == np.float32 else a, _bits(b) if b.dtype == np.float32 else b), what
        for k_ in list(env) + ["SGPU_STREAM"]:
            monkeypatch.delenv(k_)
