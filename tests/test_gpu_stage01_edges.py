"""Stage 0 and stage 1 of the search kernel (search_stage01.inc) at their structural edges, on the cases of
tests/stage01_cases.py: row halves of 0 ... 129 entries, absent rows, empty 64-row blocks, 1 ... 129 chunks per descriptor
block, queries of 1 ... 513 components, the hashed row directory's displaced, wrapped and absent keys, the u32 binary search
over 0 ... 3 rows, list groups at the equality of dots_cap and qg, more streams than wavefronts, list selection under ties,
signs and cuts, the lookup table's clearing between a workgroup's queries under every layout, and sort_first_list around
the workgroup size. Dots: ix.summary_distances (the kernel's MODE_DOTS) equals orc.summary_distances as uint32 bits under
SGPU_BLOCK 512 and 1024. Searches: under SGPU_BLOCK 512 and 1024 the launch configuration's hook, fed the launch's facts,
(hash_ok from sgpu_debug_plan_seeds), names the layout, qg, dots_cap, workgroup size and variant the run is there for and
agrees with the launch's statistics and with the lane's report of the variant that ran (sgpu_debug_lane_variant);
the rows are the oracle's bit for bit (n, ids in order, score bits) and pass the float64 model's checkers; the counted pass's
counters [0..6] equal orc.batch_search_counts per query. test_stage01_cases_cpu.py proves without a device that the cases
reach their edges. No test here forces an abort code or a fault. Run with `-m gpu`."""
import functools

import numpy as np
import pytest
import torch

import coop_cases as CC
import hash_cases as H
import stage01_cases as S
import stream_cases as SC
import test_stage01_cases_cpu as CPU
from seismic_amd import _native

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _uploaded(name):
    """(case, uploaded index) - once per module."""
    case = S.make(name)
    ix = case.build()
    ix.upload(0)
    return case, ix


def _chip():
    p = torch.cuda.get_device_properties(0)
    return p.multi_processor_count, int(getattr(p, "shared_memory_per_block", 160 * 1024))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("block", S.BLOCKS)
@pytest.mark.parametrize("name", S.DOT_CASES)
def test_summary_dots_are_the_oracles_bit_for_bit(name, block):
    case, ix = _uploaded(name)
    with CC.knobs(dict(SGPU_BLOCK=str(block))):
        for (lst, q), want in zip(case.dots, CPU.oracle_dots(name)):
            got = ix.summary_distances(case.P(lst), *case.queries[q])
            assert len(got) == len(want), (name, lst, q, len(got), len(want))
            bad = np.flatnonzero(_bits(got) != _bits(want))
            assert len(bad) == 0, "%s list %d query %s block %d: %d of %d dots differ, first at block %d: device %r, oracle %r" % (
                name, lst, q, block, len(bad), len(want), bad[0], got[bad[0]], want[bad[0]])


def _assert_rows(got, want, pick, what):
    (gs, gi, gn), (ws, wi, wn) = got, want
    assert np.array_equal(gn, wn[pick]), (what, np.flatnonzero(gn != wn[pick])[:8])
    bad = np.flatnonzero((gi != wi[pick]).any(axis=1) | (_bits(gs) != _bits(ws)[pick]).any(axis=1))
    if len(bad):
        q = int(bad[0])
        at = int(np.flatnonzero((gi[q] != wi[pick[q]]) | (_bits(gs)[q] != _bits(ws)[pick[q]]))[0])
        raise AssertionError("%s: query %d differs first at rank %d: device (%r, %d), oracle (%r, %d); %d of %d rows differ" % (
            what, q, at, gs[q, at], gi[q, at], ws[pick[q], at], wi[pick[q], at], len(bad), len(gn)))


@pytest.mark.parametrize("block", S.BLOCKS)
@pytest.mark.parametrize("name", S.SEARCH_CASES)
def test_searches_are_the_oracles_rows_and_counters(name, block):
    case, ix = _uploaded(name)
    n_cu, max_lds = _chip()
    for run in case.runs.values():
        what = "%s %s block %d" % (name, run.name, block)
        Q = case.batch(run)
        nq = len(Q[0]) - 1
        pick = np.arange(nq) % len(run.queries)
        ws, wi, wn, wc = CPU.oracle_counts(name, run.name)
        env = S.knob_env(case, run, block)
        with CC.knobs(env):
            b = _native.DeviceBatch(ix, *Q, run.k)
            stats = b.run(run.k, run.cut, run.hf, run.first_sorted)            # (raises unless SGPU_OK)
            rows = b.fetch(run.k)
            # hash_ok of this very batch, from the host plan's own seed search (equal to the restatement's: hash_cases.py)
            ok, _ = _native.debug_plan_seeds(ix, *Q, run.cut)
            assert ok == H.seeds(Q[0], Q[1], case.dim, case.cw, case.value_type, "SGPU_NO_HASH" in env)[0], (what, ok)
            facts = dict(SC.plan_facts(case, ix, run, Q), n_cu=n_cu, max_lds=max_lds, hash_ok=ok)
            h = _native.debug_launch_config(heap_factor=run.hf, **facts)
            # proof of variant: the hook names what the run is there for, the lane reports that variant and the launch took
            # that workgroup and that much LDS
            assert (h["block"], h["coop"], h["streamed"]) == (block, 2 if run.coop else 0, 0 if run.coop else 1), (what, h)
            assert stats.block == h["block"] and stats.n_queries == nq, (what, stats.block, stats.n_queries)
            v = _native.debug_lane_variant(ix)
            assert v == {k_: h[k_] for k_ in ("lookup", "streamed", "coop", "counted")}, (what, v, h)
            if "SGPU_FORCE_HASH" in run.env:
                assert ok == 1, what                   # (every query of these batches has a seed: stage01_cases._check_lookup)
            for k_, v_ in run.expect.items():
                assert h[k_] == v_, (what, k_, h[k_], v_)
            assert stats.lds_bytes == h["lds_bytes"], (what, stats.lds_bytes, h["lds_bytes"])
            if run.cycle and not run.coop:
                assert stats.grid < nq and np.gcd(stats.grid, len(run.queries)) == 1, (what, stats.grid)   # every workgroup goes on
            _assert_rows(rows, (ws, wi, wn), pick, what)
            CPU.check_rows_against_the_model(name, run.name)                   # (the float64 checks, on these very rows)
            # the counted pass: same rows, and the per-query work counters - entries and matched rows witness the row tables
            b.run_counted(run.k, run.cut, run.hf, run.first_sorted)
            _assert_rows(b.fetch(run.k), (ws, wi, wn), pick, what + " counted")
            got = b.fetch_stats()[:, :7].astype(np.int64)
            want = wc[pick][:, :7].astype(np.int64)
            bad = np.flatnonzero((got != want).any(axis=1))
            assert len(bad) == 0, "%s: counters of query %d: device %s, oracle %s (%s)" % (
                what, bad[0], got[bad[0]].tolist(), want[bad[0]].tolist(), ", ".join(SC.orc.COUNT_NAMES[:7]))
            b.close()
